/* silent_speech_hip.h -- C ABI of libsilent_speech_hip.so: the MI355X (gfx950) implementation of the
 * EMG->mel transduction TRAINING hot path of dgaddy/silent_speech (plus, per SURVEY section 8f, the CTC loss of the
 * recognition trainer and the input-conditioning kernel of the device-side pipeline).
 *
 * The reference is pure Python/PyTorch and has no FFI seam; its seam for this path is the set of
 * torch operator calls made by architecture.py / transformer.py / transduction_model.py / align.py /
 * data_utils.py.  Each entry point below replaces the reference call sites cited next to it
 * (file:line are relative to the reference repository root).  Conventions:
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer (HBM) unless marked [host];
 *   - `stream` is a hipStream_t passed as void*; nothing here synchronises the device;
 *   - `dtype`: SS_F32 (0) or SS_BF16 (1) is the activation/compute type; statistics, losses,
 *     gradients of parameters and optimizer state are always f32;
 *   - return 0 on success; non-zero on error, with a message available from ss_last_error();
 *   - inputs are never modified unless documented (the reference's in-place EMG shift,
 *     architecture.py:67-68, is such a case and is mirrored by ss_emg_prepare's `shift`).
 * The Python binding a maintainer of the reference would add is a ctypes stub.
 */
#ifndef SILENT_SPEECH_HIP_H
#define SILENT_SPEECH_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SS_F32 0
#define SS_BF16 1
#define SS_F32X3 3   /* ss_gemm dtype_in only: f32 operands in memory, arithmetic on three bf16 MFMAs per product (operands split
                        hi + lo in registers, f32 accumulate: 16-17 significant bits per operand instead of 24 / 8) */

const char* ss_last_error(void);
/* Library/ABI version and the GPU architecture the kernels were compiled for ("gfx950"). */
/* Bumped whenever a struct layout or an entry-point signature changes (3: ss_gemm_epilogue column-statistics fields, the plan /
 * attention-image / LayerNorm-workspace entry points, ss_dtw_cumulative; 4: ss_loss_index_tables; 5: gate recomputation arguments of ss_bn_backward_sums / ss_bn_backward_apply; 7: ss_split_planes / ss_gemm_planes, ss_dw_job.flags, up to 24 jobs per grouped launch; 8: ss_stft_logmel_fft, the rejected-frame counter behind the matrix of ss_phoneme_confusion; 9: planes_hi / planes_lo / planes_only of ss_gemm_epilogue, dropout groups of the GEMM epilogue are row-major; 10: ss_emg_features_batch; 11: the ss_voc_* vocoder entry points; 12: the ragged-batch inference entry points ss_bn_apply_ragged, ss_relpos_attention_forward_ragged, ss_plan_forward_ragged; 13: ss_ctc_beam_search / ss_ctc_beam_workspace_bytes; 14: ss_word_lm, ss_ctc_word_beam_search / ss_ctc_word_beam_workspace_bytes, ss_word_ngram_score; 15: ss_audio_resample_batch / ss_audio_resample_supported / ss_audio_resample_limits, ss_audio_level_batch; 16: ss_spectral_gate_profile / ss_spectral_gate_batch / ss_spectral_gate_limits; 17: ss_stft_logmel_fft_backward / ss_stft_logmel_fft_backward_workspace_bytes; 18: ss_ctc_align / ss_ctc_align_workspace_bytes; 19: ss_spectral_gate_ns_batch; 20: ss_iir_filtfilt / ss_iir_filtfilt_workspace_bytes / ss_linear_resample / ss_reflect_pad removed, a single signal is a batch of one; 21: ss_word_state_lm, ss_ctc_word_state_beam_search / ss_ctc_word_state_beam_workspace_bytes, ss_word_state_score; 22: ss_edit_distance / ss_edit_distance_workspace_bytes, ss_nbest_risk; 23: ss_ctc_nbest_logp / ss_ctc_nbest_workspace_bytes / ss_ctc_nbest_backward, ss_nbest_expected_risk).  Bindings must compare it with SS_ABI_VERSION at load time: a stale
 * library paired with newer headers would otherwise read garbage struct fields instead of failing. */
#define SS_ABI_VERSION 23
int ss_abi_version(void);
const char* ss_target_arch(void);

/* ---------------------------------------------------------------------------------------------
 * Row addressing: logical row i starts at element
 *      base + (i / rows_per_batch) * batch_stride + (i % rows_per_batch) * row_stride
 * (rows_per_batch <= 0 means "one batch").  Expresses plain matrices, the zero-padded (B, T+2, C)
 * activation buffers, the overlapping 3C-wide im2col rows of the k=3 convolutions and strided
 * scatter of their input gradients. */
typedef struct ss_rowmap {
    int64_t base;
    int64_t batch_stride;
    int64_t row_stride;
    int32_t rows_per_batch;
} ss_rowmap;

typedef struct ss_gemm_epilogue {
    const float* bias;      /* [N] f32 or NULL                                                        */
    const void* gate;       /* out-typed tensor addressed like C or NULL: out = gate>0 ? out*gate_scale : 0
                               (ReLU + inverted-dropout backward from the SAVED activation)           */
    float gate_scale;
    float alpha;            /* scale applied to the accumulator first                                 */
    int32_t relu;           /* F.relu  (architecture.py:32; transformer.py:57)                        */
    float dropout_p;        /* nn.Dropout in training mode (transformer.py:57); counter-based hash RNG  */
    uint64_t seed;
    uint32_t rng_stream;    /* dropout site id; element (row, col) is element row * N + col of the stream (4 consecutive elements share a draw group) */
    int32_t mode;           /* 0 store, 1 C += v, 2 atomicAdd(C, v) (f32 out; required for split_k>1) */
    int32_t col_mod, col_mul, col_div_mul; /* optional output column permutation
                               col -> (col % col_mod)*col_mul + (col / col_mod)*col_div_mul           */
    float log_clamp;        /* > 0: v = log(max(v, log_clamp)) (data_utils.py:29-30 dynamic range compression) */
    void* c2;               /* optional second copy of the result, element (row, col) at
                               c2[rowmap2(row) + col*col_stride2] -- the [b][col][t] transposed copies
                               the attention kernels read as MFMA B operands                          */
    ss_rowmap cmap2;
    int64_t col_stride2;
    /* optional per-column statistics of the STORED result (f32, accumulated with atomics; the caller zeroes them):
       col_sum[n] += sum_m (C[m][n] - shift[n]),  col_sumsq[n] += sum_m (C[m][n] - shift[n])^2   (shift NULL = 0, col_sumsq may be NULL).
       Serves nn.Linear bias gradients (column sums of dY) and the BatchNorm batch statistics of a convolution output
       (architecture.py:19,21,25) without a separate pass over the tensor.  Only the 8-wave kernel computes them: ask
       ss_gemm_fuses_column_stats() first and fall back to ss_colsum / ss_bn_stats_sums when it answers 0. */
    float* col_sum;
    float* col_sumsq;
    const float* col_shift;
    /* ss_gemm_planes only (ABI 9): the stored result ALSO leaves as hi / lo bf16 planes -- hi = bf16(v), lo = bf16(v - hi), the arithmetic of
       ss_split_planes on the f32 value the kernel stores -- addressed like C (same row map, 2-byte elements), so that a consumer that is a plane
       GEMM / plane attention needs no split pass over C.  planes_only != 0: C itself is not written (C is still the address the row map refers to
       and must be non-NULL).  Column statistics, gate and accumulation apply before the split, as they do before the store.  NULL = off. */
    void* planes_hi;
    void* planes_lo;
    int32_t planes_only;
    /* The sign of a stored activation as ONE BIT per element (ABI 9), for the backward of ReLU (+ inverted dropout) -- transformer.py:57 --:
       sign_out (producer, bf16 results): byte [row * sign_pitch + col / 8], bit col % 8 = [stored C(row, col) > 0], rows = the GEMM's logical rows.
       gate_bits (consumer): out = bit ? out * gate_scale : 0 -- what `gate` does from the saved tensor, from 1/16 of its bytes; a thread requests the bits of
       its whole tile at once, so the 18 exposed load round trips per tile of the tensor form shrink to one.  N % 8 == 0.  Only some kernels of the 8-wave
       family carry these paths: ask ss_gemm_sign_bits_supported() (producer) / ss_gemm_fuses_column_stats() with gate_bits set (consumer: it rides the
       column-sum epilogue) and keep `gate` otherwise; ss_gemm refuses a launch that would ignore them. */
    void* sign_out;
    int64_t sign_pitch;
    const void* gate_bits;
    int64_t gate_bits_pitch;
} ss_gemm_epilogue;

#define SS_OP_KC 0   /* reduction index contiguous:  elem(o, r) = p[rowmap(o) + r] */
#define SS_OP_OC 1   /* outer index contiguous:      elem(o, r) = p[rowmap(r) + o] */

/* C[m][n] (+)= alpha * sum_k A(m,k) * B(n,k) on the MFMA units, f32 accumulate.
 * Replaces: nn.Conv1d k=3/k=1 (architecture.py:18,20,24 -> F.conv1d) as implicit GEMM over padded
 * activation buffers; nn.Linear (architecture.py:51,55,59; transformer.py:32,34); the per-head
 * einsum projections 'tbf,hfa->bhta' / 'bhta,haf->tbf' (transformer.py:96-98,111); and the autograd
 * backward of all of them (transduction_model.py:209): dX = dY.W (b_mode = OC), dW = dY^T.X
 * (a_mode = b_mode = OC, split_k > 1 with atomic f32 accumulation).
 * dtype_in: SS_BF16 (bf16 MFMA), SS_F32 (exact f32 MFMA 16x16x4) or SS_F32X3 (f32 operands, bf16 x 3 MFMA: ~5x the f32 rate at
 * ~1e-5 relative error per product, the "parity-grade fast mode" of the training plan, ss_plan_set_option 5). */
int ss_gemm(int dtype_in, int dtype_out, int a_mode, int b_mode, const void* A, const void* B, void* C,
            int M, int N, int K, const ss_rowmap* amap, const ss_rowmap* bmap, const ss_rowmap* cmap,
            const ss_gemm_epilogue* epilogue, int split_k, void* stream);

/* f32 operands as two bf16 planes (round 6: the parity-grade arithmetic of SS_F32X3 on the 8-wave bf16 kernel).
 * ss_split_planes: hi[i] = bf16(x[i]), lo[i] = bf16(x[i] - hi[i])  (x = hi + lo to 2^-17 relative); an elementwise pass, 16-byte aligned buffers.
 * ss_gemm_planes:  C[m][n] = epilogue(sum_k A(m,k) B(n,k)) with A = A_hi + A_lo, B = B_hi + B_lo, both operands K-contiguous and both planes
 *   of an operand addressed by the SAME row map, computed as ONE bf16 contraction of length 3 K,  [A_lo | A_hi | A_hi] . [B_hi | B_lo | B_hi]^T
 *   (three bf16 MFMAs per product, f32 accumulate; the a_lo.b_lo term, 2^-18 of the product, is dropped -- the arithmetic of SS_F32X3).
 *   f32 output only; runs on the 8-wave kernel or not at all: ss_gemm_planes_supported() answers 1 when it does (K % 64 == 0, 16-byte
 *   rows, no transposed second output, no log-clamp), and the call fails otherwise (the caller keeps ss_gemm(SS_F32X3) for such shapes).
 * Replaces, in the f32-storage plan: the f32 matmuls of architecture.py:18-24,51,55,59 and transformer.py:32,34,96-98,111 and their
 * input gradients.  Weight gradients of that mode: ss_gemm_dw_grouped with three jobs per gradient (hi.hi, hi.lo, lo.hi; flags bit 0). */
int ss_split_planes(const float* x, void* hi, void* lo, int64_t n, void* stream);
int ss_gemm_planes(int dtype_out, const void* A_hi, const void* A_lo, const void* B_hi, const void* B_lo, void* C, int M, int N, int K,
                   const ss_rowmap* amap, const ss_rowmap* bmap, const ss_rowmap* cmap, const ss_gemm_epilogue* epilogue, void* stream);
/* [host] 1 when ss_gemm with these arguments (epilogue->sign_out set or not) runs on the kernel that writes sign bits (8-wave kernel, bf16 results, no column
 * statistics, default schedule, N % 8 == 0). */
int ss_gemm_sign_bits_supported(int dtype_in, int dtype_out, int a_mode, int b_mode, const void* C, int M, int N, int K, const ss_rowmap* amap,
                                const ss_rowmap* bmap, const ss_rowmap* cmap, const ss_gemm_epilogue* epilogue, int split_k);
int ss_gemm_planes_supported(int dtype_out, const void* C, int M, int N, int K, const ss_rowmap* amap, const ss_rowmap* bmap, const ss_rowmap* cmap,
                             const ss_gemm_epilogue* epilogue); /* [host] */

/* Persistent-grid size of ss_gemm for the calling thread: 2 (default) or 1 workgroup per CU.  The weight-gradient GEMMs that
 * run on a side stream use 1 so that the dependent chain on the main stream can co-reside on every CU.  Returns the old value. */
int ss_gemm_set_blocks_per_cu(int n); /* [host] */
/* Which kernel the calling thread's last ss_gemm launch used: 0 register-staged gemm_kernel, 1 gemm_glds_kernel,
 * 2 gemm_w2_kernel, 3 / 4 gemm8_kc_kernel with 256 / 288-row tiles, 5 gemm_smallk_kernel (K <= 32, no LDS) (so that a profiler can attribute per-launch timings to
 * the kernel names rocprofv3 reports, and tests can assert which variant they exercised). */
int ss_gemm_last_kernel(void); /* [host] */
/* 1 if ss_gemm with these arguments runs a kernel that honours epilogue.col_sum / col_sumsq (the 8-wave kernel, the K <= 32 kernel); 0 otherwise (the call then fails
 * with those fields set).  Same decision procedure as ss_gemm itself (legality + cost model + knobs). */
int ss_gemm_fuses_column_stats(int dtype_in, int dtype_out, int a_mode, int b_mode, const void* C, int M, int N, int K, const ss_rowmap* amap,
                               const ss_rowmap* bmap, const ss_rowmap* cmap, const ss_gemm_epilogue* epilogue, int split_k); /* [host] */
/* Kernel-selection knobs of ss_gemm (process-wide): what = 0 two-wave kernel (0 never / 1 cost model / 2 whenever legal),
 * 1 its tile height (128 / 144, 0 = cost model), 2 eight-wave kernel (0 / 1 / 2 as above), 3 its tile height in 16-row units
 * per M-wave (8 / 9, 0 = cost model), 4 its LDS reads / DMA pieces spread between MFMA groups (0 / 1, 2 = per tile height), 5 ablation mask for kernel tuning (results are
 * wrong when non-zero), 6 the LDS-free K <= 32 kernel on / off (SS_GEMM_SMALLK).  value < 0 restores the default (environment SS_GEMM_W2, SS_GEMM_W2_BM, SS_GEMM8, SS_GEMM8_NI, SS_GEMM8_PIN,
 * SS_GEMM_DEBUG).  Returns the previous value, -1 for a bad `what`. */
int ss_gemm_set_option(int what, int value); /* [host] */

/* Grouped weight-gradient GEMMs: for every job  C[m][n] += sum_k A(k, m) * B(k, n)  (bf16 operands, f32 C, reduction over the
 * K = B*T frame rows; both operands outer-contiguous: element (k, m) of A at A[amap(k) + m]).  Replaces the autograd backward
 * of nn.Linear / nn.Conv1d / the per-head einsum projections w.r.t. their weights (transduction_model.py:209 through
 * architecture.py:18-24,51 and transformer.py:32,34,96-98,111): dW = dY^T X.  ONE persistent launch covers up to 24 jobs (e.g.
 * the four weight gradients of an encoder layer), so the K split that fills the 256 CUs -- and with it the number of f32
 * atomic accumulations -- is chosen for the group, not per GEMM.  M, N multiples of 8; amap / bmap must cut the rows into
 * batches of equal length (rows_per_batch). */
typedef struct ss_dw_job {
    const void* A;          /* dY: K rows of M contiguous bf16 */
    const void* B;          /* X : K rows of N contiguous bf16 */
    float* C;               /* M x N f32, row stride ldc; accumulated into */
    ss_rowmap amap, bmap;
    int64_t ldc;
    int32_t M, N, K;
    int32_t flags;          /* bit 0: other jobs of this launch accumulate into the same C (always atomic updates) */
} ss_dw_job;
int ss_gemm_dw_grouped(int n_jobs, const ss_dw_job* jobs /* [host] */, void* stream);
/* Tuning knobs of ss_gemm_dw_grouped for the calling thread: what = 0 K split override (0 = automatic), 1 scheduling fences,
 * 2 XCD-contiguous item order on / off (default on: neighbouring tiles of one problem share an L2). */
int ss_gemm_dw_set_option(int what, int value); /* [host] */

/* out[a][b][c] (contiguous, dims d0 x d1 x d2) (+)= scale * in[a*s0 + b*s1 + c*s2] for b < valid1 and
 * c < valid2, else 0 (zero padding).  Converts between the reference's parameter layouts (state_dict:
 * conv (O,I,k) architecture.py:18; w_q/w_k/w_v (H,d,dh), w_o (H,dh,d) transformer.py:71-74; embeddings
 * (H,2D-1,dh,1) transformer.py:159) and the GEMM-ready, head-dim-padded layouts, in both directions
 * (weights forward, gradients back).  in/out dtype: SS_F32 or SS_BF16. */
int ss_permute3d(const void* in, int in_dtype, void* out, int out_dtype, int d0, int d1, int d2,
                 int64_t s0, int64_t s1, int64_t s2, int valid1, int valid2, float scale, int accumulate,
                 void* stream);

/* The same for a whole table of jobs in one launch (per-step weight re-layout, gradient un-layout).
 * jobs_dev: device array of
 *   struct { const void* in; void* out; int64 s0,s1,s2 (input strides), o0,o1 (output strides of dims 0,1; dim 2 contiguous);
 *            int32 d0,d1,d2, valid1,valid2, in_dtype,out_dtype, accumulate; float scale; int32 first_block, nblocks, pad; }
 * job_of_block_dev[b] = job index of workgroup b (workgroups first_block .. first_block+nblocks-1 grid-stride over the job).
 * all_f32 != 0 promises that every job is f32 -> f32 (the gradient un-layout): a kernel specialised for read-modify-write runs. */
int ss_permute3d_batch(const void* jobs_dev, const int32_t* job_of_block_dev, int total_blocks, int all_f32, void* stream);

/* ---------------------------------------------------------------------------------------------
 * DTW alignment (align.py:5-14 time_warp + align.py:16-34 align_from_distances; call site
 * transduction_model.py:126,131 and :88).  Batched: one workgroup per matrix.
 * desc_dev: device array [n][10] of int64:
 *   {N, M, cost_off (elements from `costs`), stride_i, stride_j (elements), sk_off, dirs_off, bnd_off
 *    (BYTE offsets into `workspace`, sizes from ss_dtw_workspace_bytes), res_off (elements into
 *    `results`), 0}.
 * results[res_off + i], i < N: the reference's `results` list (smallest j visited in row i; 0 for
 * row 0 and for degenerate 1xM / Nx1 inputs).  Bit-exact: f32, one add per cell, first-minimum tie
 * order (up, left, diag).  The cumulative matrix itself is never written (2-bit directions are).
 * Where the recurrence takes its costs from is decided per matrix (ss_dtw_source): a matrix with one unit-stride axis of at most 1025
 * cells is read IN PLACE (2: row-major -- the lanes own columns, the kernel sweeps the transposed problem; 1: column-major, e.g. the
 * costs.T view of transduction_model.py:126 -- the lanes own rows); anything else (0: both strides > 1, a unit-stride axis longer than
 * one strip, fewer than 5 cells on it) is first copied into skewed strips inside `workspace`. */
int ss_dtw_source(int n, int m, int64_t stride_i, int64_t stride_j); /* [host] */
int64_t ss_dtw_workspace_bytes(int n, int m, int64_t* sk_bytes, int64_t* dirs_bytes, int64_t* bnd_bytes); /* [host] */
int ss_dtw_align(const float* costs, const int64_t* desc_dev, int n, int max_n, int max_m, void* workspace,
                 int32_t* results, void* stream);
/* Same, for costs already in the skewed strip layout (written by ss_silent_cost_skewed); results must
 * have been zeroed by the producer. */
int ss_dtw_align_skewed(const int64_t* desc_dev, int n, void* workspace, int32_t* results, void* stream);
/* align.py:5-14 `time_warp` itself: the dense cumulative matrix dtw_out[N][M] (contiguous) of ONE cost matrix whose element (i, j)
 * sits at costs + i*stride_i + j*stride_j (elements), in the dtype of the input (SS_F32 or SS_F64: `zeros_like(costs)`,
 * align.py:6); dtw_out[N-1][M-1] is the alignment cost.  results (optional, N ints): the reference's backtrace on that matrix
 * (align.py:16-34) -- this is how float64 input is aligned without rounding it to float32.  Not on the training path (one
 * workgroup, one barrier per anti-diagonal); batches of f32 matrices go through ss_dtw_align. */
int ss_dtw_cumulative(int dtype, const void* costs, int64_t stride_i, int64_t stride_j, int N, int M, void* dtw_out,
                      int32_t* results, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BatchNorm1d fused with ReLU / the ResBlock residual add (architecture.py:19,21,25 nn.BatchNorm1d,
 * :32 relu(bn1(conv1)), :33 bn2(conv2), :36 res_norm(residual_path), :40 relu(x + res)).
 * Activations are (B, T + 2*pad, C), C contiguous, pad in {0,1}: padded buffers carry a zero row on
 * each side of every sequence (the conv halo); pad rows of outputs are written as zeros.
 * Training: per-channel batch mean / 1/sqrt(biased var + eps) over B*T, running stats updated in place
 * (momentum, unbiased variance) as torch does; eval: from the running stats.
 * scratch: ss_bn_scratch_floats(B,T,C) floats. */
int64_t ss_bn_scratch_floats(int B, int T, int C); /* [host] */
/* Two-phase statistics so that data-parallel ranks can all-reduce between the phases (the batch
 * statistics of the reference span the WHOLE batch):  sums[3][C] = { sum(x-s), sum (x-s)^2, s } with
 * s = shift (a [C] vector identical on all ranks, e.g. running_mean) or, if NULL, the first row. */
int ss_bn_stats_sums(int dtype, const void* x, int B, int T, int C, int pad, float* scratch, const float* shift, float* sums, void* stream);
int ss_bn_finalize(const float* sums, double n_total, int C, float* mean, float* invstd, float* running_mean, float* running_var,
                   float momentum, float eps, int training, void* stream);
/* The same with the shift vector passed separately (sums = [2][C]): for sums produced by a GEMM epilogue (ss_gemm_epilogue.col_sum /
 * col_sumsq with col_shift = shift, e.g. the running mean BEFORE this update; shift may alias running_mean). */
int ss_bn_finalize_shift(const float* sums, const float* shift, double n_total, int C, float* mean, float* invstd, float* running_mean,
                         float* running_var, float momentum, float eps, int training, void* stream);
/* y = act( bn_a(xa) [+ bn_b(xb)] ),  act = ReLU if relu */
int ss_bn_apply(int dtype, const void* xa, const float* mean_a, const float* invstd_a, const float* gamma_a, const float* beta_a, int pad_xa,
                const void* xb, const float* mean_b, const float* invstd_b, const float* gamma_b, const float* beta_b, int pad_xb,
                void* y, int pad_y, int B, int T, int C, int relu, void* stream);
/* The same for a RAGGED batch in equal slots (inference; ss_plan_forward_ragged): sequence b owns rows t < lens_dev[b] * len_mul of its slot of T
 * rows (lens in model frames; len_mul = 4, 2, 1 for the three ResBlocks), rows behind that are stored as 0 -- the select that already writes the
 * pad rows, with a per-sequence bound -- so that the right tap of the next k = 3 convolution reads the zero padding an utterance has when it runs
 * alone (architecture.py:18,20 padding=1) and not its slot's filler.  The filler rows of the inputs are never converted, whatever they hold. */
int ss_bn_apply_ragged(int dtype, const void* xa, const float* mean_a, const float* invstd_a, const float* gamma_a, const float* beta_a, int pad_xa,
                       const void* xb, const float* mean_b, const float* invstd_b, const float* gamma_b, const float* beta_b, int pad_xb,
                       void* y, int pad_y, int B, int T, int C, int relu, const int32_t* lens_dev, int len_mul, void* stream);
/* autograd backward of the above (transduction_model.py:209), again in two phases:
 * sums[3][C] = { sum g, sum g*xhat_a, sum g*xhat_b } with g = dy*1[y>0]; dgamma/dbeta are ACCUMULATED (+=);
 * apply: dx = gamma*invstd*(g - sums0/n - xhat*sums{1,2}/n).
 * The ReLU gate 1[y>0] is read from the saved output y, or -- gate_beta_a != NULL -- RECOMPUTED as the sign of the forward's own
 * expression (xa - mean_a) gamma_a invstd_a + beta_a [+ the b branch] from the inputs both passes read anyway (y may then be NULL):
 * one tensor less per pass (the plan does this). */
int ss_bn_backward_sums(int dtype, const void* dy, int pad_dy, const void* y, int pad_y,
                        const void* xa, int pad_xa, const float* mean_a, const float* invstd_a,
                        const void* xb, int pad_xb, const float* mean_b, const float* invstd_b,
                        float* dgamma_a, float* dbeta_a, float* dgamma_b, float* dbeta_b,
                        float* scratch, float* sums, int B, int T, int C, int relu,
                        const float* gate_gamma_a, const float* gate_beta_a, const float* gate_gamma_b, const float* gate_beta_b, void* stream);
int ss_bn_backward_apply(int dtype, const void* dy, int pad_dy, const void* y, int pad_y,
                         const void* xa, int pad_xa, const float* mean_a, const float* invstd_a, const float* gamma_a,
                         const void* xb, int pad_xb, const float* mean_b, const float* invstd_b, const float* gamma_b,
                         const float* sums, double n_total, void* dxa, int pad_dxa, void* dxb, int pad_dxb,
                         int B, int T, int C, int relu, const float* gate_beta_a, const float* gate_beta_b, void* stream);
/* out[c] += sum_r x[r][c]  (bias gradients of nn.Linear / nn.Conv1d) */
int64_t ss_colsum_scratch_floats(int rows, int C); /* [host] */
int ss_colsum(int dtype, const void* x, int rows, int C, int64_t ld, float* scratch, float* out_accum, void* stream);

/* Post-norm residual block of the encoder layer (transformer.py:55-56, 58-59):
 *   z = x + dropout(branch);  y = LayerNorm(z) * gamma + beta        (eps 1e-5)
 * branch_inout is overwritten with z (saved for backward); mean/rstd: [rows] f32. */
int ss_add_dropout_layernorm_forward(int dtype, const void* x, void* branch_inout, const float* gamma, const float* beta, void* y,
                                     float* mean, float* rstd, int rows, int C, float eps, float dropout_p, uint64_t seed,
                                     uint32_t rng_stream, void* stream);
/* dres = dL/dz (gradient of the residual stream; may alias dy), dbranch = dres * keep/(1-p) (may be NULL);
 * dgamma/dbeta accumulated. */
int ss_layernorm_backward(int dtype, const void* dy, const void* z, const float* mean, const float* rstd, const float* gamma,
                          void* dres, void* dbranch, float* dgamma, float* dbeta, int rows, int C, float dropout_p, uint64_t seed,
                          uint32_t rng_stream, void* stream);

/* The same, also accumulating dbranch_colsum[c] += sum_rows dbranch[row][c] (as stored, i.e. rounded to dtype): the bias gradient of
 * the nn.Linear that produced the branch (linear2 of transformer.py:58), without a separate pass over dbranch. */
int ss_layernorm_backward_bias(int dtype, const void* dy, const void* z, const float* mean, const float* rstd, const float* gamma,
                               void* dres, void* dbranch, float* dgamma, float* dbeta, float* dbranch_colsum, int rows, int C, float dropout_p,
                               uint64_t seed, uint32_t rng_stream, void* stream);
/* The 16-waves-per-CU form (C = 256, 512 or 768; dbranch required): selected by passing a scratch buffer of
 * ss_layernorm_backward_scratch_floats(rows, C) floats (0 for other widths; scratch == NULL runs the round-1 form).  The column sums leave
 * as one atomic per column and workgroup (#CU workgroups); with SS_LN_DIRECT=0 they go through the scratch buffer and a second small kernel
 * instead (deterministic summation order). */
int64_t ss_layernorm_backward_scratch_floats(int rows, int C); /* [host] */
int ss_layernorm_backward_ws(int dtype, const void* dy, const void* z, const float* mean, const float* rstd, const float* gamma,
                             void* dres, void* dbranch, float* dgamma, float* dbeta, float* dbranch_colsum, float* scratch, int64_t scratch_floats,
                             int rows, int C, float dropout_p, uint64_t seed, uint32_t rng_stream, void* stream);
/* The parity-grade mode (f32 data): the LayerNorm output / the branch gradient ALSO leave as hi / lo bf16 planes (ss_split_planes' arithmetic on the stored f32
 * value), so that the plane GEMMs that consume them need no split pass (ABI 9).  NULL planes = the plain forms above. */
int ss_add_dropout_layernorm_forward_planes(int dtype, const void* x, void* branch_inout, const float* gamma, const float* beta, void* y, void* y_hi, void* y_lo,
                                            float* mean, float* rstd, int rows, int C, float eps, float dropout_p, uint64_t seed, uint32_t rng_stream, void* stream);
int ss_layernorm_backward_ws_planes(int dtype, const void* dy, const void* z, const float* mean, const float* rstd, const float* gamma,
                                    void* dres, void* dbranch, void* dbranch_hi, void* dbranch_lo, float* dgamma, float* dbeta, float* dbranch_colsum, float* scratch,
                                    int64_t scratch_floats, int rows, int C, float dropout_p, uint64_t seed, uint32_t rng_stream, void* stream);

/* EMG input conditioning: training-time shift augmentation (architecture.py:64-68: x[:, :-r] = x[:, r:],
 * x[:, -r:] = 0), cast to the compute dtype and zero halo rows: x_raw (B,T0,Cin) f32 ->
 * out_padded (B,T0+2,Cin).  shifted_copy (optional, f32 (B,T0,Cin)) receives the shifted signal so the
 * caller can mirror the reference's in-place mutation of its input. */
int ss_emg_prepare(int dtype, const float* x_raw, void* out_padded, float* shifted_copy, int B, int T0, int Cin, int shift, void* stream);

/* ---------------------------------------------------------------------------------------------
 * dtw_loss (transduction_model.py:98-157).  `head` = [pred (n_mel) | phoneme logits (n_phone)] per
 * packed frame, f32, row stride ld.  All kernels produce value AND gradient (dhead, same layout,
 * must be zero-initialised; scaled by inv_total = 1/sum(T2)); loss_accum/correct_accum are += . */
/* Per-frame index tables of one batch (the decollate_tensor + zip bookkeeping of transduction_model.py:101-111) expanded on the
 * device from one row of 8 int64 per utterance: [n_pred, n_tgt, silent, first packed pred row, first target row, offset into
 * `results`, offset into the voiced tables, offset into the silent tables].  Voiced utterance: vo_pred / vo_tgt [vo_off + i] =
 * pred_row0 + i / tgt_row0 + i; silent: si_tgt = tgt_row0 + i, si_base = pred_row0, si_res = res_off + i (i < n_tgt).  The tables
 * are what ss_voiced_loss / ss_silent_loss take; they may be sized exactly (sum of voiced n_pred / silent n_tgt, at least 1). */
int ss_loss_index_tables(const int64_t* utt_dev, int n_utt, int32_t* vo_pred, int32_t* vo_tgt, int32_t* si_tgt, int32_t* si_base,
                         int32_t* si_res, void* stream);
int ss_frame_lse(const float* head, int64_t ld, int col0, int ncls, int rows, float* lse, int32_t* argmax, void* stream);
int ss_voiced_loss(const float* head, int64_t ld, int n_mel, int n_phone, const float* lse, const int32_t* argmax, const float* Y,
                   const int64_t* phones, const int32_t* pred_row, const int32_t* tgt_row, int nframes, float lam, float inv_total,
                   float* dhead, float* loss_accum, int32_t* correct_accum, void* stream);
/* Cost matrices of the silent utterances written directly in the DTW strip layout (never dense);
 * desc as for ss_dtw_align with fields [2],[3] = first packed pred row, first target row. */
int ss_silent_cost_skewed(const float* head, int64_t ld, int n_mel, const float* lse, const float* Y, const int64_t* phones,
                          const int64_t* desc_dev, int n, int max_n, int max_m, float lam, void* workspace, int32_t* results, void* stream);
int ss_silent_loss(const float* head, int64_t ld, int n_mel, int n_phone, const float* lse, const int32_t* argmax, const float* Y,
                   const int64_t* phones, const int32_t* results, const int32_t* tgt_row, const int32_t* pred_base,
                   const int32_t* res_idx, int nframes, float lam, float inv_total, float* dhead, float* loss_accum,
                   int32_t* correct_accum, void* stream);
/* Phoneme confusion matrix of the evaluation path (transduction_model.py:130-137 silent, :147-152 voiced), accumulated ON the device:
 * confusion[pred * n_phone + target] += 1 for every target frame, pred = argmax (ss_frame_lse) of the aligned prediction row -- through
 * `results` (ss_dtw_align_skewed) for silent utterances.  Index tables as produced by ss_loss_index_tables; int32 matrix, += .
 * `confusion` holds n_phone * n_phone + 1 ints: the last one counts the frames whose prediction or target label lies outside [0, n_phone) (the
 * reference's numpy indexing raises IndexError for those, :134-137); they are left out of the matrix and the caller decides (DeviceConfusion raises). */
int ss_phoneme_confusion(const int32_t* argmax, const int64_t* phones, const int32_t* results, const int32_t* vo_pred, const int32_t* vo_tgt,
                         int n_voiced, const int32_t* si_tgt, const int32_t* si_base, const int32_t* si_res, int n_silent_frames,
                         int32_t* confusion, int n_phone, void* stream);

/* ---------------------------------------------------------------------------------------------
 * CTC loss of the recognition trainer ("next" row N1): replaces F.log_softmax + pad_sequence(decollate_tensor(...))
 * + F.ctc_loss(..., blank, reduction='mean') of recognition_model.py:96-101 on the PACKED (rows, ld) f32 logits.
 * lse = per-frame log-sum-exp over the V classes (ss_frame_lse with col0=0).  desc (device, int64 x5 per utterance,
 * sorted by frame0): first packed frame, T, first target index, S, offset (floats) of the utterance's T*(2S+1)
 * block in alpha_ws / beta_ws.  Writes nll[n_utt], loss[0] = mean_u nll_u / max(S_u, 1) and the complete
 * d loss / d logits (all `rows` x ld entries; zero outside the utterances). */
int ss_ctc_loss(const float* logits, int64_t ld, int V, int blank, const float* lse, const int64_t* desc_dev, int n_utt, int max_target_len,
                int64_t rows, const int32_t* targets, float* alpha_ws, float* beta_ws, float* nll, float* dlogits, float* loss, void* stream);

/* ---------------------------------------------------------------------------------------------
 * CTC prefix beam search with shallow fusion of a label n-gram table, the whole batch in one launch (csrc/ctc_decode.hip).
 * Inputs: f32 logits (rows, ld), classes in columns 0 .. V-1 (V <= 128, ld >= V, further columns are never read); lse = per-frame
 * log-sum-exp (ss_frame_lse with col0 = 0); blank in [0, V); utt_dev (device, int64 x2 per utterance) = first frame, frames -- the packed
 * layout (utterances back to back) and the slot layout of ss_plan_forward_ragged (first frame = b * T_max) alike; frames behind an
 * utterance's end are never read.  total_frames >= the sum of the frames (it sizes the workspace; an utterance that would exceed it, or
 * leave [0, rows), is cut short, never read out of bounds).  Beam width 1 <= W <= 128, 1 <= n_best <= W.  lm (optional, device): f32
 * natural-log probabilities (C+1, C+1, C), C = V-1 labels numbered with the blank skipped, context index C = "before the start"; all
 * entries finite.
 * Search: logp_t(c) = logit_t(c) - lse_t.  A beam entry is a label prefix with (lb, lnb), the log mass of its paths that end / do not end
 * in blank; start: the empty prefix with (0, -inf).  Per frame, for every entry p with tot = lb (+) lnb ((+) = log-add-exp):
 *   stay    lb'(p) (+)= tot + logp(blank); if p is not empty, lnb'(p) (+)= lnb + logp(last(p));
 *   extend  by every label c != blank to q = p + c: lnb'(q) (+)= (c == last(p) ? lb : tot) + logp(c).
 * A prefix reached by several routes is ONE candidate whose contributions are summed (q already in the beam while p + c produces it too).
 * score(q) = lb' (+) lnb' + sum_i (alpha * lm[q_{i-2}, q_{i-1}, q_i] + beta), the sum 0 without a table.  A candidate of score -inf does
 * not exist.  The W candidates of largest score survive; ties go to the lower candidate index (beam slot of p) * V + c (c = blank: p itself).
 * Outputs for the n_best best entries after the last frame, best first (ties: beam slot): labels (n_utt, n_best, max_len) int32 class
 * numbers, -1 behind the end (max_len >= the longest utterance's frames holds every string; longer strings keep their first max_len
 * labels), lengths (n_utt, n_best), scores and their CTC part alone (n_utt, n_best) f32 natural log.  Ranks that do not exist: length -1,
 * scores -inf.  An utterance of 0 frames yields the empty string with score 0.
 * workspace: ss_ctc_beam_workspace_bytes(n_utt, total_frames, W) bytes (the prefix trie; needs no initialisation); -1 = bad arguments. */
int64_t ss_ctc_beam_workspace_bytes(int n_utt, int64_t total_frames, int beam_width);
int ss_ctc_beam_search(const float* logits, int64_t ld, int V, int blank, int64_t rows, const float* lse, const int64_t* utt_dev, int n_utt,
                       int64_t total_frames, int beam_width, int n_best, const float* lm, float alpha, float beta, void* workspace, int max_len,
                       int32_t* labels, int32_t* lengths, float* scores, float* ctc_scores, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Word language model of the lexicon-constrained search below: a backoff n-gram over WORDS of order 1 .. 3 and the trie of their spellings,
 * all arrays on the device, natural-log f32.  Word ids are 0 .. n_vocab - 1 for the words of the lexicon; `start` (the sentence-start
 * context <s>) has an id of its own in [0, n_uni); every id is below 2^21.
 *   lex_child (n_nodes, C) int32, C = V - 1 labels numbered with the blank skipped: child node or -1; node 0 is the root; the space's column is
 *             all -1.  lex_word (n_nodes) int32: the id of the word spelled by the path to the node, or -1 (the root: -1).
 *   uni_logp / uni_bo (n_uni): ln P(w) and the backoff weight of the context (w).
 *   bi_* / tri_*: open-addressing hash tables, 64-bit keys (w1 << 21 | w; w2 << 42 | w1 << 21 | w), an all-ones key = empty slot, slot count a
 *             power of two (or 0: no table, which makes an order-2 / order-1 model), home slot = splitmix64 finaliser of the key & (slots - 1),
 *             linear probing that wraps around; *_probe = the longest probe sequence the builder needed, the lookup's loop bound.  Beside the
 *             keys: bi_logp, bi_bo, tri_logp.
 * ln P(w | w2, w1), w2 = -1 meaning "none": tri(w2, w1, w) if present; else (bo of bi(w2, w1), 0 if absent) + P2, P2 = bi(w1, w) if
 * present, else uni_bo(w1) + uni_logp(w); with w2 = -1 it is P2, and with w1 = -1 too it is uni_logp(w).
 * Every index formed from these tables is checked against the sizes given here: a malformed table gives wrong words, never a read outside
 * the arrays. */
typedef struct ss_word_lm {
    const int32_t* lex_child;
    const int32_t* lex_word;
    const float* uni_logp;
    const float* uni_bo;
    const uint64_t* bi_keys;
    const float* bi_logp;
    const float* bi_bo;
    const uint64_t* tri_keys;
    const float* tri_logp;
    int32_t n_nodes, n_vocab, n_uni, start;
    int32_t bi_slots, bi_probe, tri_slots, tri_probe;
} ss_word_lm;

/* CTC prefix beam search confined to a lexicon, with a word n-gram scored at every word end (csrc/ctc_word_decode.hip; what the reference's
 * ctcdecode does with a KenLM model, recognition_model.py:33-35 -- here from ARPA text or counted tables; parity with ctcdecode's own numbers
 * is unpinned).  Inputs, layouts, lb / lnb, stay / extend, merging of a prefix reached by several routes, "a candidate of score -inf does
 * not exist", ties to the lower candidate index, natural-log f32 and the outputs are those of ss_ctc_beam_search above.  Differences:
 *   state    an entry additionally has a lexicon node and a word context (w2, w1); start: the root and (none, start).  Both are functions of
 *            the label string, so merging is unchanged.  2 <= V, space in [0, V), space != blank.
 *   letter   extending p by c (neither blank nor space) exists only if child = lex_child[node(p)][label(c)] is in [0, n_nodes); it becomes
 *            the node; the LM score is unchanged.
 *   space    extending p by the space exists only if w = lex_word[node(p)] is in [0, n_vocab) (no leading space, no double space):
 *            LM score += alpha * ln P(w | w2, w1) + beta, the node returns to the root, the context becomes (w1, w).
 *   end      after the last frame an entry is COMPLETE if it sits at the root or on a node with a word; in the second case the last word's
 *            alpha * ln P + beta is added to its score (there is no </s> term).  Complete entries rank before incomplete ones, within each
 *            group by score, ties to the lower beam slot.
 * There is no out-of-vocabulary escape: every emitted word is a word of the lexicon.
 * Additional output: complete (n_utt, n_best) int32 = 1 / 0, -1 for a rank that does not exist.
 * workspace: ss_ctc_word_beam_workspace_bytes(n_utt, total_frames, W) bytes; -1 = bad arguments. */
int64_t ss_ctc_word_beam_workspace_bytes(int n_utt, int64_t total_frames, int beam_width);
int ss_ctc_word_beam_search(const float* logits, int64_t ld, int V, int blank, int space, int64_t rows, const float* lse, const int64_t* utt_dev,
                            int n_utt, int64_t total_frames, int beam_width, int n_best, const ss_word_lm* lm, float alpha, float beta,
                            void* workspace, int max_len, int32_t* labels, int32_t* lengths, float* scores, float* ctc_scores,
                            int32_t* complete, void* stream);
/* out[i] = ln P(w | w2, w1) of triples[i] = (w2, w1, w) (device, int32 x3) by the device function the search uses; an id outside the tables
 * (w not in [0, n_uni), w1 / w2 not in [-1, n_uni)) gives NaN. */
int ss_word_ngram_score(const ss_word_lm* lm, const int32_t* triples, int64_t n, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Word language model of ANY order 1 .. 6 as context states (what KenLM calls a state): a backoff n-gram over words and the trie of their
 * spellings, all arrays on the device, natural-log f32.  Word ids as in ss_word_lm (n_uni of them, the start context <s> among them, below 2^21).
 * A STATE is a word context the model knows: state 0 = the empty context, state 1 + w = the context (w), further ids = every n-gram of
 * 2 .. order - 1 words, numbered by increasing length.  A beam entry holds one state id whatever the order.
 *   lex_child / lex_word   as in ss_word_lm.
 *   uni_logp (n_uni)       ln P(w): the arcs out of state 0; their next state is 1 + w.
 *   st_bo (n_states)       backoff weight of the state's context (st_bo[0] = 0).
 *   st_shorter (n_states)  int32: the state of the longest proper suffix of the context that is a state (levels may be skipped); the builder
 *                          guarantees st_shorter[s] < s, the kernels do not rely on it.
 *   arc_*                  ONE open-addressing hash table for the n-grams of 2 .. order words: 64-bit key (state of the context << 21 | word), an
 *                          all-ones key = empty slot, slot count a power of two (or 0: a unigram model), home slot = splitmix64 finaliser of
 *                          key + 0x9E3779B97F4A7C15, & (slots - 1), linear probing that wraps around; arc_probe = the longest probe sequence
 *                          the builder needed (<= arc_slots), the lookup's loop bound.  Beside the keys: arc_logp = ln P(word | context) and
 *                          arc_next int32 = the state of the longest suffix of context + word that is a state.
 * ln P(w | s) and the state after w: walk s_0 = s, s_{i+1} = st_shorter[s_i] while s_i != 0, AT MOST order - 1 steps; the first s_i with an
 * arc for w gives p and next; without one p = uni_logp[w], next = 1 + w; the value is st_bo[s_0] + (st_bo[s_1] + ... + (st_bo[s_{i-1}] + p)),
 * summed from the lowest order outward -- for a model of order <= 3 the same f32 number as the rule of ss_word_lm.
 * Every index formed from these tables is checked against the sizes given here (a state, next or shorter outside [0, n_states) counts as state
 * 0), and no loop is bounded by table contents: a malformed table gives wrong words, never a read outside the arrays or an unbounded loop.
 * Not here: the KenLM binary format, parity with ctcdecode's own numbers, an out-of-vocabulary escape. */
typedef struct ss_word_state_lm {
    const int32_t* lex_child;
    const int32_t* lex_word;
    const float* uni_logp;
    const float* st_bo;
    const int32_t* st_shorter;
    const uint64_t* arc_keys;
    const float* arc_logp;
    const int32_t* arc_next;
    int32_t n_nodes, n_vocab, n_uni, n_states;
    int32_t start_state, arc_slots, arc_probe, order;
} ss_word_state_lm;

/* ss_ctc_word_beam_search with the word model as context states (csrc/ctc_word_state_decode.hip): the same search, rules, ranking and outputs;
 * an entry carries the state before the word it is spelling instead of (w2, w1).  start: the root and start_state.  Where an extension
 * creates an entry whose node spells a word w, ONE lookup (state, w) gives alpha * ln P(w | state) + beta and the state after w; the space
 * extension adds the former and moves to the latter.  1 <= order <= 6, n_states >= 1 + n_uni, start_state in [0, n_states).
 * workspace: ss_ctc_word_state_beam_workspace_bytes(n_utt, total_frames, W) bytes; -1 = bad arguments. */
int64_t ss_ctc_word_state_beam_workspace_bytes(int n_utt, int64_t total_frames, int beam_width);
int ss_ctc_word_state_beam_search(const float* logits, int64_t ld, int V, int blank, int space, int64_t rows, const float* lse, const int64_t* utt_dev,
                                  int n_utt, int64_t total_frames, int beam_width, int n_best, const ss_word_state_lm* lm, float alpha, float beta,
                                  void* workspace, int max_len, int32_t* labels, int32_t* lengths, float* scores, float* ctc_scores,
                                  int32_t* complete, void* stream);
/* out_lnp[i] = ln P(word | state), out_next[i] = the state after it, of pairs[i] = (state, word) (device, int32 x2) by the device function
 * the search uses; a state outside [0, n_states) or a word outside [0, n_uni) gives NaN and -1. */
int ss_word_state_score(const ss_word_state_lm* lm, const int32_t* pairs, int64_t n, float* out_lnp, int32_t* out_next, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Forced alignment: the best (Viterbi) alignment of a KNOWN label string to the frame posteriors, the whole batch in one launch
 * (csrc/ctc_align.hip; what torchaudio.functional.forced_align computes for one utterance).
 * Inputs: f32 logits (rows, ld), classes in columns 0 .. V-1 (V <= 4096, ld >= V, further columns are never read); lse = per-frame log-sum-exp
 * (ss_frame_lse with col0 = 0); utt_dev (device, int64 x4 per utterance) = first frame, frames T, first target index, target length S -- the
 * packed layout and the slot layout of ss_plan_forward_ragged alike; frames behind an utterance's end and rows between utterances are never
 * read.  targets: flat int32, n_targets of them; y = the S labels of the utterance.  total_frames >= the sum of the frames (it sizes the
 * workspace; an utterance that would exceed it, or leave [0, rows), is cut short, never read out of bounds).  S <= max_target_len <= 511.
 * Definition: logp_t(c) = logit_t(c) - lse_t, natural log, f32.
 *   CTC topology (blank in [0, V)): extended states s = 0 .. 2S, even = blank, odd s = token (s-1)/2.  d_0(0) = logp_0(blank), d_0(1) =
 *     logp_0(y_0), every other state -inf.  d_t(s) = best + logp_t(label(s)), best over d_{t-1}(s), d_{t-1}(s-1) and -- only if s is a token
 *     state and its label differs from the previous token's -- d_{t-1}(s-2).  A predecessor of -inf is no candidate; if none exists,
 *     d_t(s) = -inf.  The sum is ONE f32 addition best + (logit - lse) per step (no rescaling, no reassociation), so an f32 restatement
 *     reproduces the score.  score = max(d_{T-1}(2S-1), d_{T-1}(2S)).
 *   ties: among equal predecessors the smallest jump wins (stay, then s-1, then s-2); at the end d_{T-1}(2S-1) wins over an equal d_{T-1}(2S).
 *   linear topology (blank = -1, heads without a blank class): the states are the S tokens, predecessors s and s-1, start in token 0, end in
 *     token S-1, same tie rule.
 *   T = 0 and S = 0: score 0.  S = 0, T > 0: all blank under CTC, -inf under linear.  No alignment (too few frames, repeats without room for
 *     their blanks): -inf.  A label outside [0, V) or equal to the blank, or a table entry whose targets leave [0, n_targets) or exceed
 *     max_target_len: -inf, and nothing is indexed out of bounds.  A score that is not > -inf (NaN logits) is reported as -inf.
 * Outputs: score (n_utt) f32; frame_token (rows) int32 = token index within the utterance's target, -1 blank, -2 for rows of no utterance and
 * for every frame of an utterance of score -inf; parallel to targets: token_first (frame relative to the utterance's first), token_frames,
 * token_logp (f32 sum of logp over the token's frames, ascending) -- -1 / 0 / 0 for score -inf; entries of no utterance are not written.
 * workspace: ss_ctc_align_workspace_bytes(n_utt, total_frames, max_target_len) bytes (2-bit back-pointers, 256 bytes per frame; needs no
 * initialisation); -1 = bad arguments. */
int64_t ss_ctc_align_workspace_bytes(int n_utt, int64_t total_frames, int max_target_len);
int ss_ctc_align(const float* logits, int64_t ld, int V, int blank, int64_t rows, const float* lse, const int64_t* utt_dev, int n_utt,
                 int64_t total_frames, int max_target_len, const int32_t* targets, int64_t n_targets, void* workspace, float* score,
                 int32_t* frame_token, int32_t* token_first, int32_t* token_frames, float* token_logp, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Scoring transcripts: the Levenshtein distance of token strings with its error breakdown and alignment, a batch of pairs in one launch, and the
 * minimum-Bayes-risk pass over n-best lists (csrc/edit_distance.hip; what jiwer / rapidfuzz compute for one pair on the host).
 * Inputs: tokens (n_tokens) int32, flat; seqs (device, int64 x2 per sequence) = first token, length; pairs (device, int32 x2 per pair) =
 * reference sequence a, hypothesis sequence b.  Tokens are compared by ==.  A sequence has at most 1023 tokens.
 * Definition: D[0][j] = j, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (a[i-1] != b[j-1]), D[i-1][j] + 1, D[i][j-1] + 1), distance = D[n_a][n_b].
 *   ties: the predecessor of a cell is the FIRST of {diagonal, up (a reference token is deleted), left (a hypothesis token is inserted)} that
 *     attains the minimum; in row 0 it is left, in column 0 up.  (hits, substitutions, deletions, insertions) are the counts of the path these
 *     predecessors define from (n_a, n_b) back to (0, 0): hits + S + D = n_a, hits + S + I = n_b, S + D + I = distance.  The kernel carries the
 *     counts forward with the distance -- the chosen predecessor is the same cell either way -- so the counts need no backtrace.
 *   Parity with the tie choice of jiwer / rapidfuzz (which of several alignments of least cost they report) is UNPINNED, as parity with ctcdecode
 *     is: neither is available to compare against.  The distance itself, and with it WER / CER, does not depend on the ties.
 * Outputs: dist (n_pairs) int32; counts (n_pairs, 4) int32 = hits, substitutions, deletions, insertions.
 * Alignment (ops_first != NULL): ops_first (device, n_pairs + 1 int64, non-decreasing) gives pair p the bytes [ops_first[p], ops_first[p + 1]) of
 *   ops (n_ops int8), at least n_a + n_b of them: one byte per step of the path FROM THE BEGINNING, 0 hit, 1 substitution, 2 deletion, 3
 *   insertion, then -1 to the end of the pair's bytes; bytes of no pair are not written.  workspace: ss_edit_distance_workspace_bytes(n_pairs,
 *   n_ops) bytes (2-bit back-pointers; needs no initialisation); -1 = bad arguments.  ops_first = NULL: distance and counts only, no workspace.
 * Bad table entries are cut short, never read out of bounds: a pair with a sequence index outside [0, n_seq), a negative length, a length above
 *   1023, a span that leaves [0, n_tokens), or (alignment) bytes that leave [0, n_ops) or are fewer than n_a + n_b gets dist = -1, counts = -1
 *   and -1 in whatever of its ops bytes lie inside ops; every other pair is unaffected.  n_pairs = 0 launches nothing. */
int64_t ss_edit_distance_workspace_bytes(int64_t n_pairs, int64_t n_ops);
int ss_edit_distance(const int32_t* tokens, int64_t n_tokens, const int64_t* seqs, int64_t n_seq, const int32_t* pairs, int64_t n_pairs,
                     int32_t* dist, int32_t* counts, int8_t* ops, const int64_t* ops_first, int64_t n_ops, void* workspace, void* stream);
/* Minimum-Bayes-risk selection from n-best lists, two launches.  tokens, seqs as above; groups (device, int64 x2 per group) = first sequence, K:
 * the 1 <= K <= max_k <= 128 consecutive sequences of one list in rank order (groups should not share sequences); weights (n_seq) f32, the
 * posterior of every sequence within its list.
 * dmat (n_dmat int32): group g's K x K matrix of distances (the definition above; symmetric, every unordered pair computed once, diagonal 0),
 *   row-major at the sum of K_h^2 over h < g.  risk (n_seq) f64, parallel to weights: risk[first + i] = sum_k weights[first + k] * dmat[i][k],
 *   accumulated in f64 in ascending k (an f32 times an integer below 2^11 is exact in f64, so the value depends on the order alone).
 *   pick (n_groups) int32 = the smallest i of least risk.
 * Bad table entries: a K outside 1 .. 128 takes no room in dmat and gives pick -1; a group whose sequences leave [0, n_seq) or whose matrix
 *   leaves [0, n_dmat), a bad sequence in a group (its row and column of dmat are -1) or a NaN risk give pick -1 and NaN risks for the
 *   sequences of the group that exist.  Entries of risk outside every group are not written.  n_groups = 0 launches nothing. */
int ss_nbest_risk(const int32_t* tokens, int64_t n_tokens, const int64_t* seqs, int64_t n_seq, const int64_t* groups, int n_groups, int max_k,
                  const float* weights, int32_t* dmat, int64_t n_dmat, double* risk, int32_t* pick, void* stream);

/* ---------------------------------------------------------------------------------------------
 * n-best lists as a training criterion (csrc/ctc.hip): the full-sum CTC log-likelihood of SEVERAL label strings per utterance with its
 * gradient, and the expected risk of the lists under their own posterior (minimum expected word error, MWER).
 * Notation: utterance u has the frames [f0_u, f0_u + T_u) of the packed (rows, ld) f32 logits, p_t(c) = softmax(logit_t)[c] over the V classes
 *   (lse as for ss_ctc_loss), and a list of K_u >= 0 hypotheses; a hypothesis is a string of S <= 511 class numbers, never the blank.
 * Tables: utt (device, int64 x4 per utterance) = first frame, frames, first hypothesis, K (utterances do not share frames; the hypotheses of a
 *   list are consecutive); hyp (device, int64 x3 per hypothesis) = first label in targets, S, offset (floats) of the hypothesis' T_u (2 S + 1)
 *   block in the alpha and the beta workspace (blocks do not overlap).
 * ss_ctc_nbest_logp: logp[h] = ln sum_{alignments of h} prod_t p_t(.), f32 natural log: exactly -nll of ss_ctc_loss's alpha / beta kernel, which
 *   runs unchanged (for a list of one hypothesis that is the reference the bits equal -nll); -inf where no alignment exists (T < S + repeats,
 *   T = 0 < S).  max_target_len >= the longest hypothesis (it sizes the launch: 2 max_target_len + 1 <= 1024 states, LDS as for ss_ctc_loss).
 *   workspace: ss_ctc_nbest_workspace_bytes(n_hyp, ws_floats) bytes, ws_floats = the sum of the blocks; needs no initialisation and is what
 *   ss_ctc_nbest_backward reads (descriptors, alpha, beta); -1 = bad arguments.
 *   Bad table entries are cut short on the device, never followed: a hypothesis that belongs to no list, whose utterance leaves [0, rows), whose
 *   labels leave targets[0, n_targets) or are no class or the blank, that is longer than max_target_len or whose block leaves the workspace
 *   gets logp = -inf and touches nothing; every other hypothesis is unaffected.  n_hyp = 0 launches nothing.
 * ss_ctc_nbest_backward: for a cotangent g[h] per hypothesis the complete rows x ld gradient
 *     dlogits[t][c] = sum_{h in list(u), logp_h finite} g_h (occ_h[t][c] - p_t(c)),
 *   occ_h[t][c] = sum_{s: ext_label_h(s) = c} alpha_t(s) beta_t(s) / (p_t(c) P_h), the posterior that h emits class c at frame t.  A hypothesis
 *   with logp = -inf contributes nothing whatever its g (no NaN, unlike ss_ctc_loss).  EVERY frame is written: frames outside every utterance,
 *   frames of an utterance with K_u = 0 and the columns c >= V get 0 (the logits of such frames are not read).  The hypotheses of a frame are
 *   accumulated in ascending list order by one wave; no float atomics on global memory.  The same tables, targets, workspace and logp as the
 *   forward call; whatever the tables hold, nothing outside the workspace, targets and the rows is touched.
 * ss_nbest_expected_risk: groups (device, int64 x2 per list) = first hypothesis, 0 <= K <= 128.  With all sums over the entries of FINITE logp,
 *   in f64 and ascending order:  post_k = softmax_k(scale logp_k),  e_u = mean_k cost_k,  risk_u = sum_k post_k (cost_k - e_u),
 *   loss[0] = mean of risk_u over the n_used lists that have a finite entry (0 if there is none), and
 *     dlogp[k] = d loss / d logp_k = scale post_k (cost_k - e_u - risk_u) / n_used.
 *   Outputs: loss (f32), risk (n_groups, f64), post and dlogp (n_hyp, f32 roundings of the f64 values); entries of non-finite logp, of no list
 *   or of a refused list get post = dlogp = 0.  A list without a finite entry (K = 0 included) has no posterior: risk NaN, not part of the mean.
 *   Bad table entries: a K outside 0 .. 128 or a list that leaves [0, n_hyp) gives risk NaN and zero cotangents for that list; the other lists
 *   are unaffected.  Costs are finite.  One launch (one workgroup, a wave per list at a time). */
int64_t ss_ctc_nbest_workspace_bytes(int64_t n_hyp, int64_t ws_floats);
int ss_ctc_nbest_logp(const float* logits, int64_t ld, int V, int blank, int64_t rows, const float* lse, const int64_t* utt_dev, int n_utt,
                      const int64_t* hyp_dev, int64_t n_hyp, int max_target_len, const int32_t* targets, int64_t n_targets, void* workspace,
                      int64_t ws_floats, float* logp, void* stream);
int ss_ctc_nbest_backward(const float* logits, int64_t ld, int V, int blank, int64_t rows, const float* lse, const int64_t* utt_dev, int n_utt,
                          int64_t n_hyp, const int32_t* targets, const void* workspace, int64_t ws_floats, const float* logp, const float* g,
                          float* dlogits, void* stream);
int ss_nbest_expected_risk(const float* logp, const float* cost, int64_t n_hyp, const int64_t* groups, int n_groups, double scale, float* loss,
                           double* risk, float* post, float* dlogp, void* stream);

/* AdamW over a flat f32 arena (transduction_model.py:178,210).  step is 1-based. */
int ss_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int step, float grad_scale, void* stream);
int ss_cast_f32(const float* in, void* out, int out_dtype, int64_t n, void* stream);
/* Input conditioning of the dataset on the device ("next" row N3): out = limit * tanh(((x - mean[c]) / std[c]) / pre_div / limit)
 * with mean/std optional (both NULL = no affine; C = row length they index) and limit <= 0 = no clipping.
 * raw EMG: pre_div 20, limit 50 (read_emg.py:227-228); EMG features: FeatureNormalizer + limit 8 (read_emg.py:231-233);
 * mel targets: FeatureNormalizer only (read_emg.py:231).  In place is allowed. */
int ss_soft_clip(const float* x, float* out, int64_t n, int C, const float* mean, const float* stdv, float pre_div, float limit, void* stream);

/* combine_fixed_length (data_utils.py:158-167; call sites transduction_model.py:200-202) as ONE gather: concatenates n device
 * blobs and zero-fills the tail of `out` (total_bytes).  table_dev = n source pointers followed by n + 1 cumulative byte offsets
 * (int64 each, device memory); granule (16, 8, 4 or 1) must divide every offset, pointer and total_bytes. */
int ss_concat_pad(const void* table_dev, int n, void* out, int64_t total_bytes, int granule, void* stream);

/* mel target extraction (data_utils.py:39-62): reflect pad (:51); the STFT itself is ss_gemm against a
 * windowed DFT matrix with overlapping hop-strided rows; magnitude (:57); mel matmul + log clamp (:59-60)
 * is ss_gemm with epilogue.log_clamp. */
/* data_utils.py:76 np.clip + :51 reflect pad for EVERY utterance of a ragged batch in one launch: utterance b is
 * y[offsets_dev[b] .. + lengths_dev[b]); row b of out[B][ld_out] gets its clipped (clip != 0), reflect-padded signal and zeros
 * behind it.  min_len = the shortest length (host-known; reflect needs pad < length).  A (B, L) matrix is offsets b * row stride. */
int ss_reflect_pad_ragged(const float* y, const int64_t* offsets_dev, const int32_t* lengths_dev, float* out, int B, int min_len,
                          int pad, int64_t ld_out, int clip, void* stream);
int ss_stft_magnitude(const float* spec, int64_t ld_spec, int n_bins, float* mag, int64_t ld_mag, int rows, void* stream);
/* The whole of data_utils.py:51-60 (and :76's np.clip when clip != 0) for n_fft = 1024 as ONE kernel (csrc/mel.hip: an LDS radix-8 FFT per frame, one
 * wave per frame), reading the caller's signals in place: signal b is y[offsets_dev[b] .. + lengths_dev[b]) (a ragged batch) or, with both arrays NULL,
 * row b of a [B][uniform_len] matrix.  Frame f (< F) of a signal covers its reflect-padded samples f * hop - pad .. + 1024 (F.pad(..., 'reflect'), :51;
 * pad < length; samples behind the padded signal count as 0, as in the zero-filled rows of ss_reflect_pad_ragged), windowed by window[1024]
 * (torch.hann_window, :49), one-sided spectrum, sqrt(re^2 + im^2 + 1e-9) (:57), the mel filterbank (:59) in SPARSE form -- band m = sum_j
 * band_w[band_off[m] + j] * mag[band_lo[m] + j], j < band_cnt[m]: the non-zero run of row m of librosa.filters.mel, padded with zero weights to a
 * multiple of 4 (band_lo[m] + band_cnt[m] <= 520), n_w packed weights in all; lane_bands[2][64] deals the bands to the 64 lanes (-1 = none) --,
 * log(clamp(., log_clamp)) (:60, spectral_normalize_torch) written to out[b * stride_b + f * stride_f + m * stride_m].  n_mels <= 128, n_w <= 4096. */
int ss_stft_logmel_fft(const float* y, const int64_t* offsets_dev, const int32_t* lengths_dev, int64_t uniform_len, int B, int F, int pad, int clip,
                       int n_fft, int hop, const float* window,
                       const int32_t* band_lo, const int32_t* band_cnt, const int32_t* band_off, const float* band_w, const int32_t* lane_bands, int n_mels, int n_w,
                       float log_clamp, float* out, int64_t stride_b, int64_t stride_f, int64_t stride_m, void* stream);
/* The gradient of ss_stft_logmel_fft with respect to the signals (csrc/mel_bwd.hip): g_y, laid out like y (every sample of every signal is written; with
 * clip != 0 samples with |y| > 1 get 0), from the upstream gradient g_out[b * stride_b + f * stride_f + m * stride_m] (any strides; rows f >= a ragged
 * signal's own frame count are filler and are not read).  The arguments up to n_w are the forward's; max_len = the longest signal (uniform_len for rows;
 * host-known); hop a multiple of 4.  The transposed filterbank comes per bin: bin_band[513] = m0 | m1 << 8, the (at most two) bands with a non-zero
 * weight over the bin, 255 = none, and bin_w[513][2] their weights; bin_taps = the largest number of bands over one bin (<= 2, checked).  One wave per
 * frame recomputes the spectrum and writes the windowed frame gradient into workspace[B * F][1024] f32 (ss_stft_logmel_fft_backward_workspace_bytes);
 * a second kernel sums, per sample, the frames that cover it and its reflections in a fixed order: no floating-point atomics, bitwise reproducible. */
int64_t ss_stft_logmel_fft_backward_workspace_bytes(int B, int F); /* [host] */
int ss_stft_logmel_fft_backward(const float* y, const int64_t* offsets_dev, const int32_t* lengths_dev, int64_t uniform_len, int64_t max_len, int B, int F, int pad,
                                int clip, int n_fft, int hop, const float* window,
                                const int32_t* band_lo, const int32_t* band_cnt, const int32_t* band_off, const float* band_w, const int32_t* lane_bands, int n_mels,
                                int n_w, const int32_t* bin_band, const float* bin_w, int bin_taps, float log_clamp,
                                const float* g_out, int64_t stride_b, int64_t stride_f, int64_t stride_m, float* workspace, int64_t workspace_bytes, float* g_y,
                                void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-head self-attention with learned relative-position logits (transformer.py:87-112 and
 * :162-297; closed form in csrc/attention.hip), fused: QK^T, Q.E^T (banded, |k-q| <= D-1, -1e8
 * outside), softmax, dropout (transformer.py:109), P.V.  Operands (compute dtype):
 *   qkv  [B*T][3*H*dp] (q|k|v, head, d) with the head dim zero-padded to dp (multiple of 32, <=128);
 *   qkvT [B][3*H*dp][Tp] the same transposed per sequence (2nd output of the QKV ss_gemm);
 *   E    [H][2D-1][dp];  ET [H][dp][MPt], MPt = roundup(2D-1, 32)  (ss_permute3d of the embeddings);
 *   out  [B*T][H*dp];  lse [B][H][T] f32 (saved for backward).  scale = 1/sqrt(d_qkv) (unpadded).
 * backward (transduction_model.py:209): dqkv [B*T][3*H*dp] = (dQ|dK|dV); dO/dOT like out / its
 * transposed copy [B][H*dp][Tp]; Dscratch [B][H][T] f32.  The embeddings receive no gradient
 * (transformer.py:214-218). */
/* 1 if (dtype, T, dp, D) runs the per-tile attention kernels, which read the per-sequence transposed copies qkvT / dOT;
 * 0 exactly when the transposed-score kernels run (family 2 below): then qkvT and dOT may be NULL and the producing GEMMs
 * need not emit them. */
int ss_relpos_attention_needs_transposed(int dtype, int T, int dp, int D); /* [host] */
/* Which kernels (dtype, T, dp, D) runs: 0 = per-tile (qkvT / dOT needed), 2 = transposed 32 x 32 score tiles (bf16, T <= 224:
 * csrc/attention_t.hip).  1 was the LDS-resident 16 x 16 family of rounds 1-4: retired, never returned, the number is not reused.
 * Family 2 reads the embeddings from a prepared table instead of E / ET:
 * ss_relpos_attention_table_bytes() bytes, filled by ss_relpos_attention_prepare_tables from the f32 parameter
 * (transformer.py:172-176 `embeddings`, [H][2D-1][dh] contiguous; scale = 1/sqrt(d_qkv) as in the calls below) -- E / scale in
 * MFMA-fragment order, so that Q.E accumulates in the same accumulator as Q.K and the table streams from L2 as whole KiB.
 * `tab` may be NULL for family 0; E / ET / qkvT / dOT may be NULL for family 2. */
int ss_relpos_attention_family(int dtype, int T, int dp, int D); /* [host] */
int64_t ss_relpos_attention_table_bytes(int H, int dp, int D); /* [host] */
int ss_relpos_attention_prepare_tables(const float* emb, void* tab, int H, int D, int dh, int dp, float scale, void* stream);
int ss_relpos_attention_forward(int dtype, const void* qkv, const void* qkvT, const void* E, const void* tab, void* out, float* lse,
                                int B, int H, int T, int Tp, int dp, int D, float scale, float dropout_p, uint64_t seed,
                                uint32_t rng_stream, void* stream);
int ss_relpos_attention_backward(int dtype, const void* qkv, const void* qkvT, const void* E, const void* ET, const void* tab, const void* out,
                                 const float* lse, const void* dO, const void* dOT, float* Dscratch, void* dqkv,
                                 int B, int H, int T, int Tp, int dp, int D, float scale, float dropout_p, uint64_t seed,
                                 uint32_t rng_stream, void* stream);

/* The same with SAVED PROBABILITIES: the family-2 forward leaves its normalised probabilities (bf16, 32 x 32 blocks, dropout
 * decision in the sign bit; csrc/attention_t.hip "the P image") in `pimg`, ss_relpos_attention_saved_bytes() bytes; its backward
 * reads them instead of recomputing both logit products, the skew, the exponentials and the dropout draws, and works ONLY from them
 * (the forward may still run without pimg: inference).  saved_bytes is 0 for shapes that run the per-tile kernels, which save
 * nothing: there pimg must be NULL in both calls (= the functions above). */
int64_t ss_relpos_attention_saved_bytes(int dtype, int B, int H, int T, int dp, int D); /* [host] */
int ss_relpos_attention_forward_p(int dtype, const void* qkv, const void* qkvT, const void* E, const void* tab, void* out, float* lse, void* pimg,
                                  int B, int H, int T, int Tp, int dp, int D, float scale, float dropout_p, uint64_t seed,
                                  uint32_t rng_stream, void* stream);
int ss_relpos_attention_backward_p(int dtype, const void* qkv, const void* qkvT, const void* E, const void* ET, const void* tab, const void* out,
                                   const float* lse, const void* dO, const void* dOT, float* Dscratch, void* dqkv, const void* pimg,
                                   int B, int H, int T, int Tp, int dp, int D, float scale, float dropout_p, uint64_t seed,
                                   uint32_t rng_stream, void* stream);

/* Inference forward of a RAGGED batch in equal slots (per-tile kernels, any T; dtype SS_F32, SS_F32X3 or SS_BF16): sequence b holds
 * lens_dev[b] <= T frames at the start of its slot of T rows (qkv, out) / Tp columns (qkvT).  The slot length only addresses the operands;
 * the sequence length bounds everything else: queries of sequence b see keys k < lens_dev[b] (inside the band rule above), V^T fragments and
 * K rows behind it are zeroed by select, and 16-row query tiles that start at or behind it leave before their first load (the launch covers
 * the slots; lengths stay on the device).  Rows >= lens_dev[b] of `out` are not written.  No dropout, no lse: there is no backward.
 * Rows t < lens_dev[b] equal what ss_relpos_attention_forward gives for sequence b alone (B = 1, T = lens_dev[b]). */
int ss_relpos_attention_forward_ragged(int dtype, const void* qkv, const void* qkvT, const void* E, void* out, const int32_t* lens_dev,
                                       int B, int H, int T, int Tp, int dp, int D, float scale, void* stream);

/* The parity-grade mode of the attention (round 6): f32 operands as hi / lo bf16 planes (ss_split_planes), every product of the kernels above
 * on three bf16 MFMAs (a_lo.b_hi + a_hi.b_lo + a_hi.b_hi, f32 accumulate) -- the transposed-score kernels' formulation, so bf16 rows of up to
 * 224 frames, d_head <= 96 (ss_relpos_attention_x3_supported; other shapes keep SS_F32X3 of the entry points above).  qkv / dO arrive as
 * plane pairs, out / dqkv LEAVE as plane pairs (their consumers are ss_gemm_planes / the grouped weight-gradient jobs); the table holds E / scale
 * as [hi | lo] (ss_relpos_attention_x3_prepare_tables, ss_relpos_attention_x3_table_bytes), the saved probabilities two images [hi | lo]
 * (ss_relpos_attention_x3_saved_bytes; required by the backward).  Dropout masks are those of kernel family 2.
 * Replaces the f32 arithmetic of transformer.py:87-112, :229-297 and its autograd backward. */
int ss_relpos_attention_x3_supported(int T, int dp, int D);                               /* [host] */
int64_t ss_relpos_attention_x3_saved_bytes(int B, int H, int T, int dp, int D);           /* [host] */
int64_t ss_relpos_attention_x3_table_bytes(int H, int dp, int D);                         /* [host] */
int ss_relpos_attention_x3_prepare_tables(const float* emb, void* tab, int H, int D, int dh, int dp, float scale, void* stream);
int ss_relpos_attention_x3_forward(const void* qkv_hi, const void* qkv_lo, const void* tab, void* out_hi, void* out_lo, float* lse, void* pimg,
                                   int B, int H, int T, int dp, int D, float scale, float dropout_p, uint64_t seed, uint32_t rng_stream, void* stream);
int ss_relpos_attention_x3_backward(const void* qkv_hi, const void* qkv_lo, const void* tab, const void* out_hi, const void* out_lo, const void* dO_hi, const void* dO_lo,
                                    float* Dscratch, void* dqkv_hi, void* dqkv_lo, const void* pimg,
                                    int B, int H, int T, int dp, int D, float scale, float dropout_p, uint64_t seed, uint32_t rng_stream, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Offline EMG conditioning ("next" row N4): the zero-phase IIR cascade of read_emg.py:27-38 (7 x filtfilt(iirnotch(60 h, 30)) then
 * filtfilt(butter(3, 2 Hz, 'highpass')), scipy.signal.filtfilt defaults: odd extension of 3 max(len a, len b) samples, lfilter_zi
 * initial conditions) and the np.interp resampling of read_emg.py:40-44, in f64 like numpy, for a RAGGED BATCH of R >= 1 recordings
 * (one launch sequence for all of them; a single recording is R = 1).  x / y are the recordings back to back, each (T_u, C) f64
 * time-major, packed (sum T_u, C); lengths_host = the R lengths (host memory, like coef).  Work items are (chunk, channel) pairs
 * over all recordings.
 * coef [host]: per filter 13 doubles { b[4], a[4] (a[0] = 1, zero padded), zi[3] (scipy.signal.lfilter_zi), order n, padlen }. */
int64_t ss_iir_filtfilt_batch_workspace_bytes(const int32_t* lengths_host, int R, int C, int max_padlen, int n_filt); /* [host] */
int ss_iir_filtfilt_batch(const double* x, double* y, const int32_t* lengths_host, int R, int C, int n_filt, const double* coef,
                          void* workspace, int64_t workspace_bytes, void* stream);
/* y[i] = np.interp(i / new_freq, arange(T) / old_freq, x[:, c]) for i < T_out, every recording onto its own grid; table_dev: int64 [R][4] =
 * {first input row, T, first output row, T_out} (the caller sizes T_out = len(arange(0, (T-1)/old_freq, 1/new_freq))). */
int ss_linear_resample_batch(const double* x, double* y, const int64_t* table_dev, int R, int C, double old_freq, double new_freq,
                             int64_t total_out_rows, void* stream);
/* The 14 hand-crafted features per channel of data_utils.get_emg_features (data_utils.py:85-136) for a RAGGED BATCH in one launch: x packed
 * (sum n_u, C) f64 at 516.79 Hz (what ss_linear_resample_batch wrote), out packed (total_frames, 14 C) f32, column c * 14 + j = {mean(w),
 * rms(w), rms(|p|), zero-crossing rate of p, mean(|p|), |rfft(hann16 * xs)| bins 0..8} of the frames [6 f, 6 f + 16), where xs = x - its
 * column mean, w = the 9-tap box filter applied twice ('same', each pass zero-padding its own input) and p = xs - w; f64 arithmetic, f32
 * store.  table_dev: int64 [R][4] = {first input row, n, first output row, F = n < 16 ? 0 : 1 + (n - 16) / 6}.  1 <= C <= 32. */
int ss_emg_features_batch(const double* x, float* out, const int64_t* table_dev, int R, int C, int64_t total_frames, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stored audio (csrc/audio.hip, ABI 15): the resample and the volume levelling of the reference's load_audio (data_utils.py:64-83, :19-27) for a
 * RAGGED BATCH -- all utterances back to back in one flat f32 buffer -- in one launch each.
 *
 * ss_audio_resample_batch is scipy.signal.resample_poly(x, up, down) with its defaults for every utterance: with half = 10 max(up, down) and
 * h = firwin(2 half + 1, 1 / max(up, down), window = ('kaiser', 5.0)) * up,  y[m] = sum_j x[j] h[m down + half - j up]  over the j inside the utterance
 * with 0 <= m down + half - j up <= 2 half, n_out = ceil(n up / down) outputs.  The caller designs h (in f64) and hands it over phase-major in f32:
 * coef_dev [up][taps_per_phase], coef[ph][i] = h[ph + i up] (0 past the end of h), taps_per_phase a multiple of 4 that holds 2 half / up + 1 taps,
 * 16-byte aligned, device memory.  table_dev: int64 [R][4] = {first input sample, n, first output sample, n_out} per utterance (device memory; n_out
 * may be smaller than ceil(n up / down): the signal is then cut short; zero-length utterances produce nothing).  An output is the f32 fma chain over
 * its taps in ascending order: it does not depend on the other utterances of the batch nor on how the batch is tiled.  Epilogue: y *= gains_dev[u]
 * (NULL = off; what ss_audio_level_batch wrote, or any per-utterance scale), then the clip to [-1, 1] of load_audio when flags bit 0 is set.
 * flags bit 1 (measurement only): the workgroups read the table through the caches instead of staging it in LDS; same results.
 * up == down == 1, half = 0 with the table {1, 0, 0, 0} is a copy (with the epilogue).
 * Supported (ss_audio_resample_supported() == 1; anything else is an error, there is no fallback): up * taps_per_phase <= table_floats,
 * (tile - 1) * down / up + 1 + taps_per_phase <= span of ss_audio_resample_limits (12288, 2048, 8192) and both together within 64 KB: covers 441/320, 320/441, 147/320, 160/441, 1/2, 2/1. */
int ss_audio_resample_limits(int* tile, int* span, int* table_floats);
int ss_audio_resample_supported(int up, int down, int half, int taps_per_phase);
int ss_audio_resample_batch(const float* x, float* y, const int64_t* table_dev, int R, int up, int down, int half, int taps_per_phase,
                            const float* coef_dev, const float* gains_dev, int flags, int64_t total_out, void* stream);
/* What normalize_volume (data_utils.py:19-27) needs, per utterance: level [R][2] = {max over frames of the frame RMS, max |x|}, with the frames of
 * librosa.feature.rms's defaults (length 2048, hop 512, centred with ZERO padding -- librosa >= 0.10 --, 1 + n / 512 frames), and
 * gains [R] = 0.2 / (max_rms + 0.01), replaced by 1 / max |x| where that gain would leave the peak above 1.  Either output may be NULL.
 * table_dev: int64 [R][3] = {first input sample, n, first 512-sample block = sum over the earlier utterances of ceil(n / 512)}; total_blocks = that
 * sum over all; workspace: 2 * total_blocks floats (the blocks' sums of squares and maxima: every sample is read once).  f32 arithmetic. */
int ss_audio_level_batch(const float* x, const int64_t* table_dev, int R, int64_t total_blocks, float* workspace, int64_t workspace_floats,
                         float* level, float* gains, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stationary spectral gating (csrc/spectral_gate.hip, ABI 16): the noise reduction of the reference's data_collection/clean_audio.py:53,
 * noisereduce 3's stationary gate with its defaults (restated in f64 in tests/spectral_gate_oracle.py), for a RAGGED BATCH in one flat f32 buffer.
 * N = 1024, hop 256, w = periodic Hann(1024), W = sum w; a signal of L >= 1 samples has F = ceil(L / 256) + 1 frames, frame f covers the samples
 * [256 f - 512, 256 f + 512) with zeros outside [0, L).  X = (1 / W) rfft(w frame); d = 20 log10(|X| + 2^-52), clamped from below per frequency row at
 * that row's maximum over the signal's frames - 80; gate = [d > thresh[k]] p + (1 - p); the gate is smoothed by outer(tri(n_f), tri(n_t)) / its sum
 * with zeros outside the 513 x F mask (tri(n)[d] = (n + 1 - |d|) / (n + 1), |d| <= n); y_f = irfft(X gate) W; out = sum_f w y_f / sum_f w^2 over the
 * frames that cover a sample, summed in ascending frame order (no floating-point atomics: a batch gives bit for bit what single calls give).
 * window_dev: 3 x 1024 floats = [w / W | w W / 512 | w^2], designed in f64 and rounded once (data_utils._gate_windows).
 * table_dev: int64 [R][4] = {first sample, L, first frame = sum of the earlier F, F} per signal (device memory); y uses the same sample offsets as x.
 * ss_spectral_gate_profile: thresh[k] = mean_f dc[k, .] + n_std std_f dc[k, .] (population std, dc = the clamped d) of ONE noise clip (table of one
 * row, frames = its F); db_workspace: frames x 513 doubles, rowmax_workspace: 513 dwords.
 * ss_spectral_gate_batch: thresh [513] f32 in dB (+inf closes a row, -inf opens it); 0 <= n_f <= 32, 0 <= n_t <= 8 (ss_spectral_gate_limits;
 * anything else is an error, there is no fallback; n_f = n_t = 0 is "no smoothing"); 0 <= prop_decrease <= 1.  Workspaces: bits_workspace
 * total_frames x 17 dwords (the binary gate, bit k & 31 of dword k >> 5), rowmax_workspace R x 513 dwords, frames_workspace total_frames x 1024 floats
 * (the windowed frames before the overlap-add).  bits_out (NULL = off): total_frames x 17 dwords, the final gate = own bits | rows opened by the clamp. */
int ss_spectral_gate_limits(int* max_n_f, int* max_n_t, int* row_dwords);
int ss_spectral_gate_profile(const float* x, const int64_t* table_dev, int frames, const float* window_dev, double n_std, double* db_workspace,
                             uint32_t* rowmax_workspace, float* thresh, void* stream);
int ss_spectral_gate_batch(const float* x, float* y, const int64_t* table_dev, int R, int64_t total_frames, const float* window_dev, const float* thresh,
                           int n_f, int n_t, double prop_decrease, uint32_t* bits_workspace, uint32_t* rowmax_workspace, float* frames_workspace,
                           uint32_t* bits_out, void* stream);
/* Non-stationary spectral gating (csrc/spectral_gate_ns.hip, ABI 19): noisereduce 3's default mode, restated in f64 in tests/spectral_gate_ns_oracle.py --
 * the threshold comes from the signal itself, no noise clip.  Framing, window_dev, table_dev, the limits of n_f / n_t and the overlap-add are those of
 * ss_spectral_gate_batch.  A = |X|; per frequency row the level S = the one-pole smoother s[f] = b A[f] + (1 - b) s[f - 1] run forward from s[-1] := A[0]
 * and then backward from S[F] := s[F - 1] (scipy.signal.filtfilt([b], [1, b - 1], A, padtype=None)), 0 < b <= 1
 * (b = (sqrt(1 + 4 t^2) - 1) / (2 t^2), t = time constant in frames of 256 samples: data_utils.nonstationary_coefficient);
 * r = (A - S) / S, 0 where S == 0 (digital silence gives a finite mask); m0 = 1 / (1 + exp(-(r - n_mult) slope)), slope > 0, the recurrences, r and the
 * sigmoid in f64, m0 rounded to f32 once; mask = smooth(m0) prop_decrease + (1 - prop_decrease) with outer(tri(n_f), tri(n_t)) / its sum and zeros
 * outside the 513 x F mask, f32 sums in ascending tap order (prop_decrease is applied AFTER the smoothing; in the stationary gate it comes before);
 * y_f = irfft(X mask) W; out as in ss_spectral_gate_batch.  Four launches, no floating-point atomics: a batch gives bit for bit what single calls give.
 * 1 <= R <= 65535.  Workspaces: mag_workspace and level_workspace total_frames x 513 floats each (A, replaced in place by m0; s between the two
 * passes), frames_workspace total_frames x 1024 floats.  mask_out (NULL = off): total_frames x 513 floats, the UNSMOOTHED m0. */
int ss_spectral_gate_ns_batch(const float* x, float* y, const int64_t* table_dev, int R, int64_t total_frames, const float* window_dev, double b,
                              double n_mult, double slope, int n_f, int n_t, double prop_decrease, float* mag_workspace, float* level_workspace,
                              float* frames_workspace, float* mask_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The execution plan of the transduction model as native code: ONE call enqueues the whole forward pass of Model.forward
 * (architecture.py:61-84: shift augmentation, 3 ResBlocks :29-40, w_raw_in, the post-norm relative-position encoder layers
 * transformer.py:43-60,87-112, both heads) and ONE the whole backward pass that loss.backward() (transduction_model.py:209)
 * triggers through autograd -- ~450 kernel launches per training step without a host-language round trip per kernel.
 * The plan owns no memory: device pointers (parameters, the GEMM-ready weight copies, gradient buffers, the job tables of the
 * gradient un-layout launches) are bound to NAMED slots (ss_plan_slot_name lists them; names follow the reference's
 * state_dict keys), activations live in a caller-provided workspace, the saved-for-backward pointers in a caller-kept host
 * struct of ss_plan_ctx_bytes() bytes.  dtype: SS_BF16 (MFMA bf16, f32 accumulate) or SS_F32 (exact f32 MFMA). */
typedef struct ss_model_dims {
    int32_t d_model, n_layers, n_head, d_qkv, dp /* head dim padded to 32 */, max_rel /* relative_positional_distance */, ff;
    int32_t n_head_cols /* num_outs + num_aux_outs rounded up to 8: the fused output heads */, dtype;
    float ln_eps;
} ss_model_dims;
typedef struct ss_plan ss_plan;
/* Data-parallel hook: called between the two phases of every training-mode BatchNorm (forward: n_floats = 2C sums, backward:
 * 3C) with the device pointer of the per-channel sums and the local row count; must all-reduce the sums in place on `stream`
 * and return the GLOBAL row count. */
typedef double (*ss_reduce_hook)(void* user, float* sums_dev, int n_floats, double n_local, void* stream);
/* Called from ss_plan_backward when a group of parameter gradients is final on `stream`: what = 4 + l: encoder layer l (fired
 * layer by layer, last layer first, while the backward of the earlier layers still runs), 0: the fused heads + w_raw_in (after it every
 * non-convolutional gradient is final), 1..3: ResBlock 2, 1, 0.  Lets the caller start a bucketed gradient all-reduce while the
 * rest of backward still runs. */
typedef void (*ss_event_hook)(void* user, int what, void* stream);
ss_plan* ss_plan_create(const ss_model_dims* dims);                 /* [host] NULL on error */
void ss_plan_destroy(ss_plan* plan);                                /* [host] */
int ss_plan_slot_count(const ss_plan* plan);                        /* [host] */
const char* ss_plan_slot_name(const ss_plan* plan, int slot);       /* [host] */
int ss_plan_bind(ss_plan* plan, int slot, void* device_ptr_or_value); /* [host] slots named *.total / *.all_f32 / *.bytes take integers */
int ss_plan_set_option(ss_plan* plan, int what, int value);         /* [host] 0 side stream on/off, 1 grouped dW on/off, 2 side-stream blocks per CU, 3 BatchNorm statistics / bias column sums from GEMM epilogues on/off, 4 BatchNorm backward recomputes the ReLU gate (on) or reads the saved output (off), 5 an SS_F32 plan runs its GEMMs as SS_F32X3 (bf16 x 3 MFMA on f32 operands) on/off (default off = exact f32), 6 the training-mode forward leaves x_raw untouched and only hands the shifted signal out in shifted_scratch (default off = written back in place like architecture.py:67-68), 7 an SS_F32X3 plan runs every GEMM the 8-wave kernel can take on hi / lo bf16 planes (ss_split_planes / ss_gemm_planes; default on), 8 the bound EF tables are the [hi | lo] tables of ss_relpos_attention_x3_prepare_tables: such a plan also runs its attention on planes (default off), 9 plane GEMMs whose consumers take planes (qkv, the FFN hidden activation and its gradient, dO) write them from their epilogue instead of a split pass on first use (default on), 10 a bf16 training plan keeps [FFN hidden > 0] as sign bits (ss_gemm_epilogue.sign_out) and the FFN input gradient gates from them (gate_bits; default on) */
int ss_plan_set_reduce_hook(ss_plan* plan, ss_reduce_hook fn, void* user); /* [host] */
int ss_plan_set_event_hook(ss_plan* plan, ss_event_hook fn, void* user);   /* [host] */
int64_t ss_plan_ctx_bytes(void);                                    /* [host] */
int64_t ss_plan_workspace_bytes(ss_plan* plan, int B, int T0, int training); /* [host] forward (+ backward temporaries if training) */
/* x_raw (B, T0, 8) f32 -> head [B*T0/8][n_head_cols] f32 (pred | aux logits | zero padding).  training: BatchNorm batch statistics
 * and running-stat updates, dropout (counter-based, keyed by seed), the shift augmentation by shift_r samples, whose result is also
 * written back to x_raw (the reference mutates its input, architecture.py:67-68; shifted_scratch: B*T0*8 floats, may be NULL when
 * shift_r == 0).  ctx_out [host, ss_plan_ctx_bytes()] must be kept, with the workspace, until ss_plan_backward has run. */
int ss_plan_forward(ss_plan* plan, const float* x_raw, float* shifted_scratch, void* workspace, int64_t workspace_bytes, int B, int T0,
                    int training, int shift_r, float dropout_p, uint64_t seed, float* head, void* ctx_out, void* stream);
/* Eval-mode forward of a RAGGED batch of whole utterances (evaluate.py's output loop, transduction_model.py:57-66,75-85, recognition_model.py:37-43
 * run one utterance per call): utterance b holds lens_dev[b] >= 1 model frames (8 lens[b] raw samples) at the start of slot b of x_raw (B, T0, 8),
 * zero filled behind them; head rows [b * T0/8, b * T0/8 + lens[b]) equal ss_plan_forward(B = 1, training = 0) of that utterance alone, the other
 * rows of a slot are unspecified.  Same plan, with ss_bn_apply_ragged for every BatchNorm apply and ss_relpos_attention_forward_ragged for the
 * attention (always the per-tile kernels: the QKV GEMM always writes qkvT, planes are never adopted for attention).  No context is kept: there is
 * no backward.  lens_host [host, may be NULL]: the same lengths, read only by the profile rows (attention work counted from the real lengths). */
int64_t ss_plan_workspace_bytes_ragged(ss_plan* plan, int B, int T0); /* [host] */
int ss_plan_forward_ragged(ss_plan* plan, const float* x_raw, const int32_t* lens_dev, const int32_t* lens_host, void* workspace, int64_t workspace_bytes,
                           int B, int T0, float* head, void* stream);
/* Accumulates (+=) the gradient of every bound parameter; dhead [B*T0/8][n_head_cols] f32.  The weight-gradient GEMMs, bias column sums
 * and gradient un-layouts run on side_stream (may equal stream or be NULL), joined into `stream` before the call returns. */
int ss_plan_backward(ss_plan* plan, void* ctx, const float* dhead, void* stream, void* side_stream);
/* Per-launch timing of the plan's kernels (HIP events on the launch stream; use with the side stream switched off so that
 * durations are exclusive).  ss_plan_profile_read synchronises, aggregates the records gathered since the last read by
 * kernel, clears them and returns the number of rows written. */
typedef struct ss_profile_row { char name[64]; int64_t calls; double seconds, flops /* algorithmic */, bytes /* algorithmic HBM traffic */; } ss_profile_row;
int ss_plan_profile(ss_plan* plan, int enable);                                  /* [host] returns the previous setting */
int ss_plan_profile_read(ss_plan* plan, ss_profile_row* rows, int max_rows);      /* [host] */
/* counters[i][0] += delta for n <= 16 device int64 counters (BatchNorm num_batches_tracked, architecture.py:19,21,25) in one launch */
int ss_counters_add(int n, int64_t** counters /* [host] array of device pointers */, int64_t delta, void* stream);

/* ---------------------------------------------------------------------------------------------
 * HiFi-GAN generator (vocoder.py:16-36: Generator(hparams) of the hifi_gan submodule, called on mel.T[None]): predicted mels -> audio
 * for a ragged batch of utterances packed back to back, replacing the cuDNN / MIOpen conv1d, conv_transpose1d, leaky_relu and tanh calls of
 * that module.  Every activation is f32, TIME-MAJOR: a row is one time step with its channels contiguous (torch's x[0, :, t]), utterances
 * back to back.  table_dev: int64 [n_utt][2] = {first mel frame, mel frames} per utterance, ONE table for every layer: a buffer at `scale`
 * samples per mel frame (the product of the upsampling rates applied so far) holds utterance u in rows [first * scale, (first + frames) *
 * scale).  max_frames = the longest utterance's mel frames (sizes the launch).  Every utterance has its own zero padding at both ends, by
 * predication: rows of a neighbour are never read as padding and no padded copy is made.  x3 != 0: operands split into hi + lo bf16
 * planes, three MFMAs per product, f32 accumulate (16-17 significant bits per operand); x3 == 0: one bf16 MFMA per product.
 *
 * Weight blob of one layer (built once at load time by the caller; co_pad = c_out rounded up to 16, ci_pad = c_in rounded up to 32,
 * padding zero):   f32 bias[co_pad] | bf16 hi[slots][co_pad][ci_pad] | bf16 lo[slots][co_pad][ci_pad],   hi = bf16(w), lo = bf16(w - hi).
 *   convolution (torch weight [c_out][c_in][k]):            slots = k,                       slot j         = weight[:, :, j]
 *   transposed convolution (torch weight [c_in][c_out][k]): slots = stride * ceil(k / stride), slot r * ceil(k / stride) + m = weight[:, :, r + m * stride].T
 *                                                           (zero where r + m * stride >= k): the taps of output phase r, polyphase form. */
int64_t ss_voc_blob_bytes(int slots, int c_out, int c_in);          /* [host] bytes of such a blob; -1 on bad sizes */
/* [host] bytes of the generator's activation workspace for total_frames packed mel frames: FOUR equal buffers (this value / 4 each,
 * 256-byte aligned) as wide as the widest layer (conv_pre output at c_initial channels, stage i at c_initial >> (i + 1) channels and
 * rates[0] * .. * rates[i] rows per frame): the stage input, the two ResBlock temporaries and the multi-receptive-field sum. */
int64_t ss_voc_workspace_bytes(int64_t total_frames, int c_initial, const int* rates /* [host] */, int n_ups);
/* [host] 1 if the kernels take the shape.  kind 0: ss_voc_conv1d (c_in % 8 == 0, c_out % 4 == 0, k odd, (k - 1) * dilation <= 128);
 * kind 1: ss_voc_conv_transpose1d (same channel rules, k >= stride, k - stride even); kind 2: ss_voc_tail (c_in <= 64, c_out == 1, k odd <= 15). */
int ss_voc_supported(int c_in, int c_out, int k, int dilation_or_stride, int kind);
/* Fused dilated convolution, one launch (F.leaky_relu + Conv1d(c_in, c_out, k, dilation=d, padding=(k - 1) d / 2) [+ the ResBlock's
 * `xt + x`] [+ the generator's `xs += resblock(x)` and `/ num_kernels`] of hifi_gan's ResBlock1/2.forward and Generator.forward; conv_pre with slope 1):
 *     v = bias[co] + sum_tap sum_ci W[tap][co][ci] * lrelu_slope(x[t + (tap - (k - 1) / 2) d][ci])  + (residual ? residual[t][co] : 0)
 *     out[t][co] = ((accumulate ? out[t][co] : 0) + v) * out_scale
 * x rows have c_in floats, residual / out rows c_out; out must not be x; residual may be out. */
int ss_voc_conv1d(const float* x, const void* blob, const float* residual, float* out, const int64_t* table_dev, int n_utt,
                  int64_t max_frames, int scale, int c_in, int c_out, int k, int dilation, float slope, int accumulate,
                  float out_scale, int x3, void* stream);
/* F.leaky_relu + ConvTranspose1d(c_in, c_out, k, stride, padding=(k - stride) / 2) of Generator.forward, polyphase: out row t (out has
 * scale * stride rows per mel frame) = bias + sum over taps j = (t + p) mod stride, + stride, .. of W[:, :, j] . lrelu(x[(t + p - j) / stride]),
 * p = (k - stride) / 2; no zero-stuffed intermediate exists. */
int ss_voc_conv_transpose1d(const float* x, const void* blob, float* out, const int64_t* table_dev, int n_utt, int64_t max_frames,
                            int scale, int c_in, int c_out, int k, int stride, float slope, int x3, void* stream);
/* The generator's last three calls (F.leaky_relu at torch's default slope 0.01, conv_post = Conv1d(c_in, 1, k, padding (k - 1) / 2),
 * torch.tanh) in one pass, exact f32: out[first * scale + t] = tanh(w[k c_in] + sum_j sum_c w[j c_in + c] lrelu(x[t + j - (k - 1) / 2][c])).
 * w: f32 [k][c_in] followed by the bias. */
int ss_voc_tail(const float* x, const float* w, float* out, const int64_t* table_dev, int n_utt, int64_t max_frames, int scale,
                int c_in, int k, float slope, void* stream);

#ifdef __cplusplus
}
#endif
#endif
