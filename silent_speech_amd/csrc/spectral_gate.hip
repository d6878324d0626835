// spectral_gate.hip -- stationary spectral gating of recorded audio (the reference's data_collection/clean_audio.py:53,
//     clean = nr.reduce_noise(y = data, sr = rate, y_noise = silence, stationary = True),
// noisereduce 3's stationary gate with its defaults, restated in tests/spectral_gate_oracle.py) for a RAGGED BATCH of signals on the MI355X.
// N = 1024, hop H = 256, w = periodic Hann(1024), W = sum w.  A signal of L samples has F = ceil(L / H) + 1 frames, frame f covers the samples
// [f H - 512, f H + 512) with zeros outside [0, L):
//     X[k, f] = (1 / W) sum_n w[n] frame_f[n] e^(-2 pi i k n / N),  d = 20 log10(|X| + eps), clamped from below per row k at max_f d[k, .] - 80,
//     gate m[k, f] = [d > thresh[k]] p + (1 - p),  smoothed by outer(tri(n_f), tri(n_t)) / sum with zeros outside the 513 x F mask,
//     y_f = irfft(X m_smooth) W,  out[n] = sum_f w y_f / sum_f w^2 over the frames that cover n.
// Three launches per batch, every frame ONE WAVE with the 1024-point real FFT of fft1024.h (shared with mel.hip):
//   analysis   |X| per bin -> the binary gate |X| + eps > 10^(thresh / 20) as BITS (513 per frame, a 17-dword row) and the per-(utterance, row)
//              maximum of |X| folded into a table by an integer atomicMax on the float's bits (order-independent; |X|, not |X|^2: the square
//              underflows below 1e-19 and orders the same).  The clamp only ever OPENS a row -- max_f d - 80 > thresh <=> every frame passes --, so
//              that table is all the top_db rule needs.  A wave owns a run of consecutive frames and keeps the maxima in registers until the
//              utterance changes.  In profile mode the same kernel writes d (f64) of the noise clip's frames; sg_profile_reduce_kernel turns them
//              into thresh[513] (max, clamp, mean, population std; 16 rows x 16 frame lanes per workgroup, partial sums combined in lane order).
//   synthesis  the FFT AGAIN (a stored spectrum would be 8 B x 513 per frame = 16 B per sample written and read back, the samples are 4 B each read
//              from the caches), the gate bits of the frames f - n_t .. f + n_t and the row-open bits -> the smoothed mask as INTEGER sums
//              (tri(n)[d] = (n + 1 - |d|) / (n + 1), sum tri = n + 1: counts <= 33^2 9^2, exact in f32) separably, time then frequency, zeros
//              outside the mask, one rounding to f32 -> Y = X m -> the inverse FFT as the forward passes on conj Z,
//              Z[k] = E + i O, E = (Y[k] + conj Y[512 - k]) / 2, O = (Y[k] - conj Y[512 - k]) / 2 conj W_1024^k -> times w W / 512 -> the windowed frame
//              into a workspace.
//   overlap-add one workgroup per hop: out[n] = (sum of the <= 4 windowed frames that cover n, in ASCENDING frame order) / (sum of their w^2, same
//              order).  No floating-point atomics anywhere: a sample depends on its own utterance's samples only, not on the batch, the grid or the
//              order in which waves finish.  The workspace costs 16 B written + 16 B read per sample on top of the 4 B in + 4 B out.
#include "spectral_gate_common.h"
#include "silent_speech_hip.h"

namespace {
constexpr int SG_ROW = 17;
constexpr double SG_EPS = 2.220446049250313e-16;                    // 2^-52 (np.finfo(float).eps)

// 10^(thresh / 20) in f64: +inf closes a row for good, -inf opens it (|X| + eps > 0)
__device__ __forceinline__ double sg_amp(float thresh_db) { return pow(10.0, (double)thresh_db / 20.0); }

__global__ __launch_bounds__(SG_WAVES * 64, 2) void sg_analysis_kernel(const float* __restrict__ x, const long long* __restrict__ tab, int R, long long total,
                                                                    const float* __restrict__ window, const float* __restrict__ thresh,
                                                                    unsigned* __restrict__ bits, unsigned* __restrict__ rowmax, double* __restrict__ db)
{
    __shared__ cpx tile_s[SG_WAVES][MF_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_uniform(tid >> 6);
    cpx* tl = tile_s[wv];
    cpx win[8], tw1[8], tw2[8], tw3[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { const int n = lane + 64 * q; win[q] = cpx{window[2 * n], window[2 * n + 1]}; }
    fft512_twiddles(lane, tw1, tw2, tw3);
    const cpx tw_nyq = twiddle(MF_H, MF_N);
    double amp[9];                                                   // bins lane + 64 j, and bin 512 (lane 0)
#pragma unroll
    for (int j = 0; j < 9; ++j) { const int k = lane + 64 * j; amp[j] = (thresh && k < SG_BINS) ? sg_amp(thresh[k]) : (double)INFINITY; }
    float mx[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) mx[j] = 0.f;

    long long g0, g1;
    sg_run(total, (long long)blockIdx.x * SG_WAVES + wv, (long long)gridDim.x * SG_WAVES, g0, g1);
    int u = -1;
    long long fr0 = 0, fr1 = 0;                                      // the frames of utterance u
    const float* xu = x; int L = 0;
    auto flush = [&]() {
        if (u < 0) return;
#pragma unroll
        for (int j = 0; j < 8; ++j) { atomicMax(rowmax + (long long)u * SG_BINS + lane + 64 * j, __float_as_uint(mx[j])); mx[j] = 0.f; }
        if (lane == 0) atomicMax(rowmax + (long long)u * SG_BINS + MF_H, __float_as_uint(mx[8]));
        mx[8] = 0.f;
    };
    for (long long g = g0; g < g1; ++g) {
        if (u < 0 || g >= fr1) {
            flush();
            u = wave_uniform(sg_find(tab, R, g));
            fr0 = tab[u * 4 + 2]; fr1 = fr0 + tab[u * 4 + 3];
            xu = x + tab[u * 4]; L = wave_uniform((int)tab[u * 4 + 1]);
        }
        const int f = wave_uniform((int)(g - fr0));
        cpx v[8];
        sg_load_frame(xu, L, f, lane, win, v);
        fft512(v, tl, lane, tw1, tw2);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = lane + 64 * j;
            const float mag = sg_mag(rfft_bin(tl, k, tw3[j]));
            mx[j] = fmaxf(mx[j], mag);
            if (bits) {
                const unsigned long long bal = __ballot((double)mag + SG_EPS > amp[j]);
                if (lane < 2) bits[g * SG_ROW + 2 * j + lane] = (unsigned)(bal >> (32 * lane));
            }
            if (db) db[g * SG_BINS + k] = 20.0 * log10((double)mag + SG_EPS);
        }
        if (lane == 0) {
            const float mag = sg_mag(rfft_nyquist(tl, tw_nyq));
            mx[8] = fmaxf(mx[8], mag);
            if (bits) bits[g * SG_ROW + 16] = ((double)mag + SG_EPS > amp[8]) ? 1u : 0u;
            if (db) db[g * SG_BINS + MF_H] = 20.0 * log10((double)mag + SG_EPS);
        }
    }
    flush();
}

// thresh[k] = mean_f dc[k, .] + n_std std_f dc[k, .] (population), dc = max(d, max_f d - 80); db [F][513] f64.  A workgroup takes 16 rows: thread
// (row, lane f0) walks the frames f0, f0 + 16, .. (neighbouring threads read neighbouring rows of one frame), and the 16 partial results of a row are
// combined in lane order -- a fixed order of additions, in f64.
constexpr int SG_PR = 16;
__global__ __launch_bounds__(SG_PR * SG_PR) void sg_profile_reduce_kernel(const double* __restrict__ db, int F, double n_std, float* __restrict__ thresh)
{
    __shared__ double red_s[SG_PR][SG_PR];
    const int kk = threadIdx.x % SG_PR, fl = threadIdx.x / SG_PR, k = blockIdx.x * SG_PR + kk;
    const bool ok = k < SG_BINS;
    auto combine = [&](double v, bool take_max) -> double {
        red_s[fl][kk] = v;
        __syncthreads();
        double r = red_s[0][kk];
        for (int i = 1; i < SG_PR; ++i) r = take_max ? fmax(r, red_s[i][kk]) : r + red_s[i][kk];
        __syncthreads();
        return r;
    };
    double top = -INFINITY;
    if (ok) for (int f = fl; f < F; f += SG_PR) top = fmax(top, db[(long long)f * SG_BINS + k]);
    const double floor_db = combine(top, true) - 80.0;
    double s = 0.0;
    if (ok) for (int f = fl; f < F; f += SG_PR) s += fmax(db[(long long)f * SG_BINS + k], floor_db);
    const double mean = combine(s, false) / F;
    double q = 0.0;
    if (ok) for (int f = fl; f < F; f += SG_PR) { const double d = fmax(db[(long long)f * SG_BINS + k], floor_db) - mean; q += d * d; }
    q = combine(q, false);
    if (ok && fl == 0) thresh[k] = (float)(mean + n_std * sqrt(q / F));
}

// window3 = [w / W | w W / 512 | w^2], 1024 floats each
__global__ __launch_bounds__(SG_WAVES * 64, 2) void sg_synthesis_kernel(const float* __restrict__ x, const long long* __restrict__ tab, int R, long long total,
                                                                     const float* __restrict__ window3, const float* __restrict__ thresh,
                                                                     const unsigned* __restrict__ bits, const unsigned* __restrict__ rowmax,
                                                                     int n_f, int n_t, double p, float* __restrict__ frames, unsigned* __restrict__ bits_out)
{
    __shared__ cpx tile_s[SG_WAVES][MF_TILE];
    __shared__ cpx spec_s[SG_WAVES][SG_BINS + 7];
    __shared__ float cnt_s[SG_WAVES][SG_CBUF];
    __shared__ unsigned rows_s[SG_WAVES][(2 * SG_MAX_NT + 1) * SG_ROW];
    __shared__ float mask_s[SG_WAVES][64 * SG_PER];
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_uniform(tid >> 6);
    cpx* tl = tile_s[wv]; cpx* sp = spec_s[wv]; float* cb = cnt_s[wv]; unsigned* rw = rows_s[wv]; float* mk = mask_s[wv];
    for (int i = lane; i < SG_CBUF; i += 64) cb[i] = 0.f;            // the margins stay zero: only [SG_PAD, SG_PAD + 513) is written per frame
    cpx win[8], tw1[8], tw2[8], tw3[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { const int n = lane + 64 * q; win[q] = cpx{window3[2 * n], window3[2 * n + 1]}; }
    fft512_twiddles(lane, tw1, tw2, tw3);
    const cpx tw_nyq = twiddle(MF_H, MF_N);
    const double norm = (double)(n_f + 1) * (n_f + 1) * (double)(n_t + 1) * (n_t + 1);

    long long g0, g1;
    sg_run(total, (long long)blockIdx.x * SG_WAVES + wv, (long long)gridDim.x * SG_WAVES, g0, g1);
    int u = -1, F = 0, L = 0;
    long long fr0 = 0, fr1 = 0;
    const float* xu = x;
    unsigned open = 0;                                                // bit j: row lane + 64 j is open in every frame (top_db)
    for (long long g = g0; g < g1; ++g) {
        if (u < 0 || g >= fr1) {
            u = wave_uniform(sg_find(tab, R, g));
            fr0 = tab[u * 4 + 2]; F = wave_uniform((int)tab[u * 4 + 3]); fr1 = fr0 + F;
            xu = x + tab[u * 4]; L = wave_uniform((int)tab[u * 4 + 1]);
            open = 0;
            for (int j = 0; j < 9; ++j) {
                const int k = lane + 64 * j;
                if (k < SG_BINS) {
                    const double top = (double)__uint_as_float(rowmax[(long long)u * SG_BINS + k]) + SG_EPS;      // 20 log10(top) - 80 > thresh
                    if (top * 1e-4 > sg_amp(thresh[k])) open |= 1u << j;
                }
            }
        }
        const int f = wave_uniform((int)(g - fr0));
        // ---- the gate rows of the frames f - n_t .. f + n_t (zeros where there is no frame)
        wave_lds_sync();
        for (int i = lane; i < (2 * n_t + 1) * SG_ROW; i += 64) {
            const int dt = i / SG_ROW - n_t, ff = f + dt;
            rw[i] = (ff >= 0 && ff < F) ? bits[(g + dt) * SG_ROW + (i % SG_ROW)] : 0u;
        }
        // ---- the spectrum again
        cpx v[8];
        sg_load_frame(xu, L, f, lane, win, v);
        fft512(v, tl, lane, tw1, tw2);                                // (its fences order the row / count buffers too)
#pragma unroll
        for (int j = 0; j < 8; ++j) sp[lane + 64 * j] = rfft_bin(tl, lane + 64 * j, tw3[j]);
        if (lane == 0) { sp[0][1] = 0.f; sp[MF_H] = cpx{rfft_nyquist(tl, tw_nyq)[0], 0.f}; }      // bins 0 and 512 of a real signal are real
        // ---- time taps: integer counts sum_dt (n_t + 1 - |dt|) bit[k, f + dt]; an open row is open in every frame that exists
        int cover_t = 0;
        for (int dt = -n_t; dt <= n_t; ++dt) if (f + dt >= 0 && f + dt < F) cover_t += n_t + 1 - (dt < 0 ? -dt : dt);
#pragma unroll 1
        for (int j = 0; j < 9; ++j) {
            const int k = lane + 64 * j;
            if (k < SG_BINS) {
                const int dw = k >> 5, sh = k & 31;
                const unsigned ob = (open >> j) & 1u;
                int c = 0;
                for (int dt = -n_t; dt <= n_t; ++dt) {
                    const bool there = f + dt >= 0 && f + dt < F;
                    const unsigned b = ((rw[(dt + n_t) * SG_ROW + dw] >> sh) & 1u) | ob;
                    c += there ? (int)b * (n_t + 1 - (dt < 0 ? -dt : dt)) : 0;
                }
                cb[SG_PAD + k] = (float)c;
            }
        }
        if (bits_out) {                                               // the final gate of this frame: own bits | open rows
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = lane + 64 * j;
                const unsigned long long bal = __ballot((int)(((rw[n_t * SG_ROW + (k >> 5)] >> (k & 31)) | (open >> j)) & 1u));
                if (lane < 2) bits_out[g * SG_ROW + 2 * j + lane] = (unsigned)(bal >> (32 * lane));
            }
            if (lane == 0) bits_out[g * SG_ROW + 16] = (rw[n_t * SG_ROW + 16] | (open >> 8)) & 1u;
        }
        wave_lds_sync();
        // ---- frequency taps over SG_PER consecutive bins per lane: T(k) = sum_d (n_f + 1 - |d|) c(k + d) directly for the lane's first bin, then
        // T(k + 1) = T(k) + P(k + 1) - Q(k) with the running box sums P(k) = c(k) + .. + c(k + n_f), Q(k) = c(k - n_f) + .. + c(k): small integers, exact in
        // f32, so the order of the sums does not matter.  Then the share of open bins and of the mask's inside, one rounding:
        // m = (p count + (1 - p) cover) / norm
        {
            const float* c = cb + SG_PAD + SG_PER * lane;
            float T = 0.f, P = 0.f, Q = 0.f;
            for (int d = 0; d <= n_f; ++d) { P += c[d]; Q += c[-d]; T += (float)(n_f + 1 - d) * (c[d] + (d ? c[-d] : 0.f)); }
#pragma unroll 1
            for (int i = 0; i < SG_PER; ++i) {
                const int k = SG_PER * lane + i;
                // frequency taps of this bin that fall inside [0, 512]: (n_f + 1)^2 minus the tails that are cut off
                const int lo = n_f - k > 0 ? n_f - k : 0, hi = n_f - (MF_H - k) > 0 ? n_f - (MF_H - k) : 0;
                const int cover_f = (n_f + 1) * (n_f + 1) - lo * (lo + 1) / 2 - hi * (hi + 1) / 2;
                mk[k] = (float)((p * (double)T + (1.0 - p) * (double)(cover_f * cover_t)) / norm);       // (bins behind 512: never read)
                const float Pn = P + c[i + n_f + 1] - c[i];
                T += Pn - Q;
                Q += c[i + 1] - c[i - n_f];
                P = Pn;
            }
        }
        wave_lds_sync();
        // ---- Y = X m
#pragma unroll
        for (int j = 0; j < 8; ++j) sp[lane + 64 * j] *= mk[lane + 64 * j];
        if (lane == 0) sp[MF_H] *= mk[MF_H];
        wave_lds_sync();
        // ---- inverse: v[j] = conj Z[k], Z[k] = E + i O, k = lane + 64 j
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = lane + 64 * j;
            const cpx a = sp[k], c0 = sp[MF_H - k], c = cpx{c0[0], -c0[1]};
            const cpx e = 0.5f * (a + c), o = cmul(0.5f * (a - c), cpx{tw3[j][0], -tw3[j][1]});
            v[j] = cpx{e[0] - o[1], -(e[1] + o[0])};
        }
        fft512(v, tl, lane, tw1, tw2);
        float* out = frames + g * MF_N;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int n = lane + 64 * q;
            const cpx r = tl[zpos(n)];                                // the inverse comes out conjugated: z[n] = conj(R[n]) / 512
            out[2 * n] = r[0] * window3[MF_N + 2 * n]; out[2 * n + 1] = -r[1] * window3[MF_N + 2 * n + 1];
        }
    }
}

}  // namespace

extern "C" int ss_spectral_gate_limits(int* max_n_f, int* max_n_t, int* row_dwords)
{
    if (max_n_f) *max_n_f = SG_MAX_NF;
    if (max_n_t) *max_n_t = SG_MAX_NT;
    if (row_dwords) *row_dwords = SG_ROW;
    return 0;
}

extern "C" int ss_spectral_gate_profile(const float* x, const int64_t* table_dev, int frames, const float* window_dev, double n_std, double* db_workspace,
                                        uint32_t* rowmax_workspace, float* thresh, void* stream)
{
    SS_CHECK(x && table_dev && window_dev && db_workspace && rowmax_workspace && thresh, "ss_spectral_gate_profile: null pointer");
    SS_CHECK(frames >= 2, "ss_spectral_gate_profile: an empty noise clip (a clip of L >= 1 samples has ceil(L / 256) + 1 >= 2 frames)");
    SS_CHECK(ss_memset_async(rowmax_workspace, 0, SG_BINS * sizeof(uint32_t), stream), "ss_spectral_gate_profile: memset failed");
    SS_LAUNCH(sg_analysis_kernel, dim3(sg_grid(frames)), dim3(SG_WAVES * 64), 0, stream, x, (const long long*)table_dev, 1, (long long)frames, window_dev,
              (const float*)nullptr, (unsigned*)nullptr, (unsigned*)rowmax_workspace, db_workspace);
    SS_LAUNCH(sg_profile_reduce_kernel, dim3((SG_BINS + SG_PR - 1) / SG_PR), dim3(SG_PR * SG_PR), 0, stream, (const double*)db_workspace, frames, n_std, thresh);
    SS_LAUNCH_CHECK("ss_spectral_gate_profile");
    return 0;
}

extern "C" int ss_spectral_gate_batch(const float* x, float* y, const int64_t* table_dev, int R, int64_t total_frames, const float* window_dev, const float* thresh,
                                      int n_f, int n_t, double prop_decrease, uint32_t* bits_workspace, uint32_t* rowmax_workspace, float* frames_workspace,
                                      uint32_t* bits_out, void* stream)
{
    SS_CHECK(x && y && table_dev && window_dev && thresh && bits_workspace && rowmax_workspace && frames_workspace, "ss_spectral_gate_batch: null pointer");
    SS_CHECK(R >= 1 && total_frames >= 2 * (int64_t)R, "ss_spectral_gate_batch: bad sizes (every signal has L >= 1 samples, i.e. at least 2 frames)");
    SS_CHECK(n_f >= 0 && n_f <= SG_MAX_NF && n_t >= 0 && n_t <= SG_MAX_NT, "ss_spectral_gate_batch: mask smoothing of %d bins x %d frames exceeds the kernel's bounds (%d x %d)",
             n_f, n_t, SG_MAX_NF, SG_MAX_NT);
    SS_CHECK(prop_decrease >= 0.0 && prop_decrease <= 1.0, "ss_spectral_gate_batch: prop_decrease must lie in [0, 1]");
    SS_CHECK(ss_memset_async(rowmax_workspace, 0, (size_t)R * SG_BINS * sizeof(uint32_t), stream), "ss_spectral_gate_batch: memset failed");
    const int grid = sg_grid(total_frames);
    SS_LAUNCH(sg_analysis_kernel, dim3(grid), dim3(SG_WAVES * 64), 0, stream, x, (const long long*)table_dev, R, (long long)total_frames, window_dev, thresh,
              (unsigned*)bits_workspace, (unsigned*)rowmax_workspace, (double*)nullptr);
    SS_LAUNCH(sg_synthesis_kernel, dim3(grid), dim3(SG_WAVES * 64), 0, stream, x, (const long long*)table_dev, R, (long long)total_frames, window_dev, thresh,
              (const unsigned*)bits_workspace, (const unsigned*)rowmax_workspace, n_f, n_t, prop_decrease, frames_workspace, (unsigned*)bits_out);
    SS_LAUNCH(sg_overlap_add_kernel, dim3((unsigned)(total_frames - R)), dim3(SG_HOP), 0, stream, (const float*)frames_workspace, (const long long*)table_dev, R,
              window_dev + 2 * MF_N, y);
    SS_LAUNCH_CHECK("ss_spectral_gate_batch");
    return 0;
}
