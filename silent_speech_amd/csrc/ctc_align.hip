// ctc_align.hip -- forced (Viterbi) alignment of known label strings to the frame posteriors of the recognition / transduction heads on gfx950: the
// best path of the CTC topology (or of the blank-free linear one), its score, the label of every frame and the span and log-probability of every token.
// The definition, ties included, is the one include/silent_speech_hip.h states for ss_ctc_align; tests/ctc_align_oracle.py restates it in plain Python
// and shares no code with this file.
//
// One launch aligns the batch, ONE WAVE (a 64-thread workgroup) PER UTTERANCE; nothing goes back to the host and the lengths are read on the device.
//   states   a lane owns KT consecutive tokens in registers, KT = 1, 2, 4, 8 chosen PER UTTERANCE on the device (an instance of al_run each): under the
//            CTC topology that is the token state and the blank state before it, 2 KT = 2 .. 16 consecutive extended states; the blank behind the last
//            token is the blank "before" token S.  64 * 8 = 512 >= S + 1 for S <= 511.  The lane's labels stay in registers.
//   frame    the only cross-lane traffic is the top token state of the lane below (DPP wave_shr:1, common.h).  Per state: best predecessor, strict
//            '>' from the smallest jump up (ties to the smallest jump), then ONE f32 addition best + (logit - lse).
//   gather   logit[t][label] of AL_FB = 16 frames is loaded into registers while the previous 16 frames are scanned (issue early, use late), and goes
//            through lane-private LDS slots only because the scan indexes it by a run-time frame number.
//   pointers 2 bits per state = one 32-bit word per lane and frame, written to the workspace with ordinary coalesced vector stores.
//   trace    in the same launch: the words of AL_BT = 64 frames are staged into LDS with coalesced loads, lane 0 walks them backwards (an LDS read
//            per frame instead of a dependent global load), the frame labels leave through LDS as one coalesced store per block of frames.  The walk
//            notes first frame and frame count of every token in LDS; afterwards the lanes sum the tokens' log-probabilities in parallel, frames in
//            ascending order.
//   rows     of no utterance get -2 from additional workgroups of the same launch (a row asks every table entry: rows * n_utt / 64 wave steps).
// Every loop is bounded by T, S or n_utt; there is no inter-workgroup communication and no spinning.
#include "ctc_beam_common.h"   // ctc_utt_frames / ctc_utt_locate: the clamped walk of the utterance table
#include "silent_speech_hip.h"

namespace {
constexpr int AL_FB = 16, AL_BT = 64, AL_MAX_S = 511, AL_MAX_V = 4096, AL_MAX_KT = 8, AL_FILL_ROWS = 512;

struct AlArgs {
    const float* logits; long long ld; int V, blank; long long rows; const float* lse; const long long* utt; int n_utt; long long total_frames;
    int max_s; const int* targets; long long n_targets; unsigned* ws; float* score; int* frame_token; int* token_first; int* token_frames; float* token_logp;
};
struct AlLds { float* E; unsigned* bpw; int *tfirst, *tcnt, *ft; };

// this wave's global stores become visible to its own later loads (the back-pointer words cross lanes through the workspace)
__device__ __forceinline__ void al_fence() {
#if !defined(SS_EMU)
    __threadfence();
#endif
    __syncthreads();
}

template <int KT, bool CTC>
__device__ void al_run(const AlArgs& a, const AlLds& L, int u, long long f0, long long off, int T, long long tg0, int S, bool table_ok)
{
    constexpr int NE = CTC ? KT + 1 : KT;                              // values gathered per frame: the lane's tokens, then the blank
    constexpr int SPL = CTC ? 2 * KT : KT;                             // states per lane
    const int lane = threadIdx.x;
    const int* tg = a.targets + tg0;
    int col[NE];
    bool tv[KT], skip[KT];
    int bad = table_ok ? 0 : 1;
#pragma unroll
    for (int i = 0; i < KT; ++i) {
        const int tok = lane * KT + i;
        tv[i] = tok < S;
        int y = tv[i] ? tg[tok] : 0;
        if (tv[i] && (y < 0 || y >= a.V || (CTC && y == a.blank))) { bad = 1; y = 0; }
        col[i] = y;
    }
    if constexpr (CTC) col[KT] = a.blank;
    bad = __any(bad);
    const int yp = __shfl_up(col[KT - 1], 1);
#pragma unroll
    for (int i = 0; i < KT; ++i) skip[i] = tv[i] && lane * KT + i > 0 && col[i] != (i > 0 ? col[i - 1] : yp);

    float sc = -INFINITY;
    int s_end = 0;
    const bool scan = !bad && T > 0 && (CTC || S > 0);
    if (!bad && T == 0 && S == 0) sc = 0.f;
    if (scan) {
        float raw[AL_FB][NE], rl[AL_FB];
        auto gather = [&](int t0) {
#pragma unroll
            for (int f = 0; f < AL_FB; ++f) {
                const int t = t0 + f;
                if (t < T) {
                    const long long row = f0 + t;
                    const float* x = a.logits + row * a.ld;
                    rl[f] = a.lse[row];
#pragma unroll
                    for (int j = 0; j < NE; ++j) raw[f][j] = x[col[j]];
                } else {
                    rl[f] = 0.f;
#pragma unroll
                    for (int j = 0; j < NE; ++j) raw[f][j] = 0.f;
                }
            }
        };
        float dt[KT], db[KT];                                           // token states; (CTC) the blank state before each
        unsigned* wsu = a.ws + off * 64 + lane;
        gather(0);
        for (int t0 = 0; t0 < T; t0 += AL_FB) {
#pragma unroll
            for (int f = 0; f < AL_FB; ++f)
#pragma unroll
                for (int j = 0; j < NE; ++j) L.E[(f * NE + j) * 64 + lane] = raw[f][j] - rl[f];       // lane-private slots: no barrier
            if (t0 + AL_FB < T) gather(t0 + AL_FB);
            const int nf = T - t0 < AL_FB ? T - t0 : AL_FB;
            for (int f = 0; f < nf; ++f) {
                float e[NE];
#pragma unroll
                for (int j = 0; j < NE; ++j) e[j] = L.E[(f * NE + j) * 64 + lane];
                unsigned w = 0u;
                if (t0 + f == 0) {
#pragma unroll
                    for (int i = 0; i < KT; ++i) {
                        const bool first = lane * KT + i == 0;
                        dt[i] = first && tv[i] ? e[i] : -INFINITY;
                        if constexpr (CTC) db[i] = first ? e[KT] : -INFINITY;
                    }
                } else {
                    const float below = wave_shr1(dt[KT - 1], -INFINITY);
#pragma unroll
                    for (int i = KT - 1; i >= 0; --i) {                 // downwards: dt[i - 1] is still the previous frame's
                        const float pt = i > 0 ? dt[i - 1] : below;
                        if constexpr (CTC) {
                            float best = dt[i]; unsigned bp = 0u;
                            if (db[i] > best) { best = db[i]; bp = 1u; }
                            if (skip[i] && pt > best) { best = pt; bp = 2u; }
                            float bb = db[i]; unsigned bpb = 0u;
                            if (pt > bb) { bb = pt; bpb = 1u; }
                            dt[i] = tv[i] && best > -INFINITY ? best + e[i] : -INFINITY;
                            db[i] = lane * KT + i <= S && bb > -INFINITY ? bb + e[KT] : -INFINITY;
                            w |= (bpb | (bp << 2)) << (4 * i);
                        } else {
                            float best = dt[i]; unsigned bp = 0u;
                            if (pt > best) { best = pt; bp = 1u; }
                            dt[i] = tv[i] && best > -INFINITY ? best + e[i] : -INFINITY;
                            w |= bp << (2 * i);
                        }
                    }
                }
                wsu[(long long)(t0 + f) * 64] = w;
            }
        }
        // the last frame's states through LDS (E is free now): the end state and the score
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KT; ++i) {
            if constexpr (CTC) { L.E[2 * (lane * KT + i)] = db[i]; L.E[2 * (lane * KT + i) + 1] = dt[i]; }
            else L.E[lane * KT + i] = dt[i];
        }
        __syncthreads();
        if constexpr (CTC) {
            const float vb = L.E[2 * S], vt = S > 0 ? L.E[2 * S - 1] : -INFINITY;
            if (S > 0 && vt >= vb) { sc = vt; s_end = 2 * S - 1; } else { sc = vb; s_end = 2 * S; }
        } else { sc = L.E[S - 1]; s_end = S - 1; }
    }

    if (!(sc > -INFINITY)) {                                            // no alignment exists
        if (lane == 0) a.score[u] = -INFINITY;
        for (int t = lane; t < T; t += 64) a.frame_token[f0 + t] = -2;
        for (int k = lane; k < S; k += 64) { a.token_first[tg0 + k] = -1; a.token_frames[tg0 + k] = 0; a.token_logp[tg0 + k] = 0.f; }
        return;
    }
    if (lane == 0) a.score[u] = sc;
    if (T == 0) return;

    for (int k = lane; k < S; k += 64) { L.tfirst[k] = -1; L.tcnt[k] = 0; }
    al_fence();
    int s = s_end;
    for (int tb = ((T - 1) / AL_BT) * AL_BT; tb >= 0; tb -= AL_BT) {
        const int nf = T - tb < AL_BT ? T - tb : AL_BT;
        const unsigned* src = a.ws + (off + tb) * 64 + lane;
        for (int g = 0; g < nf; g += 16) {                              // sixteen loads in flight (clamped, not predicated: one basic block), then LDS
            unsigned bw[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) bw[j] = src[(long long)(g + j < nf ? g + j : nf - 1) * 64];
#pragma unroll
            for (int j = 0; j < 16; ++j) L.bpw[(g + j) * 64 + lane] = bw[j];
        }
        __syncthreads();
        if (lane == 0) {
            for (int f = nf - 1; f >= 0; --f) {
                const int tok = CTC ? ((s & 1) ? (s >> 1) : -1) : s;
                L.ft[f] = tok;
                if (tok >= 0 && tok < S) { L.tfirst[tok] = tb + f; L.tcnt[tok] += 1; }
                s -= (int)((L.bpw[f * 64 + s / SPL] >> (2 * (s % SPL))) & 3u);
                if (s < 0) s = 0;
            }
        }
        __syncthreads();
        if (lane < nf) a.frame_token[f0 + tb + lane] = L.ft[lane];
    }
    __syncthreads();
    for (int k = lane; k < S; k += 64) {
        const int first = L.tfirst[k], n = L.tcnt[k], y = tg[k];
        float sum = 0.f;
        if (first >= 0 && first + n <= T)
            for (int j = 0; j < n; j += 8) {                            // eight loads in flight, the sum in frame order
                float v[8], l[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const long long row = f0 + first + (j + i < n ? j + i : n - 1);
                    v[i] = a.logits[row * a.ld + y]; l[i] = a.lse[row];
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) if (j + i < n) sum += v[i] - l[i];
            }
        a.token_first[tg0 + k] = first; a.token_frames[tg0 + k] = n; a.token_logp[tg0 + k] = sum;
    }
}
}

template <bool CTC>
__global__ __launch_bounds__(64) void ctc_align_kernel(const AlArgs a)
{
    __shared__ float E[AL_FB * (AL_MAX_KT + 1) * 64];                   // 36 KiB; at least 1024 floats for the last frame's states
    __shared__ unsigned bpw[AL_BT * 64];
    __shared__ int tfirst[AL_MAX_S + 1], tcnt[AL_MAX_S + 1], ft[AL_BT];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= a.n_utt) {                                  // rows of no utterance
        const long long nfill = (long long)gridDim.x - a.n_utt, fb = (long long)blockIdx.x - a.n_utt;
        for (long long r = fb * 64 + lane; r < a.rows; r += nfill * 64) {
            bool covered = false;
            long long off = 0, f0;
            for (int j = 0; j < a.n_utt; ++j) { const int n = ctc_utt_frames(a.utt, 4, j, a.total_frames, a.rows, off, f0); covered |= r >= f0 && r - f0 < n; }
            if (!covered) a.frame_token[r] = -2;
        }
        return;
    }
    const int u = blockIdx.x;
    long long off_u, f0;
    const int T = ctc_utt_locate(a.utt, 4, u, a.total_frames, a.rows, off_u, f0);
    const long long tg0 = a.utt[4 * u + 2], Sl = a.utt[4 * u + 3];
    const bool table_ok = tg0 >= 0 && Sl >= 0 && Sl <= a.max_s && tg0 <= a.n_targets - Sl;
    const int S = table_ok ? (int)Sl : 0;
    const AlLds L = {E, bpw, tfirst, tcnt, ft};
    const int need = CTC ? S + 1 : S;
    if (need <= 64) al_run<1, CTC>(a, L, u, f0, off_u, T, table_ok ? tg0 : 0, S, table_ok);
    else if (need <= 128) al_run<2, CTC>(a, L, u, f0, off_u, T, tg0, S, table_ok);
    else if (need <= 256) al_run<4, CTC>(a, L, u, f0, off_u, T, tg0, S, table_ok);
    else al_run<8, CTC>(a, L, u, f0, off_u, T, tg0, S, table_ok);
}

extern "C" int64_t ss_ctc_align_workspace_bytes(int n_utt, int64_t total_frames, int max_target_len)
{
    if (n_utt < 0 || total_frames < 0 || max_target_len < 0 || max_target_len > AL_MAX_S) return -1;
    return 256 * (total_frames + 1);
}

extern "C" int ss_ctc_align(const float* logits, int64_t ld, int V, int blank, int64_t rows, const float* lse, const int64_t* utt_dev, int n_utt,
                            int64_t total_frames, int max_target_len, const int32_t* targets, int64_t n_targets, void* workspace, float* score,
                            int32_t* frame_token, int32_t* token_first, int32_t* token_frames, float* token_logp, void* stream)
{
    SS_CHECK(V >= 1 && V <= AL_MAX_V && ld >= V, "ss_ctc_align: %d classes (1 .. %d) at row stride %lld", V, AL_MAX_V, (long long)ld);
    SS_CHECK(blank >= -1 && blank < V, "ss_ctc_align: blank %d (a class of the %d, or -1 for the linear topology)", blank, V);
    SS_CHECK(max_target_len >= 0 && max_target_len <= AL_MAX_S, "ss_ctc_align: targets of up to %d labels (0 .. %d)", max_target_len, AL_MAX_S);
    SS_CHECK(n_utt >= 0 && rows >= 0 && total_frames >= 0 && n_targets >= 0, "ss_ctc_align: negative sizes");
    SS_CHECK(total_frames <= 0x7fffffffll, "ss_ctc_align: %lld frames exceed the 32-bit frame numbers", (long long)total_frames);
    if (n_utt == 0 && rows == 0) return 0;
    SS_CHECK(frame_token || rows == 0, "ss_ctc_align: null pointer");
    SS_CHECK(n_utt == 0 || ((rows == 0 || (logits && lse)) && utt_dev && workspace && score && (n_targets == 0 || (targets && token_first && token_frames && token_logp))),
             "ss_ctc_align: null pointer");
    long long nfill = (rows + AL_FILL_ROWS - 1) / AL_FILL_ROWS;
    if (nfill > 1024) nfill = 1024;
    const AlArgs a = {logits, (long long)ld, V, blank, (long long)rows, lse, (const long long*)utt_dev, n_utt, (long long)total_frames, max_target_len,
                      (const int*)targets, (long long)n_targets, (unsigned*)workspace, score, (int*)frame_token, (int*)token_first, (int*)token_frames, token_logp};
    if (blank >= 0) SS_LAUNCH(SS_KERNEL(ctc_align_kernel<true>), dim3((unsigned)(n_utt + nfill)), dim3(64), 0, stream, a);
    else SS_LAUNCH(SS_KERNEL(ctc_align_kernel<false>), dim3((unsigned)(n_utt + nfill)), dim3(64), 0, stream, a);
    SS_LAUNCH_CHECK("ss_ctc_align");
    return 0;
}
