// edit_distance.hip -- Levenshtein distance of token strings on gfx950 with the error breakdown (hits, substitutions, deletions, insertions), the
// alignment behind it, and the minimum-Bayes-risk pass over n-best lists (all K^2 distances of a list, the expected distance of every hypothesis
// under the list's weights, the hypothesis of least risk).  The definition, ties included, is the one include/silent_speech_hip.h states for
// ss_edit_distance / ss_nbest_risk; tests/edit_distance_oracle.py restates it in plain Python and shares no code with this file.
//
// ONE WAVE (a 64-thread workgroup) PER PAIR; the tables are read on the device and nothing goes back to the host.
//   cells    a lane owns KT consecutive hypothesis columns in registers, KT = 1, 2, 4, 8, 16 chosen PER PAIR on the device from n_b <= 64 .. 1024.
//            The lanes run skewed by one reference row each (lane l is on row s - l + 1 at step s), so the only cross-lane traffic of a step is the
//            last cell of the lane below (DPP wave_shr:1, common.h); the diagonal is what that shift delivered one step earlier.  n_a + lanes - 1
//            steps of KT cells; no scan.  The reference tokens sit in LDS (4 KiB) and are fetched one step ahead of their use.
//   value    ONE int per cell: distance << 11 | hits of the path the predecessors define.  With hits + S + D = i, hits + S + I = j and
//            S + D + I = distance the other three counts of a cell follow from these two, so the four counts travel with the distance and the
//            distance-only callers (WER totals, the MBR matrix) need no pointer workspace and no backtrace.
//   pointers (alignment wanted) 2 bits per cell = the step itself (0 hit, 1 substitution, 2 deletion, 3 insertion), KT of them = one word per lane
//            and STEP, stored coalesced.  The walk runs in the same launch: the words of ED_BT = 64 steps are staged into LDS with coalesced loads,
//            lane 0 walks them (the step number of the cells on a path never increases towards the origin), the steps leave through LDS as
//            coalesced byte stores.
// Every loop is bounded by a length or a count read from the tables and clamped to the limits; no inter-workgroup communication, no spinning.
#include "common.h"
#include "silent_speech_hip.h"

namespace {
constexpr int ED_MAX_LEN = 1023, ED_BT = 64, ED_MAX_K = 128, ED_ONE = 1 << 11, ED_HITS = ED_ONE - 1, ED_MAX_GROUPS = 65535;
constexpr long long ED_MAX_PAIRS = 1ll << 24;

struct EdSeq { long long first; int len; bool ok; };
// entry idx of the sequence table, clamped: a negative length, a length above the limit, a span outside tokens or an index outside the table is "bad"
__device__ __forceinline__ EdSeq ed_seq(const long long* seqs, long long n_seq, long long n_tokens, long long idx)
{
    EdSeq q = {0, 0, false};
    if (idx < 0 || idx >= n_seq) return q;
    const long long f = seqs[2 * idx], n = seqs[2 * idx + 1];
    if (n < 0 || n > ED_MAX_LEN || f < 0 || f > n_tokens - n) return q;
    q.first = f; q.len = (int)n; q.ok = true;
    return q;
}

__device__ __forceinline__ int ed_shr1(int v, int fill) { return __float_as_int(wave_shr1(__int_as_float(v), __int_as_float(fill))); }

// this wave's global stores become visible to its own later loads (the back-pointer words cross lanes through the workspace)
__device__ __forceinline__ void ed_fence() {
#if !defined(SS_EMU)
    __threadfence();
#endif
    __syncthreads();
}

__device__ __forceinline__ void ed_stage(int* sa, const int* a, int n_a)
{
    for (int i = threadIdx.x; i < n_a; i += 64) sa[i] = a[i];
    __syncthreads();
}

// The packed cell (n_a, n_b), in every lane.  sa: the reference in LDS, n_a >= 1 tokens; b: the hypothesis, n_b >= 1 of them; wsl (BP): this pair's workspace + lane.
template <int KT, bool BP>
__device__ int ed_forward(const int* sa, int n_a, const int* b, int n_b, unsigned* wsl)
{
    const int lane = threadIdx.x;
    const int nl = (n_b + KT - 1) / KT;                                 // lanes that own a column
    int tb[KT], c[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        const int j = lane * KT + k;
        tb[k] = j < n_b ? b[j] : 0;
        c[k] = (j + 1) * ED_ONE;                                        // row 0
    }
    int diag = lane * KT * ED_ONE;
    const int steps = n_a + nl - 1;
    int a_next = sa[0];                                                 // lane 0's first row; the others start on a later step
    for (int s = 0; s < steps; ++s) {
        const int left = ed_shr1(c[KT - 1], (s + 1) * ED_ONE);          // cell (row of this step, last column of the lane below); lane 0: column 0
        const int r = s - lane, x = a_next;                             // this lane is on row r + 1
        const int rn = r + 1;
        a_next = sa[rn < 0 ? 0 : rn < n_a ? rn : n_a - 1];
        if (r >= 0 && r < n_a && lane < nl) {
            unsigned w = 0u;
            int l = left, d = diag;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const int up = c[k] + ED_ONE;
                const bool hit = x == tb[k];
                int best = d + (hit ? 1 : ED_ONE);
                unsigned op = hit ? 0u : 1u;
                if ((up >> 11) < (best >> 11)) { best = up; op = 2u; }
                if (((l + ED_ONE) >> 11) < (best >> 11)) { best = l + ED_ONE; op = 3u; }
                d = c[k]; c[k] = best; l = best;
                if constexpr (BP) w |= op << (2 * k);
            }
            if constexpr (BP) wsl[(long long)s * 64] = w;
        }
        diag = left;
    }
    const int kf = (n_b - 1) % KT;
    int v = 0;
#pragma unroll
    for (int k = 0; k < KT; ++k) if (k == kf) v = c[k];
    return __shfl(v, (n_b - 1) / KT);
}

template <bool BP>
__device__ __forceinline__ int ed_dispatch_forward(const int* sa, int n_a, const int* b, int n_b, unsigned* wsl)
{
    if (n_b <= 64) return ed_forward<1, BP>(sa, n_a, b, n_b, wsl);
    if (n_b <= 128) return ed_forward<2, BP>(sa, n_a, b, n_b, wsl);
    if (n_b <= 256) return ed_forward<4, BP>(sa, n_a, b, n_b, wsl);
    if (n_b <= 512) return ed_forward<8, BP>(sa, n_a, b, n_b, wsl);
    return ed_forward<16, BP>(sa, n_a, b, n_b, wsl);
}

struct EdLds { unsigned* bpw; signed char* ops; int* at; };

// the steps of the path from (n_a, n_b) back to row 0 or column 0 into L.ops[.. n_path), lane 0 walking; the cell it stops in into L.at
__device__ void ed_walk(const EdLds& L, const unsigned* wsl, int n_a, int n_b, int n_path)
{
    const int lane = threadIdx.x;
    const int kt = n_b <= 64 ? 1 : n_b <= 128 ? 2 : n_b <= 256 ? 4 : n_b <= 512 ? 8 : 16;
    const int sh = n_b <= 64 ? 0 : n_b <= 128 ? 1 : n_b <= 256 ? 2 : n_b <= 512 ? 3 : 4;
    const int steps = n_a + (n_b + kt - 1) / kt - 1;
    int i = n_a, j = n_b, t = n_path - 1;
    const int s_top = n_a - 1 + ((n_b - 1) >> sh);
    for (int sb = (s_top / ED_BT) * ED_BT; sb >= 0; sb -= ED_BT) {
        const int nf = steps - sb < ED_BT ? steps - sb : ED_BT;
        const unsigned* src = wsl + (long long)sb * 64;
        for (int g = 0; g < nf; g += 16) {                              // sixteen loads in flight (clamped, not predicated), then LDS
            unsigned bw[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) bw[q] = src[(long long)(g + q < nf ? g + q : nf - 1) * 64];
#pragma unroll
            for (int q = 0; q < 16; ++q) L.bpw[(g + q) * 64 + lane] = bw[q];
        }
        __syncthreads();
        if (lane == 0) {
            while (i > 0 && j > 0) {                                    // every turn lowers i or j
                const int ln = (j - 1) >> sh, s = i - 1 + ln;
                if (s < sb) break;
                const unsigned op = (L.bpw[(s - sb) * 64 + ln] >> (2 * ((j - 1) & (kt - 1)))) & 3u;
                if (t >= 0) L.ops[t] = (signed char)op;
                --t;
                if (op != 3u) --i;
                if (op != 2u) --j;
            }
        }
        __syncthreads();
    }
    if (lane == 0) { L.at[0] = i; L.at[1] = j; }
    __syncthreads();
}
}

template <bool BP>
__global__ __launch_bounds__(64) void edit_distance_kernel(const int* tokens, long long n_tokens, const long long* seqs, long long n_seq, const int* pairs,
                                                           int* dist, int* counts, signed char* ops, const long long* ops_first, long long n_ops, unsigned* ws)
{
    __shared__ int sa[ED_MAX_LEN + 1];
    __shared__ unsigned bpw[BP ? ED_BT * 64 : 1];
    __shared__ signed char sops[BP ? 2 * ED_MAX_LEN + 2 : 1];
    __shared__ int at[2];
    const int lane = threadIdx.x;
    const long long p = blockIdx.x;
    const EdSeq A = ed_seq(seqs, n_seq, n_tokens, pairs[2 * p]), B = ed_seq(seqs, n_seq, n_tokens, pairs[2 * p + 1]);
    bool ok = A.ok && B.ok;
    const int n_a = A.len, n_b = B.len;
    long long of0 = 0, room = 0;
    if constexpr (BP) {
        of0 = ops_first[p];
        const long long of1 = ops_first[p + 1];
        const bool region = of0 >= 0 && of0 <= of1 && of1 <= n_ops;
        room = region ? of1 - of0 : 0;
        ok = ok && region && room >= n_a + n_b;
    }
    if (!ok) {
        if (lane == 0) dist[p] = -1;
        if (lane < 4) counts[4 * p + lane] = -1;
        if constexpr (BP) for (long long x = lane; x < room; x += 64) ops[of0 + x] = -1;
        return;
    }
    ed_stage(sa, tokens + A.first, n_a);
    unsigned* wsl = BP ? ws + (of0 + 64 * p) * 64 + lane : nullptr;
    const int v = n_a > 0 && n_b > 0 ? ed_dispatch_forward<BP>(sa, n_a, tokens + B.first, n_b, wsl) : (n_a + n_b) * ED_ONE;      // an empty side: row 0 / column 0
    const int d = v >> 11, hits = v & ED_HITS, ins = d - n_a + hits, del = d - n_b + hits, sub = d - ins - del;
    if (lane == 0) { dist[p] = d; counts[4 * p] = hits; counts[4 * p + 1] = sub; counts[4 * p + 2] = del; counts[4 * p + 3] = ins; }
    if constexpr (BP) {
        const int n_path = hits + sub + del + ins;
        const EdLds L = {bpw, sops, at};
        int i = n_a, j = n_b;
        if (n_a > 0 && n_b > 0) {
            ed_fence();
            ed_walk(L, wsl, n_a, n_b, n_path);
            i = at[0]; j = at[1];
        }
        const int lead = i + j;                                         // the path begins along row 0 (insertions) or column 0 (deletions)
        const signed char first = i > 0 ? 2 : 3;
        for (long long x = lane; x < room; x += 64) ops[of0 + x] = x < lead ? first : x < n_path ? sops[x] : (signed char)-1;
    }
}

namespace {
// sum over h < g of K_h^2 (a K outside 1 .. 128 counts 0): where group g's matrix starts; in every lane
__device__ long long ed_group_offset(const long long* groups, int g)
{
    long long acc = 0;
    if (g <= 64) {                                                      // a short table: every lane reads it whole (uniform loads), no exchange
        for (int h = 0; h < g; ++h) {
            const long long K = groups[2 * h + 1];
            if (K >= 1 && K <= ED_MAX_K) acc += K * K;
        }
        return acc;
    }
    for (int h = threadIdx.x; h < g; h += 64) {
        const long long K = groups[2 * h + 1];
        if (K >= 1 && K <= ED_MAX_K) acc += K * K;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    return acc;
}
}

// launch 1 of ss_nbest_risk: workgroup (c, g) owns cell c = i K + k of group g; i < k computes and writes both halves, i == k the diagonal
__global__ __launch_bounds__(64) void nbest_dmat_kernel(const int* tokens, long long n_tokens, const long long* seqs, long long n_seq, const long long* groups,
                                                        int* dmat, long long n_dmat)
{
    __shared__ int sa[ED_MAX_LEN + 1];
    const int lane = threadIdx.x, g = blockIdx.y;
    const long long first = groups[2 * g], Kl = groups[2 * g + 1];
    if (Kl < 1 || Kl > ED_MAX_K) return;
    const int K = (int)Kl, c = blockIdx.x;
    if (c >= K * K) return;
    const int i = c / K, k = c - i * K;
    if (i > k) return;
    const long long off = ed_group_offset(groups, g);
    if (off > n_dmat - K * K) return;
    const bool gok = first >= 0 && first <= n_seq - K;
    EdSeq A = {0, 0, false}, B = A;
    if (gok) { A = ed_seq(seqs, n_seq, n_tokens, first + i); B = ed_seq(seqs, n_seq, n_tokens, first + k); }
    if (i == k) {
        if (lane == 0) dmat[off + (long long)i * K + i] = A.ok ? 0 : -1;
        return;
    }
    int d = -1;
    if (A.ok && B.ok) {
        ed_stage(sa, tokens + A.first, A.len);
        d = (A.len > 0 && B.len > 0 ? ed_dispatch_forward<false>(sa, A.len, tokens + B.first, B.len, nullptr) : (A.len + B.len) * ED_ONE) >> 11;
    }
    if (lane == 0) { dmat[off + (long long)i * K + k] = d; dmat[off + (long long)k * K + i] = d; }
}

// launch 2: one wave per group; risk in f64, ascending k; the smallest index of least risk
__global__ __launch_bounds__(64) void nbest_risk_kernel(const long long* groups, long long n_seq, const float* weights, const int* dmat, long long n_dmat,
                                                        double* risk, int* pick)
{
    const int lane = threadIdx.x, g = blockIdx.x;
    const long long first = groups[2 * g], Kl = groups[2 * g + 1];
    if (Kl < 1 || Kl > ED_MAX_K) { if (lane == 0) pick[g] = -1; return; }
    const int K = (int)Kl;
    const long long off = ed_group_offset(groups, g);
    const bool gok = first >= 0 && first <= n_seq - K;
    if (!gok || off > n_dmat - K * K) { if (lane == 0) pick[g] = -1; if (gok) for (int r = lane; r < K; r += 64) risk[first + r] = __builtin_nan(""); return; }
    const int* D = dmat + off;
    const float* w = weights + first;
    double acc[2] = {0.0, 0.0};
    int bad = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = lane + 64 * h;
        if (r < K) {
            double a = 0.0;
            for (int k = 0; k < K; ++k) {
                const int d = D[r * K + k];
                if (d < 0) bad = 1;
                a += (double)w[k] * (double)d;
            }
            if (a != a) bad = 1;
            acc[h] = a;
        }
    }
    bad = __any(bad);
    if (bad) {
        for (int r = lane; r < K; r += 64) risk[first + r] = __builtin_nan("");
        if (lane == 0) pick[g] = -1;
        return;
    }
    double best = __builtin_inf();
    int idx = 0x7fffffff;
    if (lane < K) { risk[first + lane] = acc[0]; best = acc[0]; idx = lane; }
    if (lane + 64 < K) { risk[first + lane + 64] = acc[1]; if (acc[1] < best) { best = acc[1]; idx = lane + 64; } }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ob = __shfl_xor(best, m);
        const int oi = __shfl_xor(idx, m);
        if (ob < best || (ob == best && oi < idx)) { best = ob; idx = oi; }
    }
    if (lane == 0) pick[g] = idx;
}

extern "C" int64_t ss_edit_distance_workspace_bytes(int64_t n_pairs, int64_t n_ops)
{
    if (n_pairs < 0 || n_pairs > ED_MAX_PAIRS || n_ops < 0 || n_ops > ED_MAX_PAIRS * 2 * ED_MAX_LEN) return -1;
    return 256 * (n_ops + 64 * n_pairs);
}

extern "C" int ss_edit_distance(const int32_t* tokens, int64_t n_tokens, const int64_t* seqs, int64_t n_seq, const int32_t* pairs, int64_t n_pairs,
                                int32_t* dist, int32_t* counts, int8_t* ops, const int64_t* ops_first, int64_t n_ops, void* workspace, void* stream)
{
    SS_CHECK(n_tokens >= 0 && n_seq >= 0 && n_pairs >= 0 && n_ops >= 0, "ss_edit_distance: negative sizes");
    SS_CHECK(n_pairs <= ED_MAX_PAIRS, "ss_edit_distance: %lld pairs (at most %lld in one launch)", (long long)n_pairs, ED_MAX_PAIRS);
    SS_CHECK(n_ops <= ED_MAX_PAIRS * 2 * ED_MAX_LEN, "ss_edit_distance: %lld alignment bytes", (long long)n_ops);
    if (n_pairs == 0) return 0;
    SS_CHECK(pairs && dist && counts && (n_seq == 0 || seqs) && (n_tokens == 0 || tokens), "ss_edit_distance: null pointer");
    SS_CHECK(!ops_first || ((ops || n_ops == 0) && workspace), "ss_edit_distance: the alignment needs ops, ops_first and a workspace");
    if (ops_first)
        SS_LAUNCH(SS_KERNEL(edit_distance_kernel<true>), dim3((unsigned)n_pairs), dim3(64), 0, stream, (const int*)tokens, (long long)n_tokens, (const long long*)seqs,
                  (long long)n_seq, (const int*)pairs, (int*)dist, (int*)counts, (signed char*)ops, (const long long*)ops_first, (long long)n_ops, (unsigned*)workspace);
    else
        SS_LAUNCH(SS_KERNEL(edit_distance_kernel<false>), dim3((unsigned)n_pairs), dim3(64), 0, stream, (const int*)tokens, (long long)n_tokens, (const long long*)seqs,
                  (long long)n_seq, (const int*)pairs, (int*)dist, (int*)counts, (signed char*)nullptr, (const long long*)nullptr, 0ll, (unsigned*)nullptr);
    SS_LAUNCH_CHECK("ss_edit_distance");
    return 0;
}

extern "C" int ss_nbest_risk(const int32_t* tokens, int64_t n_tokens, const int64_t* seqs, int64_t n_seq, const int64_t* groups, int n_groups, int max_k,
                             const float* weights, int32_t* dmat, int64_t n_dmat, double* risk, int32_t* pick, void* stream)
{
    SS_CHECK(n_tokens >= 0 && n_seq >= 0 && n_groups >= 0 && n_dmat >= 0, "ss_nbest_risk: negative sizes");
    SS_CHECK(n_groups <= ED_MAX_GROUPS, "ss_nbest_risk: %d groups (at most %d in one call)", n_groups, ED_MAX_GROUPS);
    SS_CHECK(max_k >= 1 && max_k <= ED_MAX_K, "ss_nbest_risk: groups of up to %d sequences (1 .. %d)", max_k, ED_MAX_K);
    if (n_groups == 0) return 0;
    SS_CHECK(groups && pick && (n_dmat == 0 || dmat) && (n_seq == 0 || (seqs && weights && risk)) && (n_tokens == 0 || tokens), "ss_nbest_risk: null pointer");
    SS_LAUNCH(SS_KERNEL(nbest_dmat_kernel), dim3((unsigned)(max_k * max_k), (unsigned)n_groups), dim3(64), 0, stream, (const int*)tokens, (long long)n_tokens,
              (const long long*)seqs, (long long)n_seq, (const long long*)groups, (int*)dmat, (long long)n_dmat);
    SS_LAUNCH_CHECK("ss_nbest_risk (distances)");
    SS_LAUNCH(SS_KERNEL(nbest_risk_kernel), dim3((unsigned)n_groups), dim3(64), 0, stream, (const long long*)groups, (long long)n_seq, weights, (const int*)dmat,
              (long long)n_dmat, risk, (int*)pick);
    SS_LAUNCH_CHECK("ss_nbest_risk");
    return 0;
}
