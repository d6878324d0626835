// ctc_decode.hip -- CTC prefix beam search of the recognition model on gfx950, with shallow fusion of a label n-gram table ("next" row N1; the
// reference decodes with ctcdecode's beam search, recognition_model.py:33-35,48-49).  The algorithm is the one include/silent_speech_hip.h states
// for ss_ctc_beam_search; tests/ctc_beam_oracle.py restates it in plain Python and shares no code with this file.
//
// One launch decodes the batch, ONE WORKGROUP (256 threads) PER UTTERANCE, the frames of an utterance in sequence inside it; nothing goes back to the
// host between frames and the utterance lengths are read on the device.
//   beam     up to W entries, double-buffered in LDS: lb / lnb (log mass of the prefix's paths that end / do not end in blank), the accumulated LM
//            score, the last two labels (repeat rule, trigram context), the prefix length, its trie node, and two 64-bit fingerprints: of the prefix
//            and of the prefix without its last label.
//   merging  a candidate p + c is the SAME prefix as a beam entry q exactly when q without its last label is p and last(q) = c.  Per frame every
//            entry q looks its parent up among the entries (length and fingerprint, W LDS reads); if it is there, p's extension by last(q) is folded
//            into q's lnb' and suppressed as a new prefix.  (A parent slot carried along from the extension that made q is not enough: p can be
//            pruned while q survives and re-enter the beam later through p's own parent.)  Two different prefixes of one length sharing a 64-bit
//            fingerprint would be merged wrongly; at < 2^14 comparisons per frame that is below 1e-12 per utterance.
//   select   the W best of the Wc * V candidates: their scores as order-preserving 32-bit keys in LDS, a radix select (4 passes of an 8-bit
//            histogram in LDS, integer atomics) finds the W-th largest key, then everything above it and the first ties IN CANDIDATE ORDER
//            (index p * V + c) are compacted with a prefix sum -- deterministic, no sort.  Only the final n_best are ranked.
//   strings  a trie in the global workspace, node = (parent node, label); an extension that enters the beam in frame t as slot s gets node
//            1 + t W + s, so at most W nodes appear per frame and ids need no allocator.  The final walk to the root takes at most T steps and
//            leaves the utterance's node range never, whatever the workspace holds.
// Arithmetic: natural-log f32 like the oracle's f32 mode, log-add-exp through the hardware exp2 / log2.
#include "common.h"
#include "silent_speech_hip.h"
#include <math.h>

namespace {
constexpr int BS_THREADS = 256, BS_MAX_W = 128, BS_MAX_V = 128;
constexpr float BS_LOG2E = 1.4426950408889634f, BS_LN2 = 0.6931471805599453f;
typedef unsigned long long bs_u64;

// ln(e^a + e^b); -inf is a real -inf here (exp2(-inf) = 0), only "both -inf" needs the guard
__device__ __forceinline__ float bs_lae(float a, float b) {
    const float m = fmaxf(a, b), lo = fminf(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + BS_LN2 * fast_log2(1.f + fast_exp2((lo - m) * BS_LOG2E));
}
// order-preserving key of a score; 0 = "this candidate does not exist" (score -inf or NaN), every existing one is > 0x007fffff
__device__ __forceinline__ unsigned bs_key(float s) {
    if (!(s > -INFINITY)) return 0u;
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ bs_u64 bs_mix(bs_u64 h, int c) {       // splitmix64 finaliser over (fingerprint of p, label)
    bs_u64 x = h + 0x9E3779B97F4A7C15ull * (bs_u64)(c + 1);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
// LDS words (4 bytes) for beam width W and V classes -- the host check and the kernel's carve-up below follow the same list
__host__ __device__ inline size_t bs_lds_words(int W, int V) { return (size_t)26 * W + V + 512 + 16 + (size_t)W * V; }

struct BsBeam {                                                    // the two beam buffers, [2][W] each
    bs_u64 *h, *hp; float *lb, *lnb, *lm; int *last, *ctx2, *node, *len;
};
struct BsLm { const float* tab; float a, b; int blank, C; };
__device__ __forceinline__ int bs_label(int c, int blank) { return c - (c > blank ? 1 : 0); }      // class -> label number (blank skipped)
// q = p + c: its lnb' contribution and its LM score
__device__ __forceinline__ void bs_extend(const BsBeam& B, int op, const float* tot, int p, const float* lp, int c, const BsLm& L, float& v, float& l) {
    const int lastp = B.last[op];
    v = (c == lastp ? B.lb[op] : tot[p]) + lp[c];
    l = B.lm[op];
    if (L.tab) {
        const int c2 = B.ctx2[op], i2 = c2 < 0 ? L.C : bs_label(c2, L.blank), i1 = lastp < 0 ? L.C : bs_label(lastp, L.blank);
        l += L.a * L.tab[((long long)i2 * (L.C + 1) + i1) * L.C + bs_label(c, L.blank)] + L.b;
    }
}
}

__global__ __launch_bounds__(BS_THREADS) void ctc_beam_kernel(const float* __restrict__ logits, long long ld, int V, int blank, long long rows,
                                                              const float* __restrict__ lse, const long long* __restrict__ utt, long long total_frames, int W,
                                                              int n_best, const float* __restrict__ lmtab, float lm_a, float lm_b, int* __restrict__ trie, int L_max,
                                                              int* __restrict__ labels, int* __restrict__ lengths, float* __restrict__ scores, float* __restrict__ ctc_scores)
{
    SS_DYN_SMEM(smem);
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    BsBeam B;
    B.h = (bs_u64*)smem; B.hp = B.h + 2 * W;
    B.lb = (float*)(B.hp + 2 * W); B.lnb = B.lb + 2 * W; B.lm = B.lnb + 2 * W;
    B.last = (int*)(B.lm + 2 * W); B.ctx2 = B.last + 2 * W; B.node = B.ctx2 + 2 * W; B.len = B.node + 2 * W;
    float* tot = (float*)(B.len + 2 * W); float* nlb = tot + W; float* nlnb = nlb + W;
    int* pslot = (int*)(nlnb + W);
    float* lp = (float*)(pslot + W);
    int* hist = (int*)(lp + V);                                          // [2][256]
    int* wsum = hist + 512; int* st = wsum + 8;                          // st: 0 key prefix found so far, 1 rank still wanted below it, 2 "all candidates survive"
    unsigned* key = (unsigned*)(st + 8);                                 // [W * V]
    const BsLm L = {lmtab, lm_a, lm_b, blank, V - 1};

    // this utterance's frames and its trie range; whatever the table holds, the frames read stay inside [0, rows) and the nodes inside the workspace
    long long off = 0;
    for (int j = 0; j < u; ++j) { long long n = utt[2 * j + 1]; if (n < 0) n = 0; if (n > total_frames - off) n = total_frames - off; off += n; }
    long long f0 = utt[2 * u], Tl = utt[2 * u + 1];
    if (Tl < 0) Tl = 0;
    if (Tl > total_frames - off) Tl = total_frames - off;
    if (f0 < 0 || f0 > rows || Tl > rows - f0) Tl = 0;
    const int T = (int)Tl;
    int* tr = trie + 2 * (off * W + u);                                  // nodes 0 (the root, never written) .. T W
    const long long out0 = (long long)u * n_best;

    int cur = 0, Wc = 1;
    if (tid == 0) { B.h[0] = 0x5851F42D4C957F2Dull; B.hp[0] = 0; B.lb[0] = 0.f; B.lnb[0] = -INFINITY; B.lm[0] = 0.f; B.last[0] = -1; B.ctx2[0] = -1; B.node[0] = 0; B.len[0] = 0; }
    for (long long i = tid; i < (long long)n_best * L_max; i += BS_THREADS) labels[out0 * L_max + i] = -1;
    const int cl = tid - 128;                                            // the upper two waves fetch the frame's log-probabilities, one frame ahead
    const bool loader = cl >= 0 && cl < V;
    float nx = 0.f, nl = 0.f;                                            // logit and lse of the next frame: used (and waited for) one frame later
    if (loader && T > 0) { nx = logits[f0 * ld + cl]; nl = lse[f0]; }
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const int o = cur * W, n = (cur ^ 1) * W, N = Wc * V;
        // ---- A: log-probabilities of the frame; per entry its total and the slot of its parent prefix
        if (loader) { lp[cl] = nx - nl; if (t + 1 < T) { nx = logits[(f0 + t + 1) * ld + cl]; nl = lse[f0 + t + 1]; } }
        if (tid < Wc) {
            tot[tid] = bs_lae(B.lb[o + tid], B.lnb[o + tid]);
            const bs_u64 want = B.hp[o + tid]; const int wl = B.len[o + tid] - 1;
            int ps = -1;
            for (int j = 0; j < Wc; ++j) if (B.len[o + j] == wl && B.h[o + j] == want) ps = j;
            pslot[tid] = ps;
        }
        __syncthreads();
        // ---- B: keys of the extensions.  A thread owns the candidates [i0, i1) (an odd chunk: consecutive lanes on different banks) through all phases
        const int chunk = ((N + BS_THREADS - 1) / BS_THREADS) | 1;
        const int i0 = tid * chunk < N ? tid * chunk : N, i1 = i0 + chunk < N ? i0 + chunk : N;
        const int p0 = i0 / V, c0 = i0 - p0 * V;
        for (int i = i0, p = p0, c = c0; i < i1; ++i) {
            if (c != blank) { float v, l; bs_extend(B, o + p, tot, p, lp, c, L, v, l); key[i] = bs_key(v + l); }
            if (++c == V) { c = 0; ++p; }
        }
        __syncthreads();
        // ---- C: the entries themselves ("stay"), with the parent's extension folded in and suppressed
        if (tid < Wc) {
            const int p = tid, c = B.last[o + p], pp = pslot[p];
            const float a = tot[p] + lp[blank];
            float b = c >= 0 ? B.lnb[o + p] + lp[c] : -INFINITY;
            if (pp >= 0) { b = bs_lae(b, (c == B.last[o + pp] ? B.lb[o + pp] : tot[pp]) + lp[c]); key[pp * V + c] = 0u; }
            nlb[p] = a; nlnb[p] = b;
            key[p * V + blank] = bs_key(bs_lae(a, b) + B.lm[o + p]);
        }
        hist[tid] = 0; hist[256 + tid] = 0;
        if (tid == 0) { st[0] = 0; st[1] = W; st[2] = 0; }
        __syncthreads();
        // ---- radix select: the key of rank W (st[0]) and how many of its ties are taken (st[1])
        for (int d = 0; d < 4; ++d) {
            int* hd = hist + (d & 1) * 256;
            const unsigned prefix = (unsigned)st[0]; const int sh = 24 - 8 * d;
            for (int i = i0; i < i1; ++i) { const unsigned k = key[i]; if (k && (d == 0 || (k >> (sh + 8)) == prefix)) atomicAdd(&hd[(k >> sh) & 255u], 1); }
            if (d > 0) hist[((d + 1) & 1) * 256 + tid] = 0;
            __syncthreads();
            if (wave == 0) {                                              // lane l: digits 4 l .. 4 l + 3; suffix sums over the lanes
                const int b0 = hd[4 * lane], b1 = hd[4 * lane + 1], b2 = hd[4 * lane + 2], b3 = hd[4 * lane + 3], s = b0 + b1 + b2 + b3;
                const int rem = st[1];                                    // every lane has read it before the owner of the digit rewrites it below
                int suf = s;
                for (int sft = 1; sft < 64; sft <<= 1) { const int v = __shfl_down(suf, sft); if (lane + sft < 64) suf += v; }
                const int total = __shfl(suf, 0), above = suf - s;
                if (d == 0 && total <= W) { if (lane == 0) { st[0] = 0; st[1] = 0; st[2] = 1; } }
                else if (above < rem && rem <= suf) {
                    int dg = 3, ab = above;
                    if (rem > ab + b3) { ab += b3; dg = 2; if (rem > ab + b2) { ab += b2; dg = 1; if (rem > ab + b1) { ab += b1; dg = 0; } } }
                    st[0] = (int)((prefix << 8) | (unsigned)(4 * lane + dg)); st[1] = rem - ab;
                }
            }
            __syncthreads();
            if (st[2]) break;
        }
        const unsigned K = (unsigned)st[0]; const int rem = st[1];
        // ---- compaction in candidate order
        int gt = 0, eq = 0;
        for (int i = i0; i < i1; ++i) { const unsigned k = key[i]; gt += k > K; eq += k == K; }
        const int pk = gt | (eq << 16);
        int x = pk;
        for (int sft = 1; sft < 64; sft <<= 1) { const int v = __shfl_up(x, sft); if (lane >= sft) x += v; }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        int base = 0, all = 0;
        for (int w = 0; w < BS_THREADS / 64; ++w) { const int v = wsum[w]; if (w < wave) base += v; all += v; }
        const int before = base + x - pk;
        int eqr = before >> 16, slot = (before & 0xffff) + (eqr < rem ? eqr : rem);
        const int Wn = (all & 0xffff) + ((all >> 16) < rem ? (all >> 16) : rem);
        for (int i = i0, p = p0, c = c0; i < i1; ++i) {
            const unsigned k = key[i];
            const bool take = k > K || (k == K && eqr < rem);
            if (k == K) ++eqr;
            if (take && slot < W) {
                const int s = n + slot, op = o + p;
                if (c == blank) {
                    B.h[s] = B.h[op]; B.hp[s] = B.hp[op]; B.lb[s] = nlb[p]; B.lnb[s] = nlnb[p]; B.lm[s] = B.lm[op];
                    B.last[s] = B.last[op]; B.ctx2[s] = B.ctx2[op]; B.node[s] = B.node[op]; B.len[s] = B.len[op];
                } else {
                    float v, l; bs_extend(B, op, tot, p, lp, c, L, v, l);
                    const int id = 1 + t * W + slot;
                    B.h[s] = bs_mix(B.h[op], c); B.hp[s] = B.h[op]; B.lb[s] = -INFINITY; B.lnb[s] = v; B.lm[s] = l;
                    B.last[s] = c; B.ctx2[s] = B.last[op]; B.node[s] = id; B.len[s] = B.len[op] + 1;
                    tr[2 * (long long)id] = B.node[op]; tr[2 * (long long)id + 1] = c;
                }
                ++slot;
            }
            if (++c == V) { c = 0; ++p; }
        }
        __syncthreads();
        cur ^= 1; Wc = Wn < W ? Wn : W;
    }

    // ---- the n_best best of the last beam, best first (ties: beam slot), and their strings
    const int o = cur * W;
    float cs = -INFINITY, sc = -INFINITY;
    if (tid < Wc) { cs = bs_lae(B.lb[o + tid], B.lnb[o + tid]); sc = cs + B.lm[o + tid]; }
    if (tid < W) key[tid] = tid < Wc ? bs_key(sc) : 0u;
    __syncthreads();
    if (tid < Wc) {
        const unsigned k = key[tid];
        int rank = 0;
        for (int j = 0; j < Wc; ++j) { const unsigned kj = key[j]; rank += kj > k || (kj == k && j < tid); }
        if (rank < n_best) {
            const int len = B.len[o + tid];
            lengths[out0 + rank] = len; scores[out0 + rank] = sc; ctc_scores[out0 + rank] = cs;
            int* lab = labels + (out0 + rank) * L_max;
            const long long last_id = (long long)T * W;
            int nd = B.node[o + tid];
            for (int s = 0; s < T && nd > 0 && nd <= last_id; ++s) {
                const int pos = len - 1 - s, par = tr[2 * (long long)nd], c = tr[2 * (long long)nd + 1];
                if (pos >= 0 && pos < L_max) lab[pos] = c;
                nd = par;
            }
        }
    } else if (tid < n_best) { lengths[out0 + tid] = -1; scores[out0 + tid] = -INFINITY; ctc_scores[out0 + tid] = -INFINITY; }
}

extern "C" int64_t ss_ctc_beam_workspace_bytes(int n_utt, int64_t total_frames, int beam_width)
{
    if (n_utt < 0 || total_frames < 0 || beam_width < 1 || beam_width > BS_MAX_W) return -1;
    return 8 * (total_frames * beam_width + n_utt + 1);
}

extern "C" int ss_ctc_beam_search(const float* logits, int64_t ld, int V, int blank, int64_t rows, const float* lse, const int64_t* utt_dev, int n_utt,
                                  int64_t total_frames, int beam_width, int n_best, const float* lm, float alpha, float beta, void* workspace, int max_len,
                                  int32_t* labels, int32_t* lengths, float* scores, float* ctc_scores, void* stream)
{
    SS_CHECK(V >= 1 && V <= BS_MAX_V, "ss_ctc_beam_search: %d classes (1 .. %d)", V, BS_MAX_V);
    SS_CHECK(blank >= 0 && blank < V && ld >= V, "ss_ctc_beam_search: bad blank %d / row stride %lld for %d classes", blank, (long long)ld, V);
    SS_CHECK(beam_width >= 1 && beam_width <= BS_MAX_W, "ss_ctc_beam_search: beam width %d (1 .. %d)", beam_width, BS_MAX_W);
    SS_CHECK(n_best >= 1 && n_best <= beam_width, "ss_ctc_beam_search: n_best %d (1 .. beam width %d)", n_best, beam_width);
    SS_CHECK(n_utt >= 0 && rows >= 0 && total_frames >= 0 && max_len >= 1, "ss_ctc_beam_search: negative sizes");
    SS_CHECK(total_frames * beam_width + n_utt < 0x7fffffffll / 2, "ss_ctc_beam_search: %lld frames at width %d exceed the 32-bit node ids", (long long)total_frames, beam_width);
    if (n_utt == 0) return 0;
    SS_CHECK(logits && lse && utt_dev && workspace && labels && lengths && scores && ctc_scores, "ss_ctc_beam_search: null pointer");
    const size_t smem = 4 * bs_lds_words(beam_width, V);
    SS_CHECK(smem <= 160 * 1024, "ss_ctc_beam_search: %zu bytes of LDS needed", smem);
    static size_t granted = 0;
    if (granted < smem) { if (!ss_grant_lds((const void*)ctc_beam_kernel, smem)) { ss_set_error("ss_ctc_beam_search: cannot reserve %zu bytes of LDS", smem); return 1; } granted = smem; }
    SS_LAUNCH(ctc_beam_kernel, dim3(n_utt), dim3(BS_THREADS), smem, stream, logits, (long long)ld, V, blank, (long long)rows, lse, (const long long*)utt_dev,
              (long long)total_frames, beam_width, n_best, lm, alpha, beta, (int*)workspace, max_len, (int*)labels, (int*)lengths, scores, ctc_scores);
    SS_LAUNCH_CHECK("ss_ctc_beam_search");
    return 0;
}
