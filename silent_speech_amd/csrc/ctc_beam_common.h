// ctc_beam_common.h -- what the CTC decoders share: the frame loop and the final ranking of the two prefix beam searches (ctc_decode.hip: label n-gram
// table; ctc_word_decode.hip: lexicon and word n-gram), their arithmetic helpers and host-side checks, and the clamped walk of the utterance table
// that ctc_align.hip uses as well.  ONE definition of each; a search supplies a Policy (below) and nothing else.
//
// One launch decodes the batch, ONE WORKGROUP (256 threads) PER UTTERANCE, the frames of an utterance in sequence inside it; nothing goes back to the
// host between frames and the utterance lengths are read on the device.
//   beam     up to W entries, double-buffered in LDS.  The core fields (CbBeam): lb / lnb (log mass of the prefix's paths that end / do not end in
//            blank), the accumulated LM score, the last label (repeat rule), the prefix length, its trie node, and two 64-bit fingerprints: of the
//            prefix and of the prefix without its last label.  A policy adds its own fields per entry.
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
//   loading  the upper two waves fetch the frame's logits and lse one frame ahead.
// Arithmetic: natural-log f32 like the oracles' f32 mode, log-add-exp through the hardware exp2 / log2.
//
// A Policy is a struct the kernel fills and hands to cb_search; every call is resolved at compile time and inlined:
//   static constexpr int EXTRA                     its 4-byte fields per beam entry: LDS bytes = 4 cb_lds_words(EXTRA, W, V)
//   static constexpr bool REPORTS_COMPLETE         whether the `complete` output exists
//   struct Fields                                  its fields of one entry, in registers
//   void carve(int* x, int W)                      takes its [2][W] arrays from the 2 EXTRA W words at x
//   Fields root() const                            its fields of the empty prefix
//   Fields load(e) const / void store(e, f)        entry e's fields out of / into LDS
//   unsigned extension_key(B, op, c, v) const      phase B: the key of entry op extended by class c (never the blank), v = the extension's lnb';
//                                                  0 = no such candidate
//   Fields extend(B, op, c, lm) const              compaction: the fields of the new entry op + c, and its LM score in lm; reads, stores nothing
//   void final(B, e, cs, sc, done) const           ranking: from the CTC score cs of entry e its score and whether it is complete (complete entries
//                                                  rank first; a policy without the notion says 1 for all)
#pragma once
#include "common.h"
#include <math.h>

namespace {
// ------------------------------------------------------------------ the utterance table (beam searches and ctc_align.hip; needs nothing below)
// Frames of entry j of an utterance table (`stride` int64 per entry: first frame, frames, ...) and its first frame, clamped: `off` (the frames of the
// entries before it) is advanced, and whatever the table holds the result stays inside the workspace (total_frames) and inside [0, rows).
__device__ __forceinline__ int ctc_utt_frames(const long long* utt, int stride, int j, long long total_frames, long long rows, long long& off, long long& f0) {
    f0 = utt[stride * j];
    long long n = utt[stride * j + 1];
    const long long room = total_frames - off;
    if (n < 0) n = 0;
    if (n > room) n = room;
    off += n;
    if (f0 < 0 || f0 > rows || n > rows - f0) n = 0;
    return (int)n;
}
// The same for entry u from the start of the table: `off` = the frames of the entries before u
__device__ __forceinline__ int ctc_utt_locate(const long long* utt, int stride, int u, long long total_frames, long long rows, long long& off, long long& f0) {
    long long at = 0;
    for (int j = 0; j < u; ++j) ctc_utt_frames(utt, stride, j, total_frames, rows, at, f0);
    off = at;
    return ctc_utt_frames(utt, stride, u, total_frames, rows, at, f0);
}

// ------------------------------------------------------------------ the beam searches
constexpr int CB_THREADS = 256, CB_MAX_W = 128, CB_MAX_V = 128;
constexpr float CB_LOG2E = 1.4426950408889634f, CB_LN2 = 0.6931471805599453f;
typedef unsigned long long cb_u64;

// ln(e^a + e^b); -inf is a real -inf here (exp2(-inf) = 0), only "both -inf" needs the guard
__device__ __forceinline__ float cb_lae(float a, float b) {
    const float m = fmaxf(a, b), lo = fminf(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + CB_LN2 * fast_log2(1.f + fast_exp2((lo - m) * CB_LOG2E));
}
// order-preserving key of a score; 0 = "this candidate does not exist" (score -inf or NaN), every existing one is > 0x007fffff
__device__ __forceinline__ unsigned cb_key(float s) {
    if (!(s > -INFINITY)) return 0u;
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ cb_u64 cb_fin(cb_u64 x) {              // splitmix64 finaliser
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
__device__ __forceinline__ cb_u64 cb_mix(cb_u64 h, int c) { return cb_fin(h + 0x9E3779B97F4A7C15ull * (cb_u64)(c + 1)); }    // fingerprint of p + c
__device__ __forceinline__ int cb_label(int c, int blank) { return c - (c > blank ? 1 : 0); }      // class -> label number (blank skipped)

// LDS words (4 bytes) for beam width W, V classes and a policy of `extra` fields -- the host check and cb_search's carve-up follow the same list
inline size_t cb_lds_words(int extra, int W, int V) { return (size_t)(24 + 2 * extra) * W + V + 512 + 16 + (size_t)W * V; }

struct CbBeam {                                                    // the core fields of the two beam buffers, [2][W] each
    cb_u64 *h, *hp; float *lb, *lnb, *lm; int *last, *node, *len;
};
struct CbArgs {
    const float* logits; long long ld; int V, blank; long long rows; const float* lse; const long long* utt; long long total_frames; int W, n_best;
    int* trie; int L_max; int* labels; int* lengths; float* scores; float* ctc_scores; int* complete;
};

template <class Policy>
__device__ __forceinline__ void cb_search(Policy& P, const CbArgs& a)
{
    SS_DYN_SMEM(smem);
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = a.V, W = a.W, blank = a.blank, n_best = a.n_best, L_max = a.L_max;
    const float* logits = a.logits; const float* lse = a.lse; const long long ld = a.ld;
    CbBeam B;
    B.h = (cb_u64*)smem; B.hp = B.h + 2 * W;
    B.lb = (float*)(B.hp + 2 * W); B.lnb = B.lb + 2 * W; B.lm = B.lnb + 2 * W;
    B.last = (int*)(B.lm + 2 * W);
    int* extra = B.last + 2 * W;                                         // the policy's fields sit between the core's
    P.carve(extra, W);
    B.node = extra + 2 * Policy::EXTRA * W; B.len = B.node + 2 * W;
    float* tot = (float*)(B.len + 2 * W); float* nlb = tot + W; float* nlnb = nlb + W;
    int* pslot = (int*)(nlnb + W);
    float* lp = (float*)(pslot + W);
    int* hist = (int*)(lp + V);                                          // [2][256]
    int* wsum = hist + 512; int* st = wsum + 8;                          // st: 0 key prefix found so far, 1 rank still wanted below it, 2 "all candidates survive"
    unsigned* key = (unsigned*)(st + 8);                                 // [W * V]

    // this utterance's frames and its trie range; whatever the table holds, the frames read stay inside [0, rows) and the nodes inside the workspace
    long long off, f0;
    const int T = ctc_utt_locate(a.utt, 2, u, a.total_frames, a.rows, off, f0);
    int* tr = a.trie + 2 * (off * W + u);                                // nodes 0 (the root, never written) .. T W
    const long long out0 = (long long)u * n_best;

    int cur = 0, Wc = 1;
    if (tid == 0) { B.h[0] = 0x5851F42D4C957F2Dull; B.hp[0] = 0; B.lb[0] = 0.f; B.lnb[0] = -INFINITY; B.lm[0] = 0.f; B.last[0] = -1; B.node[0] = 0; B.len[0] = 0; P.store(0, P.root()); }
    for (long long i = tid; i < (long long)n_best * L_max; i += CB_THREADS) a.labels[out0 * L_max + i] = -1;
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
            tot[tid] = cb_lae(B.lb[o + tid], B.lnb[o + tid]);
            const cb_u64 want = B.hp[o + tid]; const int wl = B.len[o + tid] - 1;
            int ps = -1;
            for (int j = 0; j < Wc; ++j) if (B.len[o + j] == wl && B.h[o + j] == want) ps = j;
            pslot[tid] = ps;
        }
        __syncthreads();
        // ---- B: keys of the extensions.  A thread owns the candidates [i0, i1) (an odd chunk: consecutive lanes on different banks) through all phases
        const int chunk = ((N + CB_THREADS - 1) / CB_THREADS) | 1;
        const int i0 = tid * chunk < N ? tid * chunk : N, i1 = i0 + chunk < N ? i0 + chunk : N;
        const int p0 = i0 / V, c0 = i0 - p0 * V;
        for (int i = i0, p = p0, c = c0; i < i1; ++i) {
            if (c != blank) { const int op = o + p; key[i] = P.extension_key(B, op, c, (c == B.last[op] ? B.lb[op] : tot[p]) + lp[c]); }
            if (++c == V) { c = 0; ++p; }
        }
        __syncthreads();
        // ---- C: the entries themselves ("stay"), with the parent's extension folded in and suppressed
        if (tid < Wc) {
            const int p = tid, c = B.last[o + p], pp = pslot[p];
            const float sa = tot[p] + lp[blank];
            float sb = c >= 0 ? B.lnb[o + p] + lp[c] : -INFINITY;
            if (pp >= 0) { sb = cb_lae(sb, (c == B.last[o + pp] ? B.lb[o + pp] : tot[pp]) + lp[c]); key[pp * V + c] = 0u; }
            nlb[p] = sa; nlnb[p] = sb;
            key[p * V + blank] = cb_key(cb_lae(sa, sb) + B.lm[o + p]);
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
        // ---- compaction in candidate order; a new entry gets its trie node and the policy's fields here
        int gt = 0, eq = 0;
        for (int i = i0; i < i1; ++i) { const unsigned k = key[i]; gt += k > K; eq += k == K; }
        const int pk = gt | (eq << 16);
        int x = pk;
        for (int sft = 1; sft < 64; sft <<= 1) { const int v = __shfl_up(x, sft); if (lane >= sft) x += v; }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        int base = 0, all = 0;
        for (int w = 0; w < CB_THREADS / 64; ++w) { const int v = wsum[w]; if (w < wave) base += v; all += v; }
        const int before = base + x - pk;
        int eqr = before >> 16, slot = (before & 0xffff) + (eqr < rem ? eqr : rem);
        const int Wn = (all & 0xffff) + ((all >> 16) < rem ? (all >> 16) : rem);
        for (int i = i0, p = p0, c = c0; i < i1; ++i) {
            const unsigned k = key[i];
            const bool take = k > K || (k == K && eqr < rem);
            if (k == K) ++eqr;
            if (take && slot < W) {
                const int s = n + slot, op = o + p;
                // everything of entry op is read (the policy's table reads included) before the first store: no LDS read waits behind a store
                if (c == blank) {
                    const cb_u64 h = B.h[op], hp = B.hp[op]; const float lb = nlb[p], lnb = nlnb[p], lm = B.lm[op];
                    const int last = B.last[op], node = B.node[op], len = B.len[op];
                    const typename Policy::Fields f = P.load(op);
                    B.h[s] = h; B.hp[s] = hp; B.lb[s] = lb; B.lnb[s] = lnb; B.lm[s] = lm;
                    B.last[s] = last; P.store(s, f); B.node[s] = node; B.len[s] = len;
                } else {
                    const float v = (c == B.last[op] ? B.lb[op] : tot[p]) + lp[c];
                    const cb_u64 hp = B.h[op]; const int np = B.node[op], len = B.len[op] + 1;
                    float lm;
                    const typename Policy::Fields f = P.extend(B, op, c, lm);
                    const int id = 1 + t * W + slot;
                    B.h[s] = cb_mix(hp, c); B.hp[s] = hp; B.lb[s] = -INFINITY; B.lnb[s] = v; B.lm[s] = lm;
                    B.last[s] = c; P.store(s, f); B.node[s] = id; B.len[s] = len;
                    tr[2 * (long long)id] = np; tr[2 * (long long)id + 1] = c;
                }
                ++slot;
            }
            if (++c == V) { c = 0; ++p; }
        }
        __syncthreads();
        cur ^= 1; Wc = Wn < W ? Wn : W;
    }

    // ---- the n_best best of the last beam: complete entries first, then by score, ties: beam slot; and their strings
    const int o = cur * W;
    float cs = -INFINITY, sc = -INFINITY;
    int done = 0;
    if (tid < Wc) { cs = cb_lae(B.lb[o + tid], B.lnb[o + tid]); P.final(B, o + tid, cs, sc, done); }
    if (tid < W) { key[tid] = tid < Wc ? cb_key(sc) : 0u; pslot[tid] = done; }
    __syncthreads();
    if (tid < Wc) {
        const unsigned k = key[tid];
        int rank = 0;
        for (int j = 0; j < Wc; ++j) { const unsigned kj = key[j]; const int dj = pslot[j]; rank += dj > done || (dj == done && (kj > k || (kj == k && j < tid))); }
        if (rank < n_best) {
            const int len = B.len[o + tid];
            a.lengths[out0 + rank] = len; a.scores[out0 + rank] = sc; a.ctc_scores[out0 + rank] = cs;
            if constexpr (Policy::REPORTS_COMPLETE) a.complete[out0 + rank] = done;
            int* lab = a.labels + (out0 + rank) * L_max;
            const long long last_id = (long long)T * W;
            int nd = B.node[o + tid];
            for (int s = 0; s < T && nd > 0 && nd <= last_id; ++s) {
                const int pos = len - 1 - s, par = tr[2 * (long long)nd], c = tr[2 * (long long)nd + 1];
                if (pos >= 0 && pos < L_max) lab[pos] = c;
                nd = par;
            }
        }
    } else if (tid < n_best) {
        a.lengths[out0 + tid] = -1; a.scores[out0 + tid] = -INFINITY; a.ctc_scores[out0 + tid] = -INFINITY;
        if constexpr (Policy::REPORTS_COMPLETE) a.complete[out0 + tid] = -1;
    }
}

// ------------------------------------------------------------------ host side
inline int64_t cb_workspace_bytes(int n_utt, int64_t total_frames, int beam_width)
{
    if (n_utt < 0 || total_frames < 0 || beam_width < 1 || beam_width > CB_MAX_W) return -1;
    return 8 * (total_frames * beam_width + n_utt + 1);
}
// the argument checks the two searches share (`who` needs at least v_min classes); *smem = the LDS bytes of a policy with `extra` fields
inline int cb_check_args(const char* who, int v_min, int extra, int64_t ld, int V, int blank, int64_t rows, int n_utt, int64_t total_frames, int beam_width,
                         int n_best, int max_len, size_t* smem)
{
    SS_CHECK(V >= v_min && V <= CB_MAX_V, "%s: %d classes (%d .. %d)", who, V, v_min, CB_MAX_V);
    SS_CHECK(blank >= 0 && blank < V && ld >= V, "%s: bad blank %d / row stride %lld for %d classes", who, blank, (long long)ld, V);
    SS_CHECK(beam_width >= 1 && beam_width <= CB_MAX_W, "%s: beam width %d (1 .. %d)", who, beam_width, CB_MAX_W);
    SS_CHECK(n_best >= 1 && n_best <= beam_width, "%s: n_best %d (1 .. beam width %d)", who, n_best, beam_width);
    SS_CHECK(n_utt >= 0 && rows >= 0 && total_frames >= 0 && max_len >= 1, "%s: negative sizes", who);
    SS_CHECK(total_frames * beam_width + n_utt < 0x7fffffffll / 2, "%s: %lld frames at width %d exceed the 32-bit node ids", who, (long long)total_frames, beam_width);
    *smem = 4 * cb_lds_words(extra, beam_width, V);
    SS_CHECK(*smem <= 160 * 1024, "%s: %zu bytes of LDS needed", who, *smem);
    return 0;
}
}
