// ctc_word_decode.hip -- CTC prefix beam search confined to a lexicon, with a word n-gram with backoff scored at every word end, on gfx950 (what the
// reference's ctcdecode does with a KenLM model, recognition_model.py:33-35; here the model comes from ARPA text or from counts).  The algorithm is
// the one include/silent_speech_hip.h states for ss_ctc_word_beam_search; tests/ctc_word_beam_oracle.py restates it in plain Python and shares no code
// with this file.  The frame loop is that of ctc_decode.hip (one 256-thread workgroup per utterance, the beam double-buffered in LDS, radix select,
// ordered compaction, the string trie in the workspace, loader waves one frame ahead) and is COPIED, not shared, so that the object code of the
// existing search stays what it is.  New per entry:
//   lx       its lexicon node (0 = the root); a letter extension exists only if lex_child[lx][label] is a node -- the row is read from global
//            memory in phase B (a thread's chunk is consecutive classes of one entry, so consecutive addresses);
//   w2, w1   the two words before the one being spelled (-1 = none), wd = the word lx spells (-1 = none);
//   wt       alpha * ln P(wd | w2, w1) + beta, -inf if lx spells no word.  It is computed ONCE, when the entry is created in the compaction phase
//            (wb_lnp: the trigram, the two bigram probes and the two unigram reads are independent and issued together); phase B (the space
//            extension) and the final ranking only read it.
// Every table index is checked against the sizes of ss_word_lm: hash slots are masked (idx & (slots - 1) < slots for ANY slots >= 1), probe
// counts are bounded by the slot counts on the host, child nodes and word ids are range-checked where they are read.
#include "common.h"
#include "silent_speech_hip.h"
#include <math.h>

namespace {
constexpr int WB_THREADS = 256, WB_MAX_W = 128, WB_MAX_V = 128;
constexpr float WB_LOG2E = 1.4426950408889634f, WB_LN2 = 0.6931471805599453f;
typedef unsigned long long wb_u64;
constexpr wb_u64 WB_EMPTY = ~0ull;

// ln(e^a + e^b); -inf is a real -inf here (exp2(-inf) = 0), only "both -inf" needs the guard
__device__ __forceinline__ float wb_lae(float a, float b) {
    const float m = fmaxf(a, b), lo = fminf(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + WB_LN2 * fast_log2(1.f + fast_exp2((lo - m) * WB_LOG2E));
}
// order-preserving key of a score; 0 = "this candidate does not exist" (score -inf or NaN), every existing one is > 0x007fffff
__device__ __forceinline__ unsigned wb_key(float s) {
    if (!(s > -INFINITY)) return 0u;
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ wb_u64 wb_fin(wb_u64 x) {              // splitmix64 finaliser
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
__device__ __forceinline__ wb_u64 wb_mix(wb_u64 h, int c) { return wb_fin(h + 0x9E3779B97F4A7C15ull * (wb_u64)(c + 1)); }    // fingerprint of p + c
__device__ __forceinline__ unsigned wb_home(wb_u64 key) { return (unsigned)wb_fin(key + 0x9E3779B97F4A7C15ull); }           // home slot before masking
// LDS words (4 bytes) for beam width W and V classes -- the host check and the kernel's carve-up below follow the same list
__host__ __device__ inline size_t wb_lds_words(int W, int V) { return (size_t)34 * W + V + 512 + 16 + (size_t)W * V; }
__device__ __forceinline__ int wb_label(int c, int blank) { return c - (c > blank ? 1 : 0); }      // class -> label number (blank skipped)

// ln P(w | w2, w1) by the backoff rule of the header.  The caller guarantees 0 <= w < n_uni and -1 <= w1, w2 < n_uni.
__device__ __forceinline__ float wb_lnp(const ss_word_lm& L, int w2, int w1, int w) {
    const float uw = L.uni_logp[w];
    if (w1 < 0) return uw;
    const float b1 = L.uni_bo[w1];
    const bool bi = L.bi_slots > 0, ctx = bi && w2 >= 0, tri = L.tri_slots > 0 && w2 >= 0;
    const wb_u64 kb = ((wb_u64)w1 << 21) | (wb_u64)w, kc = ((wb_u64)(w2 < 0 ? 0 : w2) << 21) | (wb_u64)w1, kt = ((wb_u64)(w2 < 0 ? 0 : w2) << 42) | kb;
    const unsigned mb = (unsigned)(L.bi_slots - 1), mt = (unsigned)(L.tri_slots - 1);
    const unsigned sb = wb_home(kb), sc = wb_home(kc), st = wb_home(kt);
    int fb = -1, fc = -1, ft = -1;
    bool db = !bi, dc = !ctx, dt = !tri;                              // done: found, met an empty slot, or out of probes
    const int nb = bi ? L.bi_probe : 0, nt = tri ? L.tri_probe : 0, n = nb > nt ? nb : nt;
    for (int j = 0; j < n && !(db && dc && dt); ++j) {
        const unsigned ib = (sb + j) & mb, ic = (sc + j) & mb, it = (st + j) & mt;
        const wb_u64 xb = db || j >= nb ? WB_EMPTY : L.bi_keys[ib];     // three independent loads per step
        const wb_u64 xc = dc || j >= nb ? WB_EMPTY : L.bi_keys[ic];
        const wb_u64 xt = dt || j >= nt ? WB_EMPTY : L.tri_keys[it];
        if (!db) { if (xb == kb) fb = (int)ib; db = xb == kb || xb == WB_EMPTY; }
        if (!dc) { if (xc == kc) fc = (int)ic; dc = xc == kc || xc == WB_EMPTY; }
        if (!dt) { if (xt == kt) ft = (int)it; dt = xt == kt || xt == WB_EMPTY; }
    }
    if (ft >= 0) return L.tri_logp[ft];
    const float p2 = fb >= 0 ? L.bi_logp[fb] : b1 + uw;
    if (w2 < 0) return p2;
    return (fc >= 0 ? L.bi_bo[fc] : 0.f) + p2;
}

struct WbBeam {                                                    // the two beam buffers, [2][W] each
    wb_u64 *h, *hp; float *lb, *lnb, *lm, *wt; int *last, *node, *len, *lx, *wd, *w2, *w1;
};
}

__global__ __launch_bounds__(WB_THREADS) void ctc_word_beam_kernel(const float* __restrict__ logits, long long ld, int V, int blank, int space, long long rows,
                                                                   const float* __restrict__ lse, const long long* __restrict__ utt, long long total_frames, int W,
                                                                   int n_best, ss_word_lm L, float lm_a, float lm_b, int* __restrict__ trie, int L_max,
                                                                   int* __restrict__ labels, int* __restrict__ lengths, float* __restrict__ scores,
                                                                   float* __restrict__ ctc_scores, int* __restrict__ complete)
{
    SS_DYN_SMEM(smem);
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    WbBeam B;
    B.h = (wb_u64*)smem; B.hp = B.h + 2 * W;
    B.lb = (float*)(B.hp + 2 * W); B.lnb = B.lb + 2 * W; B.lm = B.lnb + 2 * W; B.wt = B.lm + 2 * W;
    B.last = (int*)(B.wt + 2 * W); B.node = B.last + 2 * W; B.len = B.node + 2 * W;
    B.lx = B.len + 2 * W; B.wd = B.lx + 2 * W; B.w2 = B.wd + 2 * W; B.w1 = B.w2 + 2 * W;
    float* tot = (float*)(B.w1 + 2 * W); float* nlb = tot + W; float* nlnb = nlb + W;
    int* pslot = (int*)(nlnb + W);
    float* lp = (float*)(pslot + W);
    int* hist = (int*)(lp + V);                                          // [2][256]
    int* wsum = hist + 512; int* st = wsum + 8;                          // st: 0 key prefix found so far, 1 rank still wanted below it, 2 "all candidates survive"
    unsigned* key = (unsigned*)(st + 8);                                 // [W * V]
    const int C = V - 1;

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
    if (tid == 0) {
        B.h[0] = 0x5851F42D4C957F2Dull; B.hp[0] = 0; B.lb[0] = 0.f; B.lnb[0] = -INFINITY; B.lm[0] = 0.f; B.wt[0] = -INFINITY;
        B.last[0] = -1; B.node[0] = 0; B.len[0] = 0; B.lx[0] = 0; B.wd[0] = -1; B.w2[0] = -1; B.w1[0] = L.start;
    }
    for (long long i = tid; i < (long long)n_best * L_max; i += WB_THREADS) labels[out0 * L_max + i] = -1;
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
            tot[tid] = wb_lae(B.lb[o + tid], B.lnb[o + tid]);
            const wb_u64 want = B.hp[o + tid]; const int wl = B.len[o + tid] - 1;
            int ps = -1;
            for (int j = 0; j < Wc; ++j) if (B.len[o + j] == wl && B.h[o + j] == want) ps = j;
            pslot[tid] = ps;
        }
        __syncthreads();
        // ---- B: keys of the extensions.  A thread owns the candidates [i0, i1) (an odd chunk: consecutive lanes on different banks) through all phases
        const int chunk = ((N + WB_THREADS - 1) / WB_THREADS) | 1;
        const int i0 = tid * chunk < N ? tid * chunk : N, i1 = i0 + chunk < N ? i0 + chunk : N;
        const int p0 = i0 / V, c0 = i0 - p0 * V;
        for (int i = i0, p = p0, c = c0; i < i1; ++i) {
            if (c != blank) {
                const int op = o + p;
                const float v = (c == B.last[op] ? B.lb[op] : tot[p]) + lp[c];
                unsigned k;
                if (c == space) k = wb_key(v + (B.lm[op] + B.wt[op]));                      // wt = -inf: the entry spells no word, no candidate
                else { const int ch = L.lex_child[(long long)B.lx[op] * C + wb_label(c, blank)]; k = ch >= 0 && ch < L.n_nodes ? wb_key(v + B.lm[op]) : 0u; }
                key[i] = k;
            }
            if (++c == V) { c = 0; ++p; }
        }
        __syncthreads();
        // ---- C: the entries themselves ("stay"), with the parent's extension folded in and suppressed
        if (tid < Wc) {
            const int p = tid, c = B.last[o + p], pp = pslot[p];
            const float a = tot[p] + lp[blank];
            float b = c >= 0 ? B.lnb[o + p] + lp[c] : -INFINITY;
            if (pp >= 0) { b = wb_lae(b, (c == B.last[o + pp] ? B.lb[o + pp] : tot[pp]) + lp[c]); key[pp * V + c] = 0u; }
            nlb[p] = a; nlnb[p] = b;
            key[p * V + blank] = wb_key(wb_lae(a, b) + B.lm[o + p]);
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
        // ---- compaction in candidate order; a new entry gets its lexicon node, its word context and its cached word term here
        int gt = 0, eq = 0;
        for (int i = i0; i < i1; ++i) { const unsigned k = key[i]; gt += k > K; eq += k == K; }
        const int pk = gt | (eq << 16);
        int x = pk;
        for (int sft = 1; sft < 64; sft <<= 1) { const int v = __shfl_up(x, sft); if (lane >= sft) x += v; }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        int base = 0, all = 0;
        for (int w = 0; w < WB_THREADS / 64; ++w) { const int v = wsum[w]; if (w < wave) base += v; all += v; }
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
                    B.h[s] = B.h[op]; B.hp[s] = B.hp[op]; B.lb[s] = nlb[p]; B.lnb[s] = nlnb[p]; B.lm[s] = B.lm[op]; B.wt[s] = B.wt[op];
                    B.last[s] = B.last[op]; B.node[s] = B.node[op]; B.len[s] = B.len[op];
                    B.lx[s] = B.lx[op]; B.wd[s] = B.wd[op]; B.w2[s] = B.w2[op]; B.w1[s] = B.w1[op];
                } else {
                    const float v = (c == B.last[op] ? B.lb[op] : tot[p]) + lp[c];
                    float l = B.lm[op];
                    int lx = 0, w2 = B.w2[op], w1 = B.w1[op], wd = -1;
                    if (c == space) { l += B.wt[op]; w2 = w1; w1 = B.wd[op]; }
                    else {
                        lx = L.lex_child[(long long)B.lx[op] * C + wb_label(c, blank)];
                        if (lx < 0 || lx >= L.n_nodes) lx = 0;           // (the candidate existed, so this is the node phase B saw)
                        if (lx > 0) { wd = L.lex_word[lx]; if (wd < 0 || wd >= L.n_vocab) wd = -1; }
                    }
                    const int id = 1 + t * W + slot;
                    B.h[s] = wb_mix(B.h[op], c); B.hp[s] = B.h[op]; B.lb[s] = -INFINITY; B.lnb[s] = v; B.lm[s] = l;
                    B.wt[s] = wd >= 0 ? lm_a * wb_lnp(L, w2, w1, wd) + lm_b : -INFINITY;
                    B.last[s] = c; B.node[s] = id; B.len[s] = B.len[op] + 1;
                    B.lx[s] = lx; B.wd[s] = wd; B.w2[s] = w2; B.w1[s] = w1;
                    tr[2 * (long long)id] = B.node[op]; tr[2 * (long long)id + 1] = c;
                }
                ++slot;
            }
            if (++c == V) { c = 0; ++p; }
        }
        __syncthreads();
        cur ^= 1; Wc = Wn < W ? Wn : W;
    }

    // ---- the n_best best of the last beam: complete entries first, then by score (an unfinished last word scored), ties: beam slot
    const int o = cur * W;
    float cs = -INFINITY, sc = -INFINITY;
    int done = 0;
    if (tid < Wc) {
        const float wt = B.wt[o + tid]; const bool word = B.lx[o + tid] != 0 && wt > -INFINITY;
        cs = wb_lae(B.lb[o + tid], B.lnb[o + tid]); sc = cs + (B.lm[o + tid] + (word ? wt : 0.f));
        done = B.lx[o + tid] == 0 || word;
    }
    if (tid < W) { key[tid] = tid < Wc ? wb_key(sc) : 0u; pslot[tid] = done; }
    __syncthreads();
    if (tid < Wc) {
        const unsigned k = key[tid];
        int rank = 0;
        for (int j = 0; j < Wc; ++j) { const unsigned kj = key[j]; const int dj = pslot[j]; rank += dj > done || (dj == done && (kj > k || (kj == k && j < tid))); }
        if (rank < n_best) {
            const int len = B.len[o + tid];
            lengths[out0 + rank] = len; scores[out0 + rank] = sc; ctc_scores[out0 + rank] = cs; complete[out0 + rank] = done;
            int* lab = labels + (out0 + rank) * L_max;
            const long long last_id = (long long)T * W;
            int nd = B.node[o + tid];
            for (int s = 0; s < T && nd > 0 && nd <= last_id; ++s) {
                const int pos = len - 1 - s, par = tr[2 * (long long)nd], c = tr[2 * (long long)nd + 1];
                if (pos >= 0 && pos < L_max) lab[pos] = c;
                nd = par;
            }
        }
    } else if (tid < n_best) { lengths[out0 + tid] = -1; scores[out0 + tid] = -INFINITY; ctc_scores[out0 + tid] = -INFINITY; complete[out0 + tid] = -1; }
}

__global__ __launch_bounds__(WB_THREADS) void word_ngram_score_kernel(ss_word_lm L, const int* __restrict__ triples, long long n, float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * WB_THREADS + threadIdx.x;
    if (i >= n) return;
    const int w2 = triples[3 * i], w1 = triples[3 * i + 1], w = triples[3 * i + 2];
    const bool ok = w >= 0 && w < L.n_uni && w1 >= -1 && w1 < L.n_uni && w2 >= -1 && w2 < L.n_uni;
    out[i] = ok ? wb_lnp(L, w1 < 0 ? -1 : w2, w1, w) : NAN;
}

static int wb_check_lm(const ss_word_lm* lm, const char* who, bool lexicon)
{
    SS_CHECK(lm, "%s: null language model", who);
    SS_CHECK(lm->n_uni >= 1 && lm->n_uni <= (1 << 21) && lm->n_vocab >= 0 && lm->n_vocab <= lm->n_uni && lm->start >= 0 && lm->start < lm->n_uni,
             "%s: %d word ids (1 .. 2^21), %d of them words, start id %d", who, lm->n_uni, lm->n_vocab, lm->start);
    SS_CHECK(lm->uni_logp && lm->uni_bo, "%s: null unigram arrays", who);
    SS_CHECK(lm->bi_slots >= 0 && (lm->bi_slots & (lm->bi_slots - 1)) == 0 && lm->bi_probe >= 0 && lm->bi_probe <= lm->bi_slots,
             "%s: %d bigram slots (0 or a power of two), longest probe %d", who, lm->bi_slots, lm->bi_probe);
    SS_CHECK(lm->tri_slots >= 0 && (lm->tri_slots & (lm->tri_slots - 1)) == 0 && lm->tri_probe >= 0 && lm->tri_probe <= lm->tri_slots,
             "%s: %d trigram slots (0 or a power of two), longest probe %d", who, lm->tri_slots, lm->tri_probe);
    SS_CHECK(lm->bi_slots == 0 || (lm->bi_keys && lm->bi_logp && lm->bi_bo), "%s: null bigram table", who);
    SS_CHECK(lm->tri_slots == 0 || (lm->tri_keys && lm->tri_logp), "%s: null trigram table", who);
    if (lexicon) SS_CHECK(lm->n_nodes >= 1 && lm->lex_child && lm->lex_word, "%s: the lexicon needs its root (%d nodes)", who, lm->n_nodes);
    return 0;
}

extern "C" int64_t ss_ctc_word_beam_workspace_bytes(int n_utt, int64_t total_frames, int beam_width)
{
    if (n_utt < 0 || total_frames < 0 || beam_width < 1 || beam_width > WB_MAX_W) return -1;
    return 8 * (total_frames * beam_width + n_utt + 1);
}

extern "C" int ss_ctc_word_beam_search(const float* logits, int64_t ld, int V, int blank, int space, int64_t rows, const float* lse, const int64_t* utt_dev,
                                       int n_utt, int64_t total_frames, int beam_width, int n_best, const ss_word_lm* lm, float alpha, float beta,
                                       void* workspace, int max_len, int32_t* labels, int32_t* lengths, float* scores, float* ctc_scores,
                                       int32_t* complete, void* stream)
{
    SS_CHECK(V >= 2 && V <= WB_MAX_V, "ss_ctc_word_beam_search: %d classes (2 .. %d)", V, WB_MAX_V);
    SS_CHECK(blank >= 0 && blank < V && ld >= V, "ss_ctc_word_beam_search: bad blank %d / row stride %lld for %d classes", blank, (long long)ld, V);
    SS_CHECK(space >= 0 && space < V && space != blank, "ss_ctc_word_beam_search: space class %d (0 .. %d, not the blank %d)", space, V - 1, blank);
    SS_CHECK(beam_width >= 1 && beam_width <= WB_MAX_W, "ss_ctc_word_beam_search: beam width %d (1 .. %d)", beam_width, WB_MAX_W);
    SS_CHECK(n_best >= 1 && n_best <= beam_width, "ss_ctc_word_beam_search: n_best %d (1 .. beam width %d)", n_best, beam_width);
    SS_CHECK(n_utt >= 0 && rows >= 0 && total_frames >= 0 && max_len >= 1, "ss_ctc_word_beam_search: negative sizes");
    SS_CHECK(total_frames * beam_width + n_utt < 0x7fffffffll / 2, "ss_ctc_word_beam_search: %lld frames at width %d exceed the 32-bit node ids", (long long)total_frames, beam_width);
    if (wb_check_lm(lm, "ss_ctc_word_beam_search", true)) return 1;
    if (n_utt == 0) return 0;
    SS_CHECK(logits && lse && utt_dev && workspace && labels && lengths && scores && ctc_scores && complete, "ss_ctc_word_beam_search: null pointer");
    const size_t smem = 4 * wb_lds_words(beam_width, V);
    SS_CHECK(smem <= 160 * 1024, "ss_ctc_word_beam_search: %zu bytes of LDS needed", smem);
    static size_t granted = 0;
    if (granted < smem) { if (!ss_grant_lds((const void*)ctc_word_beam_kernel, smem)) { ss_set_error("ss_ctc_word_beam_search: cannot reserve %zu bytes of LDS", smem); return 1; } granted = smem; }
    SS_LAUNCH(ctc_word_beam_kernel, dim3(n_utt), dim3(WB_THREADS), smem, stream, logits, (long long)ld, V, blank, space, (long long)rows, lse, (const long long*)utt_dev,
              (long long)total_frames, beam_width, n_best, *lm, alpha, beta, (int*)workspace, max_len, (int*)labels, (int*)lengths, scores, ctc_scores, (int*)complete);
    SS_LAUNCH_CHECK("ss_ctc_word_beam_search");
    return 0;
}

extern "C" int ss_word_ngram_score(const ss_word_lm* lm, const int32_t* triples, int64_t n, float* out, void* stream)
{
    if (wb_check_lm(lm, "ss_word_ngram_score", false)) return 1;
    SS_CHECK(n >= 0 && n < 0x7fffffffll * WB_THREADS, "ss_word_ngram_score: %lld triples", (long long)n);
    if (n == 0) return 0;
    SS_CHECK(triples && out, "ss_word_ngram_score: null pointer");
    SS_LAUNCH(word_ngram_score_kernel, dim3((unsigned)((n + WB_THREADS - 1) / WB_THREADS)), dim3(WB_THREADS), 0, stream, *lm, (const int*)triples, (long long)n, out);
    SS_LAUNCH_CHECK("ss_word_ngram_score");
    return 0;
}
