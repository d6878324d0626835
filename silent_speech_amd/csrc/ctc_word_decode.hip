// ctc_word_decode.hip -- CTC prefix beam search confined to a lexicon, with a word n-gram with backoff scored at every word end, on gfx950 (what the
// reference's ctcdecode does with a KenLM model, recognition_model.py:33-35; here the model comes from ARPA text or from counts).  The algorithm is
// the one include/silent_speech_hip.h states for ss_ctc_word_beam_search; tests/ctc_word_beam_oracle.py restates it in plain Python and shares no code
// with this file.
//
// The search itself -- frame loop, selection, trie, final ranking -- is cb_search of ctc_beam_common.h, shared with ctc_decode.hip.  This file is its
// policy for the lexicon and the word model, the n-gram lookup, and the lookup as an entry point of its own (ss_word_ngram_score).  Per entry:
//   lx       its lexicon node (0 = the root); a letter extension exists only if lex_child[lx][label] is a node -- the row is read from global
//            memory in phase B (a thread's chunk is consecutive classes of one entry, so consecutive addresses);
//   w2, w1   the two words before the one being spelled (-1 = none), wd = the word lx spells (-1 = none);
//   wt       alpha * ln P(wd | w2, w1) + beta, -inf if lx spells no word.  It is computed ONCE, when the entry is created in the compaction phase
//            (wb_lnp: the trigram, the two bigram probes and the two unigram reads are independent and issued together); phase B (the space
//            extension) and the final ranking only read it.
// An entry is complete at a word boundary or where lx spells a word; complete entries rank first, an unfinished last word that is a word is scored.
// Every table index is checked against the sizes of ss_word_lm: hash slots are masked (idx & (slots - 1) < slots for ANY slots >= 1), probe
// counts are bounded by the slot counts on the host, child nodes and word ids are range-checked where they are read.
#include "ctc_beam_common.h"
#include "silent_speech_hip.h"

namespace {
constexpr cb_u64 WB_EMPTY = ~0ull;
__device__ __forceinline__ unsigned wb_home(cb_u64 key) { return (unsigned)cb_fin(key + 0x9E3779B97F4A7C15ull); }           // home slot before masking

// ln P(w | w2, w1) by the backoff rule of the header.  The caller guarantees 0 <= w < n_uni and -1 <= w1, w2 < n_uni.
__device__ __forceinline__ float wb_lnp(const ss_word_lm& L, int w2, int w1, int w) {
    const float uw = L.uni_logp[w];
    if (w1 < 0) return uw;
    const float b1 = L.uni_bo[w1];
    const bool bi = L.bi_slots > 0, ctx = bi && w2 >= 0, tri = L.tri_slots > 0 && w2 >= 0;
    const cb_u64 kb = ((cb_u64)w1 << 21) | (cb_u64)w, kc = ((cb_u64)(w2 < 0 ? 0 : w2) << 21) | (cb_u64)w1, kt = ((cb_u64)(w2 < 0 ? 0 : w2) << 42) | kb;
    const unsigned mb = (unsigned)(L.bi_slots - 1), mt = (unsigned)(L.tri_slots - 1);
    const unsigned sb = wb_home(kb), sc = wb_home(kc), st = wb_home(kt);
    int fb = -1, fc = -1, ft = -1;
    bool db = !bi, dc = !ctx, dt = !tri;                              // done: found, met an empty slot, or out of probes
    const int nb = bi ? L.bi_probe : 0, nt = tri ? L.tri_probe : 0, n = nb > nt ? nb : nt;
    for (int j = 0; j < n && !(db && dc && dt); ++j) {
        const unsigned ib = (sb + j) & mb, ic = (sc + j) & mb, it = (st + j) & mt;
        const cb_u64 xb = db || j >= nb ? WB_EMPTY : L.bi_keys[ib];     // three independent loads per step
        const cb_u64 xc = dc || j >= nb ? WB_EMPTY : L.bi_keys[ic];
        const cb_u64 xt = dt || j >= nt ? WB_EMPTY : L.tri_keys[it];
        if (!db) { if (xb == kb) fb = (int)ib; db = xb == kb || xb == WB_EMPTY; }
        if (!dc) { if (xc == kc) fc = (int)ic; dc = xc == kc || xc == WB_EMPTY; }
        if (!dt) { if (xt == kt) ft = (int)it; dt = xt == kt || xt == WB_EMPTY; }
    }
    if (ft >= 0) return L.tri_logp[ft];
    const float p2 = fb >= 0 ? L.bi_logp[fb] : b1 + uw;
    if (w2 < 0) return p2;
    return (fc >= 0 ? L.bi_bo[fc] : 0.f) + p2;
}

struct WbPolicy {
    static constexpr int EXTRA = 5;
    static constexpr bool REPORTS_COMPLETE = true;
    const ss_word_lm& L; float a, b; int blank, space, C;
    float* wt; int *lx, *wd, *w2, *w1;

    struct Fields { float wt; int lx, wd, w2, w1; };
    __device__ __forceinline__ void carve(int* x, int W) { wt = (float*)x; lx = x + 2 * W; wd = lx + 2 * W; w2 = wd + 2 * W; w1 = w2 + 2 * W; }
    __device__ __forceinline__ Fields root() const { return {-INFINITY, 0, -1, -1, L.start}; }
    __device__ __forceinline__ Fields load(int e) const { return {wt[e], lx[e], wd[e], w2[e], w1[e]}; }
    __device__ __forceinline__ void store(int e, const Fields& f) { wt[e] = f.wt; lx[e] = f.lx; wd[e] = f.wd; w2[e] = f.w2; w1[e] = f.w1; }
    __device__ __forceinline__ unsigned extension_key(const CbBeam& B, int op, int c, float v) const {
        if (c == space) return cb_key(v + (B.lm[op] + wt[op]));                                // wt = -inf: the entry spells no word, no candidate
        const int ch = L.lex_child[(long long)lx[op] * C + cb_label(c, blank)];
        return ch >= 0 && ch < L.n_nodes ? cb_key(v + B.lm[op]) : 0u;
    }
    // a new entry gets its lexicon node, its word context and its cached word term
    __device__ __forceinline__ Fields extend(const CbBeam& B, int op, int c, float& lm) const {
        Fields f = {-INFINITY, 0, -1, w2[op], w1[op]};
        lm = B.lm[op];
        if (c == space) { lm += wt[op]; f.w2 = f.w1; f.w1 = wd[op]; }
        else {
            f.lx = L.lex_child[(long long)lx[op] * C + cb_label(c, blank)];
            if (f.lx < 0 || f.lx >= L.n_nodes) f.lx = 0;                 // (the candidate existed, so this is the node phase B saw)
            if (f.lx > 0) { f.wd = L.lex_word[f.lx]; if (f.wd < 0 || f.wd >= L.n_vocab) f.wd = -1; }
        }
        if (f.wd >= 0) f.wt = a * wb_lnp(L, f.w2, f.w1, f.wd) + b;
        return f;
    }
    __device__ __forceinline__ void final(const CbBeam& B, int e, float cs, float& sc, int& done) const {
        const float t = wt[e]; const bool word = lx[e] != 0 && t > -INFINITY;
        sc = cs + (B.lm[e] + (word ? t : 0.f));
        done = lx[e] == 0 || word;
    }
};
}

__global__ __launch_bounds__(CB_THREADS) void ctc_word_beam_kernel(const float* __restrict__ logits, long long ld, int V, int blank, int space, long long rows,
                                                                   const float* __restrict__ lse, const long long* __restrict__ utt, long long total_frames, int W,
                                                                   int n_best, ss_word_lm L, float lm_a, float lm_b, int* __restrict__ trie, int L_max,
                                                                   int* __restrict__ labels, int* __restrict__ lengths, float* __restrict__ scores,
                                                                   float* __restrict__ ctc_scores, int* __restrict__ complete)
{
    WbPolicy P = {L, lm_a, lm_b, blank, space, V - 1, nullptr, nullptr, nullptr, nullptr, nullptr};
    cb_search(P, CbArgs{logits, ld, V, blank, rows, lse, utt, total_frames, W, n_best, trie, L_max, labels, lengths, scores, ctc_scores, complete});
}

__global__ __launch_bounds__(CB_THREADS) void word_ngram_score_kernel(ss_word_lm L, const int* __restrict__ triples, long long n, float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * CB_THREADS + threadIdx.x;
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

extern "C" int64_t ss_ctc_word_beam_workspace_bytes(int n_utt, int64_t total_frames, int beam_width) { return cb_workspace_bytes(n_utt, total_frames, beam_width); }

extern "C" int ss_ctc_word_beam_search(const float* logits, int64_t ld, int V, int blank, int space, int64_t rows, const float* lse, const int64_t* utt_dev,
                                       int n_utt, int64_t total_frames, int beam_width, int n_best, const ss_word_lm* lm, float alpha, float beta,
                                       void* workspace, int max_len, int32_t* labels, int32_t* lengths, float* scores, float* ctc_scores,
                                       int32_t* complete, void* stream)
{
    size_t smem;
    if (cb_check_args("ss_ctc_word_beam_search", 2, WbPolicy::EXTRA, ld, V, blank, rows, n_utt, total_frames, beam_width, n_best, max_len, &smem)) return 1;
    SS_CHECK(space >= 0 && space < V && space != blank, "ss_ctc_word_beam_search: space class %d (0 .. %d, not the blank %d)", space, V - 1, blank);
    if (wb_check_lm(lm, "ss_ctc_word_beam_search", true)) return 1;
    if (n_utt == 0) return 0;
    SS_CHECK(logits && lse && utt_dev && workspace && labels && lengths && scores && ctc_scores && complete, "ss_ctc_word_beam_search: null pointer");
    static size_t granted = 0;
    if (granted < smem) { if (!ss_grant_lds((const void*)ctc_word_beam_kernel, smem)) { ss_set_error("ss_ctc_word_beam_search: cannot reserve %zu bytes of LDS", smem); return 1; } granted = smem; }
    SS_LAUNCH(ctc_word_beam_kernel, dim3(n_utt), dim3(CB_THREADS), smem, stream, logits, (long long)ld, V, blank, space, (long long)rows, lse, (const long long*)utt_dev,
              (long long)total_frames, beam_width, n_best, *lm, alpha, beta, (int*)workspace, max_len, (int*)labels, (int*)lengths, scores, ctc_scores, (int*)complete);
    SS_LAUNCH_CHECK("ss_ctc_word_beam_search");
    return 0;
}

extern "C" int ss_word_ngram_score(const ss_word_lm* lm, const int32_t* triples, int64_t n, float* out, void* stream)
{
    if (wb_check_lm(lm, "ss_word_ngram_score", false)) return 1;
    SS_CHECK(n >= 0 && n < 0x7fffffffll * CB_THREADS, "ss_word_ngram_score: %lld triples", (long long)n);
    if (n == 0) return 0;
    SS_CHECK(triples && out, "ss_word_ngram_score: null pointer");
    SS_LAUNCH(word_ngram_score_kernel, dim3((unsigned)((n + CB_THREADS - 1) / CB_THREADS)), dim3(CB_THREADS), 0, stream, *lm, (const int*)triples, (long long)n, out);
    SS_LAUNCH_CHECK("ss_word_ngram_score");
    return 0;
}
