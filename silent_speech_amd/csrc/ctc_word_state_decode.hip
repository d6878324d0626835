// ctc_word_state_decode.hip -- the lexicon-constrained CTC prefix beam search of ctc_word_decode.hip with a word n-gram of ANY order 1 .. 6, held as
// context states (include/silent_speech_hip.h: ss_word_state_lm, ss_ctc_word_state_beam_search; the representation is KenLM's).  A beam entry carries
// ONE state id -- the longest suffix of its word history that the model knows as a context -- so entry size and key width do not depend on the order.
// tests/ctc_word_state_oracle.py restates the contract with whole word histories in plain Python and shares no code with this file.
//
// The search itself is cb_search of ctc_beam_common.h; this file is its policy, the lookup and the lookup as an entry point (ss_word_state_score).
// Per entry:
//   lx, wd   its lexicon node and the word that node spells (-1 = none), as in ctc_word_decode.hip;
//   st       the state BEFORE the word being spelled;
//   wt, nx   alpha * ln P(wd | st) + beta and the state AFTER wd, both from ONE lookup when the entry is created (ws_lookup); -inf / unused if lx
//            spells no word.  The space extension and the final ranking only read them.
// The lookup: (1) the suffix links of st, a COUNTED loop of order - 1 <= 5 dependent loads (state -> shorter state, the backoffs beside them);
// (2) the probes (state_i << 21 | word) of all levels together -- up to 5 independent loads per probe step, as wb_lnp issues its three;
// (3) the highest level that holds the arc gives ln P and the next state, the backoffs of the levels above it are added from the lowest order
// outward out of a register array.  Every index is checked against the sizes of ss_word_state_lm: hash slots are masked, probe counts are
// bounded by arc_probe <= arc_slots on the host, a state / next / shorter outside [0, n_states) counts as state 0, child nodes and word ids
// are range-checked where they are read.
#include "ctc_beam_common.h"
#include "silent_speech_hip.h"

namespace {
constexpr cb_u64 WS_EMPTY = ~0ull;
constexpr int WS_LEVELS = 5;                                             // the longest context: order - 1 words
__device__ __forceinline__ unsigned ws_home(cb_u64 key) { return (unsigned)cb_fin(key + 0x9E3779B97F4A7C15ull); }           // home slot before masking

// ln P(w | state s) and the state after w.  The caller guarantees 0 <= w < n_uni and 0 <= s < n_states (and the host 1 + n_uni <= n_states).
__device__ __forceinline__ float ws_lookup(const ss_word_state_lm& L, int s, int w, int& next) {
    const float uw = L.uni_logp[w];
    // (1) the chain s, shorter[s], ...: cs[i] = 0 behind its end
    int cs[WS_LEVELS]; float cb[WS_LEVELS];
    int n = 0, cur = s;
    const int depth = L.order - 1;
#pragma unroll
    for (int i = 0; i < WS_LEVELS; ++i) {
        const bool live = i < depth && cur > 0 && cur < L.n_states;
        cs[i] = live ? cur : 0;
        cb[i] = live ? L.st_bo[cur] : 0.f;
        cur = live ? L.st_shorter[cur] : 0;
        n += live;
    }
    // (2) one probe sequence per level, stepped together
    const bool table = L.arc_slots > 0;
    const unsigned mask = (unsigned)(L.arc_slots - 1);
    cb_u64 k[WS_LEVELS]; unsigned hm[WS_LEVELS]; int f[WS_LEVELS]; bool d[WS_LEVELS];
    bool all = true;
#pragma unroll
    for (int i = 0; i < WS_LEVELS; ++i) {
        k[i] = ((cb_u64)cs[i] << 21) | (cb_u64)w;
        hm[i] = ws_home(k[i]);
        f[i] = -1;
        d[i] = !(table && cs[i] > 0);                                   // done: found, met an empty slot, or nothing to look for
        all = all && d[i];
    }
    const int np = table ? L.arc_probe : 0;
    for (int j = 0; j < np && !all; ++j) {
        all = true;
#pragma unroll
        for (int i = 0; i < WS_LEVELS; ++i) {
            const unsigned ix = (hm[i] + (unsigned)j) & mask;
            const cb_u64 x = d[i] ? WS_EMPTY : L.arc_keys[ix];          // independent loads
            if (!d[i]) { if (x == k[i]) f[i] = (int)ix; d[i] = x == k[i] || x == WS_EMPTY; }
            all = all && d[i];
        }
    }
    // (3) the first level of the chain that holds the arc; without one the unigram behind the whole chain
    int hit = n, slot = -1;
#pragma unroll
    for (int i = WS_LEVELS - 1; i >= 0; --i) if (f[i] >= 0) { hit = i; slot = f[i]; }
    float v = uw;
    int nx = 1 + w;
    if (slot >= 0) { v = L.arc_logp[slot]; nx = L.arc_next[slot]; }
    if (nx < 0 || nx >= L.n_states) nx = 0;
#pragma unroll
    for (int i = WS_LEVELS - 1; i >= 0; --i) if (i < hit) v = cb[i] + v;
    next = nx;
    return v;
}

struct WsPolicy {
    static constexpr int EXTRA = 5;
    static constexpr bool REPORTS_COMPLETE = true;
    const ss_word_state_lm& L; float a, b; int blank, space, C;
    float* wt; int *lx, *wd, *st, *nx;

    struct Fields { float wt; int lx, wd, st, nx; };
    __device__ __forceinline__ void carve(int* x, int W) { wt = (float*)x; lx = x + 2 * W; wd = lx + 2 * W; st = wd + 2 * W; nx = st + 2 * W; }
    __device__ __forceinline__ Fields root() const { return {-INFINITY, 0, -1, L.start_state, 0}; }
    __device__ __forceinline__ Fields load(int e) const { return {wt[e], lx[e], wd[e], st[e], nx[e]}; }
    __device__ __forceinline__ void store(int e, const Fields& f) { wt[e] = f.wt; lx[e] = f.lx; wd[e] = f.wd; st[e] = f.st; nx[e] = f.nx; }
    __device__ __forceinline__ unsigned extension_key(const CbBeam& B, int op, int c, float v) const {
        if (c == space) return cb_key(v + (B.lm[op] + wt[op]));                                // wt = -inf: the entry spells no word, no candidate
        const int ch = L.lex_child[(long long)lx[op] * C + cb_label(c, blank)];
        return ch >= 0 && ch < L.n_nodes ? cb_key(v + B.lm[op]) : 0u;
    }
    // a new entry gets its lexicon node, its state and -- if the node spells a word -- the word term and the state behind the word
    __device__ __forceinline__ Fields extend(const CbBeam& B, int op, int c, float& lm) const {
        Fields f = {-INFINITY, 0, -1, st[op], 0};
        lm = B.lm[op];
        if (c == space) { lm += wt[op]; f.st = nx[op]; }                   // (nx was range-checked by the lookup that made it)
        else {
            f.lx = L.lex_child[(long long)lx[op] * C + cb_label(c, blank)];
            if (f.lx < 0 || f.lx >= L.n_nodes) f.lx = 0;                 // (the candidate existed, so this is the node phase B saw)
            if (f.lx > 0) { f.wd = L.lex_word[f.lx]; if (f.wd < 0 || f.wd >= L.n_vocab) f.wd = -1; }
        }
        if (f.wd >= 0) f.wt = a * ws_lookup(L, f.st, f.wd, f.nx) + b;
        return f;
    }
    __device__ __forceinline__ void final(const CbBeam& B, int e, float cs, float& sc, int& done) const {
        const float t = wt[e]; const bool word = lx[e] != 0 && t > -INFINITY;
        sc = cs + (B.lm[e] + (word ? t : 0.f));
        done = lx[e] == 0 || word;
    }
};
}

__global__ __launch_bounds__(CB_THREADS) void ctc_word_state_beam_kernel(const float* __restrict__ logits, long long ld, int V, int blank, int space, long long rows,
                                                                         const float* __restrict__ lse, const long long* __restrict__ utt, long long total_frames, int W,
                                                                         int n_best, ss_word_state_lm L, float lm_a, float lm_b, int* __restrict__ trie, int L_max,
                                                                         int* __restrict__ labels, int* __restrict__ lengths, float* __restrict__ scores,
                                                                         float* __restrict__ ctc_scores, int* __restrict__ complete)
{
    WsPolicy P = {L, lm_a, lm_b, blank, space, V - 1, nullptr, nullptr, nullptr, nullptr, nullptr};
    cb_search(P, CbArgs{logits, ld, V, blank, rows, lse, utt, total_frames, W, n_best, trie, L_max, labels, lengths, scores, ctc_scores, complete});
}

__global__ __launch_bounds__(CB_THREADS) void word_state_score_kernel(ss_word_state_lm L, const int* __restrict__ pairs, long long n, float* __restrict__ out_lnp,
                                                                      int* __restrict__ out_next)
{
    const long long i = (long long)blockIdx.x * CB_THREADS + threadIdx.x;
    if (i >= n) return;
    const int s = pairs[2 * i], w = pairs[2 * i + 1];
    const bool ok = s >= 0 && s < L.n_states && w >= 0 && w < L.n_uni;
    int next = -1;
    const float v = ok ? ws_lookup(L, s, w, next) : NAN;
    out_lnp[i] = v; out_next[i] = next;
}

static int ws_check_lm(const ss_word_state_lm* lm, const char* who, bool lexicon)
{
    SS_CHECK(lm, "%s: null language model", who);
    SS_CHECK(lm->order >= 1 && lm->order <= 6, "%s: order %d (1 .. 6)", who, lm->order);
    SS_CHECK(lm->n_uni >= 1 && lm->n_uni <= (1 << 21) && lm->n_vocab >= 0 && lm->n_vocab <= lm->n_uni, "%s: %d word ids (1 .. 2^21), %d of them words", who,
             lm->n_uni, lm->n_vocab);
    SS_CHECK(lm->n_states > lm->n_uni && lm->start_state >= 0 && lm->start_state < lm->n_states,
             "%s: %d states (the empty context and one per word id: at least %d), start state %d", who, lm->n_states, lm->n_uni + 1, lm->start_state);
    SS_CHECK(lm->uni_logp && lm->st_bo && lm->st_shorter, "%s: null unigram or state arrays", who);
    SS_CHECK(lm->arc_slots >= 0 && (lm->arc_slots & (lm->arc_slots - 1)) == 0 && lm->arc_probe >= 0 && lm->arc_probe <= lm->arc_slots,
             "%s: %d arc slots (0 or a power of two), longest probe %d", who, lm->arc_slots, lm->arc_probe);
    SS_CHECK(lm->arc_slots == 0 || (lm->arc_keys && lm->arc_logp && lm->arc_next), "%s: null arc table", who);
    if (lexicon) SS_CHECK(lm->n_nodes >= 1 && lm->lex_child && lm->lex_word, "%s: the lexicon needs its root (%d nodes)", who, lm->n_nodes);
    return 0;
}

extern "C" int64_t ss_ctc_word_state_beam_workspace_bytes(int n_utt, int64_t total_frames, int beam_width) { return cb_workspace_bytes(n_utt, total_frames, beam_width); }

extern "C" int ss_ctc_word_state_beam_search(const float* logits, int64_t ld, int V, int blank, int space, int64_t rows, const float* lse, const int64_t* utt_dev,
                                             int n_utt, int64_t total_frames, int beam_width, int n_best, const ss_word_state_lm* lm, float alpha, float beta,
                                             void* workspace, int max_len, int32_t* labels, int32_t* lengths, float* scores, float* ctc_scores,
                                             int32_t* complete, void* stream)
{
    size_t smem;
    if (cb_check_args("ss_ctc_word_state_beam_search", 2, WsPolicy::EXTRA, ld, V, blank, rows, n_utt, total_frames, beam_width, n_best, max_len, &smem)) return 1;
    SS_CHECK(space >= 0 && space < V && space != blank, "ss_ctc_word_state_beam_search: space class %d (0 .. %d, not the blank %d)", space, V - 1, blank);
    if (ws_check_lm(lm, "ss_ctc_word_state_beam_search", true)) return 1;
    if (n_utt == 0) return 0;
    SS_CHECK(logits && lse && utt_dev && workspace && labels && lengths && scores && ctc_scores && complete, "ss_ctc_word_state_beam_search: null pointer");
    static size_t granted = 0;
    if (granted < smem) { if (!ss_grant_lds((const void*)ctc_word_state_beam_kernel, smem)) { ss_set_error("ss_ctc_word_state_beam_search: cannot reserve %zu bytes of LDS", smem); return 1; } granted = smem; }
    SS_LAUNCH(ctc_word_state_beam_kernel, dim3(n_utt), dim3(CB_THREADS), smem, stream, logits, (long long)ld, V, blank, space, (long long)rows, lse, (const long long*)utt_dev,
              (long long)total_frames, beam_width, n_best, *lm, alpha, beta, (int*)workspace, max_len, (int*)labels, (int*)lengths, scores, ctc_scores, (int*)complete);
    SS_LAUNCH_CHECK("ss_ctc_word_state_beam_search");
    return 0;
}

extern "C" int ss_word_state_score(const ss_word_state_lm* lm, const int32_t* pairs, int64_t n, float* out_lnp, int32_t* out_next, void* stream)
{
    if (ws_check_lm(lm, "ss_word_state_score", false)) return 1;
    SS_CHECK(n >= 0 && n < 0x7fffffffll * CB_THREADS, "ss_word_state_score: %lld pairs", (long long)n);
    if (n == 0) return 0;
    SS_CHECK(pairs && out_lnp && out_next, "ss_word_state_score: null pointer");
    SS_LAUNCH(word_state_score_kernel, dim3((unsigned)((n + CB_THREADS - 1) / CB_THREADS)), dim3(CB_THREADS), 0, stream, *lm, (const int*)pairs, (long long)n, out_lnp, (int*)out_next);
    SS_LAUNCH_CHECK("ss_word_state_score");
    return 0;
}
