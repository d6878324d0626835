// ctc_decode.hip -- CTC prefix beam search of the recognition model on gfx950, with shallow fusion of a label n-gram table ("next" row N1; the
// reference decodes with ctcdecode's beam search, recognition_model.py:33-35,48-49).  The algorithm is the one include/silent_speech_hip.h states
// for ss_ctc_beam_search; tests/ctc_beam_oracle.py restates it in plain Python and shares no code with this file.
//
// The search itself -- frame loop, selection, trie, final ranking -- is cb_search of ctc_beam_common.h.  This file is its policy for the label table:
//   ctx2     per entry, the label before the last one: with the core's `last` the trigram context of the next label;
//   score    the LM score of p + c is p's + alpha * table[ctx2(p)][last(p)][c] + beta, read in phase B for the key and again for the entries that
//            enter the beam; without a table it stays 0 and the score of an entry is its CTC score.
// Every entry is complete: there is no `complete` output.
#include "ctc_beam_common.h"
#include "silent_speech_hip.h"

namespace {
struct BsPolicy {
    static constexpr int EXTRA = 1;
    static constexpr bool REPORTS_COMPLETE = false;
    const float* tab; float a, b; int blank, C;
    int* ctx2;

    struct Fields { int ctx2; };
    __device__ __forceinline__ void carve(int* x, int) { ctx2 = x; }
    __device__ __forceinline__ Fields root() const { return {-1}; }
    __device__ __forceinline__ Fields load(int e) const { return {ctx2[e]}; }
    __device__ __forceinline__ void store(int e, const Fields& f) { ctx2[e] = f.ctx2; }
    __device__ __forceinline__ float extended_lm(const CbBeam& B, int op, int lastp, int c) const {
        float l = B.lm[op];
        if (tab) {
            const int c2 = ctx2[op], i2 = c2 < 0 ? C : cb_label(c2, blank), i1 = lastp < 0 ? C : cb_label(lastp, blank);
            l += a * tab[((long long)i2 * (C + 1) + i1) * C + cb_label(c, blank)] + b;
        }
        return l;
    }
    __device__ __forceinline__ unsigned extension_key(const CbBeam& B, int op, int c, float v) const { return cb_key(v + extended_lm(B, op, B.last[op], c)); }
    __device__ __forceinline__ Fields extend(const CbBeam& B, int op, int c, float& lm) const { const int lastp = B.last[op]; lm = extended_lm(B, op, lastp, c); return {lastp}; }
    __device__ __forceinline__ void final(const CbBeam& B, int e, float cs, float& sc, int& done) const { sc = cs + B.lm[e]; done = 1; }
};
}

__global__ __launch_bounds__(CB_THREADS) void ctc_beam_kernel(const float* __restrict__ logits, long long ld, int V, int blank, long long rows,
                                                              const float* __restrict__ lse, const long long* __restrict__ utt, long long total_frames, int W,
                                                              int n_best, const float* __restrict__ lmtab, float lm_a, float lm_b, int* __restrict__ trie, int L_max,
                                                              int* __restrict__ labels, int* __restrict__ lengths, float* __restrict__ scores, float* __restrict__ ctc_scores)
{
    BsPolicy P = {lmtab, lm_a, lm_b, blank, V - 1, nullptr};
    cb_search(P, CbArgs{logits, ld, V, blank, rows, lse, utt, total_frames, W, n_best, trie, L_max, labels, lengths, scores, ctc_scores, nullptr});
}

extern "C" int64_t ss_ctc_beam_workspace_bytes(int n_utt, int64_t total_frames, int beam_width) { return cb_workspace_bytes(n_utt, total_frames, beam_width); }

extern "C" int ss_ctc_beam_search(const float* logits, int64_t ld, int V, int blank, int64_t rows, const float* lse, const int64_t* utt_dev, int n_utt,
                                  int64_t total_frames, int beam_width, int n_best, const float* lm, float alpha, float beta, void* workspace, int max_len,
                                  int32_t* labels, int32_t* lengths, float* scores, float* ctc_scores, void* stream)
{
    size_t smem;
    if (cb_check_args("ss_ctc_beam_search", 1, BsPolicy::EXTRA, ld, V, blank, rows, n_utt, total_frames, beam_width, n_best, max_len, &smem)) return 1;
    if (n_utt == 0) return 0;
    SS_CHECK(logits && lse && utt_dev && workspace && labels && lengths && scores && ctc_scores, "ss_ctc_beam_search: null pointer");
    static size_t granted = 0;
    if (granted < smem) { if (!ss_grant_lds((const void*)ctc_beam_kernel, smem)) { ss_set_error("ss_ctc_beam_search: cannot reserve %zu bytes of LDS", smem); return 1; } granted = smem; }
    SS_LAUNCH(ctc_beam_kernel, dim3(n_utt), dim3(CB_THREADS), smem, stream, logits, (long long)ld, V, blank, (long long)rows, lse, (const long long*)utt_dev,
              (long long)total_frames, beam_width, n_best, lm, alpha, beta, (int*)workspace, max_len, (int*)labels, (int*)lengths, scores, ctc_scores);
    SS_LAUNCH_CHECK("ss_ctc_beam_search");
    return 0;
}
