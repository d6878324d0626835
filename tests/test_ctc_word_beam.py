"""Lexicon-constrained CTC prefix beam search with a word n-gram on the device (csrc/ctc_word_decode.hip, torch.ops.silent_speech.ctc_word_beam_search
and word_ngram_score, recognition_model.WordNgramLM / beam_decode* / test): the oracle against the exact ranking of all allowed label strings, the
device against that ranking where nothing is pruned and against tests/ctc_word_beam_oracle.py (plain Python, float64) where the beam prunes, the
n-gram lookup alone at its edges, the rules one by one, bit for bit against itself across layouts and batches, the host builders, the ops and
recognition_model.test.

Score bars.  Exact regime (T <= 6, at most 3 words, |score| < 32, asserted): a frame costs a prefix one log-add-exp and one addition, a word
one multiply-add and one addition, each rounded to at most one f32 ulp of the running value (< 2^-19 below 32) plus one ulp of the hardware
exp2 / log2 on a term <= ln 2 -- (6 frames + 3 words) x 3 roundings x 2^-19 = 5.2e-5 = EXACT_BAR.  Pruned regime: per shape, 4 x the largest
deviation (top-1 score or its CTC part) of the oracle's OWN float32 run from its float64 run on these inputs (measured on the CPU, listed in
PRUNED below; the factor covers the hardware exp2 / log2 and another summation order).  The float32 oracle agreed with the float64 one on top-1,
top-3 and the complete flags of every utterance of every shape here, so the 90 % cap is not what lets the kernel pass."""
import io
import math

import numpy as np
import pytest
import torch

from silent_speech_amd import recognition_model as rm
from silent_speech_amd import torch_ops
from silent_speech_amd.architecture import Model
from tests import ctc_word_beam_oracle as oracle
from tests.backend import dev, is_emu  # noqa: F401
from tests.ctc_beam_helpers import from_probs as _from_probs, layout as _layout, noise as _noise, same as _same, strings as _strings

EXACT_BAR = (6 + 3) * 3 * 2.0 ** -19
ALPHA, BETA = 0.8, 0.5


def _tables(lm, dev):
    lm = lm.to(dev)
    return (lm.lex_child, lm.lex_word, lm.uni, lm.bi_keys, lm.bi_val, lm.tri_keys, lm.tri_val, lm.n_words, lm.start, lm.bi_probe, lm.tri_probe)


def _search(dev, lm, utts, W, n_best, alpha=ALPHA, beta=BETA, blank=None, space=None, **how):
    """utts: list of (T_i, V) float32 arrays, laid out by ctc_beam_helpers.layout(**how).  Returns numpy (labels, lengths, scores, ctc scores, complete)."""
    flat, utt, V, total, longest = _layout(dev, utts, **how)
    out = torch.ops.silent_speech.ctc_word_beam_search(flat, utt, V, V - 1 if blank is None else blank, V - 2 if space is None else space,
                                                       total, longest, W, n_best, *_tables(lm, dev), alpha, beta)
    return tuple(t.cpu().numpy() for t in out)


def _chars(V):
    """V - 2 letters and the space: labels 0 .. V - 2 = classes 0 .. V - 2, the blank is class V - 1"""
    return ''.join(chr(0x100 + i) for i in range(V - 2)) + ' '


def _hand_lm(V, words, uni=None, bi=None, tri=None, min_slots=0):
    """words as tuples of letter classes; uniform unigrams and zero backoffs unless given"""
    chars = _chars(V)
    n = len(words)
    if uni is None:
        uni = np.zeros((n + 1, 2))
        uni[:n, 0] = -math.log(n)
    return rm.WordNgramLM([''.join(chars[c] for c in w) for w in words], uni, bi or {}, tri or {}, chars, min_slots)


def _random_lm(V, n_words, max_letters, seed, min_slots=0):
    """A seeded random lexicon of n_words words of 1 .. max_letters letters and random tables: ~4 bigrams per context word, ~4 trigrams per word."""
    rng = np.random.default_rng(seed)
    chars = _chars(V)
    words = set()
    while len(words) < n_words:
        words.add(''.join(chars[i] for i in rng.integers(0, V - 2, rng.integers(1, max_letters + 1))))
    words = sorted(words)
    n = len(words)
    uni = np.zeros((n + 1, 2))
    x = rng.standard_normal(n) * 1.5
    uni[:n, 0] = x - np.log(np.exp(x).sum())
    uni[:, 1] = -rng.random(n + 1)
    uni[n, 0] = -99.0
    bi = {}
    for w1 in range(n + 1):
        for w in rng.choice(n, 4, replace=False):
            bi[(w1, int(w))] = (-4 * rng.random(), -rng.random())
    pairs = sorted(bi)
    tri = {}
    for j in rng.choice(len(pairs), n, replace=False):
        for w in rng.choice(n, 4, replace=False):
            tri[pairs[j] + (int(w),)] = -4 * rng.random()
    return rm.WordNgramLM(words, uni, bi, tri, chars, min_slots)


# ---------------------------------------------------------------------------------------------- 1. the oracle against brute force
# classes a = 0, b = 1, space = 2, blank = 3; the words a, ab, ba, bab; bigrams and trigrams that reach every level of the backoff rule
def _tiny_lm():
    uni = np.array([[-1.0, -0.3], [-1.7, -0.2], [-1.2, -0.6], [-2.1, -0.1], [-99.0, -0.4]])
    bi = {(4, 0): (-0.7, -0.25), (4, 2): (-1.1, -0.5), (0, 1): (-0.9, -0.35), (1, 0): (-0.4, -0.15), (2, 3): (-1.3, -0.45), (0, 0): (-1.9, -0.2)}
    tri = {(4, 0, 1): -0.5, (4, 2, 3): -0.8, (0, 1, 0): -0.6, (0, 0, 2): -1.4}
    return _hand_lm(4, [(0,), (0, 1), (1, 0), (1, 0, 1)], uni, bi, tri)


@pytest.mark.parametrize('T,seed', [(5, 0), (5, 1), (6, 2)])
def test_oracle_reproduces_the_exact_ranking_of_every_allowed_string(T, seed):
    """With a beam at least as wide as the number of prefixes, every prefix's final score is the exact float64 log-likelihood of that label
    string (oracle/ctc_ref.ctc_utterance over all strings of up to T labels the lexicon allows) + alpha score_words + beta n_words."""
    lm = _tiny_lm()
    tab = oracle.Tables.of(lm, 3)
    x = _noise(np.random.default_rng(seed), T, 4, 3, 1.5)
    exact = oracle.brute_force(x, 3, 2, tab, ALPHA, BETA)
    got = oracle.beam_search(x, 3, 2, 4 ** 7, tab, ALPHA, BETA, n_best=4 ** 7)
    assert len(exact) == len(got) > 2 * T
    want = {q: (s, ll, done) for q, s, ll, done in exact}
    for q, score, ctc, done in got:
        assert abs(score - want[q][0]) < 1e-9 and abs(ctc - want[q][1]) < 1e-9 and done == want[q][2], q
        # the brute-force score restated through the model's own host rule: alpha * score_words + beta per word
        words = bytes(q).split(bytes([2]))
        ids = [tab.word_of[w] for w in words if w in tab.word_of] if all(w in tab.word_of for w in words[:-1]) else None
        n_scored = len(words) - 1 + (words[-1] in tab.word_of)
        assert ids is not None and len(ids) == n_scored
        assert abs(score - ctc - (ALPHA * lm.score_words(ids).sum() + BETA * n_scored)) < 1e-6
    assert [q for q, *_ in got[:8]] == [q for q, *_ in exact[:8]]
    assert not any(done for *_, done in exact[sum(done for *_, done in exact):])     # complete strings first
    for q, *_ in exact:                                                   # nothing the rules forbid: no leading or double space, lexicon words only
        assert q[:1] != (2,) and all(w in tab.word_of for w in bytes(q).split(bytes([2]))[:-1])


# ---------------------------------------------------------------------------------------------- 2. exact regime on the device
# seeds chosen with brute force alone so that adjacent ranks of the first 17 strings differ by more than 1e-3 (asserted below)
EXACT_SEEDS = {5: 0, 6: 0}
_EXACT = {}


def _exact_case(T):
    if T not in _EXACT:
        lm = _tiny_lm()
        tab = oracle.Tables.of(lm, 3)
        x = _noise(np.random.default_rng(EXACT_SEEDS[T]), T, 4, 3, 1.5)
        ranking = oracle.brute_force(x, 3, 2, tab, ALPHA, BETA)
        gaps = [abs(ranking[i][1] - ranking[i + 1][1]) for i in range(16)]
        assert min(gaps) > 1e-3, (T, min(gaps))
        live = []
        oracle.beam_search(x, 3, 2, 128, tab, ALPHA, BETA, trace=live)
        assert max(live) <= 128, live                                    # candidates per frame: nothing is pruned at width 128
        assert max(abs(s) for _, s, _, _ in ranking[:16]) < 32 and max(len(bytes(q).split(bytes([2]))) for q, *_ in ranking[:16]) <= 3
        f32 = oracle.beam_search(x, 3, 2, 128, tab, ALPHA, BETA, n_best=16, dtype=np.float32)
        _EXACT[T] = (lm, x, ranking, max(abs(f32[r][1] - ranking[r][1]) for r in range(16)))
    return _EXACT[T]


@pytest.mark.parametrize('T', [5, 6])
def test_exact_regime_equals_the_brute_force_ranking(dev, T):
    lm, x, ranking, f32_dev = _exact_case(T)
    out = _search(dev, lm, [x], 128, 16)
    assert _strings(out, 0) == [q for q, *_ in ranking[:16]]
    dev_max = max(abs(float(out[2][0, r]) - ranking[r][1]) for r in range(16))
    ctc_max = max(abs(float(out[3][0, r]) - ranking[r][2]) for r in range(16))
    print('exact regime, T = %d: largest score deviation %.3e, CTC part %.3e (bar %.1e; the float32 oracle: %.3e)' % (T, dev_max, ctc_max, EXACT_BAR, f32_dev))
    assert dev_max < EXACT_BAR and ctc_max < EXACT_BAR and f32_dev < EXACT_BAR
    assert out[4][0].tolist() == [int(done) for *_, done in ranking[:16]]


# ---------------------------------------------------------------------------------------------- 3. pruned regime against the float64 oracle
# (T, V, W) -> utterances, words, longest word, seed of the lexicon, largest deviation of the float32 oracle's top-1 score / CTC part from the
# float64 oracle's on these inputs; the bar = 4 x the larger of the two.  (The lexicon seed of the width-1 shape was chosen with the oracle
# alone so that some of its winners are incomplete.)
PRUNED = {
    (60, 8, 16): (10, 40, 3, 116, 1.576e-05, 1.279e-05),
    (120, 12, 16): (10, 60, 4, 204, 3.433e-05, 3.996e-05),
    (64, 38, 100): (4, 300, 5, 330, 5.073e-05, 4.992e-05),
    (16, 128, 128): (3, 500, 5, 912, 3.652e-06, 5.693e-06),
    (50, 38, 1): (10, 300, 5, 23, 2.480e-05, 2.876e-05),
    (400, 38, 100): (1, 300, 5, 666, 3.114e-04, 2.914e-04),
}
EMU_UTTERANCES = 3                                                       # the emulator tier decodes the first few utterances of a shape
_REF, _LMS = {}, {}


def _pruned_lm(shape):
    if shape not in _LMS:
        T, V, W = shape
        _LMS[shape] = _random_lm(V, PRUNED[shape][1], PRUNED[shape][2], PRUNED[shape][3])
    return _LMS[shape]


def _pruned_inputs(shape):
    T, V, W = shape
    n = PRUNED[shape][0]
    rng = np.random.default_rng(T * 1000 + V)
    return [_noise(rng, T - (i * T) // (8 * n), V, V - 1, 2.0 + rng.random()) for i in range(n)]     # ragged: T down to ~7/8 T


def _reference(tag, i, make):
    """Oracle results, computed once per (case, utterance) and shared between the backends."""
    if (tag, i) not in _REF:
        _REF[(tag, i)] = make()
    return _REF[(tag, i)]


def _check_against_oracle(out, refs, bar, what):
    top1 = top3 = flags = 0
    worst = worst_ctc = 0.0
    for b, ref in enumerate(refs):
        got = _strings(out, b)
        top1 += got[:1] == [q for q, *_ in ref[:1]]
        top3 += got[:3] == [q for q, *_ in ref[:3]]
        flags += out[4][b, :len(ref)].tolist() == [int(r[3]) for r in ref] and (out[4][b, len(ref):] == -1).all()
        worst = max(worst, abs(float(out[2][b, 0]) - ref[0][1]))
        worst_ctc = max(worst_ctc, abs(float(out[3][b, 0]) - ref[0][2]))
    n = len(refs)
    print('%s: top-1 %d / %d, top-3 %d / %d, complete flags %d / %d, largest top-1 deviation: score %.3e, CTC part %.3e (bar %.3e)'
          % (what, top1, n, top3, n, flags, n, worst, worst_ctc, bar))
    assert top1 >= 0.9 * n and top3 >= 0.9 * n and flags >= 0.9 * n
    assert worst <= bar and worst_ctc <= bar


@pytest.mark.parametrize('shape', list(PRUNED))
def test_pruned_regime_matches_the_float64_oracle(dev, shape):
    T, V, W = shape
    if is_emu(dev) and T > 200:
        pytest.skip('400 frames at width 100: GPU only')
    xs = _pruned_inputs(shape)
    if shape == (400, 38, 100):
        assert min(x.shape[0] for x in xs) * W > 32767                   # node ids leave 15 bits in every utterance
    xs = xs[:EMU_UTTERANCES] if is_emu(dev) else xs
    n_best = min(3, W)
    lm = _pruned_lm(shape)
    tab = oracle.Tables.of(lm, V - 1)
    refs = [_reference(shape, i, lambda: oracle.beam_search(x, V - 1, V - 2, W, tab, ALPHA, BETA, n_best=n_best)) for i, x in enumerate(xs)]
    assert all(len(r[0][0]) > 0 for r in refs)                           # not degenerate: every winner holds words
    if W == 1 and not is_emu(dev):
        assert 2 <= sum(not r[0][3] for r in refs) <= len(refs) - 2      # complete and incomplete winners both appear
    out = _search(dev, lm, xs, W, n_best)
    _check_against_oracle(out, refs, 4 * max(PRUNED[shape][4:6]), 'shape %s' % (shape,))


def test_score_minus_ctc_part_is_the_word_model_through_score_words(dev):
    """score - ctc_score of the winner = alpha * sum score_words + beta * n_words over its words (an unfinished last word that is a word counted)."""
    shape = (60, 8, 16)
    T, V, W = shape
    lm, xs = _pruned_lm(shape), _pruned_inputs(shape)[:EMU_UTTERANCES]
    out = _search(dev, lm, xs, W, 1)
    index = {w: i for i, w in enumerate(lm.words)}
    for b in range(len(xs)):
        text = ''.join(lm.chars[c] for c in _strings(out, b)[0])
        words = text.split(' ')
        scored = words[:-1] + ([words[-1]] if words[-1] in index else [])
        assert scored and all(w in index for w in scored)
        want = ALPHA * lm.score_words([index[w] for w in scored]).sum() + BETA * len(scored)
        assert abs(float(out[2][b, 0]) - float(out[3][b, 0]) - want) <= 4 * max(PRUNED[shape][4:6])
        assert out[4][b, 0] == int(words[-1] == '' or words[-1] in index)


# ---------------------------------------------------------------------------------------------- 4. the lookup alone
# magnitudes in the tables below stay under 8 and a score sums at most three of them (bigram backoff + unigram backoff + unigram), so an f32 sum is
# within 2 roundings x ulp(16) / 2 = 2^-20 of the float64 sum of the same f32 table entries; the bar allows 4 ulps of 16: 4 x 2^-20 = 3.8e-6
LOOKUP_BAR = 4 * 2.0 ** -20


def _score(dev, lm, triples):
    lm = lm.to(dev)
    t = torch.tensor(triples, dtype=torch.int32).reshape(len(triples), 3).to(dev)
    return lm.score_triples(t).cpu().numpy()


def _want(lm, triples):
    return np.array([lm.score_words([w], context=(w2, w1))[0] for w2, w1, w in triples])


def test_lookup_hits_and_misses_at_every_level(dev):
    lm = _tiny_lm()
    S = lm.start
    cases = [(S, 0, 1),         # trigram hit
             (0, 1, 0),         # trigram hit, no start context
             (4, 0, 0),         # trigram miss, bigram (4, 0) has a backoff, bigram (0, 0) hit
             (0, 0, 1),         # trigram miss, context backoff of (0, 0), bigram (0, 1) hit
             (1, 0, 3),         # trigram miss, context (1, 0) present, bigram (0, 3) miss -> unigram backoff of 0 + unigram 3
             (3, 3, 3),         # a miss at every level: no trigram, no context bigram (backoff 0), no bigram
             (3, 1, 0),         # the context bigram (3, 1) is missing: backoff 0, bigram (1, 0) hit
             (-1, S, 0),        # the start context: bigram hit
             (-1, S, 3),        # the start context: bigram miss
             (-1, 2, 3),        # no w2, bigram hit
             (-1, -1, 2),       # no context at all: the unigram
             (S, 2, 3)]         # trigram hit behind the start
    got, want = _score(dev, lm, cases), _want(lm, cases)
    assert np.abs(got - want).max() <= LOOKUP_BAR, (got, want)
    assert abs(want[0] - (-0.5)) < 1e-6 and abs(want[4] - (-0.15 - 0.3 - 2.1)) < 1e-6 and abs(want[5] - (-0.1 - 2.1)) < 1e-6 and abs(want[8] - (-0.4 - 2.1)) < 1e-6
    bad = _score(dev, lm, [(0, 0, 5), (0, 5, 0), (-2, 0, 0), (0, 0, -1)])                      # ids outside the tables: NaN, nothing read
    assert np.isnan(bad).all()


def test_lookup_of_order_2_and_order_1_models(dev):
    full = _tiny_lm()
    words = [tuple(full.chars.index(ch) for ch in w) for w in full.words]
    bi_only = _hand_lm(4, words, full.unigrams, full.bigrams, None)
    uni_only = _hand_lm(4, words, full.unigrams, None, None)
    assert (full.order, bi_only.order, uni_only.order) == (3, 2, 1) and uni_only.bi_keys.numel() == 0 and bi_only.tri_keys.numel() == 0
    cases = [(4, 0, 1), (0, 1, 0), (1, 0, 3), (-1, 4, 0), (3, 3, 3)]
    for lm in (bi_only, uni_only):
        got, want = _score(dev, lm, cases), _want(lm, cases)
        assert np.abs(got - want).max() <= LOOKUP_BAR
    assert abs(_want(bi_only, cases)[0] - (-0.25 - 0.9)) < 1e-6 and abs(_want(uni_only, cases)[0] - (-0.3 - 1.7)) < 1e-6


def test_lookup_wraps_around_the_table_end_and_walks_the_longest_probe(dev):
    """64 slots forced; five bigrams and five trigrams whose home is the LAST slot: the probe sequences run 63, 0, 1, 2, 3, and the last key
    needs the recorded maximum of 5 probes.  Word id 0 and word id n_words - 1 are among them."""
    n = 300
    slots = 64
    pairs = [(a, b) for a in (0, n - 1, 7, n) for b in range(n)]
    home = rm._ngram_home([(a << 21) | b for a, b in pairs]) & np.uint64(slots - 1)
    bi_keys = [p for p, h in zip(pairs, home) if h == slots - 1][:5]
    apart = [p for p, h in zip(pairs, home) if 16 <= h < 48]             # two more bigrams, far from that run: word ids 0 and n - 1 on both sides
    extra = [next(p for p in apart if p[0] == 0), next(p for p in apart if p[0] == n - 1), next(p for p in apart if p[1] in (0, n - 1))]
    trips = [(a, b, c) for a, b in bi_keys[:2] + extra[:2] for c in range(n)]
    thome = rm._ngram_home([(a << 42) | (b << 21) | c for a, b, c in trips]) & np.uint64(slots - 1)
    tri_keys = [t for t, h in zip(trips, thome) if h == slots - 1][:5]
    assert len(bi_keys) == 5 and len(tri_keys) == 5
    rng = np.random.default_rng(4)
    uni = np.zeros((n + 1, 2))
    uni[:, 0], uni[:, 1] = -7 * rng.random(n + 1), -rng.random(n + 1)
    bi = {k: (-4 * rng.random(), -rng.random()) for k in bi_keys + extra}
    tri = {k: -4 * rng.random() for k in tri_keys}
    lm = rm.WordNgramLM(['w%d' % i for i in range(n)], uni, bi, tri, 'w0123456789 ', min_slots=slots)
    assert lm.bi_keys.numel() == slots and lm.tri_keys.numel() == slots and lm.bi_probe == 5 and lm.tri_probe == 5
    keys = lm.bi_keys.numpy()
    assert keys[slots - 1] != -1 and (keys[:4] != -1).all() and keys[4] == -1      # wrapped: the run starts in the last slot and goes on at the front
    tkeys = lm.tri_keys.numpy()
    assert tkeys[slots - 1] != -1 and (tkeys[:4] != -1).all() and tkeys[4] == -1
    cases = [(-1, a, b) for a, b in bi_keys] + list(tri_keys) + [(-1, a, b) for a, b in extra] + [(0, n - 1, 0), (n - 1, 0, n - 1), (-1, 0, n - 1), (-1, n - 1, 0), (5, 0, n - 1), (-1, -1, 0), (-1, -1, n - 1)]
    cases += [(a, b, (c + 1) % n) for a, b, c in tri_keys]              # misses that walk the same full runs
    got, want = _score(dev, lm, cases), _want(lm, cases)
    assert np.abs(got - want).max() <= LOOKUP_BAR
    for (a, b), g in zip(bi_keys, got[:5]):
        assert abs(g - float(bi[(a, b)][0])) <= LOOKUP_BAR
    for k, g in zip(tri_keys, got[5:10]):
        assert abs(g - float(np.float32(tri[k]))) <= LOOKUP_BAR


# ---------------------------------------------------------------------------------------------- 5. semantics
def test_best_path_spells_a_non_word_and_the_result_is_the_best_lexicon_word(dev):
    """Classes a, b, space, blank; the words ab and ba.  The frames say a, blank, a: the plain search returns "aa", which is no word."""
    lm = _hand_lm(4, [(0, 1), (1, 0)])
    x = _from_probs([[0.7, 0.2, 0.05, 0.05], [0.1, 0.1, 0.1, 0.7], [0.6, 0.3, 0.05, 0.05]])
    plain = torch.ops.silent_speech.ctc_beam_search(torch.from_numpy(x).to(dev), torch.tensor([[0, 3]], dtype=torch.int64).to(dev), 4, 3, 3, 3, 16, 1, None, 0.0, 0.0)
    assert plain[0][0, 0, :int(plain[1][0, 0])].tolist() == [0, 0]
    ranking = oracle.brute_force(x, 3, 2, oracle.Tables.of(lm, 3), ALPHA, BETA)
    out = _search(dev, lm, [x], 16, 3)
    assert _strings(out, 0) == [q for q, *_ in ranking[:3]]
    assert _strings(out, 0)[0] in ((0, 1), (1, 0)) and out[4][0, 0] == 1
    assert abs(float(out[2][0, 0]) - ranking[0][1]) < EXACT_BAR


def test_a_sentence_wins_only_through_its_trigram(dev):
    """The words a and b.  The frames spell "a b" and then a last word that is b by a small margin; the trigram (a, b, a) turns it into a.
    Without the trigram the result is "a b b"."""
    sp, bl = 2, 3
    hi = [0.9, 0.03, 0.03, 0.04]
    x = _from_probs([hi, [0.03, 0.03, 0.9, 0.04], [0.03, 0.9, 0.03, 0.04], [0.03, 0.03, 0.9, 0.04], [0.44, 0.48, 0.04, 0.04]])
    uni = np.array([[-0.7, 0.0], [-0.7, 0.0], [-99.0, 0.0]])
    with_tri = _hand_lm(4, [(0,), (1,)], uni, {}, {(0, 1, 0): -0.05})
    without = _hand_lm(4, [(0,), (1,)], uni, {}, {})
    for lm, want in ((with_tri, (0, sp, 1, sp, 0)), (without, (0, sp, 1, sp, 1))):
        ref = oracle.beam_search(x, bl, sp, 16, oracle.Tables.of(lm, bl), 1.0, 0.0, n_best=2)
        out = _search(dev, lm, [x], 16, 2, alpha=1.0, beta=0.0)
        assert ref[0][0] == want and _strings(out, 0) == [q for q, *_ in ref]
        assert abs(float(out[2][0, 0]) - ref[0][1]) < EXACT_BAR


@pytest.mark.parametrize('T', [0, 1, 2])
def test_short_utterances_mark_missing_ranks(dev, T):
    lm = _tiny_lm()
    x = _noise(np.random.default_rng(20 + T), 4, 4, 3, 1.5)[:T]
    ranking = oracle.brute_force(x, 3, 2, oracle.Tables.of(lm, 3), ALPHA, BETA)
    assert len(ranking) == {0: 1, 1: 3, 2: 6}[T]                         # "", a, b | and "a ", ab, ba ("b " ends no word, aa and bb start none)
    out = _search(dev, lm, [x, _noise(np.random.default_rng(1), 3, 4, 3, 1.5)], 128, 16)      # (a neighbour, so that T = 0 is not an empty launch)
    n = len(ranking)
    assert _strings(out, 0) == [q for q, *_ in ranking]
    assert max(abs(float(out[2][0, r]) - ranking[r][1]) for r in range(n)) < EXACT_BAR
    assert out[4][0, :n].tolist() == [int(done) for *_, done in ranking]
    assert (out[1][0, n:] == -1).all() and (out[2][0, n:] == -np.inf).all() and (out[3][0, n:] == -np.inf).all() and (out[4][0, n:] == -1).all()
    assert (out[0][0, n:] == -1).all()
    if T == 0:
        assert out[1][0, 0] == 0 and out[2][0, 0] == 0.0 and out[4][0, 0] == 1


def test_a_complete_entry_outranks_a_better_scoring_incomplete_one(dev):
    """The one word is ab.  The frames say a: "a" has almost all the mass but is no word and no word boundary; the empty string is complete."""
    lm = _hand_lm(4, [(0, 1)])
    x = _from_probs([[0.9, 0.03, 0.03, 0.04], [0.9, 0.03, 0.03, 0.04]])
    out = _search(dev, lm, [x], 8, 8)
    got, flags, scores = _strings(out, 0), out[4][0, :len(_strings(out, 0))].tolist(), out[2][0]
    assert got[0] != (0,) and (0,) in got and () in got
    i, j = got.index(()), got.index((0,))
    assert flags[i] == 1 and flags[j] == 0 and i < j and scores[j] > scores[i] + 3.0 and scores[j] == scores[:len(got)].max()
    assert flags == sorted(flags, reverse=True)                           # all complete entries, then the others
    ref = oracle.beam_search(x, 3, 2, 8, oracle.Tables.of(lm, 3), ALPHA, BETA, n_best=8)
    assert got == [q for q, *_ in ref] and flags == [int(r[3]) for r in ref]
    one = _search(dev, lm, [x], 1, 1)                                     # width 1 follows "a" and can only report an incomplete result
    assert _strings(one, 0) == [(0,)] and one[4][0, 0] == 0


# ---------------------------------------------------------------------------------------------- 6. isolation and layouts
def _iso_case():
    rng = np.random.default_rng(77)
    return _random_lm(6, 12, 3, 5), [_noise(rng, T, 6, 5, 2.5) for T in (13, 1, 9, 14, 5)]


def test_each_utterance_alone_equals_itself_in_a_batch_bit_for_bit(dev):
    lm, xs = _iso_case()
    L = max(x.shape[0] for x in xs)
    batch = _search(dev, lm, xs, 8, 3)
    assert _same(batch, _search(dev, lm, xs, 8, 3))                       # two runs of the same call
    for b, x in enumerate(xs):
        alone = _search(dev, lm, [x], 8, 3)
        assert np.array_equal(alone[0][0], batch[0][b, :, :alone[0].shape[2]]) and (batch[0][b, :, alone[0].shape[2]:] == -1).all()
        assert all(np.array_equal(alone[k][0], batch[k][b]) for k in (1, 2, 3, 4)), b
    assert batch[0].shape == (5, 3, L) and any(len(q) > 2 for q in (_strings(batch, b)[0] for b in range(5)))


def test_layouts_read_nothing_but_the_utterances(dev):
    lm, xs = _iso_case()
    want = _search(dev, lm, xs, 8, 3)
    assert _same(want, _search(dev, lm, xs, 8, 3, gaps=[3, 0, 7, 1, 5]))  # packed, first frames that are no multiple of anything, NaN between
    assert _same(want, _search(dev, lm, xs, 8, 3, layout='slots'))        # the slot layout of forward_utterances, NaN in every filler row
    assert _same(want, _search(dev, lm, xs, 8, 3, ld=11))                 # ld > V, NaN in the extra columns
    assert _same(want, _search(dev, lm, xs, 8, 3, layout='slots', ld=8))


# ---------------------------------------------------------------------------------------------- 7. host
CORPUS = ['the cat sat', 'the cat ran', 'the dog sat', 'a cat sat', 'the cat sat down', 'a dog ran', 'The Dog, ran.', 'down the cat', 'the cat', 'sat']


def test_word_ngram_lm_from_texts_equals_hand_counts():
    tt = rm.TextTransform()
    lm = rm.WordNgramLM.from_texts(CORPUS, tt, discount=0.75, add_k=0.5)
    assert lm.words == ['a', 'cat', 'dog', 'down', 'ran', 'sat', 'the'] and lm.n_words == 7 and lm.order == 3 and lm.start == 7
    a, cat, dog, down, ran, sat, the = range(7)
    S, N = 7, 28                                                         # 28 words in the ten lines
    assert sum(len(tt.clean_text(t).split()) for t in CORPUS) == N

    def p1(c):
        return (c + 0.5) / (N + 0.5 * 7)
    counts = {'the': 7, 'cat': 6, 'sat': 5, 'dog': 3, 'ran': 3, 'a': 2, 'down': 2}
    for w, c in counts.items():
        assert abs(float(lm.unigrams[lm.words.index(w), 0]) - math.log(p1(c))) < 1e-6
    # after "the": cat x5, dog x2 -- 7 in all
    assert abs(float(lm.bigrams[(the, cat)][0]) - math.log((5 - 0.75) / 7)) < 1e-6 and abs(float(lm.bigrams[(the, dog)][0]) - math.log((2 - 0.75) / 7)) < 1e-6
    bo_the = (1 - (5 - 0.75) / 7 - (2 - 0.75) / 7) / (1 - p1(6) - p1(3))
    assert abs(float(lm.unigrams[the, 1]) - math.log(bo_the)) < 1e-6
    # the lines start with: the x6, a x2, down, sat
    assert abs(float(lm.bigrams[(S, the)][0]) - math.log((6 - 0.75) / 10)) < 1e-6 and abs(float(lm.bigrams[(S, a)][0]) - math.log((2 - 0.75) / 10)) < 1e-6
    # after (the, cat): sat x2, ran x1 and twice the end of the line -- 3 in all
    assert abs(float(lm.trigrams[(the, cat, sat)]) - math.log((2 - 0.75) / 3)) < 1e-6 and abs(float(lm.trigrams[(the, cat, ran)]) - math.log((1 - 0.75) / 3)) < 1e-6
    # its backoff: what the discount took, over the bigram mass of the words not seen after (the, cat); after "cat": sat x3, ran x1 -- 4 in all
    p_cat_sat, p_cat_ran = (3 - 0.75) / 4, (1 - 0.75) / 4
    bo = (1 - (2 - 0.75) / 3 - (1 - 0.75) / 3) / (1 - p_cat_sat - p_cat_ran)
    assert abs(float(lm.bigrams[(the, cat)][1]) - math.log(bo)) < 1e-6
    assert (S, the, cat) in lm.trigrams and (cat, sat, down) in lm.trigrams and (the, cat, down) not in lm.trigrams
    # every seen context, and one unseen one, is a distribution over the vocabulary
    contexts = [(-1, S), (-1, the), (S, the), (the, cat), (cat, sat), (a, dog), (-1, down), (S, sat), (down, down), (ran, a)]
    assert (down, down) not in lm.bigrams and (ran, a) not in lm.bigrams
    for ctx in contexts:
        total = sum(math.exp(lm.score_words([w], context=ctx)[0]) for w in range(7))
        assert abs(total - 1.0) < 1e-6, (ctx, total)
    # a sentence through score_words: the start context, then trigram contexts
    s = lm.score_words([the, cat, sat])
    assert abs(s[0] - float(lm.bigrams[(S, the)][0])) < 1e-12 and abs(s[1] - float(lm.trigrams[(S, the, cat)])) < 1e-12 and abs(s[2] - float(lm.trigrams[(the, cat, sat)])) < 1e-12
    assert lm.score_words([the, cat], dtype=np.float32).dtype == np.float32 and lm.word_ids('The cat!', tt) == [the, cat]
    bi, uni = rm.WordNgramLM.from_texts(CORPUS, tt, order=2, add_k=0.5), rm.WordNgramLM.from_texts(CORPUS, tt, order=1, add_k=0.5)
    assert (bi.order, uni.order) == (2, 1) and not bi.trigrams and not uni.bigrams and bi.bigrams.keys() == lm.bigrams.keys()
    assert abs(sum(math.exp(uni.score_words([w], context=(the, cat))[0]) for w in range(7)) - 1.0) < 1e-6
    # the lexicon: root -> 'c' -> 'a' -> 't' spells cat; the space's column is empty; label numbers are indices into chars
    node = 0
    for ch in 'cat':
        node = int(lm.lex_child[node, tt.chars.index(ch)])
        assert node > 0
    assert int(lm.lex_word[node]) == cat and int(lm.lex_word[0]) == -1 and (lm.lex_child[:, tt.chars.index(' ')] == -1).all()
    assert tuple(lm.lex_child.shape) == (int(lm.lex_word.numel()), len(tt.chars)) and lm.lex_child.dtype == torch.int32
    assert sorted(int(w) for w in lm.lex_word if w >= 0) == list(range(7))


def _same_model(x, y, tol=0.0):
    assert x.words == y.words and x.chars == y.chars and x.bigrams.keys() == y.bigrams.keys() and x.trigrams.keys() == y.trigrams.keys()
    assert np.abs(x.unigrams[:-1] - y.unigrams[:-1]).max() <= tol and abs(float(x.unigrams[-1, 1] - y.unigrams[-1, 1])) <= tol
    assert all(abs(float(x.bigrams[k][i] - y.bigrams[k][i])) <= tol for k in x.bigrams for i in (0, 1))
    assert all(abs(float(x.trigrams[k] - y.trigrams[k])) <= tol for k in x.trigrams)
    assert torch.equal(x.lex_child, y.lex_child) and torch.equal(x.lex_word, y.lex_word) and torch.equal(x.bi_keys, y.bi_keys) and torch.equal(x.tri_keys, y.tri_keys)
    assert (x.bi_probe, x.tri_probe) == (y.bi_probe, y.tri_probe)


def test_write_arpa_from_arpa_and_save_load_reproduce_the_tables(tmp_path):
    tt = rm.TextTransform()
    lm = rm.WordNgramLM.from_texts(CORPUS, tt, add_k=0.5)
    path = str(tmp_path / 'lm.arpa')
    lm.write_arpa(path)
    back = rm.WordNgramLM.from_arpa(path, tt)
    _same_model(lm, back, 2e-6)                                           # 9 significant digits of log10 in the text: below one f32 ulp of values < 16
    with open(path) as f:
        _same_model(back, rm.WordNgramLM.from_arpa(f, tt))
    npz = str(tmp_path / 'lm.npz')
    lm.save(npz)
    again = rm.WordNgramLM.load(npz)
    _same_model(lm, again)
    assert torch.equal(again.bi_val, lm.bi_val) and torch.equal(again.tri_val, lm.tri_val) and torch.equal(again.uni, lm.uni)
    assert lm.to('cpu').n_words == 7 and lm.to('cpu').order == 3


ARPA = """
\\data\\
ngram 1=9
ngram 2=5
ngram 3=2

\\1-grams:
-99\t<s>\t-0.5
-1.0\t</s>
-2.0\t<unk>\t-0.1
-0.6\tHello\t-0.3
-0.9\tworld!
-1.5\thello\t-0.2
-1.2\tcaf\u00e9\t-0.4
-1.1\tit's\t-0.25
-1.3\t...

\\2-grams:
-0.2\t<s> Hello\t-0.15
-0.4\tHello world!
-0.7\tworld! </s>
-0.3\tHello caf\u00e9\t-0.1
-0.5\tit's Hello

\\3-grams:
-0.1\t<s> Hello world!
-0.35\tHello world! caf\u00e9

\\end\\
""".replace('\\', '\\')


def test_from_arpa_reads_a_hand_written_file():
    tt = rm.TextTransform()
    lm = rm.WordNgramLM.from_arpa(io.StringIO(ARPA), tt)
    # "Hello" (-0.6) beats "hello" (-1.5) for the spelling hello; "café" cannot be spelled, "..." cleans to nothing; "it's" becomes its
    assert lm.words == ['hello', 'its', 'world'] and lm.start == 3 and lm.order == 3
    hello, its, world, S = 0, 1, 2, 3
    ln10 = math.log(10.0)
    assert abs(float(lm.unigrams[hello, 0]) + 0.6 * ln10) < 1e-6 and abs(float(lm.unigrams[hello, 1]) + 0.3 * ln10) < 1e-6
    assert abs(float(lm.unigrams[world, 0]) + 0.9 * ln10) < 1e-6 and float(lm.unigrams[world, 1]) == 0.0          # a missing backoff is 0
    assert abs(float(lm.unigrams[S, 1]) + 0.5 * ln10) < 1e-6 and lm.unigrams.dtype == np.float32
    assert set(lm.bigrams) == {(S, hello), (hello, world), (its, hello)}                                         # </s> and café n-grams are gone
    assert abs(float(lm.bigrams[(S, hello)][0]) + 0.2 * ln10) < 1e-6 and abs(float(lm.bigrams[(S, hello)][1]) + 0.15 * ln10) < 1e-6
    assert float(lm.bigrams[(hello, world)][1]) == 0.0
    assert set(lm.trigrams) == {(S, hello, world)} and abs(float(lm.trigrams[(S, hello, world)]) + 0.1 * ln10) < 1e-6
    s = lm.score_words([hello, world, its])
    want = [-0.2 * ln10, -0.1 * ln10, (0.0 + 0.0 - 1.1) * ln10]          # trigram miss, context (hello, world) has no backoff, bigram miss, bo(world) = 0
    assert np.abs(s - np.array(want)).max() < 1e-6


def test_an_order_4_arpa_file_raises():
    text = ARPA.replace('ngram 3=2', 'ngram 3=2\nngram 4=1').replace('\\end\\', '\\4-grams:\n-0.1\t<s> Hello world! Hello\n\n\\end\\')
    with pytest.raises(ValueError):
        rm.WordNgramLM.from_arpa(io.StringIO(text), rm.TextTransform())


# ---------------------------------------------------------------------------------------------- 8. ops
def _args(dev, **kw):
    lm = kw.pop('model', None) or _random_lm(6, 12, 3, 5)
    x = _noise(np.random.default_rng(5), 12, 6, 5, 2.0)
    t = lm.to(dev)
    a = dict(logits=torch.from_numpy(x).to(dev), utt=torch.tensor([[0, 7], [7, 5]], dtype=torch.int64).to(dev), V=6, blank=5, space=4, total_frames=12, max_len=7,
             beam_width=4, n_best=2, lex_child=t.lex_child, lex_word=t.lex_word, uni=t.uni, bi_keys=t.bi_keys, bi_val=t.bi_val, tri_keys=t.tri_keys, tri_val=t.tri_val,
             n_vocab=t.n_words, start=t.start, bi_probe=t.bi_probe, tri_probe=t.tri_probe, alpha=0.8, beta=0.5)
    a.update(kw)
    return tuple(a.values())


def test_ops_are_registered_and_pass_opcheck(dev):
    assert 'ctc_word_beam_search' in torch_ops.OPS and 'word_ngram_score' in torch_ops.OPS
    torch.library.opcheck(torch.ops.silent_speech.ctc_word_beam_search.default, _args(dev), test_utils=('test_schema', 'test_faketensor'))
    uni_only = rm.WordNgramLM(['%s' % chr(0x100 + i) for i in range(4)], np.zeros((5, 2)), None, None, _chars(6))
    torch.library.opcheck(torch.ops.silent_speech.ctc_word_beam_search.default, _args(dev, model=uni_only), test_utils=('test_schema', 'test_faketensor'))
    t = _random_lm(6, 12, 3, 5).to(dev)
    triples = torch.tensor([[-1, 12, 0], [0, 1, 2]], dtype=torch.int32).to(dev)
    torch.library.opcheck(torch.ops.silent_speech.word_ngram_score.default, (triples, t.uni, t.bi_keys, t.bi_val, t.tri_keys, t.tri_val, t.bi_probe, t.tri_probe),
                          test_utils=('test_schema', 'test_faketensor'))


@pytest.mark.parametrize('bad', [dict(beam_width=0), dict(beam_width=129), dict(n_best=5), dict(n_best=0), dict(space=5), dict(space=6), dict(space=-1),
                                 dict(blank=6), dict(V=129), dict(V=7), dict(max_len=0), dict(lex_child='wrong shape'), dict(lex_word='wrong shape'),
                                 dict(uni='other device'), dict(bi_keys='other device'), dict(start=13), dict(n_vocab=14), dict(bi_probe=1 << 20),
                                 dict(tri_val='wrong shape')])
def test_bad_arguments_raise(dev, bad):
    good = _args(dev)
    names = ['logits', 'utt', 'V', 'blank', 'space', 'total_frames', 'max_len', 'beam_width', 'n_best', 'lex_child', 'lex_word', 'uni', 'bi_keys', 'bi_val',
             'tri_keys', 'tri_val', 'n_vocab', 'start', 'bi_probe', 'tri_probe', 'alpha', 'beta']
    (name, what), = bad.items()
    t = good[names.index(name)]
    if what == 'wrong shape':
        what = {'lex_child': lambda: t[:, :-1].contiguous(), 'lex_word': lambda: t[:-1].contiguous(), 'tri_val': lambda: t[:t.numel() // 2].contiguous()}[name]()
    elif what == 'other device':
        what = t.cpu() if t.is_cuda else t.double()                       # tables that are not where the logits are (the emulator has one device: a wrong dtype)
    with pytest.raises(RuntimeError):
        torch.ops.silent_speech.ctc_word_beam_search(*_args(dev, **{name: what}))
    labels, lengths, _, _, complete = torch.ops.silent_speech.ctc_word_beam_search(*good)         # and the library is fine afterwards
    assert tuple(labels.shape) == (2, 2, 7) and int(lengths.min()) >= 0 and int(complete.min()) >= 0


def test_word_ngram_score_refuses_bad_tables(dev):
    t = _random_lm(6, 12, 3, 5).to(dev)
    triples = torch.tensor([[-1, 12, 0]], dtype=torch.int32).to(dev)
    good = (triples, t.uni, t.bi_keys, t.bi_val, t.tri_keys, t.tri_val, t.bi_probe, t.tri_probe)
    for i, bad in [(0, triples.long()), (0, triples[:, :2].contiguous()), (1, t.uni[:1].contiguous()), (2, t.bi_keys[:-1].contiguous()), (3, t.bi_val.cpu() if t.bi_val.is_cuda else t.bi_val.double()), (7, 1 << 20)]:
        with pytest.raises(RuntimeError):
            torch.ops.silent_speech.word_ngram_score(*(good[:i] + (bad,) + good[i + 1:]))
    assert torch.isfinite(torch.ops.silent_speech.word_ngram_score(*good)).all()


# ---------------------------------------------------------------------------------------------- 9. recognition_model.test with a WordNgramLM
@pytest.mark.parametrize('branch', ['single', 'whole', 'packed'])
def test_recognition_test_with_a_word_lm(dev, monkeypatch, branch):
    """test(..., decoder='beam', lm=WordNgramLM) in its three branches: every predicted word is a word of the lexicon, the strings are the
    oracle's on the model's own logits, and the returned number is the WER of those strings."""
    from tests.test_ctc_beam import _dataset, _references
    ds, m = _dataset(dev, 1 if is_emu(dev) and branch == 'single' else None)
    tt, V = ds.text_transform, len(ds.text_transform.chars) + 1
    lm = rm.WordNgramLM.from_texts(_references(ds) + CORPUS, tt)          # (the transcripts, and a few more words to choose among)
    assert lm.n_words > 7
    seen = []
    if branch == 'whole':
        real = Model.forward_utterances

        def keep(self, raws):
            out = real(self, raws)
            seen.append(out)
            return out
        monkeypatch.setattr(Model, 'forward_utterances', keep)
        kw = dict(batch_size=4, whole_utterances=True)
    else:
        real = Model.forward

        def keep(self, *a, **k):
            out = real(self, *a, **k)
            seen.append(out)
            return out
        monkeypatch.setattr(Model, 'forward', keep)
        kw = dict(batch_size=1) if branch == 'single' else dict(batch_size=4)
    search = dict(beam_width=8, lm=lm, alpha=1.5, beta=1.85)
    got = rm.test(m, ds, dev, decoder='beam', **search, **kw)
    assert seen
    space = tt.chars.index(' ')
    decoded, logits_of = [], []
    if branch == 'whole':
        for logits in seen:
            decoded += rm.beam_decode_utterances(logits, space=space, **search)
            logits_of += [y.cpu().numpy() for y in logits]
    else:
        lengths = [[p.shape[1]] for p in seen] if branch == 'single' else \
            [b['lengths'] for b in torch.utils.data.DataLoader(ds, batch_size=4, collate_fn=ds.collate_raw)]
        assert len(lengths) == len(seen)
        for pred, ls in zip(seen, lengths):
            decoded += rm.beam_decode(pred, ls, V - 1, space=space, **search)
            flat, at = pred.reshape(-1, V).cpu().numpy(), 0
            for n in ls:
                logits_of.append(flat[at:at + int(n)])
                at += int(n)
    texts = [tt.int_to_text(q) for q in decoded]
    assert len(texts) == len(ds)
    assert got == rm.wer(_references(ds), texts)
    vocabulary = set(lm.words)
    assert all(w in vocabulary for t in texts for w in t.split(' ') if w) and all('  ' not in t and not t.startswith(' ') for t in texts)
    tab = oracle.Tables.of(lm, V - 1)
    same = sum(list(oracle.beam_search(x, V - 1, space, 8, tab, 1.5, 1.85)[0][0]) == q for x, q in zip(logits_of, decoded))
    print('%s: %d of %d strings equal the oracle\'s' % (branch, same, len(decoded)))
    assert same >= 0.9 * len(decoded)
    with pytest.raises(ValueError):
        rm.test(m, ds, dev, decoder='beam', lm=(rm.LabelNgramLM.from_texts(_references(ds), tt), lm), **kw)
