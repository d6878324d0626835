"""Lexicon-constrained CTC prefix beam search with a word n-gram of any order up to 6 held as context states (csrc/ctc_word_state_decode.hip,
torch.ops.silent_speech.ctc_word_state_beam_search and word_state_score, recognition_model.WordStateLM / beam_decode* / test): the lookup alone
against the full-history backoff rule of tests/ctc_word_state_oracle.py (plain Python, no states) and, for models of order <= 3, against the table
path number for number; the oracle against the exact ranking of all allowed label strings; the device against that ranking where nothing is
pruned, against the float64 oracle where the beam prunes and against ctc_word_beam_search on the same order-3 model; layouts and batches bit for
bit; the host builders, the ops and recognition_model.test.

Score bars.  Lookup: `_lookup_bar(order)`, derived there.  Exact regime (T <= 7, at most 4 words, |score| < 32, asserted): the derivation of
tests/test_ctc_word_beam.py -- a frame costs a prefix one log-add-exp and one addition, a word one multiply-add and one addition, each rounded to
at most one f32 ulp of the running value (< 2^-19 below 32), plus one ulp of the hardware exp2 / log2 on a term <= ln 2 per frame; the third
unit of a word covers the lookup's own sum (at most 4 backoffs added to a probability, magnitudes below 2 in the hand models, so every partial
sum is below 16 and the 4 additions cost at most 4 x 2^-21 = 2^-19) -- (frames + words) x 3 roundings x 2^-19 = `_exact_bar(frames, words)`,
6.3e-5 for 7 frames and 4 words.  Pruned regime: per shape, 4 x the largest deviation (top-1 score or its CTC part) of the oracle's OWN float32
run from its float64 run on these inputs (measured on the CPU, listed in PRUNED; the factor covers the hardware exp2 / log2 and another
summation order).  The lexicon seeds of PRUNED were chosen with the oracle alone so that its float32 run agrees with its float64 run on top-1,
top-3 and the complete flags of EVERY utterance of every shape, so the 90 % cap is not what lets the kernel pass."""
import collections
import io
import math

import numpy as np
import pytest
import torch

from silent_speech_amd import _lib
from silent_speech_amd import recognition_model as rm
from silent_speech_amd import torch_ops
from silent_speech_amd.architecture import Model
from tests import backend
from tests import ctc_word_state_oracle as oracle
from tests import test_ctc_word_beam as sibling                          # its model builders, ARPA text and corpus (the module, so that none of its tests is collected here)
from tests.backend import dev, is_emu  # noqa: F401
from tests.ctc_beam_helpers import from_probs as _from_probs, layout as _layout, noise as _noise, same as _same, strings as _strings

ALPHA, BETA = 0.8, 0.5


def _exact_bar(frames, words):
    return (frames + words) * 3 * 2.0 ** -19


def _lookup_bar(order):
    """Table magnitudes stay below 8 and a score sums at most `order` of them (order - 1 backoffs and a probability), so every partial sum is
    below 8 order <= 2^e, e = ceil(log2(8 order)), where an f32 addition costs at most half an ulp = 2^(e - 25); order - 1 additions against the
    float64 sum of the same f32 table entries, doubled: 2 (order - 1) 2^(e - 25) -- 1.9e-5 for order 6, 5.7e-6 for order 4."""
    e = math.ceil(math.log2(8 * order))
    return 2 * (order - 1) * 2.0 ** (e - 25)


def _tables(lm, dev):
    lm = lm.to(dev)
    return (lm.lex_child, lm.lex_word, lm.uni_logp, lm.st_bo, lm.st_shorter, lm.arc_keys, lm.arc_logp, lm.arc_next, lm.n_words, lm.start_state, lm.arc_probe, lm.order)


def _search(dev, lm, utts, W, n_best, alpha=ALPHA, beta=BETA, **how):
    """utts: list of (T_i, V) float32 arrays, laid out by ctc_beam_helpers.layout(**how).  Returns numpy (labels, lengths, scores, ctc scores, complete)."""
    flat, utt, V, total, longest = _layout(dev, utts, **how)
    out = torch.ops.silent_speech.ctc_word_state_beam_search(flat, utt, V, V - 1, V - 2, total, longest, W, n_best, *_tables(lm, dev), alpha, beta)
    return tuple(t.cpu().numpy() for t in out)


def _score(dev, lm, pairs):
    lm = lm.to(dev)
    lnp, nxt = lm.score_states(torch.tensor(pairs, dtype=torch.int32).reshape(len(pairs), 2).to(dev))
    return lnp.cpu().numpy(), nxt.cpu().numpy()


def _hand_lm(V, words, ngrams, order=None, min_slots=0):
    """words as tuples of letter classes"""
    chars = sibling._chars(V)
    return rm.WordStateLM([''.join(chars[c] for c in w) for w in words], ngrams, chars, order, min_slots)


def _random_lm(V, n_words, max_letters, seed, order, longest=None, per=4, hubs=None, cap=400):
    """A seeded random lexicon of n_words words of 1 .. max_letters letters and a random PREFIX-CLOSED model: every context word gets `per`
    bigrams; on every further level (up to `longest`, default the order) at most `cap` n-grams of the level below become contexts with `per`
    n-grams each.  hubs: that many of the shortest words are the ones the n-grams of >= 3 words continue with (and half of the bigrams), and
    contexts made of them come first under the cap -- a search over noise then meets the high levels often enough to test them."""
    rng = np.random.default_rng(seed)
    chars = sibling._chars(V)
    words = set()
    while len(words) < n_words:
        words.add(''.join(chars[i] for i in rng.integers(0, V - 2, rng.integers(1, max_letters + 1))))
    words = sorted(words)
    n = len(words)
    hub = sorted(range(n), key=lambda w: (len(words[w]), w))[:hubs] if hubs else list(range(n))
    is_hub = set(hub)
    x = rng.standard_normal(n) * 1.5
    grams = {(w,): (float(x[w] - np.log(np.exp(x).sum())), -float(rng.random())) for w in range(n)}
    grams[(n,)] = (-7.5, -float(rng.random()))
    level = sorted(grams)
    for k in range(2, (longest or order) + 1):
        if k > 2:
            level = [level[i] for i in rng.permutation(len(level))]
            level.sort(key=lambda g: sum(w not in is_hub for w in g))     # stable: fewest words outside the hubs first
            level = level[:cap]
        new = {}
        for h in level:
            if k == 2 and hubs:
                ws = np.concatenate([rng.choice(hub, per // 2, replace=False), rng.choice(n, per - per // 2, replace=False)])
            else:
                ws = rng.choice(hub, min(per, len(hub)), replace=False)
            for w in ws:
                new[h + (int(w),)] = (-4 * float(rng.random()), -float(rng.random()) if k < order else 0.0)
        grams.update(new)
        level = sorted(new)
    return rm.WordStateLM(words, grams, chars, order)


# ---------------------------------------------------------------------------------------------- 1. the lookup alone
# five words 0 .. 4, the start context S = 5, order 5.  The chains (S, 0, 1, 2, 3) and (0, 1, 2, 3, 4) reach every level; (2, 3, 0) is a state
# whose longest shorter state is (0): (3, 0) is no n-gram, so its suffix link skips the bigram level
def _order5_lm(min_slots=0):
    S = 5
    g = {(0,): (-1.0, -0.3), (1,): (-1.7, -0.2), (2,): (-1.2, -0.6), (3,): (-2.1, -0.1), (4,): (-1.9, -0.7), (S,): (-7.5, -0.4),
         (S, 0): (-0.7, -0.25), (0, 1): (-0.9, -0.35), (1, 2): (-0.4, -0.15), (2, 3): (-1.3, -0.45), (1, 0): (-1.9, -0.2), (3, 4): (-0.8, -0.55),
         (S, 0, 1): (-0.5, -0.05), (0, 1, 2): (-0.6, -0.65), (1, 2, 3): (-1.4, -0.75), (2, 3, 0): (-1.1, -0.85),
         (S, 0, 1, 2): (-0.3, -0.95), (0, 1, 2, 3): (-0.2, -0.12), (2, 3, 0, 1): (-1.6, -0.22),
         (S, 0, 1, 2, 3): (-0.15, 0.0), (0, 1, 2, 3, 4): (-0.45, 0.0)}
    return _hand_lm(7, [(0,), (1,), (2,), (3,), (4,)], g, 5, min_slots)


def _check_lookup(dev, lm, histories_and_words, bar):
    """lnp against the float64 full-history rule, next by MEANING: its context is the longest known suffix of history + word."""
    tab = oracle.Tables.of(lm, len(lm.chars))
    pairs = [(lm.state_of(h), w) for h, w in histories_and_words]
    lnp, nxt = _score(dev, lm, pairs)
    want = np.array([tab.lnp(h, w) for h, w in histories_and_words])
    assert np.isfinite(lnp).all() and np.abs(lnp - want).max() <= bar, np.abs(lnp - want).max()
    for (h, w), s in zip(histories_and_words, nxt):
        assert lm.context_of(s) == tab.known_context(tuple(h) + (w,)), (h, w, int(s))
    return lnp, nxt, tab


def test_lookup_hits_and_misses_at_every_level_of_an_order_5_model(dev):
    lm = _order5_lm()
    S = lm.start
    assert lm.order == 5 and lm.start_state == 6 and lm.n_states == 1 + 6 + 6 + 4 + 3 and lm.context_of(lm.start_state) == (S,)
    assert lm.context_of(lm.st_shorter[lm.state_of((2, 3, 0))]) == (0,)   # the link that skips a level
    assert all(int(lm.st_shorter[s]) < s for s in range(1, lm.n_states))
    cases = [((S, 0, 1, 2), 3),        # 0: the 5-gram
             ((4, 0, 1, 2), 3),        # 1: (4, 0, 1, 2) is unknown, the state is (0, 1, 2): the 4-gram (0, 1, 2, 3)
             ((S, 0, 1), 2),           # 2: a context shorter than order - 1 words: the 4-gram (S, 0, 1, 2)
             ((0, 1), 2),              # 3: the trigram
             ((3,), 4),                # 4: the bigram
             ((), 2),                  # 5: the empty context: the unigram
             ((S, 0, 1, 2), 0),        # 6: a miss at every level: four backoffs and the unigram
             ((2, 3, 0), 4),           # 7: a miss through the link that skips a level: bo(2, 3, 0) + bo(0) + uni(4)
             ((2, 3, 0), 1),           # 8: the 4-gram (2, 3, 0, 1), which is itself the state behind it
             ((S,), 0),                # 9: the start context: a bigram
             ((S,), 3),                # 10: the start context, no bigram
             ((0, 1, 2, 3), 4),        # 11: the 5-gram without the start
             ((1, 2, 3), 4),           # 12: no 4-gram (1, 2, 3, 4), no trigram (2, 3, 4): two backoffs and the bigram (3, 4)
             ((1, 0), 1)]              # 13: state (1, 0): no arc; its link leads to (0), which has the bigram (0, 1)
    lnp, nxt, tab = _check_lookup(dev, lm, cases, _lookup_bar(5))
    hand = {0: -0.15, 1: -0.2, 2: -0.3, 3: -0.6, 4: -0.8, 5: -1.2, 6: -0.95 - 0.65 - 0.15 - 0.6 - 1.0, 7: -0.85 - 0.3 - 1.9, 8: -1.6, 9: -0.7,
            10: -0.4 - 2.1, 11: -0.45, 12: -0.75 - 0.45 - 0.8, 13: -0.2 - 0.9}
    for i, v in hand.items():
        assert abs(lnp[i] - v) < 1e-5, (i, lnp[i], v)
    assert lm.context_of(nxt[0]) == (0, 1, 2, 3) and lm.context_of(nxt[8]) == (2, 3, 0, 1) and lm.context_of(nxt[13]) == (0, 1) and lm.context_of(nxt[6]) == (0,) and lm.context_of(nxt[5]) == (2,)
    assert {tab.levels[k] > 0 for k in (1, 2, 3, 4, 5)} == {True}
    host = np.array([lm.score_words([w], context=h if h else (-1,))[0] for h, w in cases])
    assert np.abs(host - lnp).max() <= _lookup_bar(5)
    bad, bad_next = _score(dev, lm, [(lm.n_states, 0), (-1, 0), (0, 6), (0, -1), (1 << 30, 1 << 30)])        # ids outside the tables: NaN and -1, nothing read
    assert np.isnan(bad).all() and (bad_next == -1).all()


@pytest.mark.parametrize('order,longest,n_words,seed', [(4, 4, 7, 1), (5, 5, 9, 2), (6, 6, 12, 3), (6, 4, 8, 4)])
def test_lookup_of_random_prefix_closed_models_equals_the_full_history_rule(dev, order, longest, n_words, seed):
    """Every state x every word, and 3 000 random histories of order - 1 words mapped through state_of.  (6, 4): the longest n-gram is shorter
    than the order."""
    lm = _random_lm(6, n_words, 2, seed, order, longest, per=3, cap=60)
    n = lm.n_words
    assert max(len(g) for g in lm.ngrams) == longest and lm.order == order
    cases = [(lm.context_of(s), w) for s in range(lm.n_states) for w in range(n)]
    rng = np.random.default_rng(seed)
    for _ in range(3000):
        h = [int(w) for w in rng.integers(0, n, order - 1)]
        if rng.random() < 0.2:
            h[0] = lm.start
        cases.append((tuple(h), int(rng.integers(0, n))))
    _, _, tab = _check_lookup(dev, lm, cases, _lookup_bar(order))
    assert all(tab.levels[k] > 0 for k in range(1, longest + 1)) and not any(tab.levels[k] for k in range(longest + 1, 8))


def test_models_of_order_3_and_below_give_the_numbers_of_the_table_path(dev):
    """from_ngram_lm of a WordNgramLM: score_states at state_of of the context == score_triples, as f32, for every (w2, w1, w)."""
    full = sibling._tiny_lm()
    words = [tuple(full.chars.index(ch) for ch in w) for w in full.words]
    models = [sibling._random_lm(6, 12, 3, 5), full, sibling._hand_lm(4, words, full.unigrams, full.bigrams, None), sibling._hand_lm(4, words, full.unigrams, None, None)]
    for table in models:
        lm = rm.WordStateLM.from_ngram_lm(table)
        assert lm.order == 3 and all(lm.context_of(lm.state_of(g)) == g for g in table.bigrams)
        n = table.n_words
        triples = [(w2, w1, w) for w1 in range(-1, n + 1) for w2 in (range(-1, n + 1) if w1 >= 0 else [-1]) for w in range(n)]
        want = table.to(dev).score_triples(torch.tensor(triples, dtype=torch.int32).to(dev)).cpu().numpy()
        got, _ = _score(dev, lm, [(lm.state_of([x for x in (w2, w1) if x >= 0]), w) for w2, w1, w in triples])
        assert got.dtype == np.float32 and want.dtype == np.float32 and (got == want).all(), np.abs(got - want).max()


def test_lookup_wraps_around_the_table_end_and_walks_the_longest_probe(dev):
    """64 slots forced; five arcs whose home is the LAST slot -- three bigrams out of unigram states (the low end of the state ids) and two
    trigrams out of bigram states (the high end) --: the probe sequences run 63, 0, 1, 2, 3 and the last key needs the recorded maximum of 5
    probes.  Word ids 0 and n_words - 1 are among the keys and the lookups."""
    n, slots, mask = 300, 64, np.uint64(63)
    pairs = [(a, b) for a in (0, n - 1, 7, n) for b in range(n)]
    home = rm._ngram_home([((1 + a) << 21) | b for a, b in pairs]) & mask
    last = [p for p, h in zip(pairs, home) if h == slots - 1]
    apart = [p for p, h in zip(pairs, home) if 16 <= h < 48]
    bigrams = last[:3] + [next(p for p in apart if p[0] == 0 and p[1] != 0), next(p for p in apart if p[0] == n - 1 and p[1] != n - 1)]
    state = {g: 1 + (n + 1) + i for i, g in enumerate(sorted(bigrams))}   # order 3: the bigrams are the states behind the unigrams
    trips = [g + (c,) for g in bigrams for c in (0, n - 1) + tuple(range(1, n - 1))]
    thome = rm._ngram_home([(state[t[:2]] << 21) | t[2] for t in trips]) & mask
    at_last = [t for t, h in zip(trips, thome) if h == slots - 1]
    trigrams, absent = at_last[:2], at_last[2:4] + last[3:5]              # absent: keys with the same home that are not in the table
    assert len(trigrams) == 2 and len(absent) == 4
    rng = np.random.default_rng(4)
    grams = {(w,): (-7 * rng.random(), -rng.random()) for w in range(n + 1)}
    grams.update({g: (-4 * rng.random(), -rng.random()) for g in bigrams})
    grams.update({g: (-4 * rng.random(), 0.0) for g in trigrams})
    lm = rm.WordStateLM(['w%d' % i for i in range(n)], grams, 'w0123456789 ', 3, min_slots=slots)
    assert lm.arc_keys.numel() == slots and lm.arc_probe == 5 and lm.n_states == 1 + (n + 1) + 5 and [lm._state[g] for g in sorted(bigrams)] == sorted(state.values())
    keys = lm.arc_keys.numpy()
    assert keys[slots - 1] != -1 and (keys[:4] != -1).all() and keys[4] == -1       # wrapped: the run starts in the last slot and goes on at the front
    cases = [(g[:-1], g[-1]) for g in bigrams + trigrams + absent]        # hits and misses that walk the full run
    cases += [((0,), n - 1), ((n - 1,), 0), ((), 0), ((), n - 1), ((n,), 0), (bigrams[3], n - 1), (bigrams[4], 0), (trigrams[0][:2], 0), (trigrams[1][:2], n - 1), (sorted(bigrams)[-1], 0)]
    assert {0, 1, lm.n_states - 1} <= {lm.state_of(h) for h, _ in cases}    # states from both ends of the id range
    lnp, _, _ = _check_lookup(dev, lm, cases, _lookup_bar(3))
    for g, v in zip(bigrams + trigrams, lnp):
        assert abs(v - float(lm.ngrams[g][0])) <= _lookup_bar(3)


def test_malformed_suffix_links_end_on_the_emulator():
    """Emulator tier only, never a GPU: a st_shorter that points at itself or outside the table and next states outside it.  The lookup's link
    walk is a counted loop and every id is range-checked, so the call returns, every value is a float or NaN and every next state is inside
    the table."""
    backend._ensure_emu()
    _lib.use_library_for_testing(backend.EMU)
    lm = _order5_lm()
    n_states = lm.n_states
    shorter, nxt = lm.st_shorter.clone(), lm.arc_next.clone()
    shorter[1:] = torch.arange(1, n_states, dtype=torch.int32)            # every link points at its own state
    shorter[7], shorter[9], shorter[11] = n_states + 5, -3, 2 ** 31 - 1
    nxt[::2], nxt[1::4] = 2 ** 31 - 1, -7
    pairs = torch.tensor([(s, w) for s in range(n_states) for w in range(lm.n_words + 1)], dtype=torch.int32)
    lnp, to = torch.ops.silent_speech.word_state_score(pairs, lm.uni_logp, lm.st_bo, shorter, lm.arc_keys, lm.arc_logp, nxt, lm.arc_probe, lm.order)
    assert lnp.dtype == torch.float32 and lnp.shape == (len(pairs),) and not torch.isinf(lnp).any()
    assert int(to.min()) >= 0 and int(to.max()) < n_states
    x = _noise(np.random.default_rng(0), 9, 7, 6, 2.0)
    flat, utt, V, total, longest = _layout(torch.device('cpu'), [x])
    out = torch.ops.silent_speech.ctc_word_state_beam_search(flat, utt, V, V - 1, V - 2, total, longest, 8, 3, lm.lex_child, lm.lex_word, lm.uni_logp, lm.st_bo,
                                                             shorter, lm.arc_keys, lm.arc_logp, nxt, lm.n_words, lm.start_state, lm.arc_probe, lm.order, ALPHA, BETA)
    assert int(out[1][0, 0]) >= 0


# ---------------------------------------------------------------------------------------------- 2. the oracle against brute force
# classes a = 0, b = 1, space = 2, blank = 3; the words a, b, ab; n-grams that reach every level along "a b a b"
def _tiny_lm(order):
    S = 3
    g = {(0,): (-1.0, -0.3), (1,): (-1.3, -0.2), (2,): (-1.6, -0.6), (S,): (-7.5, -0.4),
         (S, 0): (-0.7, -0.25), (0, 1): (-0.9, -0.35), (1, 0): (-0.4, -0.15), (0, 0): (-1.9, -0.2), (S, 2): (-1.1, -0.5),
         (S, 0, 1): (-0.5, -0.45), (0, 1, 0): (-0.6, -0.55), (1, 0, 1): (-0.8, -0.1), (0, 0, 2): (-1.4, -0.05),
         (S, 0, 1, 0): (-0.3, -0.65), (0, 1, 0, 1): (-0.2, -0.75),
         (S, 0, 1, 0, 1): (-0.1, 0.0)}
    g = {k: (v[0], v[1] if len(k) < order else 0.0) for k, v in g.items() if len(k) <= order}
    return _hand_lm(4, [(0,), (1,), (0, 1)], g, order)


EXACT_CASES = [(4, 5, 1), (4, 6, 0), (5, 7, 3)]                          # (order, T, seed of the frames): seeds chosen with brute force alone, see _exact_case
_EXACT = {}


@pytest.mark.parametrize('order,T,seed', [(4, 5, 0), (4, 5, 1), (4, 6, 2), (5, 7, 3)])
def test_oracle_reproduces_the_exact_ranking_of_every_allowed_string(order, T, seed):
    """With a beam at least as wide as the number of prefixes, every prefix's final score is the exact float64 log-likelihood of that label
    string (oracle/ctc_ref.ctc_utterance over all strings of up to T labels the lexicon allows) + alpha score_words + beta n_words."""
    lm = _tiny_lm(order)
    tab = oracle.Tables.of(lm, 3)
    x = _noise(np.random.default_rng(seed), T, 4, 3, 1.5)
    exact = oracle.brute_force(x, 3, 2, tab, ALPHA, BETA)
    got = oracle.beam_search(x, 3, 2, 4 ** 8, tab, ALPHA, BETA, n_best=4 ** 8)
    assert len(exact) == len(got) > 2 * T
    want = {q: (s, ll, done) for q, s, ll, done in exact}
    for q, score, ctc, done in got:
        assert abs(score - want[q][0]) < 1e-9 and abs(ctc - want[q][1]) < 1e-9 and done == want[q][2], q
        # the brute-force score restated through the model's own host rule: alpha * score_words + beta per word
        words = bytes(q).split(bytes([2]))
        ids = [tab.word_of[w] for w in words if w in tab.word_of]
        n_scored = len(words) - 1 + (words[-1] in tab.word_of)
        assert len(ids) == n_scored
        assert abs(score - ctc - (ALPHA * lm.score_words(ids).sum() + BETA * n_scored)) < 1e-6
    assert [q for q, *_ in got[:8]] == [q for q, *_ in exact[:8]]
    assert not any(done for *_, done in exact[sum(done for *_, done in exact):])     # complete strings first
    assert all(tab.levels[k] > 0 for k in range(1, min(order, (T + 1) // 2 + 1) + 1))  # "a b a b" (7 labels) is where the 5-gram answers


# ---------------------------------------------------------------------------------------------- 3. exact regime on the device
def _exact_case(order, T, seed):
    """Adjacent ranks of the first 17 strings differ by more than 1e-3 and nothing is pruned at width 128 (both asserted)."""
    if (order, T) not in _EXACT:
        lm = _tiny_lm(order)
        tab = oracle.Tables.of(lm, 3)
        x = _noise(np.random.default_rng(seed), T, 4, 3, 1.5)
        ranking = oracle.brute_force(x, 3, 2, tab, ALPHA, BETA)
        gaps = [abs(ranking[i][1] - ranking[i + 1][1]) for i in range(16)]
        assert min(gaps) > 1e-3, (T, min(gaps))
        live = []
        oracle.beam_search(x, 3, 2, 128, tab, ALPHA, BETA, trace=live)
        assert max(live) <= 128, live                                    # candidates per frame: nothing is pruned at width 128
        assert max(abs(s) for _, s, _, _ in ranking[:16]) < 32 and max(len(bytes(q).split(bytes([2]))) for q, *_ in ranking[:16]) <= 4
        f32 = oracle.beam_search(x, 3, 2, 128, tab, ALPHA, BETA, n_best=16, dtype=np.float32)
        _EXACT[(order, T)] = (lm, x, ranking, max(abs(f32[r][1] - ranking[r][1]) for r in range(16)))
    return _EXACT[(order, T)]


@pytest.mark.parametrize('order,T,seed', EXACT_CASES)
def test_exact_regime_equals_the_brute_force_ranking(dev, order, T, seed):
    lm, x, ranking, f32_dev = _exact_case(order, T, seed)
    bar = _exact_bar(7, 4)
    out = _search(dev, lm, [x], 128, 16)
    assert _strings(out, 0) == [q for q, *_ in ranking[:16]]
    dev_max = max(abs(float(out[2][0, r]) - ranking[r][1]) for r in range(16))
    ctc_max = max(abs(float(out[3][0, r]) - ranking[r][2]) for r in range(16))
    print('exact regime, order %d, T = %d: largest score deviation %.3e, CTC part %.3e (bar %.1e; the float32 oracle: %.3e)' % (order, T, dev_max, ctc_max, bar, f32_dev))
    assert dev_max < bar and ctc_max < bar and f32_dev < bar
    assert out[4][0].tolist() == [int(done) for *_, done in ranking[:16]]


def test_a_sentence_wins_only_through_its_5_gram(dev):
    """The words a and b.  The frames spell "a b a b" and then a last word that is b by a small margin; the 5-gram (a, b, a, b, a) turns it
    into a.  With that one n-gram removed the result is "a b a b b".  Every lower n-gram of the chain scores like a unigram, so only the
    5-gram tells the two models apart; nine frames and five words set the bar."""
    sp, bl = 2, 3
    a, b, s = [0.9, 0.03, 0.03, 0.04], [0.03, 0.9, 0.03, 0.04], [0.03, 0.03, 0.9, 0.04]
    x = _from_probs([a, s, b, s, a, s, b, s, [0.44, 0.48, 0.04, 0.04]])
    g = {(0,): (-0.7, 0.0), (1,): (-0.7, 0.0), (2,): (-7.5, 0.0), (0, 1): (-0.7, 0.0), (0, 1, 0): (-0.7, 0.0), (0, 1, 0, 1): (-0.7, 0.0)}
    with_5 = _hand_lm(4, [(0,), (1,)], {**g, (0, 1, 0, 1, 0): (-0.05, 0.0)}, 5)
    without = _hand_lm(4, [(0,), (1,)], g, 5)
    for lm, want in ((with_5, (0, sp, 1, sp, 0, sp, 1, sp, 0)), (without, (0, sp, 1, sp, 0, sp, 1, sp, 1))):
        ref = oracle.beam_search(x, bl, sp, 16, oracle.Tables.of(lm, bl), 1.0, 0.0, n_best=2)
        assert ref[0][0] == want
        out = _search(dev, lm, [x], 16, 2, alpha=1.0, beta=0.0)
        assert _strings(out, 0) == [q for q, *_ in ref]
        assert abs(float(out[2][0, 0]) - ref[0][1]) < _exact_bar(9, 5)


# ---------------------------------------------------------------------------------------------- 4. pruned regime against the float64 oracle
# (T, V, W) -> utterances, order, words, longest word, hub words, n-grams per context, seed of the lexicon, largest deviation of the float32 oracle's top-1 score / CTC
# part from the float64 oracle's on these inputs; the bar = 4 x the larger of the two.  (The seeds were chosen with the oracle alone, see the
# module docstring; the one of the width-1 shape also so that some of its winners are incomplete.)
PRUNED = {
    (60, 8, 16): (10, 5, 40, 3, 6, 4, 2, 1.135e-05, 9.232e-06),
    (50, 38, 1): (10, 4, 30, 3, None, 8, 3, 3.779e-05, 2.977e-05),
    (64, 38, 100): (4, 5, 300, 5, 12, 4, 0, 2.661e-05, 2.395e-05),
}
EMU_UTTERANCES = 3                                                       # the emulator tier decodes the first few utterances of a shape
_REF, _LMS = {}, {}


def _pruned_lm(shape):
    if shape not in _LMS:
        _, order, n_words, letters, hubs, per, seed = PRUNED[shape][:7]
        _LMS[shape] = _random_lm(shape[1], n_words, letters, seed, order, per=per, hubs=hubs)
    return _LMS[shape]


def _pruned_inputs(shape):
    T, V, W = shape
    n = PRUNED[shape][0]
    rng = np.random.default_rng(T * 1000 + V)
    return [_noise(rng, T - (i * T) // (8 * n), V, V - 1, 2.0 + rng.random()) for i in range(n)]     # ragged: T down to ~7/8 T


def _reference(shape, i, x):
    """Oracle results and the n-gram levels that answered, computed once per (shape, utterance) and shared between the backends."""
    if (shape, i) not in _REF:
        T, V, W = shape
        tab = oracle.Tables.of(_pruned_lm(shape), V - 1)
        _REF[(shape, i)] = (oracle.beam_search(x, V - 1, V - 2, W, tab, ALPHA, BETA, n_best=min(3, W)), tab.levels)
    return _REF[(shape, i)]


@pytest.mark.parametrize('shape', list(PRUNED))
def test_pruned_regime_matches_the_float64_oracle(dev, shape):
    T, V, W = shape
    xs = _pruned_inputs(shape)
    lm = _pruned_lm(shape)
    assert lm.order == PRUNED[shape][1] == max(len(g) for g in lm.ngrams)
    refs = [_reference(shape, i, x) for i, x in enumerate(xs)]           # the oracle decodes every utterance on both tiers
    levels = sum((lv for _, lv in refs), collections.Counter())
    refs = [r for r, _ in refs]
    assert all(len(r[0][0]) > 0 for r in refs)                           # not degenerate: every winner holds words
    assert sum(levels[k] for k in range(4, 7)) > 0 and levels[1] > 0, levels      # the levels the table search does not have answered lookups
    if W == 1:
        assert 2 <= sum(not r[0][3] for r in refs) <= len(refs) - 2      # complete and incomplete winners both appear
    if is_emu(dev):
        xs, refs = xs[:EMU_UTTERANCES], refs[:EMU_UTTERANCES]
    out = _search(dev, lm, xs, W, min(3, W))
    sibling._check_against_oracle(out, refs, 4 * max(PRUNED[shape][7:9]), 'shape %s, lookups answered per level %s' % (shape, dict(sorted(levels.items()))))


# ---------------------------------------------------------------------------------------------- 5. the same strings as the table search
def test_an_order_3_model_decodes_as_the_table_search_does(dev):
    """from_ngram_lm of the sibling test's random order-3 model at (60, 8, 16): labels, lengths and complete flags equal ctc_word_beam_search's,
    the scores and their CTC parts are the same f32 numbers."""
    shape = (60, 8, 16)
    table = sibling._pruned_lm(shape)
    xs = sibling._pruned_inputs(shape)[:EMU_UTTERANCES if is_emu(dev) else None]
    want = sibling._search(dev, table, xs, 16, 3)
    got = _search(dev, rm.WordStateLM.from_ngram_lm(table), xs, 16, 3)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert got[2].dtype == np.float32 and all(len(_strings(got, b)[0]) > 2 for b in range(len(xs)))


# ---------------------------------------------------------------------------------------------- 6. isolation and layouts
def _iso_case():
    rng = np.random.default_rng(77)
    return _random_lm(6, 12, 3, 5, 4, per=3, cap=60), [_noise(rng, T, 6, 5, 2.5) for T in (13, 1, 9, 14, 5)]


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


@pytest.mark.parametrize('T', [0, 1, 2])
def test_short_utterances_mark_missing_ranks(dev, T):
    lm = _tiny_lm(4)
    x = _noise(np.random.default_rng(20 + T), 4, 4, 3, 1.5)[:T]
    ranking = oracle.brute_force(x, 3, 2, oracle.Tables.of(lm, 3), ALPHA, BETA)
    assert len(ranking) == {0: 1, 1: 3, 2: 6}[T]                         # "", a, b | and "a ", "b ", ab (aa, ba and bb start no word)
    out = _search(dev, lm, [x, _noise(np.random.default_rng(1), 3, 4, 3, 1.5)], 128, 16)      # (a neighbour, so that T = 0 is not an empty launch)
    n = len(ranking)
    assert _strings(out, 0) == [q for q, *_ in ranking]
    assert max(abs(float(out[2][0, r]) - ranking[r][1]) for r in range(n)) < _exact_bar(7, 4)
    assert out[4][0, :n].tolist() == [int(done) for *_, done in ranking]
    assert (out[1][0, n:] == -1).all() and (out[2][0, n:] == -np.inf).all() and (out[3][0, n:] == -np.inf).all() and (out[4][0, n:] == -1).all()
    assert (out[0][0, n:] == -1).all()
    if T == 0:
        assert out[1][0, 0] == 0 and out[2][0, 0] == 0.0 and out[4][0, 0] == 1


# ---------------------------------------------------------------------------------------------- 7. host builders
ARPA4 = sibling.ARPA.replace('ngram 3=2', 'ngram 3=2\nngram 4=2').replace('\\end\\', '\\4-grams:\n-0.15\t<s> Hello world! Hello\n-0.45\t<s> Hello world! caf\u00e9\n\n\\end\\')


def test_from_arpa_reads_a_hand_written_order_4_file():
    tt = rm.TextTransform()
    lm = rm.WordStateLM.from_arpa(io.StringIO(ARPA4), tt)
    assert lm.words == ['hello', 'its', 'world'] and lm.start == 3 and lm.order == 4 and lm.start_state == 4
    hello, its, world, S = 0, 1, 2, 3
    ln10 = math.log(10.0)
    g = lm.ngrams
    assert abs(float(g[(hello,)][0]) + 0.6 * ln10) < 1e-6 and abs(float(g[(hello,)][1]) + 0.3 * ln10) < 1e-6 and float(g[(world,)][1]) == 0.0
    assert abs(float(g[(S,)][1]) + 0.5 * ln10) < 1e-6 and g[(S,)][0].dtype == np.float32
    assert {k for k in g if len(k) == 2} == {(S, hello), (hello, world), (its, hello)}                           # </s> and café n-grams are gone
    assert {k for k in g if len(k) > 2} == {(S, hello, world), (S, hello, world, hello)}
    assert abs(float(g[(S, hello, world, hello)][0]) + 0.15 * ln10) < 1e-6 and abs(float(g[(S, hello)][1]) + 0.15 * ln10) < 1e-6
    s = lm.score_words([hello, world, hello, its])
    want = [-0.2 * ln10, -0.1 * ln10, -0.15 * ln10, (0.0 - 0.3 - 1.1) * ln10]      # the last: no arc out of (hello), bo(hello) + uni(its)
    assert np.abs(s - np.array(want)).max() < 1e-6
    assert lm.context_of(lm.state_of((S, hello, world))) == (S, hello, world) and lm.context_of(lm.state_of((its, hello, world))) == (hello, world)
    with pytest.raises(ValueError):
        rm.WordNgramLM.from_arpa(io.StringIO(ARPA4), tt)                  # the table model still stops at order 3


def test_an_order_7_arpa_file_and_a_model_that_is_not_prefix_closed_raise():
    seven = ARPA4.replace('ngram 4=2', 'ngram 4=2\nngram 7=1').replace('\\end\\', '\\7-grams:\n-0.1\t<s> Hello world! Hello world! Hello world!\n\n\\end\\')
    with pytest.raises(ValueError, match='order 7'):
        rm.WordStateLM.from_arpa(io.StringIO(seven), rm.TextTransform())
    uni = {(w,): (-1.0, 0.0) for w in range(3)}
    with pytest.raises(ValueError, match=r'\(0, 1, 0\)'):
        rm.WordStateLM(['a', 'b'], {**uni, (0, 1, 0): (-0.5, 0.0)}, 'ab ')                 # (0, 1) is missing
    with pytest.raises(ValueError):
        rm.WordStateLM(['a', 'b'], {**uni, (0, 2): (-0.5, 0.0)}, 'ab ')                    # the start context does not lead
    with pytest.raises(ValueError):
        rm.WordStateLM(['a', 'b'], {(0,): (-1.0, 0.0), (1,): (-1.0, 0.0)}, 'ab ')                # no unigram of the start context
    with pytest.raises(ValueError):
        rm.WordStateLM(['a', 'b'], uni, 'ab ', order=7)
    assert rm.WordStateLM(['a', 'b'], uni, 'ab ').order == 2 and rm.WordStateLM.MAX_ORDER == 6


def test_from_texts_of_order_3_equals_the_table_model_number_for_number():
    tt = rm.TextTransform()
    for order in (1, 2, 3):
        table = rm.WordNgramLM.from_texts(sibling.CORPUS, tt, order=order, add_k=0.5)
        lm = rm.WordStateLM.from_texts(sibling.CORPUS, tt, order=order, add_k=0.5)
        want = {(w,): tuple(table.unigrams[w]) for w in range(table.n_words + 1)}
        want.update(table.bigrams)
        want.update({g: (p, np.float32(0.0)) for g, p in table.trigrams.items()})
        assert lm.words == table.words and lm.ngrams.keys() == want.keys() and lm.order == max(order, 1)
        assert all(lm.ngrams[g][0] == want[g][0] and lm.ngrams[g][1] == want[g][1] for g in want)


def test_from_texts_of_order_5_is_a_distribution_in_every_state():
    tt = rm.TextTransform()
    texts = ['the cat sat on the mat', 'the cat sat on the hat', 'a cat sat on the mat', 'the dog sat on a mat', 'the cat ran', 'on the mat the cat sat down']
    lm = rm.WordStateLM.from_texts(texts, tt, order=5)
    assert lm.order == 5 and max(len(g) for g in lm.ngrams) == 5 and lm.n_states > 1 + lm.n_words + 1
    for s in range(lm.n_states):
        total = sum(math.exp(lm.score_words([w], context=lm.context_of(s) or (-1,))[0]) for w in range(lm.n_words))
        assert abs(total - 1.0) < 1e-6, (lm.context_of(s), total)
    the, cat, sat, on = (lm.words.index(w) for w in ('the', 'cat', 'sat', 'on'))
    assert (lm.start, the, cat, sat, on) in lm.ngrams and (cat, sat, on, the) in lm.ngrams


def _same_model(x, y, tol=0.0):
    assert x.words == y.words and x.chars == y.chars and x.order == y.order and x.ngrams.keys() == y.ngrams.keys()
    assert all(abs(float(x.ngrams[g][i] - y.ngrams[g][i])) <= tol for g in x.ngrams if g != (x.start,) for i in (0, 1))
    assert abs(float(x.ngrams[(x.start,)][1] - y.ngrams[(x.start,)][1])) <= tol
    for name in ('lex_child', 'lex_word', 'st_shorter', 'arc_keys', 'arc_next'):
        assert torch.equal(getattr(x, name), getattr(y, name)), name
    assert x.arc_probe == y.arc_probe and x.n_states == y.n_states


def test_write_arpa_from_arpa_and_save_load_reproduce_the_model(tmp_path):
    tt = rm.TextTransform()
    lm = rm.WordStateLM.from_texts(sibling.CORPUS, tt, order=4, add_k=0.5)
    path = str(tmp_path / 'lm.arpa')
    lm.write_arpa(path)
    back = rm.WordStateLM.from_arpa(path, tt)
    _same_model(lm, back, 2e-6)                                           # 9 significant digits of log10 in the text: below one f32 ulp of values < 16
    with open(path) as f:
        _same_model(back, rm.WordStateLM.from_arpa(f, tt))
    npz = str(tmp_path / 'lm.npz')
    lm.save(npz)
    again = rm.WordStateLM.load(npz)
    _same_model(lm, again)
    assert torch.equal(again.arc_logp, lm.arc_logp) and torch.equal(again.st_bo, lm.st_bo) and torch.equal(again.uni_logp, lm.uni_logp)
    assert lm.to('cpu').n_words == 7 and lm.to('cpu').order == 4 and lm.word_ids('The cat!', tt) == [lm.words.index('the'), lm.words.index('cat')]


# ---------------------------------------------------------------------------------------------- 8. ops
_NAMES = ['logits', 'utt', 'V', 'blank', 'space', 'total_frames', 'max_len', 'beam_width', 'n_best', 'lex_child', 'lex_word', 'uni_logp', 'st_bo', 'st_shorter',
          'arc_keys', 'arc_logp', 'arc_next', 'n_vocab', 'start_state', 'arc_probe', 'order', 'alpha', 'beta']


def _args(dev, **kw):
    lm = kw.pop('model', None) or _iso_case()[0]
    x = _noise(np.random.default_rng(5), 12, 6, 5, 2.0)
    t = lm.to(dev)
    a = dict(logits=torch.from_numpy(x).to(dev), utt=torch.tensor([[0, 7], [7, 5]], dtype=torch.int64).to(dev), V=6, blank=5, space=4, total_frames=12, max_len=7,
             beam_width=4, n_best=2, lex_child=t.lex_child, lex_word=t.lex_word, uni_logp=t.uni_logp, st_bo=t.st_bo, st_shorter=t.st_shorter, arc_keys=t.arc_keys,
             arc_logp=t.arc_logp, arc_next=t.arc_next, n_vocab=t.n_words, start_state=t.start_state, arc_probe=t.arc_probe, order=t.order, alpha=0.8, beta=0.5)
    assert list(a) == _NAMES
    a.update(kw)
    return tuple(a.values())


def test_ops_are_registered_and_pass_opcheck(dev):
    assert 'ctc_word_state_beam_search' in torch_ops.OPS and 'word_state_score' in torch_ops.OPS
    torch.library.opcheck(torch.ops.silent_speech.ctc_word_state_beam_search.default, _args(dev), test_utils=('test_schema', 'test_faketensor'))
    uni_only = rm.WordStateLM(['%s' % chr(0x100 + i) for i in range(4)], {(w,): (-1.0, 0.0) for w in range(5)}, sibling._chars(6))
    assert uni_only.arc_keys.numel() == 0
    torch.library.opcheck(torch.ops.silent_speech.ctc_word_state_beam_search.default, _args(dev, model=uni_only), test_utils=('test_schema', 'test_faketensor'))
    t = _iso_case()[0].to(dev)
    pairs = torch.tensor([[t.start_state, 0], [0, 1], [t.n_states - 1, 2]], dtype=torch.int32).to(dev)
    torch.library.opcheck(torch.ops.silent_speech.word_state_score.default, (pairs, t.uni_logp, t.st_bo, t.st_shorter, t.arc_keys, t.arc_logp, t.arc_next, t.arc_probe, t.order),
                          test_utils=('test_schema', 'test_faketensor'))


@pytest.mark.parametrize('bad', [dict(beam_width=0), dict(beam_width=129), dict(n_best=5), dict(n_best=0), dict(space=5), dict(space=6), dict(space=-1),
                                 dict(blank=6), dict(V=129), dict(max_len=0), dict(lex_child='wrong shape'), dict(lex_word='wrong shape'),
                                 dict(uni_logp='other device'), dict(arc_keys='other device'), dict(start_state=-1), dict(start_state='n_states'), dict(n_vocab=14),
                                 dict(arc_probe=1 << 20), dict(arc_probe='slots + 1'), dict(arc_keys='not a power of two'), dict(order=0), dict(order=7),
                                 dict(st_shorter='wrong shape'), dict(arc_next='wrong shape')])
def test_bad_arguments_raise(dev, bad):
    good = _args(dev)
    (name, what), = bad.items()
    t = good[_NAMES.index(name)]
    more = {}
    if what == 'wrong shape':
        what = t[:, :-1].contiguous() if t.dim() == 2 else t[:-1].contiguous()
    elif what == 'other device':
        what = t.cpu() if t.is_cuda else t.double()                       # tables that are not where the logits are (the emulator has one device: a wrong dtype)
    elif what == 'n_states':
        what = good[_NAMES.index('st_bo')].numel()
    elif what == 'slots + 1':
        what = good[_NAMES.index('arc_keys')].numel() + 1
    elif what == 'not a power of two':                                    # all three arc arrays shortened alike: only the slot count is wrong
        slots = t.numel() - 3
        what, more = t[:slots].contiguous(), dict(arc_logp=good[_NAMES.index('arc_logp')][:slots].contiguous(), arc_next=good[_NAMES.index('arc_next')][:slots].contiguous(), arc_probe=1)
    with pytest.raises(RuntimeError):
        torch.ops.silent_speech.ctc_word_state_beam_search(*_args(dev, **{name: what}, **more))
    labels, lengths, _, _, complete = torch.ops.silent_speech.ctc_word_state_beam_search(*good)         # and the library is fine afterwards
    assert tuple(labels.shape) == (2, 2, 7) and int(lengths.min()) >= 0 and int(complete.min()) >= 0


def test_the_library_checks_the_model_before_any_launch(dev):
    """The C entry points themselves (no op in front): order, slot count, probe bound and start state are refused with a message."""
    import ctypes
    L = _lib.lib()
    t = _iso_case()[0].to(dev)
    pairs = torch.zeros((1, 2), dtype=torch.int32).to(dev)
    out, nxt = torch.empty(1).to(dev), torch.empty(1, dtype=torch.int32).to(dev)

    def model(**kw):
        lm = torch_ops._word_state_tables('test', pairs.device, t.uni_logp, t.st_bo, t.st_shorter, t.arc_keys, t.arc_logp, t.arc_next, t.arc_probe, t.order)
        for k, v in kw.items():
            setattr(lm, k, v)
        return lm
    for kw, word in [(dict(order=0), b'order'), (dict(order=7), b'order'), (dict(arc_slots=t.arc_keys.numel() - 1), b'arc slots'),
                     (dict(arc_probe=t.arc_keys.numel() + 1), b'longest probe'), (dict(start_state=t.n_states), b'start state'), (dict(n_states=t.n_words), b'states')]:
        rc = L.ss_word_state_score(ctypes.byref(model(**kw)), _lib.ptr(pairs), 1, _lib.ptr(out), _lib.ptr(nxt), None)
        assert rc != 0 and word in L.ss_last_error(), (kw, L.ss_last_error())
    assert L.ss_word_state_score(ctypes.byref(model()), _lib.ptr(pairs), 1, _lib.ptr(out), _lib.ptr(nxt), _lib.stream_of(pairs)) == 0
    assert L.ss_ctc_word_state_beam_workspace_bytes(2, 12, 4) == 8 * (12 * 4 + 3) and L.ss_ctc_word_state_beam_workspace_bytes(2, 12, 129) == -1


def test_word_state_score_refuses_bad_tables(dev):
    t = _iso_case()[0].to(dev)
    pairs = torch.tensor([[t.start_state, 0]], dtype=torch.int32).to(dev)
    good = (pairs, t.uni_logp, t.st_bo, t.st_shorter, t.arc_keys, t.arc_logp, t.arc_next, t.arc_probe, t.order)
    for i, bad in [(0, pairs.long()), (0, torch.zeros((1, 3), dtype=torch.int32).to(dev)), (2, t.st_bo[:-1].contiguous()), (2, t.st_bo[:t.n_words].contiguous()),
                   (4, t.arc_keys[:-1].contiguous()), (5, t.arc_logp.cpu() if t.arc_logp.is_cuda else t.arc_logp.double()), (7, 1 << 20), (8, 0), (8, 7)]:
        with pytest.raises(RuntimeError):
            torch.ops.silent_speech.word_state_score(*(good[:i] + (bad,) + good[i + 1:]))
    lnp, nxt = torch.ops.silent_speech.word_state_score(*good)
    assert torch.isfinite(lnp).all() and 0 <= int(nxt[0]) < t.n_states


# ---------------------------------------------------------------------------------------------- 9. the entry points
def test_beam_decode_takes_the_state_model_and_checks_its_labels(dev):
    lm, xs = _iso_case()
    x = xs[0]
    pred = torch.from_numpy(x).to(dev).reshape(1, x.shape[0], 6)
    got = rm.beam_decode(pred, [x.shape[0]], beam_width=8, lm=lm, alpha=ALPHA, beta=BETA)
    assert [tuple(got[0])] == _strings(_search(dev, lm, [x], 8, 1), 0)
    nbest = rm.beam_decode(pred, [x.shape[0]], beam_width=8, n_best=3, lm=lm, alpha=ALPHA, beta=BETA)
    assert [tuple(q) for q, _ in nbest[0]] == _strings(_search(dev, lm, [x], 8, 3), 0)
    with pytest.raises(ValueError, match='WordStateLM spells with'):
        rm.beam_decode(torch.zeros(1, 4, 9).to(dev), [4], lm=lm)


def test_recognition_test_with_a_state_lm(dev, monkeypatch):
    """test(..., decoder='beam', lm=WordStateLM) in the 'whole' branch: the strings are the ones the oracle decodes from the model's own logits,
    and the returned number is their WER."""
    from tests.test_ctc_beam import _dataset, _references
    ds, m = _dataset(dev)
    tt, V = ds.text_transform, len(ds.text_transform.chars) + 1
    lm = rm.WordStateLM.from_texts(_references(ds) + sibling.CORPUS, tt, order=5)
    assert lm.n_words > 7 and lm.order == 5
    seen = []
    real = Model.forward_utterances

    def keep(self, raws):
        out = real(self, raws)
        seen.append(out)
        return out
    monkeypatch.setattr(Model, 'forward_utterances', keep)
    search = dict(beam_width=8, lm=lm, alpha=1.5, beta=1.85)
    got = rm.test(m, ds, dev, decoder='beam', batch_size=4, whole_utterances=True, **search)
    assert seen
    space = tt.chars.index(' ')
    tab = oracle.Tables.of(lm, V - 1)
    texts, decoded = [], []
    for logits in seen:
        decoded += [tt.int_to_text(q) for q in rm.beam_decode_utterances(logits, space=space, **search)]
        texts += [tt.int_to_text(list(oracle.beam_search(y.cpu().numpy(), V - 1, space, 8, tab, 1.5, 1.85)[0][0])) for y in logits]
    assert len(texts) == len(ds) and decoded == texts
    assert got == rm.wer(_references(ds), texts)
    vocabulary = set(lm.words)
    assert all(w in vocabulary for t in texts for w in t.split(' ') if w) and all('  ' not in t and not t.startswith(' ') for t in texts)
