"""CTC prefix beam search on the device (csrc/ctc_decode.hip, torch.ops.silent_speech.ctc_beam_search, recognition_model.beam_decode*):
against the exact ranking of all label strings where nothing is pruned, against tests/ctc_beam_oracle.py (plain Python, float64) where
the beam prunes, bit for bit against itself across layouts and batches, with a label n-gram table fused in, and through the Python surface.

Score bars.  Exact regime (T <= 4, |score| < 16): a frame costs a prefix one log-add-exp and one addition, each rounded to at most one f32
ulp of the running value (< 2^-20 below 16) plus one ulp of the hardware exp2 / log2 on a term <= ln 2 -- 4 frames x 3 roundings x 2^-20 =
1.2e-5; EXACT_BAR = 2e-5.  Pruned regime: per shape, 4 x the largest top-1 score deviation of the oracle's OWN float32 run from its float64
run on these inputs (measured on the CPU, listed in PRUNED below; the factor covers the hardware exp2 / log2 and another summation order).
The float32 oracle agreed with the float64 one on top-1 and top-3 of every utterance of every shape here, so the 90 % cap is not what lets
the kernel pass."""
import math

import numpy as np
import pytest
import torch

from silent_speech_amd import recognition_model as rm
from silent_speech_amd import torch_ops
from silent_speech_amd.architecture import Model
from tests import ctc_beam_oracle as oracle
from tests.backend import dev, is_emu  # noqa: F401
from tests.ctc_beam_helpers import from_probs as _from_probs, layout as _layout, noise as _noise, same as _same, strings as _strings

EXACT_BAR = 2e-5


def _search(dev, utts, blank, W, n_best, lm=None, alpha=0.0, beta=0.0, **how):
    """utts: list of (T_i, V) float32 arrays, laid out by ctc_beam_helpers.layout(**how).  Returns numpy (labels, lengths, scores, ctc scores)."""
    flat, utt, V, total, longest = _layout(dev, utts, **how)
    if lm is not None:
        lm = torch.as_tensor(lm, dtype=torch.float32).to(dev)
    out = torch.ops.silent_speech.ctc_beam_search(flat, utt, V, blank, total, longest, W, n_best, lm, alpha, beta)
    return tuple(t.cpu().numpy() for t in out)


# ---------------------------------------------------------------------------------------------- 0. the oracle itself
@pytest.mark.parametrize('T,blank,seed', [(5, 3, 0), (5, 0, 1), (5, 1, 2), (6, 3, 3)])
def test_oracle_reproduces_the_exact_likelihood_of_every_string(T, blank, seed):
    """With a beam at least as wide as the number of prefixes, every prefix's final score is the exact float64 log-likelihood of that label
    string (oracle/ctc_ref.ctc_utterance over all strings of up to T labels)."""
    x = _noise(np.random.default_rng(seed), T, 4, blank, 1.5)
    exact = oracle.brute_force(x, blank)
    got = oracle.beam_search(x, blank, 4 ** 7, n_best=4 ** 7)
    assert len(exact) == len(got) > 3 ** (T // 2)
    want = dict(exact)
    for q, score, ctc in got:
        assert abs(score - want[q]) < 1e-9 and ctc == score, q
    assert [q for q, _, _ in got[:5]] == [q for q, _ in exact[:5]]


# ---------------------------------------------------------------------------------------------- 1. exact regime
# seeds chosen with brute force alone so that adjacent ranks of the first 17 strings differ by more than 1e-3 (asserted below)
EXACT_SEEDS = {3: 10, 0: 10}
_EXACT = {}


def _exact_case(blank):
    if blank not in _EXACT:
        x = _noise(np.random.default_rng(EXACT_SEEDS[blank]), 4, 4, blank, 1.5)
        ranking = oracle.brute_force(x, blank)
        gaps = [ranking[i][1] - ranking[i + 1][1] for i in range(16)]
        assert min(gaps) > 1e-3, (blank, min(gaps))
        _EXACT[blank] = (x, ranking)
    return _EXACT[blank]


@pytest.mark.parametrize('blank', [3, 0])
def test_exact_regime_equals_the_brute_force_ranking(dev, blank):
    x, ranking = _exact_case(blank)
    out = _search(dev, [x], blank, 128, 16)
    assert _strings(out, 0) == [q for q, _ in ranking[:16]]
    dev_max = max(abs(float(out[2][0, r]) - ranking[r][1]) for r in range(16))
    print('exact regime, blank %d: largest score deviation %.3e (bar %.1e)' % (blank, dev_max, EXACT_BAR))
    assert dev_max < EXACT_BAR
    assert np.array_equal(out[2], out[3])                                # no table: the score is its CTC part


@pytest.mark.parametrize('T', [0, 1, 2])
def test_exact_regime_short_utterances_mark_missing_ranks(dev, T):
    x = _noise(np.random.default_rng(20 + T), 4, 4, 3, 1.5)[:T]
    ranking = oracle.brute_force(x, 3)                                   # T = 0: [((), 0)]; 1: 4 strings; 2: 10 (the doubles need 3 frames)
    assert len(ranking) == {0: 1, 1: 4, 2: 10}[T]
    out = _search(dev, [x, _noise(np.random.default_rng(1), 3, 4, 3, 1.5)], 3, 128, 16)       # (a neighbour, so that T = 0 is not an empty launch)
    n = len(ranking)
    assert _strings(out, 0) == [q for q, _ in ranking]
    assert max(abs(float(out[2][0, r]) - ranking[r][1]) for r in range(n)) < EXACT_BAR
    assert (out[1][0, n:] == -1).all() and (out[2][0, n:] == -np.inf).all() and (out[3][0, n:] == -np.inf).all()
    assert (out[0][0, n:] == -1).all()
    if T == 0:
        assert out[1][0, 0] == 0 and out[2][0, 0] == 0.0


# ---------------------------------------------------------------------------------------------- 2. the rules best-path decoding gets wrong
def test_label_mass_beats_the_best_path(dev):
    """Two frames of p(a) = 0.4, p(blank) = 0.6: the best path is blank blank (0.36), the string "a" has 0.64."""
    x = _from_probs([[0.4, 0.6], [0.4, 0.6]])
    out = _search(dev, [x], 1, 4, 2)
    assert _strings(out, 0) == [(0,), ()]
    assert abs(float(out[2][0, 0]) - math.log(0.64)) < EXACT_BAR and abs(float(out[2][0, 1]) - math.log(0.36)) < EXACT_BAR
    pred = torch.from_numpy(x).to(dev).reshape(1, 2, 2)
    assert rm.greedy_decode(pred, [2], 1) == [[]]
    assert rm.beam_decode(pred, [2], 1, beam_width=4) == [[0]]


def test_repeats_collapse_unless_a_blank_separates_them(dev):
    hi, lo = 0.9, 0.05                                                   # classes a, b, blank
    a, blank = [hi, lo, lo], [lo, lo, hi]
    out = _search(dev, [_from_probs([a, a, blank, a]), _from_probs([a, a, a])], 2, 8, 1)
    assert _strings(out, 0) == [(0, 0)] and _strings(out, 1) == [(0,)]


def test_winner_needs_the_merged_mass_of_two_routes(dev):
    """Classes a, b, blank.  After frame 1 the beam holds "" (0.499) and "a" (0.499).  In frame 2 the string "a" is reached by staying on "a"
    (0.499 (0.1 + 0.35) = 0.22455) AND by extending "" (0.499 x 0.35 = 0.17465); "ab" has 0.499 x 0.55 = 0.27445, "b" slightly more.  Either
    route alone loses to "b"; their sum, 0.3992, wins."""
    f1, f2 = [0.499, 0.002, 0.499], [0.35, 0.55, 0.10]
    stay, ext = f1[0] * (f2[2] + f2[0]), f1[2] * f2[0]
    b = f1[2] * f2[1] + f1[1] * (f2[2] + f2[1])
    assert max(stay, ext) < b < stay + ext
    out = _search(dev, [_from_probs([f1, f2])], 2, 8, 2)
    assert _strings(out, 0) == [(0,), (1,)]
    assert abs(float(out[2][0, 0]) - math.log(stay + ext)) < EXACT_BAR and abs(float(out[2][0, 1]) - math.log(b)) < EXACT_BAR


REENTRY_BAR = 8 * 3 * 2.0 ** -20                                       # the exact regime's reasoning (see the module docstring) at 8 frames: 2.3e-5


@pytest.mark.parametrize('V,W,T,seed', [(3, 3, 7, 451), (4, 3, 8, 53)])
def test_pruned_parent_that_re_enters_the_beam_is_merged_with_its_child(dev, V, W, T, seed):
    """The case a carried parent slot cannot handle (seeds found with the oracle alone): the prefix p is pruned while its child q = p + c
    stays, p comes back later as an extension of ITS parent, and from the next frame on p + c must be folded into q again.  Without that
    the beam holds q twice, each copy with part of the mass.  q is the final winner here, so its score carries the folded mass."""
    x = (np.random.default_rng(seed).standard_normal((T, V)) * 2).astype(np.float32)
    trace = []
    ref = oracle.beam_search(x, V - 1, W, W, trace=trace)
    events = [(t, q) for t in range(1, T - 1) for q in trace[t]
              if q and q in trace[t - 1] and q[:-1] in trace[t] and q[:-1] not in trace[t - 1]]
    assert any(q == ref[0][0] for _, q in events), events
    out = _search(dev, [x], V - 1, W, W)
    got = _strings(out, 0)
    assert got == [q for q, _, _ in ref] and len(set(got)) == len(got)
    assert max(abs(float(out[2][0, r]) - ref[r][1]) for r in range(len(ref))) < REENTRY_BAR


# ---------------------------------------------------------------------------------------------- 3. pruned regime against the float64 oracle
# (T, V, W) -> utterances, largest |top-1 score of the float32 oracle - of the float64 oracle| on these inputs, the bar = 4 x that
PRUNED = {
    (40, 6, 8): (10, 2.714e-06, 1.085e-05),
    (120, 12, 16): (10, 1.527e-05, 6.108e-05),
    (64, 38, 100): (4, 1.318e-05, 5.270e-05),
    (16, 128, 128): (3, 4.501e-06, 1.800e-05),
    (50, 38, 1): (10, 8.486e-06, 3.394e-05),
    (400, 38, 100): (1, 6.617e-05, 2.647e-04),
}
EMU_UTTERANCES = 3                                                       # the emulator tier decodes the first few utterances of a shape (~10 ms per frame)
_REF = {}


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
    top1 = top3 = 0
    worst = 0.0
    for b, ref in enumerate(refs):
        got = _strings(out, b)
        top1 += got[:1] == [q for q, _, _ in ref[:1]]
        top3 += got[:3] == [q for q, _, _ in ref[:3]]
        worst = max(worst, abs(float(out[2][b, 0]) - ref[0][1]))
    print('%s: top-1 %d / %d, top-3 %d / %d, largest top-1 score deviation %.3e (bar %.3e)' % (what, top1, len(refs), top3, len(refs), worst, bar))
    assert top1 >= 0.9 * len(refs) and top3 >= 0.9 * len(refs)
    assert worst <= bar


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
    refs = [_reference(shape, i, lambda: oracle.beam_search(x, V - 1, W, n_best)) for i, x in enumerate(xs)]
    out = _search(dev, xs, V - 1, W, n_best)
    _check_against_oracle(out, refs, PRUNED[shape][2], 'shape %s' % (shape,))


# ---------------------------------------------------------------------------------------------- 5. isolation and determinism
def _iso_inputs():
    rng = np.random.default_rng(77)
    return [_noise(rng, T, 6, 5, 2.5) for T in (13, 1, 9, 14, 5)]


def test_each_utterance_alone_equals_itself_in_a_batch_bit_for_bit(dev):
    xs = _iso_inputs()
    L = max(x.shape[0] for x in xs)
    batch = _search(dev, xs, 5, 8, 3)
    assert _same(batch, _search(dev, xs, 5, 8, 3))                        # two runs of the same call
    for b, x in enumerate(xs):
        alone = _search(dev, [x], 5, 8, 3)
        assert np.array_equal(alone[0][0], batch[0][b, :, :alone[0].shape[2]]) and (batch[0][b, :, alone[0].shape[2]:] == -1).all()
        assert all(np.array_equal(alone[k][0], batch[k][b]) for k in (1, 2, 3)), b
    assert batch[0].shape == (5, 3, L)


def test_layouts_read_nothing_but_the_utterances(dev):
    xs = _iso_inputs()
    want = _search(dev, xs, 5, 8, 3)
    assert _same(want, _search(dev, xs, 5, 8, 3, gaps=[3, 0, 7, 1, 5]))   # packed, first frames that are no multiple of anything, NaN between
    assert _same(want, _search(dev, xs, 5, 8, 3, layout='slots'))         # the slot layout of forward_utterances, NaN in every filler row
    assert _same(want, _search(dev, xs, 5, 8, 3, ld=11))                  # ld > V, NaN in the extra columns
    assert _same(want, _search(dev, xs, 5, 8, 3, layout='slots', ld=8))


# ---------------------------------------------------------------------------------------------- 6. fusion of a label n-gram table
LM_SHAPE, LM_UTTERANCES = (60, 8, 16), 10
LM_F32_DEV, LM_BAR = 1.594e-05, 6.378e-05                                          # as in PRUNED: the float32 oracle's deviation on these inputs, 4 x that


def _lm_case():
    T, V, W = LM_SHAPE
    rng = np.random.default_rng(606)
    table = rng.standard_normal((V, V, V - 1)) * 1.5
    table = (table - np.log(np.exp(table).sum(2, keepdims=True))).astype(np.float32)
    return [_noise(rng, T - i, V, V - 1, 2.0 + rng.random()) for i in range(LM_UTTERANCES)], table


def test_lm_fusion_matches_the_oracle_and_changes_the_result(dev):
    T, V, W = LM_SHAPE
    xs, table = _lm_case()
    assert np.allclose(np.exp(table.astype(np.float64)).sum(2), 1.0, atol=1e-6)
    xs = xs[:EMU_UTTERANCES] if is_emu(dev) else xs
    refs = [_reference('lm', i, lambda: oracle.beam_search(x, V - 1, W, 3, lm=table, alpha=0.8, beta=0.5)) for i, x in enumerate(xs)]
    fused = _search(dev, xs, V - 1, W, 3, lm=table, alpha=0.8, beta=0.5)
    _check_against_oracle(fused, refs, LM_BAR, 'label table, shape %s' % (LM_SHAPE,))
    for b, ref in enumerate(refs):                                        # the CTC part alone is reported beside the fused score
        assert abs(float(fused[3][b, 0]) - ref[0][2]) <= LM_BAR
    plain = _search(dev, xs, V - 1, W, 3)
    assert all(_strings(fused, b)[0] != _strings(plain, b)[0] for b in range(len(xs)))
    zero = _search(dev, xs, V - 1, W, 3, lm=table, alpha=0.0, beta=0.0)
    assert _same(zero, plain)


CORPUS = ['ab', 'abc', 'b a', 'aab', 'ba', 'abab', 'c', 'ca', 'a b', 'bb']


def test_label_ngram_lm_from_texts_equals_hand_counts(tmp_path):
    tt = rm.TextTransform()
    C = len(tt.chars)
    a, b, c, sp = (tt.chars.index(ch) for ch in 'abc ')
    lm = rm.LabelNgramLM.from_texts(CORPUS, tt, add_k=0.5)
    t = lm.table.double()
    assert tuple(t.shape) == (C + 1, C + 1, C) and lm.table.dtype == torch.float32
    assert torch.allclose(t.exp().sum(2), torch.ones(C + 1, C + 1, dtype=torch.float64), atol=1e-5)      # every context is a distribution

    def p(n, total):
        return math.log((n + 0.5) / (total + 0.5 * C))
    # first labels of the ten lines, context (before the start, before the start): a x5, b x3, c x2
    firsts = [line[0] for line in CORPUS]
    assert (firsts.count('a'), firsts.count('b'), firsts.count('c')) == (5, 3, 2)
    assert abs(float(t[C, C, a]) - p(5, 10)) < 1e-6 and abs(float(t[C, C, b]) - p(3, 10)) < 1e-6 and abs(float(t[C, C, c]) - p(2, 10)) < 1e-6
    # after (start, a): 'ab', 'abc', 'abab' -> b x3; 'aab' -> a; 'a b' -> space: 5 in all
    assert abs(float(t[C, a, b]) - p(3, 5)) < 1e-6 and abs(float(t[C, a, a]) - p(1, 5)) < 1e-6 and abs(float(t[C, a, sp]) - p(1, 5)) < 1e-6
    # after (a, b): 'abc' -> c; 'abab' -> a; ('ab', 'aab', second 'ab' of 'abab' end there): 2 in all
    assert abs(float(t[a, b, c]) - p(1, 2)) < 1e-6 and abs(float(t[a, b, a]) - p(1, 2)) < 1e-6 and abs(float(t[a, b, b]) - p(0, 2)) < 1e-6
    assert abs(float(t[b, c, a]) - p(0, 0)) < 1e-6                       # an unseen context is uniform
    # bigram / unigram tables are constant along the axes they do not look at
    bi, uni = rm.LabelNgramLM.from_texts(CORPUS, tt, add_k=0.5, order=2).table, rm.LabelNgramLM.from_texts(CORPUS, tt, add_k=0.5, order=1).table
    assert torch.equal(bi, bi[:1].expand_as(bi)) and torch.equal(uni, uni[:1, :1].expand_as(uni))
    n_ab = sum(line.count('ab') for line in CORPUS)
    n_a = sum(line[:-1].count('a') for line in CORPUS)
    assert abs(float(bi[0, a, b]) - p(n_ab, n_a)) < 1e-6
    n_all = sum(len(line) for line in CORPUS)
    assert abs(float(uni[0, 0, b]) - p(sum(line.count('b') for line in CORPUS), n_all)) < 1e-6
    path = str(tmp_path / 'lm.npz')
    lm.save(path)
    assert torch.equal(rm.LabelNgramLM.load(path).table, lm.table) and lm.to('cpu').n_labels == C


# ---------------------------------------------------------------------------------------------- 7. the surface
def _args(dev, **kw):
    x = _noise(np.random.default_rng(5), 12, 6, 5, 2.0)
    a = dict(logits=torch.from_numpy(x).to(dev), utt=torch.tensor([[0, 7], [7, 5]], dtype=torch.int64).to(dev), V=6, blank=5, total_frames=12, max_len=7,
             beam_width=4, n_best=2, lm=None, alpha=0.0, beta=0.0)
    a.update(kw)
    return tuple(a.values())


def test_op_is_registered_and_passes_opcheck(dev):
    assert 'ctc_beam_search' in torch_ops.OPS
    torch.library.opcheck(torch.ops.silent_speech.ctc_beam_search.default, _args(dev), test_utils=('test_schema', 'test_faketensor'))
    table = torch.zeros(6, 6, 5).to(dev)
    torch.library.opcheck(torch.ops.silent_speech.ctc_beam_search.default, _args(dev, lm=table, alpha=0.5, beta=0.1), test_utils=('test_schema', 'test_faketensor'))


@pytest.mark.parametrize('bad', [dict(beam_width=0), dict(beam_width=129), dict(n_best=5), dict(n_best=0), dict(blank=6), dict(blank=-1), dict(V=129),
                                 dict(V=7), dict(max_len=0), dict(lm='wrong shape')])
def test_bad_arguments_raise(dev, bad):
    if bad.get('lm') == 'wrong shape':
        bad = dict(lm=torch.zeros(6, 6, 6).to(dev))
    with pytest.raises(RuntimeError):
        torch.ops.silent_speech.ctc_beam_search(*_args(dev, **bad))
    labels, lengths, _, _ = torch.ops.silent_speech.ctc_beam_search(*_args(dev))          # and the library is fine afterwards
    assert tuple(labels.shape) == (2, 2, 7) and int(lengths.min()) >= 0


def _dataset(dev, n=None):
    from silent_speech_amd.synthetic import SyntheticEMGDataset
    n = n or (2 if is_emu(dev) else 6)
    ds = SyntheticEMGDataset(n, seed=3, min_frames=8, max_frames=16 if is_emu(dev) else 48, silent_fraction=0.0)
    torch.manual_seed(1)
    m = Model(ds.num_features, len(ds.text_transform.chars) + 1, model_size=16, num_layers=1, dropout=0.0, compute_dtype=torch.float32).to(dev)
    return ds, m


def _references(ds):
    return [ds.text_transform.int_to_text(torch.as_tensor(ds[i]['text_int']).tolist()) for i in range(len(ds))]


@pytest.mark.parametrize('branch', ['single', 'whole', 'packed'])
def test_recognition_test_with_the_beam_decoder(dev, monkeypatch, branch):
    """test(..., decoder='beam') in its three branches equals decoding the logits of that branch directly; with defaults it is greedy."""
    ds, m = _dataset(dev, 1 if is_emu(dev) and branch == 'single' else None)      # (one model call per utterance in that branch)
    tt, V = ds.text_transform, len(ds.text_transform.chars) + 1
    table = rm.LabelNgramLM.from_texts(_references(ds), tt, add_k=0.5)
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
    search = dict(beam_width=8, lm=table, alpha=0.3, beta=0.2)
    got = rm.test(m, ds, dev, decoder='beam', **search, **kw)
    assert seen
    lm_dev = table.to(dev)
    texts, greedy = [], []
    if branch == 'whole':
        for logits in seen:
            dec = rm.beam_decode_utterances(logits, **dict(search, lm=lm_dev))
            assert len(dec) == len(logits) and all(isinstance(q, list) for q in dec)
            # the same logits through the packed entry point, one utterance per row of T_max frames
            T = max(y.shape[0] for y in logits)
            pred = torch.stack([torch.cat([y, y.new_zeros(T - y.shape[0], V)]) for y in logits])
            for b, y in enumerate(logits):
                assert rm.beam_decode(pred[b:b + 1], [y.shape[0]], beam_width=8, lm=lm_dev, alpha=0.3, beta=0.2) == [dec[b]]
            nb = rm.beam_decode_utterances(logits, beam_width=8, n_best=3)
            assert all(1 <= len(r) <= 3 and all(s1 >= s2 for (_, s1), (_, s2) in zip(r, r[1:])) for r in nb)
            assert [r[0][0] for r in nb] == rm.beam_decode_utterances(logits, beam_width=8)
            texts += [tt.int_to_text(q) for q in dec]
            greedy += [tt.int_to_text(q) for q in rm.greedy_decode_utterances(logits)]
    else:
        lengths = [[p.shape[1]] for p in seen] if branch == 'single' else \
            [b['lengths'] for b in torch.utils.data.DataLoader(ds, batch_size=4, collate_fn=ds.collate_raw)]
        assert len(lengths) == len(seen)
        for pred, ls in zip(seen, lengths):
            texts += [tt.int_to_text(q) for q in rm.beam_decode(pred, ls, V - 1, **dict(search, lm=lm_dev))]
            greedy += [tt.int_to_text(q) for q in rm.greedy_decode(pred, ls, V - 1)]
    assert len(texts) == len(ds)
    assert got == rm.wer(_references(ds), texts)
    assert len(greedy) == len(ds)
    assert rm.test(m, ds, dev, **kw) == rm.wer(_references(ds), greedy)     # test() with defaults still reports the greedy decoder's number
    with pytest.raises(ValueError):
        rm.test(m, ds, dev, decoder='viterbi')
