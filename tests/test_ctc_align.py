"""Forced alignment on the device (csrc/ctc_align.hip, torch.ops.silent_speech.ctc_forced_align, recognition_model.forced_align* / word_segments /
align): the oracle against brute force, the tie rules on all-equal logits, constructed posteriors, repeats and infeasible cases, the arg-max path,
random logits against tests/ctc_align_oracle.py in float64, the CTC loss kernel as an upper bound, bit-for-bit isolation, and the Python surface.

Frame blocks of the kernel: AL_FB = 16 frames per gather block, AL_BT = 64 frames per backtrace block; a lane owns 1, 2, 4 or 8 tokens, chosen from
S + 1 (CTC) or S (linear) <= 64, 128, 256, 512.  SHAPES below puts T one below, at and one above 16, 32, 64 and 128, and S on both sides of every
instance edge of both topologies.

Score bar of the random cases: per case 4 x the largest |score of the oracle's own float32 run - of its float64 run| over the case's utterances,
computed in the test (the float32 run: log-sum-exp, logit - lse and one addition per frame, all in float32).  Measured: the largest float32
deviation per case was 5.2e-5 .. 2.3e-4 for SHAPES (bars 2.1e-4 .. 1.4e-3), 3.6e-4 / 5.5e-4 for LARGE, 5.9e-5 / 8.6e-5 for the slot cases, 9.8e-4
(CTC) and 1.7e-4 (linear) at S = 511 / T = 520, 1.1e-6 .. 3.9e-5 for the arg-max paths (T = 40 .. 130); the largest is 2.4e-7 of |score|.  The
kernel's own deviation from the float64 oracle equalled the float32 oracle's to all printed digits on the emulator tier and stayed within 1e-4 of
it on the MI355X (another log-sum-exp).  The float32 oracle's paths equalled the float64 oracle's on every utterance of every case (asserted), and
so did the kernel's on both tiers, so the 95 % cap on path equality is not what lets the kernel pass."""
import math

import numpy as np
import pytest
import torch

from silent_speech_amd import recognition_model as rm
from silent_speech_amd import torch_ops
from silent_speech_amd.architecture import Model
from tests import ctc_align_oracle as oracle
from tests.backend import dev, is_emu  # noqa: F401

NINF = -np.inf


def _align(dev, utts, ys, blank, layout='packed', ld=None, gaps=None, max_s=None, extra_targets=0):
    """utts: list of (T_i, V) float32 arrays, ys: their label lists.  layout 'packed': back to back, or with gaps[i] NaN rows in front of utterance
    i; 'slots': slot b starts at b * T_max, NaN filler.  ld > V: NaN in the extra columns.  Returns (list of rm.Alignment, raw frame_token)."""
    V = utts[0].shape[1]
    ld = ld or V
    frames = [int(x.shape[0]) for x in utts]
    if layout == 'slots':
        first = [b * max(frames) for b in range(len(utts))]
        rows = len(utts) * max(frames)
    else:
        gaps = gaps or [0] * len(utts)
        first, at = [], 0
        for g, n in zip(gaps, frames):
            first.append(at + g)
            at += g + n
        rows = at
    flat = np.full((rows, ld), np.nan, dtype=np.float32)
    for f0, x in zip(first, utts):
        flat[f0:f0 + x.shape[0], :V] = x
    S = [len(y) for y in ys]
    t0 = [extra_targets + int(v) for v in np.concatenate([[0], np.cumsum(S)])[:-1]]
    tg = np.asarray([7] * extra_targets + [c for y in ys for c in y], dtype=np.int32)
    utt = torch.tensor([[f, n, g, s] for f, n, g, s in zip(first, frames, t0, S)], dtype=torch.int64).reshape(len(utts), 4).to(dev)
    out = torch.ops.silent_speech.ctc_forced_align(torch.from_numpy(flat).to(dev), utt, torch.from_numpy(tg).to(dev), V, blank, sum(frames),
                                                   max(S) if max_s is None else max_s)
    score, ft, tf, tn, tl = (t.cpu().numpy() for t in out)
    covered = np.zeros(rows, dtype=bool)
    for f0, n in zip(first, frames):
        covered[f0:f0 + n] = True
    assert (ft[~covered] == -2).all()                                    # rows of no utterance
    return [rm.Alignment(float(score[b]), ft[first[b]:first[b] + frames[b]], tf[t0[b]:t0[b] + S[b]], tn[t0[b]:t0[b] + S[b]], tl[t0[b]:t0[b] + S[b]])
            for b in range(len(utts))], ft


def _same(a, b):
    return (a.score == b.score or (math.isnan(a.score) and math.isnan(b.score))) and all(
        np.array_equal(p, q) and p.dtype == q.dtype for p, q in zip(a[1:], b[1:])) and np.array_equal(a.token_logp.view(np.int32), b.token_logp.view(np.int32))


def _infeasible(al, T, S):
    return al.score == NINF and al.frames.tolist() == [-2] * T and al.token_first.tolist() == [-1] * S and al.token_frames.tolist() == [0] * S and \
        al.token_logp.tolist() == [0.0] * S


def _labels(rng, S, V, blank, repeats=None):
    """S labels without the blank; repeats = None: as they fall, 0: no two equal neighbours."""
    classes = [c for c in range(V) if c != blank]
    y = [int(classes[i]) for i in rng.integers(0, len(classes), S)]
    if repeats == 0:
        for k in range(1, S):
            while y[k] == y[k - 1]:
                y[k] = int(classes[rng.integers(0, len(classes))])
    return y


def _repeats(y):
    return sum(a == b for a, b in zip(y, y[1:]))


# ---------------------------------------------------------------------------------------------- 1. the oracle itself
@pytest.mark.parametrize('blank', [3, 0, -1])
def test_oracle_finds_the_maximum_over_all_paths(blank):
    rng = np.random.default_rng(11 + blank)
    seen = 0
    for T in range(0, 7):
        for S in range(0, 4):
            for rep in range(2):
                x = (rng.standard_normal((T, 4)) * 1.5).astype(np.float32)
                y = _labels(rng, S, 4, blank)
                paths = oracle.brute_force(x, y, blank)
                score, frames = oracle.align(x, y, blank)
                if not paths:
                    assert score == NINF and frames is None
                    continue
                seen += 1
                assert abs(score - paths[0][0]) < 1e-12
                assert frames in [f for s, f in paths if abs(s - paths[0][0]) < 1e-12]
                assert abs(oracle.rescore(x, y, blank, frames) - score) < 1e-12
                assert all(abs(oracle.rescore(x, y, blank, f) - s) < 1e-12 for s, f in paths[:5])
    assert seen > 20


# ---------------------------------------------------------------------------------------------- 2. ties
@pytest.mark.parametrize('y,blank,T,want', [
    ([0, 1], 3, 5, [0, 1, 1, 1, 1]), ([0, 0], 3, 5, [0, -1, 1, 1, 1]), ([0, 1], -1, 5, [0, 1, 1, 1, 1]),
    ([0, 1], 3, 2, [0, 1]), ([0, 0], 3, 3, [0, -1, 1]), ([0, 1], -1, 2, [0, 1]), ([2], 3, 1, [0]), ([0, 1, 1, 2], 3, 5, [0, 1, -1, 2, 3])])
def test_tie_rule_on_all_equal_logits(dev, y, blank, T, want):
    x = np.zeros((T, 4), dtype=np.float32)
    (al,), _ = _align(dev, [x], [y], blank)
    assert al.frames.tolist() == want
    assert oracle.align(x, y, blank)[1] == want and oracle.align(x, y, blank, np.float32)[1] == want
    assert abs(al.score + T * math.log(4.0)) < 2e-6 * T


def test_tie_rule_equals_the_oracle_on_further_sizes(dev):
    cases = [(T, S, blank) for blank in (4, 0, -1) for T, S in [(4, 1), (7, 3), (9, 4), (17, 5), (20, 9), (33, 12), (70, 66), (140, 65)]]
    rng = np.random.default_rng(2)
    for blank in (4, 0, -1):
        sub = [(T, S) for T, S, b in cases if b == blank]
        ys = [_labels(rng, S, 5, blank, repeats=0 if T < 2 * S else None) for T, S in sub]
        xs = [np.zeros((T, 5), dtype=np.float32) for T, _ in sub]
        als, _ = _align(dev, xs, ys, blank)
        for x, y, al in zip(xs, ys, als):
            score, frames = oracle.align(x, y, blank, np.float32)
            assert frames is not None and al.frames.tolist() == frames, (blank, x.shape[0], len(y))


# ---------------------------------------------------------------------------------------------- 3. constructed posteriors
def _from_probs(rows):
    return np.log(np.asarray(rows, dtype=np.float64)).astype(np.float32)


@pytest.mark.parametrize('topology', ['ctc', 'linear'])
def test_constructed_posteriors_have_the_obvious_path(dev, topology):
    V, blank = 3, (2 if topology == 'ctc' else -1)
    path = [2, 0, 0, 2, 1, 2] if topology == 'ctc' else [0, 0, 0, 1, 1, 2]
    y = [0, 1] if topology == 'ctc' else [0, 1, 2]
    want_frames = [-1, 0, 0, -1, 1, -1] if topology == 'ctc' else [0, 0, 0, 1, 1, 2]
    want_first, want_n = ([1, 4], [2, 1]) if topology == 'ctc' else ([0, 3, 5], [3, 2, 1])
    x = _from_probs([[0.6 if c == p else 0.2 for c in range(V)] for p in path])
    lp = oracle.log_probs(x)
    (al,), _ = _align(dev, [x], [y], blank)
    assert al.frames.tolist() == want_frames and al.token_first.tolist() == want_first and al.token_frames.tolist() == want_n
    want_score = sum(lp[t, p] for t, p in enumerate(path))
    assert abs(al.score - want_score) <= 1e-6 * abs(want_score)
    for k, (f, n) in enumerate(zip(want_first, want_n)):
        want = sum(lp[t, y[k]] for t in range(f, f + n))
        assert abs(al.token_logp[k] - want) <= 1e-6 * abs(want)
    blanks = sum(lp[t, blank] for t, k in enumerate(want_frames) if k < 0)
    assert abs(float(al.token_logp.astype(np.float64).sum()) + blanks - al.score) <= 1e-6 * abs(al.score)


# ---------------------------------------------------------------------------------------------- 4. repeats, infeasible and empty cases
def test_repeats_need_their_blank(dev):
    rng = np.random.default_rng(4)
    x2, x3 = (rng.standard_normal((2, 4)) * 3).astype(np.float32), (rng.standard_normal((3, 4)) * 3).astype(np.float32)
    als, _ = _align(dev, [x2, x3], [[0, 0], [0, 0]], 3)
    assert _infeasible(als[0], 2, 2)
    assert als[1].frames.tolist() == [0, -1, 1] and als[1].token_first.tolist() == [0, 2] and als[1].token_frames.tolist() == [1, 1]
    lp = oracle.log_probs(x3)
    assert abs(als[1].score - (lp[0, 0] + lp[1, 3] + lp[2, 0])) < 1e-5
    als, _ = _align(dev, [x2, x3], [[0, 0], [0, 0]], -1)                 # no blank to need: the linear topology aligns both
    assert als[0].frames.tolist() == [0, 1] and als[1].frames.tolist() == oracle.align(x3, [0, 0], -1)[1]


@pytest.mark.parametrize('blank', [3, -1])
def test_degenerate_sizes(dev, blank):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((4, 4)) * 2).astype(np.float32)
    xs = [x[:2], x, x[:0], x[:0], x]
    ys = [[0, 1, 2], [], [], [1], [1, 2]]                                # S > T; S = 0; T = 0 and S = 0; T = 0 and S > 0; a feasible neighbour
    als, _ = _align(dev, xs, ys, blank)
    assert _infeasible(als[0], 2, 3)
    if blank >= 0:
        assert als[1].frames.tolist() == [-1] * 4 and abs(als[1].score - float(oracle.log_probs(x)[:, 3].sum())) < 1e-5
    else:
        assert _infeasible(als[1], 4, 0)
    assert als[2].score == 0.0 and als[2].frames.size == 0 and als[2].token_first.size == 0
    assert _infeasible(als[3], 0, 1)
    score, frames = oracle.align(x, [1, 2], blank)
    assert als[4].frames.tolist() == frames and abs(als[4].score - score) < 1e-5


def test_bad_label_is_refused_in_python_and_minus_infinity_in_the_op(dev):
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((5, 4)) * 2).astype(np.float32)
    for blank, y in [(3, [0, 4]), (3, [0, -1]), (3, [0, 3]), (-1, [0, 4]), (-1, [-1, 1]), (3, [2 ** 30, 1])]:
        als, _ = _align(dev, [x, x], [y, [0, 1]], blank)
        assert _infeasible(als[0], 5, 2), (blank, y)
        assert als[1].frames.tolist() == oracle.align(x, [0, 1], blank)[1]
        with pytest.raises(ValueError):
            rm.forced_align(torch.from_numpy(x).to(dev).reshape(1, 5, 4), [5], [y], None if blank >= 0 else 0, topology='ctc' if blank >= 0 else 'linear')
    pred = torch.from_numpy(x).to(dev).reshape(1, 5, 4)
    for bad in [dict(lengths=[6]), dict(lengths=[-1]), dict(targets=[[0] * 512]), dict(topology='hmm'), dict(targets=[[0], [1]])]:
        kw = dict(lengths=[5], targets=[[0, 1]], topology='ctc')
        kw.update(bad)
        with pytest.raises(ValueError):
            rm.forced_align(pred, kw['lengths'], kw['targets'], topology=kw['topology'])
    # a table entry whose targets leave the array or exceed max_target_len: -inf, nothing out of bounds
    utt = torch.tensor([[0, 5, 1, 2], [0, 5, 0, 2], [0, 5, -1, 1]], dtype=torch.int64).to(dev)
    out = torch.ops.silent_speech.ctc_forced_align(torch.from_numpy(x).to(dev), utt, torch.tensor([0, 1], dtype=torch.int32).to(dev), 4, 3, 15, 2)
    assert out[0].cpu().tolist()[0] == NINF and out[0].cpu().tolist()[2] == NINF and out[0].cpu().tolist()[1] > NINF
    out = torch.ops.silent_speech.ctc_forced_align(torch.from_numpy(x).to(dev), utt[1:2], torch.tensor([0, 1], dtype=torch.int32).to(dev), 4, 3, 5, 1)
    assert out[0].cpu().tolist() == [NINF] and out[1].cpu().tolist() == [-2] * 5


# ---------------------------------------------------------------------------------------------- 6. random logits against the float64 oracle
# (S, T): S <= 9 with T around the frame blocks; S >= 31: T = the number given + the repeats of the labels, or 'min' = S + repeats, the shortest
# feasible length, 'min-1' (no alignment), 'S' = S frames for labels without repeats
SHAPES = [(3, 15), (3, 16), (3, 17), (5, 31), (5, 32), (5, 33), (7, 63), (7, 64), (7, 65), (9, 127), (9, 128), (9, 129), (2, 8), (1, 1),
          (31, 'min'), (31, 'min-1'), (32, 'S'), (63, 'min'), (64, 'S'), (64, 70), (65, 'min'), (127, 'min'), (128, 'min-1'), (128, 130), (129, 'min')]
LARGE = [(255, 'min'), (256, 'S'), (256, 270), (257, 'min')]             # 4 tokens per lane, and the first sizes with 8
RANDOM_CASES = [(V, scale, topology, 'SHAPES') for V in (5, 38) for scale in (1.0, 3.0) for topology in ('ctc', 'linear')] + \
    [(38, 1.0, 'ctc', 'LARGE'), (5, 3.0, 'linear', 'LARGE')]
_REF = {}


def _random_inputs(V, scale, topology, shapes=SHAPES):
    blank = V - 1 if topology == 'ctc' else -1
    rng = np.random.default_rng(1000 * V + int(10 * scale) + (topology == 'linear'))
    xs, ys = [], []
    for S, T in shapes:
        y = _labels(rng, S, V, blank, repeats=0 if T == 'S' else None)
        r = _repeats(y) if blank >= 0 else 0
        T = {'min': S + r, 'min-1': S + r - 1, 'S': S}[T] if isinstance(T, str) else T + (r if S >= 31 else 0)
        xs.append((rng.standard_normal((T, V)) * scale).astype(np.float32))
        ys.append(y)
    return xs, ys, blank


def _references(tag, xs, ys, blank):
    """Per utterance (float64 score, float64 path, float32 score, float32 path), computed once per case and shared between the backends."""
    if tag not in _REF:
        _REF[tag] = [oracle.align(x, y, blank) + oracle.align(x, y, blank, np.float32) for x, y in zip(xs, ys)]
    return _REF[tag]


def _bar(refs):
    dev32 = [abs(r[2] - r[0]) for r in refs if r[1] is not None]
    assert all(r[1] == r[3] for r in refs), 'the float32 oracle takes another path: choose other seeds'
    return 4 * max(dev32), max(dev32)


def _check_against_oracle(als, xs, ys, blank, refs, what):
    bar, dev32 = _bar(refs)
    assert bar > 0
    same = feasible = 0
    worst = 0.0
    for al, x, y, (s64, f64, _, _) in zip(als, xs, ys, refs):
        T, S = x.shape[0], len(y)
        if f64 is None:
            assert _infeasible(al, T, S), (what, T, S)
            continue
        feasible += 1
        worst = max(worst, abs(al.score - s64))
        again = oracle.rescore(x, y, blank, al.frames.tolist())
        assert again is not None, (what, T, S, 'not an alignment')
        assert abs(again - s64) <= bar, (what, T, S)
        same += al.frames.tolist() == f64
        first, count, logp = oracle.spans(x, y, blank, al.frames.tolist())
        assert al.token_first.tolist() == first and al.token_frames.tolist() == count
        assert np.allclose(al.token_logp, logp, rtol=1e-5, atol=1e-5)
    print('%s: %d feasible of %d, same path %d, largest score deviation %.3e (float32 oracle %.3e, bar %.3e)' % (what, feasible, len(als), same, worst, dev32, bar))
    assert worst <= bar
    assert same >= 0.95 * feasible
    return feasible


@pytest.mark.parametrize('V,scale,topology,shapes', RANDOM_CASES)
def test_random_logits_match_the_float64_oracle(dev, V, scale, topology, shapes):
    """Packed layout with NaN rows between the utterances and NaN columns behind the classes."""
    xs, ys, blank = _random_inputs(V, scale, topology, {'SHAPES': SHAPES, 'LARGE': LARGE}[shapes])
    refs = _references((V, scale, topology, shapes), xs, ys, blank)
    als, _ = _align(dev, xs, ys, blank, ld=V + 3, gaps=[(3 * i) % 5 for i in range(len(xs))], extra_targets=2)
    feasible = _check_against_oracle(als, xs, ys, blank, refs, 'V %d, N(0, %g), %s' % (V, scale, topology))
    assert feasible == len(xs) - (2 if shapes == 'SHAPES' else 0)        # all but the two 'min-1' shapes


@pytest.mark.parametrize('topology', ['ctc', 'linear'])
def test_slot_layout_equals_the_packed_one(dev, topology):
    xs, ys, blank = _random_inputs(38, 3.0, topology, SHAPES[:9] + [(2, 8), (31, 'min')])
    refs = _references((38, 3.0, topology, 'slots'), xs, ys, blank)
    slots, _ = _align(dev, xs, ys, blank, layout='slots', ld=40)
    _check_against_oracle(slots, xs, ys, blank, refs, 'slots, %s' % topology)
    packed, _ = _align(dev, xs, ys, blank)
    assert all(_same(a, b) for a, b in zip(slots, packed))


@pytest.mark.parametrize('topology', ['ctc', 'linear'])
def test_longest_target(dev, topology):
    """S = 511 (1023 states under CTC, 8 tokens per lane), T = 520, and one utterance at the shortest feasible length."""
    blank = 37 if topology == 'ctc' else -1
    rng = np.random.default_rng(9)
    ys = [_labels(rng, 511, 38, blank, repeats=0), _labels(rng, 511, 38, blank), _labels(rng, 500, 38, blank)]
    frames = [520, 511 + (_repeats(ys[1]) if blank >= 0 else 0), 540]
    xs = [rng.standard_normal((T, 38)).astype(np.float32) for T in frames]
    refs = _references((topology, 'longest'), xs, ys, blank)
    als, _ = _align(dev, xs, ys, blank, ld=38)
    assert _check_against_oracle(als, xs, ys, blank, refs, 'S = 511, %s' % topology) == 3
    assert xs[0].shape[0] == 520 and len(ys[0]) == 511


# ---------------------------------------------------------------------------------------------- 5. the arg-max path, independent of the oracle's search
@pytest.mark.parametrize('V,T,scale', [(5, 40, 3.0), (38, 100, 3.0), (38, 130, 1.0)])
def test_greedy_consistency(dev, V, T, scale):
    """y = the collapse of the per-frame arg-max path: that path is the best alignment, its score the sum of the per-frame maxima."""
    blank = V - 1
    x = (np.random.default_rng(V + T).standard_normal((T, V)) * scale).astype(np.float32)
    best = x.argmax(1)
    y, frames, prev = [], [], -1
    for c in best:
        if c == blank:
            frames.append(-1)
        else:
            if c != prev:
                y.append(int(c))
            frames.append(len(y) - 1)
        prev = c
    assert 0 < len(y) <= 511
    lp = oracle.log_probs(x)
    want = float(lp.max(1).sum())
    bar = 4 * abs(oracle.align(x, y, blank, np.float32)[0] - oracle.align(x, y, blank)[0])
    (al,), _ = _align(dev, [x], [y], blank)
    print('arg-max path, V %d T %d: score deviation %.3e (bar %.3e)' % (V, T, abs(al.score - want), bar))
    assert bar > 0 and abs(al.score - want) <= bar
    assert al.frames.tolist() == frames


# ---------------------------------------------------------------------------------------------- 7. against the loss kernel
def _nll(dev, xs, ys, blank):
    V = xs[0].shape[1]
    pred = torch.from_numpy(np.concatenate(xs)).to(dev).reshape(1, -1, V)
    _, plan = rm.ctc_loss(pred, {'lengths': [x.shape[0] for x in xs], 'text_int': [torch.tensor(y, dtype=torch.int64) for y in ys]}, blank, return_plan=True)
    return plan.nll.cpu().numpy()


def test_score_is_bounded_by_the_ctc_likelihood(dev):
    """The best path is one of the paths the loss sums: score <= -nll; on near one-hot posteriors the best path carries all the mass."""
    xs, ys, blank = _random_inputs(38, 3.0, 'ctc', [(3, 17), (7, 64), (9, 30), (31, 40), (2, 8)])
    refs = _references(('loss',), xs, ys, blank)
    bar, _ = _bar(refs)
    als, _ = _align(dev, xs, ys, blank)
    nll = _nll(dev, xs, ys, blank)
    for al, v in zip(als, nll):
        assert al.score > NINF and al.score <= -float(v) + bar + 1e-6 * abs(float(v))          # (the loss kernel's own rounding: 1e-6 of |nll|)
    rng = np.random.default_rng(8)
    hot, hy = [], []
    for T in (12, 40):
        path = rng.integers(0, 5, T)
        x = np.zeros((T, 5), dtype=np.float32)
        x[np.arange(T), path] = 15.0
        hot.append(x)
        hy.append(rm._collapse(path, 4))
    als, _ = _align(dev, hot, hy, 4)
    nll = _nll(dev, hot, hy, 4)
    for al, v in zip(als, nll):
        assert abs(al.score + float(v)) < 1e-3


# ---------------------------------------------------------------------------------------------- 8. isolation
@pytest.mark.parametrize('topology', ['ctc', 'linear'])
def test_an_utterance_alone_equals_itself_inside_a_batch(dev, topology):
    shapes = [(3, 17), (5, 'min-1'), (0, 6), (7, 64), (2, 'min'), (0, 0), (65, 70), (9, 30)]
    xs, ys, blank = _random_inputs(38, 3.0, topology, shapes)
    batch, _ = _align(dev, xs, ys, blank, ld=41, gaps=[2, 0, 1, 0, 3, 0, 0, 1])
    kinds = set()
    for b, (x, y) in enumerate(zip(xs, ys)):
        (alone,), _ = _align(dev, [x], [y], blank, max_s=max(len(y), 1))
        assert _same(alone, batch[b]), (topology, b)
        kinds.add('empty' if x.shape[0] == 0 else 'none' if alone.score == NINF else 'ok')
    assert kinds == {'empty', 'none', 'ok'}
    others, _ = _align(dev, [xs[i] for i in (0, 3, 7)], [ys[i] for i in (0, 3, 7)], blank)          # without the infeasible and the empty ones
    assert all(_same(a, batch[i]) for a, i in zip(others, (0, 3, 7)))


# ---------------------------------------------------------------------------------------------- 9. the op
def _args(dev, **kw):
    x = (np.random.default_rng(5).standard_normal((12, 6)) * 2).astype(np.float32)
    a = dict(logits=torch.from_numpy(x).to(dev), utt=torch.tensor([[0, 7, 0, 2], [7, 5, 2, 3]], dtype=torch.int64).to(dev),
             targets=torch.tensor([0, 1, 2, 2, 4], dtype=torch.int32).to(dev), V=6, blank=5, total_frames=12, max_target_len=3)
    a.update(kw)
    return tuple(a.values())


def test_op_is_registered_and_passes_opcheck(dev):
    assert 'ctc_forced_align' in torch_ops.OPS
    torch.library.opcheck(torch.ops.silent_speech.ctc_forced_align.default, _args(dev), test_utils=('test_schema', 'test_faketensor'))
    torch.library.opcheck(torch.ops.silent_speech.ctc_forced_align.default, _args(dev, blank=-1), test_utils=('test_schema', 'test_faketensor'))


def test_op_refuses_bad_arguments(dev):
    good = _args(dev)
    wide = torch.zeros(2, 5, dtype=torch.int64).to(dev)
    for bad in [dict(utt=wide[:, :4]), dict(utt=good[1].to(torch.int32)), dict(logits=good[0].double()), dict(targets=good[2].to(torch.int64)),
                dict(logits=good[0].t()), dict(V=7), dict(V=0), dict(blank=6), dict(blank=-2), dict(max_target_len=512), dict(max_target_len=-1),
                dict(total_frames=-1), dict(utt=good[1][:, :2].contiguous())]:
        with pytest.raises(RuntimeError, match='ctc_forced_align'):
            torch.ops.silent_speech.ctc_forced_align(*_args(dev, **bad))
    score = torch.ops.silent_speech.ctc_forced_align(*good)[0]          # and the library is fine afterwards
    assert torch.isfinite(score).all()


# ---------------------------------------------------------------------------------------------- 10. the Python surface
def test_forced_align_and_forced_align_utterances_agree(dev):
    rng = np.random.default_rng(12)
    V, frames = 38, [9, 20, 14]
    ys = [_labels(rng, S, V, V - 1) for S in (3, 6, 0)]
    head = torch.from_numpy(np.full((3 * 20, 40), np.nan, dtype=np.float32))
    xs = [(rng.standard_normal((T, V)) * 2).astype(np.float32) for T in frames]
    for b, x in enumerate(xs):
        head[b * 20:b * 20 + x.shape[0], :V] = torch.from_numpy(x)
    head = head.to(dev)
    views = [head[b * 20:b * 20 + T, :V] for b, T in enumerate(frames)]
    packed = torch.from_numpy(np.concatenate(xs)).to(dev).reshape(1, -1, V)
    for topology in ('ctc', 'linear'):
        a = rm.forced_align(packed, frames, [torch.tensor(y) for y in ys], topology=topology)
        b = rm.forced_align_utterances(views, ys, topology=topology)
        assert len(a) == len(b) == 3 and all(_same(p, q) for p, q in zip(a, b))
        for x, y, al in zip(xs, ys, a):
            score, path = oracle.align(x, y, V - 1 if topology == 'ctc' else -1)
            assert (al.frames.tolist() == path and abs(al.score - score) < 1e-4) if path is not None else _infeasible(al, x.shape[0], len(y))
            assert isinstance(al.score, float) and al.frames.dtype == np.int32 and al.token_logp.dtype == np.float32
    with pytest.raises(ValueError):
        rm.forced_align_utterances([v.clone() for v in views], ys)
    assert rm.forced_align_utterances([], []) == []


def test_word_segments_of_a_hand_made_alignment():
    tt = rm.TextTransform()
    text = tt.text_to_int(' ab c ')
    al = rm.Alignment(-3.0, np.asarray([-1, 0, 1, 1, -1, 2, 3, 3, -1, 4, 4, 5, -1], dtype=np.int32), np.asarray([1, 2, 5, 6, 9, 11], dtype=np.int32),
                      np.asarray([1, 2, 1, 2, 2, 1], dtype=np.int32), np.asarray([-0.5, -0.2, -0.1, -0.4, -0.6, -0.3], dtype=np.float32))
    words = rm.word_segments(al, text, tt, frame_seconds=0.5)
    assert [(w, a, z) for w, a, z, _ in words] == [('ab', 1.0, 3.0), ('c', 4.5, 5.5)]
    assert abs(words[0][3] - math.exp(-0.3 / 3)) < 1e-6 and abs(words[1][3] - math.exp(-0.6 / 2)) < 1e-6
    assert rm.word_segments(al, text, tt)[0][2] == 6 * 256 / 22050
    none = rm.Alignment(NINF, np.full(13, -2, dtype=np.int32), np.full(6, -1, dtype=np.int32), np.zeros(6, dtype=np.int32), np.zeros(6, dtype=np.float32))
    assert rm.word_segments(none, text, tt) == []
    assert rm.word_segments(rm.Alignment(-1.0, np.asarray([0, 0], dtype=np.int32), np.asarray([0], dtype=np.int32), np.asarray([2], dtype=np.int32),
                                         np.asarray([-1.0], dtype=np.float32)), tt.text_to_int(' '), tt) == []


def test_align_returns_the_words_of_the_transcripts(dev, monkeypatch):
    from silent_speech_amd.synthetic import SyntheticEMGDataset
    ds = SyntheticEMGDataset(2 if is_emu(dev) else 5, seed=3, min_frames=8, max_frames=16 if is_emu(dev) else 48, silent_fraction=0.0)
    torch.manual_seed(1)
    m = Model(ds.num_features, len(ds.text_transform.chars) + 1, model_size=16, num_layers=1, dropout=0.0, compute_dtype=torch.float32).to(dev)
    m.train()
    seen = []
    forward = m.forward_utterances
    monkeypatch.setattr(m, 'forward_utterances', lambda xs: seen.append(forward(xs)) or seen[-1])
    got = rm.align(m, ds, dev, batch_size=3)
    assert m.training
    logits = [y for group in seen for y in group]
    assert len(got) == len(ds) == len(logits)
    tt = ds.text_transform
    texts = [torch.as_tensor(ds[i]['text_int']).tolist() for i in range(len(ds))]
    at = 0
    for group in seen:
        als = rm.forced_align_utterances(group, texts[at:at + len(group)])
        assert [rm.word_segments(al, t, tt) for al, t in zip(als, texts[at:at + len(group)])] == got[at:at + len(group)]
        at += len(group)
    for words, text, y in zip(got, texts, logits):
        assert [w for w, _, _, _ in words] == tt.int_to_text(text).split()
        end = 0.0
        for _, a, z, conf in words:
            assert end <= a < z <= y.shape[0] * rm.FRAME_SECONDS + 1e-12 and 0.0 < conf <= 1.0
            end = z
