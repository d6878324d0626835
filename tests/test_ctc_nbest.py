"""n-best training criterion (csrc/ctc.hip: ss_ctc_nbest_logp / ss_ctc_nbest_backward / ss_nbest_expected_risk; recognition_model.nbest_logp,
rescore_nbest, mwer_loss, train_model(mwer=)) against the float64 oracle of tests/ctc_nbest_oracle.py, on the emulator and on the MI355X.

Bars (derived from the ones fixed in tests/test_ctc_edges.py; no outliers):
  logp          1e-5 relative, the -inf pattern exact.
  gradient      per element |got - want| <= sum_h |g_h| 2e-3 (|d logp_h| + occ_h) + 1e-6 sum_h |g_h|   (h over the feasible hypotheses of the
                frame's utterance; the kernel forms occ_h as exp(.. - logp_h - lp) in f32, the error scales with that term as in ctc_grad_kernel).
  expected risk against f64 at the SAME f32 inputs: post and dlogp 1e-6 relative (f32 roundings of f64 sums; + 1e-12 absolute), risk 1e-12
                (relative to max(1, |risk|)), loss 1e-6 relative + 1e-7.
  mwer_loss     the oracle scores its lists in f64, the package in f32 within the logp bar: delta = 1e-5 max |logp| moves every posterior
                by a factor within exp(+-2 scale delta), so with C = max_k |cost_k - mean cost| of a list
                    |d risk_u| <= 2 scale delta C,   |d dlogp_k| <= 4 scale^2 delta post_k C / n_used   (first order, doubled below for the rest).
                Value: 1e-6 relative + the mean of the first; gradient: the kernel bar at the oracle's cotangents + sum_h slack_h |d logp_h|
                with slack_h twice the second + 1e-6 |dlogp_h|.
Frames behind the last utterance, the columns behind V and a spare row hold NaN and must get a gradient of exactly 0."""
import numpy as np
import pytest
import torch

from silent_speech_amd import _lib
from silent_speech_amd import recognition_model as rm
from tests import ctc_nbest_oracle as oracle
from tests.backend import dev  # noqa: F401
from tests.test_train import tiny_flags  # noqa: F401


# ---------------------------------------------------------------- the oracle, checked against itself (CPU, no kernel)
def test_oracle_gradient_matches_central_differences():
    rng = np.random.default_rng(0)
    V, blank, space = 5, 4, 3
    frames, first = [7, 6], [0, 7]
    flat = rng.standard_normal((13, V))
    refs = [[0, 3, 1], [2, 3, 0]]
    hyps = [[[0, 3, 1], [0, 1], [1, 3, 1, 3, 2]], [[2, 3, 0], [2, 2], []]]
    for w in (0.0, 0.5):
        out = oracle.mwer(flat, first, frames, refs, hyps, blank, space, scale=0.7, ctc_weight=w)
        num = np.zeros_like(flat)
        eps = 1e-6
        for i in range(flat.shape[0]):
            for j in range(V):
                hi, lo = flat.copy(), flat.copy()
                hi[i, j] += eps
                lo[i, j] -= eps
                num[i, j] = (oracle.mwer(hi, first, frames, refs, hyps, blank, space, scale=0.7, ctc_weight=w)['loss'] -
                             oracle.mwer(lo, first, frames, refs, hyps, blank, space, scale=0.7, ctc_weight=w)['loss']) / (2 * eps)
        assert np.abs(out['grad']).max() > 1e-3
        assert np.abs(num - out['grad']).max() < 1e-8, np.abs(num - out['grad']).max()
    assert abs(sum(out['dlogp'][:3])) < 1e-15 and abs(sum(out['dlogp'][3:])) < 1e-15


# ---------------------------------------------------------------- helpers
def _draw(rng, n, alphabet, repeats=0):
    """n labels, no two neighbours equal except exactly `repeats` pairs."""
    alphabet = np.asarray(alphabet)
    t = [int(rng.choice(alphabet))]
    same = set(int(i) for i in np.linspace(1, n - 1, repeats + 2)[1:-1].round()) if repeats else set()
    assert len(same) == repeats
    for i in range(1, n):
        t.append(t[-1] if i in same else int(rng.choice(alphabet[alphabet != t[-1]])))
    return t[:n]


def _tables(first, frames, hyps):
    """The tables of ss_ctc_nbest_logp, built here (not by the package)."""
    utt, hyp, flat, ws = [], [], [], 0
    for f0, T, lst in zip(first, frames, hyps):
        utt.append((f0, T, len(hyp), len(lst)))
        for h in lst:
            hyp.append((len(flat), len(h), ws))
            flat.extend(h)
            ws += T * (2 * len(h) + 1)
    return (np.asarray(utt, dtype=np.int64).reshape(-1, 4), np.asarray(hyp, dtype=np.int64).reshape(-1, 3), np.asarray(flat + [0], dtype=np.int32), ws,
            max([len(h) for lst in hyps for h in lst] or [0]))


def _run_op(dev, x2d, V, blank, first, frames, hyps, g):
    """ctc_nbest_logp on an (M, ld) matrix and its gradient twice: through autograd, and by ss_ctc_nbest_backward into a buffer pre-filled with NaN."""
    utt, hyp, flat, ws_floats, max_s = _tables(first, frames, hyps)
    x = torch.from_numpy(x2d.copy()).to(dev).requires_grad_(True)
    t = [torch.from_numpy(a).to(dev) for a in (utt, hyp, flat)]
    logp, lse, ws = torch.ops.silent_speech.ctc_nbest_logp(x, t[0], t[1], t[2], max_s, ws_floats, V, blank)
    gd = torch.from_numpy(np.asarray(g, dtype=np.float32)).to(dev)
    if len(g):
        logp.backward(gd)
        auto = x.grad.cpu().numpy()
    else:
        auto = None
    direct = torch.full_like(x.detach(), float('nan'))
    p = _lib.ptr
    M, ld = x2d.shape
    _lib.check(_lib.lib().ss_ctc_nbest_backward(p(x.detach()), ld, V, blank, M, p(lse), p(t[0]) if len(utt) else None, len(utt), len(hyp), p(t[2]), p(ws), ws_floats,
                                                p(logp.detach()) if len(hyp) else None, p(gd) if len(hyp) else None, p(direct), _lib.stream_of(x)), 'ss_ctc_nbest_backward')
    return logp.detach().cpu().numpy(), auto, direct.cpu().numpy()


def _check_logp(got, want):
    want = np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)) and not np.isnan(got).any() and not np.isposinf(got).any()
    fin = np.isfinite(want)
    ratio = np.abs(got[fin] - want[fin]) / (1e-5 * np.abs(want[fin]) + 1e-30)
    print('logp worst ratio to the bar: %.3f' % (ratio.max() if ratio.size else 0.0))
    assert (ratio <= 1.0).all(), ratio.max()


def _check_grad(got, want, bar, what='gradient'):
    assert not np.isnan(got).any(), what
    ratio = np.abs(got - want) / np.maximum(bar, 1e-300)
    ratio = np.where((bar == 0) & (got == want), 0.0, ratio)
    print('%s worst ratio to the bar: %.3f' % (what, ratio.max()))
    assert (ratio <= 1.0).all(), (what, ratio.max())


# ---------------------------------------------------------------- 1. hypotheses that share frames
@pytest.mark.parametrize('V,blank,pad', [(5, 2, 0), (65, 64, 3)])
def test_shared_frames(dev, V, blank, pad):
    rng = np.random.default_rng(V)
    alphabet = [c for c in range(V) if c != blank]
    frames, first = [9, 64, 70], [0, 9, 73]
    a, b = alphabet[0], alphabet[-1]
    hyps = [[[a, a, b]],
            [[], [b], _draw(rng, 64, alphabet)],                                           # 64 labels: SP = 129, two compute waves, T = S
            [_draw(rng, 64, alphabet), _draw(rng, 69, alphabet, repeats=2), [b], [a, a], []]]       # 69 + 2 > 70: no alignment
    g = [0.7, 0.0, -1.3, 1.3, 0.9, 5.0, -0.4, 0.3, -0.2]                                 # a zero, negatives, a list that sums to 0 and two that do not
    M, ld = 150, V + pad
    x = np.full((M, ld), np.nan, dtype=np.float32)
    x[:143, :V] = (1.5 * rng.standard_normal((143, V))).astype(np.float32)
    logp, auto, direct = _run_op(dev, x, V, blank, first, frames, hyps, g)
    flat = x[:, :V].astype(np.float64)
    flat[143:] = 0.0
    scored = oracle.nbest_logp(flat, first, frames, hyps, blank)
    want_logp = [s[0] for lst in scored for s in lst]
    assert np.isneginf(want_logp).sum() == 1 and np.isneginf(want_logp[5])
    _check_logp(logp, want_logp)
    want, bar = oracle.nbest_backward(flat, first, frames, scored, g)
    for got, what in ((auto, 'autograd'), (direct, 'direct call')):
        assert (got[143:] == 0).all() and (got[:, V:] == 0).all(), what
        _check_grad(got[:, :V], want, bar, what)


# ---------------------------------------------------------------- 2. an empty list between two others; no utterance at all
def test_empty_list_and_no_utterance(dev):
    rng = np.random.default_rng(2)
    V, blank = 7, 6
    frames, first = [12, 10, 11], [0, 12, 22]
    hyps = [[[0, 1]], [], [[2], [3, 3]]]
    x = (1.5 * rng.standard_normal((40, V))).astype(np.float32)
    x[33:] = np.nan
    g = [0.5, -1.0, 2.0]
    logp, auto, direct = _run_op(dev, x, V, blank, first, frames, hyps, g)
    flat = x.astype(np.float64)
    flat[33:] = 0.0
    scored = oracle.nbest_logp(flat, first, frames, hyps, blank)
    _check_logp(logp, [s[0] for lst in scored for s in lst])
    want, bar = oracle.nbest_backward(flat, first, frames, scored, g)
    for got in (auto, direct):
        assert (got[12:22] == 0).all() and (got[33:] == 0).all()
        _check_grad(got, want, bar)
    logp, auto, direct = _run_op(dev, x, V, blank, [], [], [], [])
    assert logp.shape == (0,) and (direct == 0).all()


# ---------------------------------------------------------------- 3. one hypothesis per utterance, the reference: the existing loss
def test_agrees_with_ctc_loss(dev):
    rng = np.random.default_rng(3)
    V, blank, row = 9, 8, 40
    lengths = [9, 70, 33]
    text = [_draw(rng, 3, range(8)), _draw(rng, 20, range(8), repeats=2), []]
    x = (1.5 * rng.standard_normal((4, row, V))).astype(np.float32)
    used = sum(lengths)
    x.reshape(-1, V)[used:] = np.nan
    example = dict(lengths=lengths, text_int=[torch.tensor(t, dtype=torch.int64) for t in text])
    a = torch.from_numpy(x.copy()).to(dev).requires_grad_(True)
    loss, plan = rm.ctc_loss(a, example, blank=blank, return_plan=True)
    loss.backward()
    b = torch.from_numpy(x.copy()).to(dev).requires_grad_(True)
    logp = rm.nbest_logp(b, lengths, [[t] for t in text], blank)
    assert torch.equal(logp.detach(), -plan.nll), (logp, plan.nll)                       # bit for bit
    n = len(lengths)
    g = [-1.0 / (max(len(t), 1) * n) for t in text]
    logp.backward(torch.tensor(g, dtype=torch.float32).to(dev))
    flat = x.reshape(-1, V).astype(np.float64)
    flat[used:] = 0.0
    first = [0, 9, 79]
    scored = oracle.nbest_logp(flat, first, lengths, [[t] for t in text], blank)
    want, bar = oracle.nbest_backward(flat, first, lengths, scored, g)
    ga, gb = a.grad.cpu().numpy().reshape(-1, V), b.grad.cpu().numpy().reshape(-1, V)
    assert (gb[used:] == 0).all()
    _check_grad(gb, want, bar, 'nbest against the oracle')
    _check_grad(gb, ga, 2 * bar, 'nbest against ctc_loss (sum of both bars)')      # at these cotangents both bars are the same expression


# ---------------------------------------------------------------- 4. expected risk
def _risk_op(dev, logp_lists, cost_lists, scale, groups=None):
    lp = np.concatenate([np.zeros(0, dtype=np.float32)] + [np.asarray(a, dtype=np.float32) for a in logp_lists])
    c = np.concatenate([np.zeros(0, dtype=np.float32)] + [np.asarray(a, dtype=np.float32) for a in cost_lists])
    if groups is None:
        sizes = [len(a) for a in logp_lists]
        groups = np.stack([np.concatenate([[0], np.cumsum(sizes)])[:-1], sizes], 1)
    lp_d = torch.from_numpy(lp).to(dev).requires_grad_(True)
    loss, risk, post, dlogp = torch.ops.silent_speech.nbest_expected_risk(lp_d, torch.from_numpy(c).to(dev), torch.from_numpy(np.asarray(groups, dtype=np.int64).reshape(-1, 2)).to(dev), scale)
    (3.0 * loss[0]).backward()
    assert torch.equal(lp_d.grad, 3.0 * dlogp)
    return float(loss.detach()[0]), risk.detach().cpu().numpy(), post.detach().cpu().numpy(), dlogp.detach().cpu().numpy(), lp, c


def test_expected_risk(dev):
    rng = np.random.default_rng(4)
    sizes = [1, 2, 64, 65, 128, 5, 6, 3]
    logps = [(-40 + 6 * rng.standard_normal(k)).astype(np.float32) for k in sizes]
    costs = [rng.integers(0, 9, k).astype(np.float32) for k in sizes]
    costs[5][:] = 4.0                                                    # equal costs: zero gradient
    logps[6][[1, 4]] = -np.inf                                           # some infeasible entries
    logps[7][:] = -np.inf                                                # no posterior: not one of the lists of the mean
    for scale in (1.0, 0.35):
        loss, risk, post, dlogp, lp32, c32 = _risk_op(dev, logps, costs, scale)
        wl, wr, wp, wd = oracle.expected_risk(logps, costs, scale)
        wp, wd = np.concatenate(wp), np.concatenate(wd)
        assert not np.isnan(post).any() and not np.isnan(dlogp).any() and not np.isnan(loss)
        assert np.isnan(risk[7]) and np.isnan(wr[7]) and not np.isnan(risk[:7]).any()
        assert (np.abs(risk[:7] - wr[:7]) <= 1e-12 * np.maximum(1.0, np.abs(wr[:7]))).all(), np.abs(risk[:7] - wr[:7]).max()
        assert (np.abs(post - wp) <= 1e-6 * np.abs(wp) + 1e-12).all(), (np.abs(post - wp) / (np.abs(wp) + 1e-30)).max()
        assert (np.abs(dlogp - wd) <= 1e-6 * np.abs(wd) + 1e-12).all(), (np.abs(dlogp - wd) / (np.abs(wd) + 1e-30)).max()
        assert abs(loss - wl) <= 1e-6 * abs(wl) + 1e-7
        first = np.concatenate([[0], np.cumsum(sizes)])
        assert risk[0] == 0 and dlogp[0] == 0 and post[0] == 1                          # K = 1
        assert (dlogp[first[5]:first[6]] == 0).all()                                     # equal costs
        inf6 = first[6] + np.array([1, 4])
        assert (post[inf6] == 0).all() and (dlogp[inf6] == 0).all()
        assert (post[first[7]:] == 0).all() and (dlogp[first[7]:] == 0).all()
        for k in range(len(sizes)):
            d = dlogp[first[k]:first[k + 1]].astype(np.float64)
            assert abs(d.sum()) <= 1e-6 * np.abs(d).sum()


def test_expected_risk_bad_group(dev):
    rng = np.random.default_rng(5)
    logps = [(-20 + 3 * rng.standard_normal(k)).astype(np.float32) for k in (3, 4)]
    costs = [rng.integers(0, 5, k).astype(np.float32) for k in (3, 4)]
    good = oracle.expected_risk(logps, costs, 1.0)
    for bad in ((0, 129), (5, 3), (-1, 2)):                              # K = 129; leaves [0, 7); first < 0
        groups = [(0, 3), bad, (3, 4)]
        loss, risk, post, dlogp, _, _ = _risk_op(dev, logps, costs, 1.0, groups)
        assert np.isnan(risk[1]) and (np.abs(risk[[0, 2]] - good[1]) <= 1e-12).all()
        assert (np.abs(dlogp - np.concatenate(good[3])) <= 1e-6 * np.abs(np.concatenate(good[3])) + 1e-12).all()
        assert abs(loss - good[0]) <= 1e-6 * abs(good[0]) + 1e-7
    loss, risk, post, dlogp, _, _ = _risk_op(dev, [], [], 1.0, np.zeros((0, 2)))
    assert loss == 0.0


# ---------------------------------------------------------------- 5 - 7. mwer_loss, rescore_nbest
V6, BLANK6, SPACE6, ROW6 = 6, 5, 4, 40
LENGTHS6 = [40, 37, 23]
REFS6 = [[0, 1, 4, 2, 3, 4, 1], [2, 4, 0, 0, 1], [3, 4, 3]]


def _pred6(seed, poison=True):
    rng = np.random.default_rng(seed)
    x = (1.2 * rng.standard_normal((3, ROW6, V6))).astype(np.float32)
    # pull the frames towards the reference, so that the lists are not all equally bad
    off = 0
    for T, ref in zip(LENGTHS6, REFS6):
        for t in range(T):
            x.reshape(-1, V6)[off + t, ref[min(t * len(ref) // T, len(ref) - 1)] if t % 3 else BLANK6] += 2.0
        off += T
    if poison:
        x.reshape(-1, V6)[sum(LENGTHS6):] = np.nan
    return x


def _example6():
    return dict(lengths=LENGTHS6, text_int=[torch.tensor(r, dtype=torch.int64) for r in REFS6])


def _check_mwer(x, loss, grad, lists, details, scale, ctc_weight):
    used = sum(LENGTHS6)
    flat = x.reshape(-1, V6).astype(np.float64)
    flat[used:] = 0.0
    first = [0, 40, 77]
    out = oracle.mwer(flat, first, LENGTHS6, REFS6, lists, BLANK6, SPACE6, scale=scale, ctc_weight=ctc_weight)
    _check_logp(details['logp'].cpu().numpy(), out['logp'])
    assert np.array_equal(details['cost'].cpu().numpy(), out['cost'])
    fin = np.isfinite(out['logp'])
    delta = 1e-5 * np.abs(out['logp'][fin]).max()
    sizes = [len(l) for l in lists]
    at = np.concatenate([[0], np.cumsum(sizes)])
    n_used = sum(1 for r in out['risk'] if r == r)
    slack, dvalue = np.zeros(len(out['logp'])), 0.0
    for u in range(len(lists)):
        sl = slice(at[u], at[u + 1])
        f = fin[sl]
        if f.any():
            C = np.abs(out['cost'][sl][f] - out['cost'][sl][f].mean()).max()
            slack[sl] = 2 * 4 * scale ** 2 * delta * out['post'][sl] * C / n_used + 1e-6 * np.abs(out['dlogp'][sl])
            dvalue += 2 * scale * delta * C / n_used
    assert abs(loss - out['loss']) <= 1e-6 * abs(out['loss']) + 2 * dvalue + 1e-7, (loss, out['loss'], dvalue)
    post = details['post'].cpu().numpy()
    assert (np.abs(post - out['post']) <= (np.expm1(2 * scale * delta) + 1e-6) * out['post'] + 1e-12).all()
    bar = out['bar'].copy()
    k = 0
    for f0, T, lst in zip(first, LENGTHS6, out['scored']):
        for logp, dlogp, occ in lst:
            bar[f0:f0 + T] += slack[k] * np.abs(dlogp)
            k += 1
    g = grad.reshape(-1, V6)
    assert (g[used:] == 0).all()
    _check_grad(g, out['grad'], bar, 'mwer_loss gradient')
    return out


LISTS6 = [[[0, 1, 4, 2, 3, 4, 1], [0, 1, 4, 2, 3], [0, 4, 2, 3, 4, 1], [1, 1, 4, 2, 4, 1]],
          [[2, 4, 0, 1], [2, 4, 0, 0, 1], [2, 0, 0, 1], []],
          [[3, 4, 3, 3], [3, 3], [4, 3], [0, 4, 3]]]


@pytest.mark.parametrize('ctc_weight', [0.0, 0.5])
def test_mwer_loss_with_given_lists(dev, ctc_weight):
    x = _pred6(6)
    pred = torch.from_numpy(x.copy()).to(dev).requires_grad_(True)
    nbest = [[(h, -1.0 * k) for k, h in enumerate(lst)] for lst in LISTS6]
    loss, details = rm.mwer_loss(pred, _example6(), space=SPACE6, blank=BLANK6, scale=0.8, ctc_weight=ctc_weight, nbest=nbest, return_details=True)
    loss.backward()
    assert [[h for h, _ in lst] for lst in details['nbest']] == LISTS6 and details['sizes'] == [4, 4, 4]
    _check_mwer(x, float(loss.detach()), pred.grad.cpu().numpy(), LISTS6, details, 0.8, ctc_weight)


def test_mwer_loss_adds_the_reference_once(dev):
    x = _pred6(7)
    pred = torch.from_numpy(x.copy()).to(dev).requires_grad_(True)
    nbest = [[(h, 0.0) for h in lst] for lst in LISTS6]
    loss, details = rm.mwer_loss(pred, _example6(), space=SPACE6, blank=BLANK6, ctc_weight=0.0, nbest=nbest, add_reference=True, return_details=True)
    loss.backward()
    lists = [[h for h, _ in lst] for lst in details['nbest']]
    assert lists == [LISTS6[0], LISTS6[1], LISTS6[2] + [REFS6[2]]] and details['sizes'] == [4, 4, 5]
    assert all(lst.count(ref) == 1 for lst, ref in zip(lists, REFS6))
    _check_mwer(x, float(loss.detach()), pred.grad.cpu().numpy(), lists, details, 1.0, 0.0)


def test_mwer_loss_decodes_its_own_lists(dev):
    x = _pred6(8, poison=False)
    pred = torch.from_numpy(x.copy()).to(dev).requires_grad_(True)
    loss, details = rm.mwer_loss(pred, _example6(), space=SPACE6, blank=BLANK6, beam_width=8, n_best=4, ctc_weight=0.0, return_details=True)
    loss.backward()
    lists = [[h for h, _ in lst] for lst in details['nbest']]
    assert all(1 <= len(lst) <= 4 for lst in lists) and sum(details['sizes']) == sum(len(lst) for lst in lists)
    _check_mwer(x, float(loss.detach()), pred.grad.cpu().numpy(), lists, details, 1.0, 0.0)
    logp = details['logp'].cpu().numpy()
    scores = np.asarray([s for lst in details['nbest'] for _, s in lst])
    assert (logp >= scores - 1e-4 * np.maximum(1.0, np.abs(scores))).all(), (logp, scores)           # a pruned sum cannot exceed the full one


def test_rescore_nbest_feeds_mbr_rerank(dev):
    x = _pred6(9, poison=False)
    pred = torch.from_numpy(x).to(dev)
    nbest = rm.beam_decode(pred, LENGTHS6, BLANK6, beam_width=8, n_best=4)
    exact = rm.rescore_nbest(pred, LENGTHS6, nbest, BLANK6)
    assert [[h for h, _ in lst] for lst in exact] == [[h for h, _ in lst] for lst in nbest]
    flat = x.reshape(-1, V6).astype(np.float64)
    scored = oracle.nbest_logp(flat, [0, 40, 77], LENGTHS6, [[h for h, _ in lst] for lst in nbest], BLANK6)
    _check_logp(np.asarray([s for lst in exact for _, s in lst]), [s[0] for lst in scored for s in lst])
    picks = rm.mbr_rerank(exact, space=SPACE6, device=dev)
    assert len(picks) == 3 and all(0 <= p < len(lst) and len(r) == len(lst) and np.isfinite(r).all() for (p, r), lst in zip(picks, exact))


# ---------------------------------------------------------------- 8. the trainer
@pytest.mark.gpu
def test_train_model_with_mwer(tiny_flags, monkeypatch):  # noqa: F811
    """train_model(mwer=) runs, changes the parameters and keeps them finite; then 12 FusedAdamW steps on mwer_loss(add_reference=True) of a fixed
    batch, lists fixed at step 0 through nbest=: the expected word errors sum_k post_k cost_k (from return_details) must not go up.  scale = 0.05:
    the log-likelihoods of an untrained model's hypotheses lie tens of nats apart over hundreds of frames, at scale 1 the posterior is one-hot and
    the figure cannot move.  Measured on an MI355X: 3.25 -> 0.014 after one step, 0.000 from the third on."""
    from silent_speech_amd.flags import FLAGS
    from silent_speech_amd.optim import FusedAdamW
    from silent_speech_amd.synthetic import SyntheticEMGDataset
    from silent_speech_amd.transduction_model import _pack_batch
    _lib.load()
    FLAGS.learning_rate, FLAGS.learning_rate_warmup = 2e-3, 4
    # the sampler drops the incomplete last batch of the 128 000-sample budget: 80 utterances of 300 .. 500 frames are two full batches and a rest
    train = SyntheticEMGDataset(80, seed=3, min_frames=300, max_frames=500)
    devset = SyntheticEMGDataset(4, seed=4, min_frames=40, max_frames=80)
    space = train.text_transform.chars.index(' ')
    calls, inner = [], rm.mwer_loss

    def counted(*a, **k):
        calls.append(k)
        return inner(*a, **k)
    monkeypatch.setattr(rm, 'mwer_loss', counted)
    model = rm.train_model(train, devset, 'cuda', n_epochs=1, max_steps=2, mwer=dict(space=space, n_best=4, beam_width=8))
    monkeypatch.undo()
    assert len(calls) == 2 and all(k['blank'] == 37 and k['n_best'] == 4 for k in calls)
    assert all(torch.isfinite(v.float()).all() for v in model.state_dict().values())
    batch = train.collate_raw(train.items[:4])
    opt = FusedAdamW(model, lr=2e-3, weight_decay=0.0)
    lists, errors = None, []
    before = model.w_out.weight.detach().clone()
    for it in range(12):
        opt.zero_grad()
        X, X_raw, sess = _pack_batch(batch, 'cuda')
        loss, details = rm.mwer_loss(model(X, X_raw, sess), batch, blank=37, space=space, n_best=4, beam_width=8, scale=0.05, add_reference=True, nbest=lists, return_details=True)
        lists = details['nbest'] if lists is None else lists
        loss.backward()
        opt.step()
        assert it or not torch.equal(before, model.w_out.weight.detach()), 'a step on mwer_loss changed no output weight'
        post, cost = details['post'].double().cpu().numpy(), details['cost'].double().cpu().numpy()
        errors.append(float((post * cost).sum()) / len(lists))
    print('largest posterior of the last step %.4f;' % float(post.max()), 'expected word errors per utterance over 12 steps:', ' '.join('%.4f' % e for e in errors))
    assert np.isfinite(errors).all() and errors[-1] <= errors[0] + 1e-6, errors
