"""The CTC loss kernels (csrc/ctc.hip) at the edges of their machinery, against the float64 recursion of oracle/ctc_ref.py.

A (utterance, direction) workgroup of ctc_alpha_beta_kernel is a pipeline of W <= 8 compute waves of 128 extended states (SP = 2 S + 1) plus a loader
wave; neighbouring waves talk through a 64-frame LDS ring and polled progress words, frames run in blocks of 8, the loader recycles four 32-frame chunk
buffers behind the slowest wave, and W comes from the longest target of the BATCH.  The cases below put S on both sides of every wave edge (SP = 127 /
129 / 131, 255 / 257 / 259, 385, 515, 1023), T on the block / chunk / ring / chunk-ring edges with more than one wave, idle waves next to busy ones,
empty utterances, class counts on both sides of the gradient kernel's 64-lane passes and at the LDS limit, a row stride above V and a class of
probability 0.  The emulator runs a workgroup's waves as cooperative fibres (no real concurrency): the index math and the protocol's logic are checked in
the CPU tier, its memory ordering and back-pressure only by the gpu tier of the same tests.

Bars (fixed in advance, no outliers): nll 1e-5 relative, loss 1e-5 relative, inf / NaN patterns exact, and per gradient element
    |got - want| <= 2e-3 (|want| + occ) + 1e-6,        occ = softmax / (max(S, 1) n) - want   (the oracle's occupancy term):
the kernel forms the occupancy as exp(m ln2 + nll - lp) in f32 with |nll| up to ~2e3, so its error scales with that term, which then cancels against the
softmax.  Frames of the packed buffer behind the last utterance (the rest of its row and one whole spare row) hold NaN and must get a gradient of exactly 0."""
import numpy as np
import pytest
import torch

from oracle.ctc_ref import ctc_loss_packed
from silent_speech_amd import recognition_model as rm
from tests.backend import dev  # noqa: F401


# ---------------------------------------------------------------- inputs and the reference
def _draw(rng, n, alphabet, repeats=None, p_repeat=None):
    """n labels from `alphabet`.  repeats = k: no two neighbours equal except exactly k pairs; p_repeat: a label repeats its predecessor with that probability."""
    alphabet = np.asarray(alphabet, dtype=np.int64)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    t = rng.choice(alphabet, n).astype(np.int64)
    if p_repeat is not None:
        for i in range(1, n):
            if rng.random() < p_repeat:
                t[i] = t[i - 1]
    if repeats is not None:
        same = set(int(i) for i in np.linspace(1, n - 1, repeats + 2)[1:-1].round()) if repeats else set()
        for i in range(1, n):
            t[i] = t[i - 1] if i in same else rng.choice(alphabet[alphabet != t[i - 1]])
        assert int((t[1:] == t[:-1]).sum()) == repeats
    return t


def _n_repeats(t):
    return int((t[1:] == t[:-1]).sum())


def _logits(rng, lengths, V, row, scale=1.5):
    """(rows, row, V) f32 packed frames with one whole spare row; everything behind the last utterance is NaN."""
    used = int(sum(lengths))
    rows = (used + row - 1) // row + 1
    x = (scale * rng.standard_normal((rows, row, V))).astype(np.float32)
    x.reshape(-1, V)[used:] = np.nan
    return x


def _reference(logits, lengths, text, blank):
    """Oracle on the frames in use (the poison replaced by 0): loss, d loss / d logits, nll, and softmax / (max(S, 1) n) per frame."""
    V = logits.shape[-1]
    used, n = int(sum(lengths)), len(lengths)
    clean = logits.astype(np.float64)
    clean.reshape(-1, V)[used:] = 0.0
    loss, d, nll = ctc_loss_packed(clean, lengths, text, blank, vec=True)
    flat = clean.reshape(-1, V)
    sm = np.exp(flat - flat.max(1, keepdims=True))
    sm /= sm.sum(1, keepdims=True)
    scale = np.zeros(flat.shape[0])
    off = 0
    for T, t in zip(lengths, text):
        scale[off:off + T] = 1.0 / (max(len(t), 1) * n)
        off += T
    return loss, d, nll, (sm * scale[:, None]).reshape(logits.shape)


def _run(dev, logits, lengths, text, blank, factor=2.0):
    x = torch.from_numpy(logits.copy()).to(dev).requires_grad_(True)
    loss, plan = rm.ctc_loss(x, dict(lengths=lengths, text_int=[torch.from_numpy(np.array(t, dtype=np.int64)) for t in text]), blank=blank, return_plan=True)
    (factor * loss).backward()
    return float(loss.detach()), x.grad.cpu().numpy(), plan.nll.cpu().numpy()


def _compare(name, got, want, used, factor=2.0, zero_cols=()):
    """The bars of the module docstring.  got = (loss, factor * dlogits, nll) of the kernels, want = _reference(...); the columns in zero_cols are
    compared with 0 instead of the oracle."""
    loss, d, nll = got
    want_loss, want_d, want_nll, sm = want
    V = d.shape[-1]
    inf = np.isposinf(want_nll)
    assert np.isfinite(want_nll[~inf]).all()
    assert np.array_equal(np.isposinf(nll), inf) and np.isfinite(nll[~inf]).all(), (name, nll, want_nll)
    nll_err = float(np.max(np.abs(nll[~inf] - want_nll[~inf]) / np.maximum(np.abs(want_nll[~inf]), 1e-300))) if (~inf).any() else 0.0
    want_d, sm = want_d.copy(), sm.copy()
    for c in zero_cols:
        want_d[..., c] = 0.0
        sm[..., c] = 0.0
    nan = np.isnan(want_d)
    occ = np.abs(sm - want_d)
    err = np.abs(d - factor * want_d)
    bar = 2e-3 * factor * (np.abs(want_d) + occ) + 1e-6
    fin = ~nan & ~np.isnan(d)
    use = float(np.max(err[fin] / bar[fin])) if fin.any() else 0.0
    at = tuple(int(i) for i in np.unravel_index(np.argmax(np.where(fin, err / bar, -1.0)), d.shape))
    print('ctc_edges %-28s nll rel err %.2e  |nll| max %.1f  grad err max %.2e  worst err / bar %.3f at %s (want %.3e, occ %.3e)'
          % (name, nll_err, float(np.max(np.abs(want_nll[~inf]))) if (~inf).any() else 0.0, float(err[fin].max()) if fin.any() else 0.0, use, at,
             factor * want_d[at], factor * occ[at]))
    np.testing.assert_allclose(nll[~inf], want_nll[~inf], rtol=1e-5)
    if inf.any():
        assert loss == np.inf and want_loss == np.inf
    else:
        assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (name, loss, want_loss)
    assert np.array_equal(np.isnan(d), nan), (name, 'NaN pattern')
    assert (err[fin] <= bar[fin]).all(), (name, use, at)
    assert not d.reshape(-1, V)[used:].any(), (name, 'gradient behind the last utterance')


_REF = {}


def _case(name, build):
    """Inputs and oracle of a case, made once and shared by the backends (read-only)."""
    if name not in _REF:
        logits, lengths, text, blank = build()
        want = _reference(logits, lengths, text, blank)
        for a in (logits,) + tuple(text) + tuple(w for w in want if isinstance(w, np.ndarray)):
            a.setflags(write=False)
        _REF[name] = (logits, lengths, text, blank, want)
    return _REF[name]


def _check(dev, name, build):
    logits, lengths, text, blank, want = _case(name, build)
    _compare(name, _run(dev, logits, lengths, text, blank), want, int(sum(lengths)))
    return want


def _random_batch(seed, lengths, tlens, V, blank, row, scale=1.5, repeats=None):
    def build():
        rng = np.random.default_rng(seed)
        alphabet = [c for c in range(V) if c != blank]
        text = [_draw(rng, n, alphabet, repeats=repeats[i] if repeats else None) for i, n in enumerate(tlens)]
        return _logits(rng, lengths, V, row, scale), list(lengths), text, blank
    return build


# ---------------------------------------------------------------- g. class counts (one compute wave)
def _v_max(W):
    """The largest V ss_ctc_loss's LDS check accepts: 4 bytes x (4 chunk buffers x 32 frames x V + W x 64 ring + W + 1 progress words + W x 72 dump) <= 160 KiB."""
    return (160 * 1024 // 4 - (W * 64 + W + 1 + W * 72)) // (4 * 32)


# (V, blank, scale): both sides of the gradient kernel's 64-lane passes and of two of them; blank first, in the middle, last; V = 70 peaky
_CLASS_COUNTS = [(1, 0, 1.5), (2, 0, 1.5), (2, 1, 1.5), (64, 0, 1.5), (64, 63, 1.5), (65, 32, 1.5), (65, 64, 1.5), (70, 35, 6.0), (129, 0, 1.5), (129, 128, 1.5)]


@pytest.mark.parametrize('V,blank,scale', _CLASS_COUNTS)
def test_ctc_class_counts(dev, V, blank, scale):
    tlens = [0, 0, 0] if V == 1 else [5, 11, 0]                           # V = 2: one label class, 10 repeated neighbours, 21 <= 23 frames
    _check(dev, 'g V=%d blank=%d' % (V, blank), _random_batch(100 + V + blank, [40, 23, 9], tlens, V, blank, 24, scale))


def test_ctc_largest_class_count_and_one_more(dev):
    V = _v_max(1)
    assert V == 318
    _check(dev, 'g V=%d (LDS limit)' % V, _random_batch(7, [40], [5], V, V // 2, 48))
    x = torch.zeros(1, 48, V + 1, device=dev)
    with pytest.raises(RuntimeError, match='LDS'):
        rm.ctc_loss(x, dict(lengths=[40], text_int=[torch.ones(5, dtype=torch.long)]), blank=0)


# ---------------------------------------------------------------- h. row stride above the class count
def test_ctc_row_stride_above_class_count(dev):
    V, ld, blank, M = 38, 48, 37, 120
    lengths, tlens = [70, 33, 9], [66, 10, 2]                             # two compute waves; 8 frames of padding
    rng = np.random.default_rng(8)
    text = [_draw(rng, n, range(V - 1)) for n in tlens]
    data = (1.5 * rng.standard_normal((M, V))).astype(np.float32)
    data[sum(lengths):] = np.nan
    wide = np.full((M, ld), np.nan, dtype=np.float32)
    wide[:, :V] = data
    plan = rm._CtcPlan(lengths, [torch.from_numpy(t) for t in text], M, dev)
    out = []
    for buf in (data, wide):
        loss, d, nll, _ = torch.ops.silent_speech.ctc_loss(torch.from_numpy(buf).to(dev), plan.desc, plan.targets, plan.n, plan.max_s, plan.ws_floats, V, blank)
        out.append((loss.cpu().numpy(), d.cpu().numpy(), nll.cpu().numpy()))
    (loss0, d0, nll0), (loss1, d1, nll1) = out
    assert d1.shape == (M, ld) and not d1[:, V:].any()                   # exactly 0 (and no NaN) in the columns that are no class
    assert np.array_equal(d1[:, :V], d0, equal_nan=True) and np.array_equal(nll1, nll0) and np.array_equal(loss1, loss0)
    want = _reference(data[None], lengths, text, blank)
    _compare('h ld=48 V=38', (float(loss1[0]), d1[None, :, :V], nll1[:len(lengths)]), want, sum(lengths), factor=1.0)


# ---------------------------------------------------------------- i. utterances without frames
@pytest.mark.parametrize('with_labels', [False, True])
def test_ctc_empty_utterances(dev, with_labels):
    """T = 0 at the start, in the middle and at the end of a batch.  The kernel's contract: nll = 0 without labels, +inf with labels (no alignment of
    no frames emits a label); the oracle is asked about the other utterances only."""
    V, blank, row = 11, 4, 50
    lengths, tlens = [0, 20, 0, 150, 0], ([3, 4, 0, 66, 2] if with_labels else [0, 4, 0, 66, 0])
    rng = np.random.default_rng(9)
    logits = _logits(rng, lengths, V, row)
    text = [_draw(rng, n, [c for c in range(V) if c != blank]) for n in tlens]
    keep = [i for i, T in enumerate(lengths) if T > 0]
    sub_l, sub_t = [lengths[i] for i in keep], [text[i] for i in keep]
    loss, d, nll = _run(dev, logits, lengths, text, blank)
    sub_loss, sub_d, sub_nll = _run(dev, logits, sub_l, sub_t, blank)
    assert [float(nll[i]) for i in range(5) if i not in keep] == [np.inf if tlens[i] else 0.0 for i in range(5) if i not in keep]
    assert np.array_equal(nll[keep], sub_nll)                             # the neighbours: the same numbers, the gradient rescaled from 1/2 to 1/5
    np.testing.assert_allclose(d * (len(lengths) / len(keep)), sub_d, rtol=1e-6, atol=0)
    w_loss, w_d, w_nll, w_sm = _reference(logits, sub_l, sub_t, blank)
    r = len(keep) / len(lengths)
    want = (np.inf if with_labels else r * w_loss, r * w_d, np.array([np.inf if tlens[i] else 0.0 for i in range(5)]), r * w_sm)
    want[2][keep] = w_nll
    _compare('i empty with_labels=%d' % with_labels, (loss, d, nll), want, sum(lengths))


# ---------------------------------------------------------------- j. a class of probability 0
def test_ctc_class_at_minus_inf(dev):
    """Logit -inf in every frame for a class that is in no target.  Its gradient is softmax - occupancy = 0 - 0; the oracle (and ATen) form the
    occupancy as exp(-inf + nll - (-inf)) = NaN there, so that column is compared with the limit 0, everything else with the oracle."""
    V, blank, dead = 11, 4, 7
    lengths, tlens = [150, 30], [66, 7]

    def build():
        rng = np.random.default_rng(10)
        logits = _logits(rng, lengths, V, 48)
        logits[..., dead] = -np.inf
        return logits, lengths, [_draw(rng, n, [c for c in range(V) if c not in (blank, dead)]) for n in tlens], blank
    logits, _, text, _, want = _case('j', build)
    used = sum(lengths)
    assert np.isnan(want[1].reshape(-1, V)[:used, dead]).all() and np.isfinite(np.delete(want[1], dead, -1)).all() and np.isfinite(want[2]).all()
    got = _run(dev, logits, lengths, text, blank)
    assert not got[1][..., dead].any()                                    # exactly 0, padding included
    _compare('j class at -inf', got, want, used, zero_cols=(dead,))


# ---------------------------------------------------------------- c. time edges with two waves
def test_ctc_time_edges_two_waves(dev):
    """S = 70 (SP = 141: two waves) at T = 71 (one repeated neighbour: the only alignment has no frame to spare), 72, 96 / 97 (a chunk), 128 / 129 (the
    chunk ring, two laps of the wave ring); next to them T = 1 without labels, T = 8 (one block) and T = 33."""
    V, blank = 11, 4
    lengths, tlens = [71, 72, 96, 97, 128, 129, 1, 8, 33], [70] * 6 + [0, 1, 16]

    def build():
        rng = np.random.default_rng(12)
        alphabet = [c for c in range(V) if c != blank]
        text = [_draw(rng, 70, alphabet, repeats=1)] + [_draw(rng, 70, alphabet, repeats=k) for k in (1, 5, 9, 12, 7)] + [_draw(rng, n, alphabet) for n in (0, 1, 16)]
        return _logits(rng, lengths, V, 100), lengths, text, blank
    want = _check(dev, 'c time edges', build)
    text = _REF['c time edges'][2]
    assert lengths[0] == tlens[0] + _n_repeats(text[0]) and np.isfinite(want[2]).all()         # feasible, T = 71 with nothing to spare


# ---------------------------------------------------------------- a, b. wave edges
def test_ctc_wave_edge_mixed_batch(dev):
    """SP = 129 (the last wave owns one blank state, nll takes alpha_T(SP - 2) from the ring), 127 and 131 either side of the edge, a 7-state utterance
    whose second wave is idle, and an utterance without labels -- in one batch, so W = 2 for all of them."""
    want = _check(dev, 'a wave edge, mixed', _random_batch(13, [140, 70, 131, 9, 140], [64, 63, 65, 3, 0], 11, 4, 100, repeats=[None, 4, None, None, None]))
    assert np.isfinite(want[2]).all()                                     # 63 labels with 4 repeated neighbours fit 70 frames: every edge is checked on finite numbers


def test_ctc_second_wave_edge(dev):
    """SP = 257 (ring nll path of the third wave), 255 and 259 either side of it."""
    want = _check(dev, 'b second wave edge', _random_batch(14, [300, 257, 260], [128, 127, 129], 11, 4, 100))
    assert np.isfinite(want[2]).all()


# ---------------------------------------------------------------- f. no alignment, in two waves
def test_ctc_infeasible_in_two_waves(dev):
    """One 64-label string over two symbols with many repeated neighbours: 100 frames cannot hold it, 140 can."""
    V, blank = 11, 4
    lengths = [100, 140]

    def build():
        rng = np.random.default_rng(15)
        t = _draw(rng, 64, [2, 9], p_repeat=0.6)
        return _logits(rng, lengths, V, 100), lengths, [t, t.copy()], blank
    want = _check(dev, 'f infeasible', build)
    t = _REF['f infeasible'][2][0]
    assert 100 < 64 + _n_repeats(t) <= 140
    assert np.array_equal(np.isposinf(want[2]), [True, False])
    assert np.isnan(want[1].reshape(-1, V)[:100]).all() and np.isfinite(want[1].reshape(-1, V)[100:240]).all()


# ---------------------------------------------------------------- e. four and five waves
@pytest.mark.parametrize('S', [192, 257])
def test_ctc_four_and_five_waves(dev, S):
    """S = 192: SP = 385, four waves, the last owns one blank state (ring nll path); S = 257: SP = 515, five waves.  T three frames above the shortest
    feasible length, and 64 frames (one lap of the wave ring) more."""
    V, blank = 11, 4

    def build():
        rng = np.random.default_rng(16 + S)
        alphabet = [c for c in range(V) if c != blank]
        text = [_draw(rng, S, alphabet), _draw(rng, S, alphabet)]
        lengths = []
        for t in text:
            lengths.append(S + _n_repeats(t) + 3 + 64 * len(lengths))
        return _logits(rng, lengths, V, 200), lengths, text, blank
    want = _check(dev, 'e S=%d' % S, build)
    assert np.isfinite(want[2]).all()


# ---------------------------------------------------------------- d. all eight waves
def test_ctc_eight_waves(dev):
    """S = 511, the longest accepted target: SP = 1023, eight compute waves, 600 frames = nine laps of the wave ring; next to a 30-frame utterance
    that keeps seven of the waves idle."""
    want = _check(dev, 'd eight waves', _random_batch(17, [600, 30], [511, 5], 40, 39, 200))
    assert np.isfinite(want[2]).all()


def test_ctc_one_label_too_many_raises(dev):
    x = torch.zeros(2, 200, 40, device=dev)
    with pytest.raises(RuntimeError, match='511-label limit'):
        rm.ctc_loss(x, dict(lengths=[400], text_int=[torch.zeros(512, dtype=torch.long)]), blank=39)
