"""The ALIGNMENT of the fused DTW loss path at its strip, step and chunk edges, bit for bit against the C oracle.

Every training step with a silent utterance runs silent_cost_skewed_kernel (csrc/loss.hip: the cost matrix written straight into the DTW kernel's skewed
strip layout) -> dtw_kernel<false> (csrc/dtw.hip, ss_dtw_align_skewed: sweep + backtrace) -> silent_loss_kernel.  tests/test_dtw.py drives the OTHER
instantiation (ss_dtw_align), the loss tests see this path through one scalar and the gradients, and a DTW path that is slightly off still has nearly the
optimal cost.  Here the inputs make every cost exactly representable (tests/dtw_loss_oracle.py), so `plan.results` of every silent utterance must EQUAL
the oracle alignment and `correct` the oracle's count, lambda != 0 included; the cases marked (+) also compare the loss (2e-5 relative, the suite's bar)
and d loss / d head (assert_close_robust 1e-4, no outliers) with a float64 recomputation and the DeviceConfusion matrix exactly.

T1 = predicted frames = DTW columns = steps (ts = T1 + 62), T2 = target frames = DTW rows; one lane owns 4 rows, a wave 256, a strip 1024; a super-step is
64 steps, the cost kernel's chunk 16 steps, the backtrace window 2048 steps.  pred / aux are column slices of ONE head matrix (the form _fused_head takes
as it is) whose spare columns and spare rows hold NaN: they must influence nothing and get a gradient of exactly 0.

Tiers: the emulator runs the generic mel widths (4 / 84 / 128; 4 on the large shapes) and two tiny cases at the model's width 80, whose quad-shared branch
is slow there; the GPU runs every case at width 80 and at one generic width, plus the 3-strip and the > 4096-work-item cases.  The emulator runs a
workgroup's waves without real concurrency: it checks index math and tie order; the LDS ring hand-off, the hand-counted waits and the boundary row's
visibility are checked only by the gpu tier of the same tests."""
import numpy as np
import pytest
import torch

from silent_speech_amd import _lib, transduction_model as tm
from tests import dtw_loss_oracle as oracle
from tests.backend import dev, is_emu  # noqa: F401
from tests.dtw_loss_oracle import Utt
from tests.util import assert_close_robust

LAMS = (0.25, 0.0, 0.5)
GENERIC = (84, 128, 4)


def _lam(T1, T2, kind):
    """The loss weight of a table case: rotates through 0.25 / 0 / 0.5; 0 where the path has no choice (one interior row or column)."""
    if min(T1, T2) <= 2:
        return 0.0
    return LAMS[(T1 + T2 + (kind == 'ints')) % 3]


def _widths(dev, T1, T2):
    """Mel widths of a table case on this tier."""
    generic = GENERIC[(T1 + T2) % 3]
    if is_emu(dev):
        return (4,) if T1 * T2 > 20000 else (generic,)
    return (80, generic)


def _run(dev, b, full=False):
    """One _dtw_loss_plan call on the batch; alignment and count always, loss / gradient / confusion matrix with full=True."""
    head = torch.from_numpy(b.head.copy()).to(dev)
    if full:
        head.requires_grad_(True)
    pred = head[:, :b.n_mel].unsqueeze(0)
    aux = head[:, b.n_mel:b.n_mel + b.n_ph].unsqueeze(0)
    assert tm._fused_head(pred, aux, b.rows, b.n_mel, b.n_ph) is head                # used as it is: no copy without the poison
    ex = dict(lengths=[u.T1 for u in b.utts], silent=[u.silent for u in b.utts],
              audio_features=[torch.from_numpy(a).to(dev) for a in b.audio], phonemes=[torch.from_numpy(p).to(dev) for p in b.phones])
    loss, correct, plan = tm._dtw_loss_plan(pred, aux, ex, b.lam)
    tag = 'n_mel %d lam %g' % (b.n_mel, b.lam)
    res = plan.results.cpu().numpy() if plan.results is not None else None
    for i, (u, row) in enumerate(zip(b.utts, plan.utt_host)):
        if not u.silent:
            continue
        off = int(row[5])
        got, want = res[off:off + u.T2], b.align[i]
        if not np.array_equal(got, want):
            k = int(np.flatnonzero(got != want)[0])
            raise AssertionError('%s, utterance %d (T1 %d, T2 %d, %s): %d of %d rows differ, first at k = %d: got %d, want %d'
                                 % (tag, i, u.T1, u.T2, u.kind, int((got != want).sum()), u.T2, k, int(got[k]), int(want[k])))
    assert int(correct.cpu()[0]) == b.correct, tag
    if full:
        got_loss = float(loss.detach().cpu())
        print('%s: loss %.9g (float64 %.9g)' % (tag, got_loss, b.loss))
        assert abs(got_loss - b.loss) <= 2e-5 * abs(b.loss), tag                      # (the ramp's loss is exactly 0 on both sides)
        loss.backward()
        g = head.grad.cpu().numpy()
        live = b.n_mel + b.n_ph
        assert_close_robust(g[:b.used, :live], b.dhead[:b.used, :live], 1e-4, name='dhead (%s)' % tag, max_outlier_frac=0)
        assert not g[b.used:].any() and not g[:, live:].any(), tag                   # poisoned rows and columns: exactly 0
        dc = tm.DeviceConfusion(b.n_ph, dev)
        dc.add(plan)
        assert np.array_equal(dc.numpy(), b.confusion), tag
    return plan


def _table_case(dev, T1, T2, kind, seed, full=False):
    for n_mel in _widths(dev, T1, T2):
        _run(dev, oracle.build([Utt(T1, T2, kind=kind)], n_mel, _lam(T1, T2, kind), seed), full)


KINDS = ('ties', 'ints')
ROWS = [(T1, T2) for T2 in (2, 5, 6, 257, 258, 1025, 1026) for T1 in (3, 40)]
STEPS = [(T1, T2) for T1 in (2, 3, 18, 19, 66, 67) for T2 in (5, 300)]
MULTI = [(T1, T2) for T2 in (1026, 1030) for T1 in (9, 67, 300)]


def test_the_case_table_uses_the_phoneme_term():
    cases = [(T1, T2, k) for T1, T2 in ROWS + STEPS + MULTI for k in KINDS]
    assert 3 * sum(_lam(*c) != 0 for c in cases) >= len(cases)


# ---------------------------------------------------------------- the log-sum-exp the costs rest on, by itself
def test_frame_lse_is_exact_on_the_constructed_logits(dev):
    """ss_frame_lse directly: lse == g_q bit for bit (expf(<= -64) vanishes in the f32 sum, logf(1.0f) == 0) and arg-max == the one class at g_q, at 6
    classes and at 70 (a second pass of the 64 lanes), 11 rows (three workgroups), a column offset and NaN in the spare columns; on rows where two or
    three classes tie at the maximum the arg-max is the FIRST of them."""
    rng = np.random.default_rng(7)
    for ncls, col0 in ((6, 4), (70, 8)):
        rows, ld = 11, col0 + ncls + 5
        head = np.full((rows, ld), np.nan, dtype=np.float32)
        g = rng.integers(0, 4, rows)
        g[:4] = (0, 1, 2, 3)
        a = g[:, None] - 64 * rng.integers(1, 4, (rows, ncls))
        hot = rng.integers(0, ncls, rows)
        hot[:3] = (0, ncls - 1, min(64, ncls - 1))
        a[np.arange(rows), hot] = g
        tie = np.zeros(rows, dtype=bool)
        tie[-3:] = True
        first = hot.copy()
        for r, cols in zip(range(rows - 3, rows), ((1, ncls - 1), (ncls - 2, ncls - 1), (3, 2, 5))):
            a[r] = g[r] - 64
            a[r, list(cols)] = g[r]
            first[r] = min(cols)
        head[:, col0:col0 + ncls] = a
        h = torch.from_numpy(head).to(dev)
        lse = torch.empty(rows, dtype=torch.float32, device=dev)
        amax = torch.empty(rows, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().ss_frame_lse(_lib.ptr(h), ld, col0, ncls, rows, _lib.ptr(lse), _lib.ptr(amax), _lib.stream_of(h)), 'ss_frame_lse')
        lse, amax = lse.cpu().numpy(), amax.cpu().numpy()
        assert np.array_equal(oracle.lse_f32(a[~tie]), g[~tie].astype(np.float32))
        assert np.array_equal(lse[~tie], g[~tie].astype(np.float32)), (ncls, lse, g)
        assert np.array_equal(amax, first), (ncls, amax, first)
        ntie = np.array([2, 2, 3])
        assert np.abs(lse[tie] - (g[tie] + np.log(ntie))).max() < 1e-6


# ---------------------------------------------------------------- one matrix per call: the table of the module's docstring
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('T1,T2', ROWS)
def test_rows_per_lane_wave_and_strip(dev, T1, T2, kind):
    """T2 = 2 (one row), 5 / 6 (the last row of lane 0 / the first of lane 1), 257 / 258 (wave 0 / wave 1), 1025 / 1026 (one strip / the first row of a second)."""
    _table_case(dev, T1, T2, kind, 100)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('T1,T2', STEPS)
def test_super_step_and_cost_chunk_edges(dev, T1, T2, kind):
    """ts = 64 / 65 / 128 / 129: exactly one and two fast super-steps of dtw_kernel<false>, and each with a generic tail of one step; ts = 64 / 65 / 80 / 81:
    whole 16-step chunks of silent_cost_skewed_kernel, and a last chunk of one step.  One wave (T2 = 5) and two (T2 = 300: the LDS ring hand-off)."""
    _table_case(dev, T1, T2, kind, 200)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('T1,T2', MULTI)
def test_multi_strip_sweep(dev, T1, T2, kind):
    """Two strips: the boundary row goes through HBM (both parities of `bnd` are written or read), every super-step takes the generic path, with fewer
    steps than a super-step, just over two and several."""
    _table_case(dev, T1, T2, kind, 400)


@pytest.mark.gpu
def test_third_strip():
    """T2 = 2050: a third strip reads the boundary row the second wrote into the buffer the first strip used."""
    _lib.load()
    for kind in KINDS:
        _table_case(torch.device('cuda'), 40, 2050, kind, 500)


@pytest.mark.gpu
def test_more_work_items_than_the_grid_cap():
    """T2 = 1026, T1 = 8200: 8 wave strips x 517 chunks > 4096 workgroups, so silent_cost_skewed_kernel's `wk += gridDim.x` loop runs."""
    _lib.load()
    _table_case(torch.device('cuda'), 8200, 1026, 'ints', 600)


# ---------------------------------------------------------------- the backtrace
@pytest.mark.parametrize('kind', ('ramp', 'const'))
def test_backtrace_across_wave_strip_and_strip_rows(dev, kind):                      # (+)
    """T1 = T2 = 1030: a ramp whose only zero-cost path is the diagonal, and an all-ties matrix (constant features); the walk crosses every lane column,
    the three wave-strip rows and the strip row, restaging its window each time."""
    for n_mel in _widths(dev, 1030, 1030):
        b = oracle.build([Utt(1030, 1030, kind=kind)], n_mel, 0.0, 700)
        if kind == 'ramp':
            assert np.array_equal(b.align[0], np.arange(1030))
        _run(dev, b, full=True)


@pytest.mark.parametrize('T1', (1986, 1987, 2110))
def test_backtrace_window_of_2048_steps(dev, T1):
    """T2 = 6, a ramp then a plateau in the predictions: the path runs left along the last row.  ts = 2048 fills the window exactly, 2049 needs a
    second one, and at T1 = 2110 the horizontal run alone is longer than a window."""
    for n_mel in _widths(dev, T1, 6):
        b = oracle.build([Utt(T1, 6, kind='plateau_pred')], n_mel, 0.0, 800)
        assert b.align[0][5] == 5
        if T1 >= 2110:
            assert T1 - 1 - b.align[0][5] > 2048
        _run(dev, b)


def test_many_targets_aligned_to_one_prediction(dev):                                # (+)
    """The mirror, a plateau in the targets (T2 = 1987, T1 = 6): almost two thousand k align to the last q -- the atomic accumulation of silent_loss_kernel."""
    for n_mel in _widths(dev, 6, 1987):
        b = oracle.build([Utt(6, 1987, kind='plateau_tgt')], n_mel, 0.0, 900)
        assert int((b.align[0] == 5).sum()) == 1987 - 5
        _run(dev, b, full=True)


# ---------------------------------------------------------------- mel widths and one mixed batch
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n_mel', (4, 84, 128))
def test_generic_mel_widths(dev, n_mel, kind):
    """The generic branch of the cost kernel at one, 21 and all 32 register quads of the target row; two wave strips, a chunk of two steps."""
    _run(dev, oracle.build([Utt(20, 300, kind=kind)], n_mel, 0.5, 1000), full=True)


@pytest.mark.parametrize('T1,T2,kind', [(3, 6, 'ints'), (19, 6, 'ties')])
def test_quad_shared_width_80_tiny(dev, T1, T2, kind):
    """The model's 80 mel bins (the quad-shared branch) at the two shapes the emulator tier affords; the seed is one at which both the phoneme term and an
    lse taken from the neighbouring frame change the oracle's path."""
    _run(dev, oracle.build([Utt(T1, T2, kind=kind)], 80, 0.25, 1100, need_lse_effect=True), full=True)


def _mixed_batch():
    return [Utt(7, silent=False), Utt(5, 1), Utt(1, 4), Utt(1987, 6, kind='plateau_pred'), Utt(33, silent=False, kind='ties'), Utt(40, 258),
            Utt(9, 1026, kind='ties')]


def test_mixed_batch(dev):                                                           # (+)
    """Voiced utterances, a 1 x M and an N x 1 matrix (no interior cell: results stay 0), the widest matrix (T1 = 1987, T2 = 6), a 1-strip and the tallest,
    a 2-strip matrix (T1 = 9, T2 = 1026) in ONE call: every matrix sees a grid larger than its own work and non-zero p0 / y0 / res_off; with T2 >> T1 more
    than a hundred targets share a predicted frame's phoneme gradient."""
    for n_mel in ((4,) if is_emu(dev) else (80, 84)):
        b = oracle.build(_mixed_batch(), n_mel, 0.5, 1200)
        assert not b.align[1].any() and not b.align[2].any()
        _run(dev, b, full=True)


# ---------------------------------------------------------------- argument errors through the Python entry
def test_mel_width_errors(dev):
    b = oracle.build([Utt(3, 5)], 132, 0.0, 1300)
    with pytest.raises(RuntimeError, match='at most 128 mel bins'):
        _run(dev, b)
    head = torch.zeros(8, 24, device=dev)
    ex = dict(lengths=[3], silent=[True], audio_features=[torch.zeros(5, 6, device=dev)], phonemes=[torch.zeros(5, dtype=torch.int64, device=dev)])
    with pytest.raises(ValueError, match='multiple of 4'):
        tm._dtw_loss_plan(head[:, :6].unsqueeze(0), head[:, 6:12].unsqueeze(0), ex, 0.0)
