"""Non-stationary spectral gating (csrc/spectral_gate_ns.hip: data_utils.reduce_noise_nonstationary / reduce_noise_nonstationary_batch /
clean_session(gate='nonstationary'), the loader's noise_gate) against the float64 restatement tests/spectral_gate_ns_oracle.py, on the emulator tier and
on the MI355X.  Every tolerance is derived in the oracle's docstring from operation counts, the f32 format and interval arithmetic; none is fitted."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.signal
import torch

from silent_speech_amd import _lib, data_utils as D
from tests import spectral_gate_ns_oracle as O
from tests.backend import dev, is_emu  # noqa: F401

LENGTHS = [1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1279, 1280, 1281, 2304, 22050]
NONE = dict(freq_mask_smooth_hz=None, time_mask_smooth_ms=None)
LIMITS = dict(freq_mask_smooth_hz=1400, time_mask_smooth_ms=100)       # (n_f, n_t) = (32, 8) at 22 050 Hz


@functools.lru_cache(maxsize=None)
def _signal(L, sr=22050, seed=3):
    """a chirp (300 -> 3000 Hz, amplitude 0.3) switched on for the middle half of the signal, over noise of 0.01 RMS; f32 (the generator of
    tests/test_spectral_gate.py)"""
    rng = np.random.default_rng(seed + L)
    t = np.arange(L) / sr
    on = (np.arange(L) >= L // 4) & (np.arange(L) < L - L // 4)
    x = 0.3 * np.sin(2 * np.pi * (300 * t + 0.5 * 2700 * t * t / max(L / sr, 1e-3))) * on + 0.01 * rng.standard_normal(L)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(L, sr=22050, tc=2.0):
    """(X, m0, dm0) of the oracle for _signal(L, sr), computed once and shared"""
    ref = O.mask0_bound(_signal(L, sr), O.coefficient(sr, tc))
    for a in ref:
        a.setflags(write=False)
    return ref


def _gate(x, sr, dev, **kw):
    out, lens, mask = D.reduce_noise_nonstationary_batch([x], sr, return_mask=True, **kw)
    F = O.n_frames(len(x))
    assert lens == [len(x)] and tuple(out.shape) == (len(x),) and out.dtype == torch.float32 and tuple(mask.shape) == (F, 513) and mask.dtype == torch.float32
    return out.cpu().numpy().astype(np.float64), mask.cpu().numpy().astype(np.float64).T


# ------------------------------------------------------------------------------------------------ 1. the oracle itself (CPU only)
@pytest.mark.parametrize('F', [1, 2, 3, 40])
def test_oracle_level_is_scipy_filtfilt(F):
    A = np.abs(np.random.default_rng(F).standard_normal((5, F)))
    for sr in (16000, 22050):
        b = O.coefficient(sr)
        want = scipy.signal.filtfilt([b], [1, b - 1], A, axis=-1, padtype=None)
        assert np.abs(O.level(A, b) - want).max() <= 1e-13


def test_oracle_pieces():
    for t, sr in ((125.0, 16000), (172.265625, 22050)):
        b = O.coefficient(sr)
        assert abs(b - (np.sqrt(1 + 4 * t * t) - 1) / (2 * t * t)) <= 1e-18 and abs(t * t * b * b + b - 1) <= 1e-12      # b solves t^2 b^2 + b - 1 = 0
        assert b == D.nonstationary_coefficient(sr)
    assert abs(O.coefficient(16000) - 0.0079681) < 5e-8 and abs(O.coefficient(22050) - 0.0057882) < 5e-8
    assert O.coefficient(22050, 0.05) == D.nonstationary_coefficient(22050, 0.05)
    A = np.full((3, 9), 0.25)
    S = O.level(A, O.coefficient(22050))
    assert np.abs(S - 0.25).max() <= 1e-15                              # a constant row is its own level: r = 0
    assert np.abs(O.sigmoid_mask(A, S, 2.0, 10.0) - 1 / (1 + np.exp(20.0))).max() <= 1e-15
    assert np.abs(O.sigmoid_mask(A, S, 1.5, 4.0) - 1 / (1 + np.exp(6.0))).max() <= 1e-15
    z = np.zeros((2, 4))
    assert np.array_equal(O.sigmoid_mask(z, O.level(z, 0.01)), np.full((2, 4), 1 / (1 + np.exp(20.0))))                   # digital silence: finite


@pytest.mark.parametrize('L', [1, 257, 2304, 22050])
def test_oracle_returns_the_signal_with_p_zero(L):
    x = _signal(L).astype(np.float64)
    out, det = O.reduce_noise(x, O.coefficient(22050), n_f=11, n_t=4, p=0.0, details=True)
    assert np.array_equal(det['mask'], np.ones_like(det['mask'])) and (np.abs(out - x) <= det['bound']).all()


@pytest.mark.parametrize('sr', [22050, 16000])
@pytest.mark.parametrize('L', [2304, 22050])
def test_the_bounds_discriminate(L, sr):
    """The interval bound on m0 is loose (up to 1.9e-2); it still rejects every one of these wrong restatements in at least one entry, while the right
    one lies inside by construction: the tolerance of tests 2 and 3 cannot hide the errors a kernel of this shape can make."""
    x = _signal(L, sr)
    X, m0, dm0 = _reference(L, sr)
    A, b = np.abs(X), O.coefficient(sr)
    S = O.level(A, b)
    assert (np.abs(O.sigmoid_mask(A, S) - m0) <= dm0).all()
    wrong = {'forward pass only': O.sigmoid_mask(A, O.forward(A, b)),
             'b of the other rate': O.sigmoid_mask(A, O.level(A, O.coefficient(16000 if sr == 22050 else 22050))),
             'S one frame late': O.sigmoid_mask(A, np.roll(S, 1, axis=1))}
    for name, m in wrong.items():
        assert (np.abs(m - m0) > dm0).any(), name
    n_f, n_t = O.smoothing(sr)
    _, det = O.reduce_noise(x, b, n_f=n_f, n_t=n_t, p=0.5, details=True)
    assert (np.abs(O.final_mask(m0, n_f, n_t, 0.5) - det['mask']) <= det['dmask']).all()
    assert (np.abs(O.final_mask(m0, n_f, n_t, 0.5, p_first=True) - det['mask']) > det['dmask']).any()                      # p before the smoothing


# ------------------------------------------------------------------------------------------------ 2. the mask stage
@pytest.mark.parametrize('tc', [2.0, 0.05])
@pytest.mark.parametrize('sr', [22050, 16000])
@pytest.mark.parametrize('L', LENGTHS)
def test_mask(dev, L, sr, tc):
    _, m0, dm0 = _reference(L, sr, tc)
    got = _gate(_signal(L, sr), sr, dev, time_constant_s=tc)[1]
    err = np.abs(got - m0)
    print('L %d sr %d tc %g: max err %.3g, bound max %.3g, share of bound > 1e-4: %.4f' % (L, sr, tc, err.max(), dm0.max(), (dm0 > 1e-4).mean()))
    assert (err <= dm0).all()
    if L == 22050:
        assert (dm0 > 1e-4).mean() < 0.10                               # the bound is not vacuous


# ------------------------------------------------------------------------------------------------ 3. the output, given the kernel's own mask
@pytest.mark.parametrize('p', [1.0, 0.5, 0.0])
@pytest.mark.parametrize('smooth', ['none', 'default', 'limits'])
def test_output_given_the_mask(dev, smooth, p):
    kw = {'none': NONE, 'default': {}, 'limits': LIMITS}[smooth]
    n_f, n_t = O.smoothing(22050, kw.get('freq_mask_smooth_hz', 500), kw.get('time_mask_smooth_ms', 50))
    assert (n_f, n_t) == {'none': (0, 0), 'default': (11, 4), 'limits': (32, 8)}[smooth]
    x = _signal(5000)
    out, m0 = _gate(x, 22050, dev, prop_decrease=p, **kw)
    ref, det = O.reduce_noise(x, O.coefficient(22050), n_f=n_f, n_t=n_t, p=p, mask0=m0, details=True)
    err = np.abs(out - ref)
    print('%s p %g: max err %.3g, bound %.3g .. %.3g' % (smooth, p, err.max(), det['bound'].min(), det['bound'].max()))
    assert (err <= det['bound']).all()


# ------------------------------------------------------------------------------------------------ 4. edges
def test_all_zero_signal(dev):
    for L in (1, 700, 3000):
        out, m0 = _gate(np.zeros(L, dtype=np.float32), 22050, dev)
        assert np.array_equal(out, np.zeros(L)) and np.isfinite(m0).all()
        assert np.abs(m0 - 1 / (1 + np.exp(20.0))).max() <= 1e-15      # r := 0 where S == 0: sigmoid(-n_mult slope), about 2e-9, within half an f32 ulp


def test_second_half_is_exact_zeros(dev):
    x = _signal(5000).copy()
    x[2500:] = 0.0
    b = O.coefficient(22050)
    _, m0, dm0 = O.mask0_bound(x, b)
    out, got = _gate(x, 22050, dev)
    assert np.isfinite(got).all() and np.isfinite(out).all() and (np.abs(got - m0) <= dm0).all()
    ref, det = O.reduce_noise(x, b, n_f=11, n_t=4, mask0=got, details=True)
    assert (np.abs(out - ref) <= det['bound']).all()


def test_float64_and_non_contiguous_input(dev):
    x = _signal(5000)
    want = D.reduce_noise_nonstationary(x, 22050)
    assert tuple(want.shape) == (5000,) and want.dtype == torch.float32
    assert torch.equal(want, D.reduce_noise_nonstationary(x.astype(np.float64), 22050))
    wide = np.zeros((5000, 2), dtype=np.float32)
    wide[:, 0] = x
    assert not wide[:, 0].flags['C_CONTIGUOUS'] and torch.equal(want, D.reduce_noise_nonstationary(wide[:, 0], 22050))
    t = torch.from_numpy(wide).to(dev)[:, 0]
    assert not t.is_contiguous() and torch.equal(want, D.reduce_noise_nonstationary(t, 22050))


# ------------------------------------------------------------------------------------------------ 5. ragged batch
def _table(offs, lens, dev):
    frames = [O.n_frames(n) for n in lens]
    fo = np.concatenate([[0], np.cumsum(frames)])
    return torch.from_numpy(np.stack([offs, lens, fo[:-1], frames], 1).astype(np.int64)).to(dev), fo


def test_ragged_batch_is_bit_identical_to_single_calls(dev):
    """seven signals, lengths 1 and 22 050 among them; +-1e6 right next to every signal and NaN between them in the flat buffer; the batch gives, bit
    for bit, what single calls give, twice, in output and mask; nothing outside the signals is written"""
    from silent_speech_amd import torch_ops  # noqa: F401
    lens = [1, 257, 1500, 22050, 1, 3000, 1024]
    sigs = [_signal(n, seed=40 + i) for i, n in enumerate(lens)]
    parts, offs, pos = [], [], 0
    for s in sigs:
        parts += [np.array([np.nan, 1e6, np.nan, -1e6], dtype=np.float32), s]
        offs.append(pos + 4)
        pos += 4 + len(s)
    parts.append(np.array([1e6, np.nan], dtype=np.float32))
    flat = torch.from_numpy(np.concatenate(parts)).to(dev)
    table, fo = _table(offs, lens, dev)
    b = D.nonstationary_coefficient(22050)
    singles = [D.reduce_noise_nonstationary_batch([s], 22050, return_mask=True) for s in sigs]
    runs = []
    for _ in range(2):
        out = torch.full_like(flat, 7.0)
        mask = torch.ops.silent_speech.spectral_gate_nonstationary(flat, out, table, D._gate_windows(flat.device), int(fo[-1]), b, 2.0, 10.0, 11, 4, 1.0, True)
        runs.append((out.cpu(), mask.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    out, mask = runs[0]
    written = np.zeros(flat.shape[0], dtype=bool)
    for u, (o, n) in enumerate(zip(offs, lens)):
        assert torch.equal(out[o:o + n], singles[u][0].cpu()) and torch.equal(mask[fo[u]:fo[u + 1]], singles[u][2].cpu()), u
        written[o:o + n] = True
    assert torch.isfinite(out).all() and torch.isfinite(mask).all() and (out.numpy()[~written] == 7.0).all()
    packed = D.reduce_noise_nonstationary_batch(sigs, 22050, return_mask=True)          # the public call: the signals back to back
    assert packed[1] == lens and torch.equal(packed[0].cpu(), torch.cat([s[0].cpu() for s in singles]))
    assert torch.equal(packed[2].cpu(), torch.cat([s[2].cpu() for s in singles]))
    none = torch.ops.silent_speech.spectral_gate_nonstationary(flat, out.to(dev), table, D._gate_windows(flat.device), int(fo[-1]), b, 2.0, 10.0, 11, 4, 1.0, False)
    assert tuple(none.shape) == (0, 513)


def test_more_frames_than_waves(dev):
    """24 signals of 65 536 samples = 6168 frames of 257 each, more than the grid has waves: a wave owns frames of two signals.  Bit-identical to single
    calls; one signal against the oracle."""
    if is_emu(dev):
        pytest.skip('the emulator pretends 2 compute units: every batch of the other tests has more frames than waves there')
    n, sr = 65536, 16000
    sigs = [_signal(n, sr, seed=100 + u) for u in range(24)]
    out, lens, mask = D.reduce_noise_nonstationary_batch(sigs, sr, return_mask=True)
    F = O.n_frames(n)
    assert mask.shape[0] == 24 * F == 6168
    for u in (0, 1, 11, 23):
        one = D.reduce_noise_nonstationary_batch([sigs[u]], sr, return_mask=True)
        assert torch.equal(out[u * n:(u + 1) * n], one[0]) and torch.equal(mask[u * F:(u + 1) * F], one[2]), u
    b, u = O.coefficient(sr), 11
    _, m0, dm0 = O.mask0_bound(sigs[u], b)
    got = mask[u * F:(u + 1) * F].cpu().numpy().astype(np.float64).T
    assert (np.abs(got - m0) <= dm0).all()
    ref, det = O.reduce_noise(sigs[u], b, n_f=16, n_t=3, mask0=got, details=True)
    assert (np.abs(out[u * n:(u + 1) * n].cpu().numpy() - ref) <= det['bound']).all()


# ------------------------------------------------------------------------------------------------ 6. the surface
def test_refusals(dev):
    x = _signal(2000)
    with pytest.raises(NotImplementedError, match='reduce_noise_nonstationary'):
        D.reduce_noise(x, 22050, stationary=False)
    for sr in (0, -22050):
        with pytest.raises(ValueError, match='sample rate must be positive'):
            D.reduce_noise_nonstationary(x, sr)
        with pytest.raises(ValueError, match='sample rate must be positive'):
            D.nonstationary_coefficient(sr)
    for tc in (0.0, -1.0):
        with pytest.raises(ValueError, match='time_constant_s must be positive'):
            D.reduce_noise_nonstationary(x, 22050, time_constant_s=tc)
    for slope in (0.0, -10.0):
        with pytest.raises(ValueError, match='sigmoid_slope_nonstationary must be positive'):
            D.reduce_noise_nonstationary(x, 22050, sigmoid_slope_nonstationary=slope)
    for p in (-0.1, 1.5):
        with pytest.raises(ValueError, match='prop_decrease'):
            D.reduce_noise_nonstationary(x, 22050, prop_decrease=p)
    with pytest.raises(ValueError, match='not supported: at most 32 x 8'):
        D.reduce_noise_nonstationary(x, 22050, freq_mask_smooth_hz=1500)                # n_f = 34
    with pytest.raises(ValueError, match='not supported: at most 32 x 8'):
        D.reduce_noise_nonstationary(x, 22050, time_mask_smooth_ms=110)                 # n_t = 9
    with pytest.raises(ValueError, match='non-empty'):
        D.reduce_noise_nonstationary(np.zeros(0, dtype=np.float32), 22050)
    with pytest.raises(ValueError, match='empty signal'):
        D.reduce_noise_nonstationary_batch([x, np.zeros(0, dtype=np.float32)], 22050)
    with pytest.raises(ValueError, match="'stationary' or 'nonstationary'"):
        D.clean_session([x], 22050, gate='adaptive')
    with pytest.raises(ValueError, match='takes no noise clip'):
        D.clean_session([x], 22050, noise=x, gate='nonstationary')
    lib = _lib.lib()
    dbl = ctypes.c_double
    rc = lib.ss_spectral_gate_ns_batch(None, None, None, 1, 2, None, dbl(0.01), dbl(2.0), dbl(10.0), 0, 0, dbl(1.0), None, None, None, None, None)
    assert rc != 0 and b'ss_spectral_gate_ns_batch: null pointer' in lib.ss_last_error()
    t = torch.zeros(4096, dtype=torch.float32, device=dev)
    q = _lib.ptr(t)

    def raw(R=1, total=2, b=0.01, n_mult=2.0, slope=10.0, n_f=0, n_t=0, p=1.0):
        rc = lib.ss_spectral_gate_ns_batch(q, q, q, R, total, q, dbl(b), dbl(n_mult), dbl(slope), n_f, n_t, dbl(p), q, q, q, None, None)
        return rc, lib.ss_last_error()
    for kw, msg in ((dict(R=0), b'bad sizes'), (dict(R=2, total=3), b'bad sizes'), (dict(b=0.0), b'coefficient b'), (dict(b=1.5), b'coefficient b'),
                    (dict(slope=0.0), b'slope must be positive'), (dict(n_f=33), b'exceeds the kernel'), (dict(n_t=9), b'exceeds the kernel'),
                    (dict(p=1.5), b'prop_decrease'), (dict(p=-0.5), b'prop_decrease')):
        rc, err = raw(**kw)
        assert rc != 0 and msg in err, (kw, err)


def test_op_is_registered_with_a_fake(dev):
    from silent_speech_amd import torch_ops
    assert 'spectral_gate_nonstationary' in torch_ops.OPS
    assert 'Tensor(a1!) out' in str(torch.ops.silent_speech.spectral_gate_nonstationary.default._schema)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        flat, tab, win = torch.empty(1000), torch.empty((2, 4), dtype=torch.int64), torch.empty((3, 1024))
        m = torch.ops.silent_speech.spectral_gate_nonstationary(flat, torch.empty(1000), tab, win, 7, 0.006, 2.0, 10.0, 11, 4, 1.0, True)
        assert tuple(m.shape) == (7, 513) and m.dtype == torch.float32
        m = torch.ops.silent_speech.spectral_gate_nonstationary(flat, torch.empty(1000), tab, win, 7, 0.006, 2.0, 10.0, 11, 4, 1.0, False)
        assert tuple(m.shape) == (0, 513)


def _session():
    """a session WITHOUT a silence clip: three recordings over noise of 0.004 RMS, a short loud burst in the second (a peak the gain lifts over 0.99)"""
    rng = np.random.default_rng(12)
    sr, out = 16000, []
    for i, n in enumerate((6000, 4500, 7000)):
        t = np.arange(n) / sr
        x = (0.08 + 0.03 * i) * np.sin(2 * np.pi * (400 + 150 * i) * t) * (np.arange(n) > n // 3) + 0.004 * rng.standard_normal(n)
        if i == 1:
            x[2000:2400] += 0.8 * np.sin(2 * np.pi * 700 * t[2000:2400])
        out.append(x.astype(np.float32))
    return out, sr


def test_clean_session_nonstationary(dev):
    """clean_session(gate='nonstationary') == levels of the raw signals -> the non-stationary gate of EVERY signal -> the resample with the session
    gains -> the peak rule, composed by hand from the public pieces; the default path still treats signals[0] as the noise clip"""
    sigs, sr = _session()
    flat, lens = D.clean_session(sigs, sr, gate='nonstationary')
    gains = D.session_gains(D.volume_levels(sigs)[0][:, 0].cpu().tolist())
    assert gains is not None
    clean, clens = D.reduce_noise_nonstationary_batch(sigs, sr)
    assert clens == [len(s) for s in sigs]
    out, out_lens = D.resample_audio_batch((clean, clens), sr, 22050, gains=gains)
    peak = D.volume_levels((out, out_lens))[0][:, 1]
    assert int((peak > 0.99).sum()) == 1
    want, want_lens = D.resample_audio_batch((out, out_lens), 1, 1, gains=torch.where(peak > 0.99, 0.99 / peak, torch.ones_like(peak)))
    assert lens == want_lens and torch.equal(flat, want)
    ungated, _ = D.resample_audio_batch(sigs[:1], sr, 22050, gains=gains[:1])
    assert not torch.equal(flat[:lens[0]], ungated)                    # signals[0] is gated too
    stationary, slens = D.clean_session(sigs, sr)
    assert slens == lens and not torch.equal(stationary, flat)


def test_device_batch_builder_gates_recordings_with_noise_gate(dev):
    """recordings with noise_gate='nonstationary' == the same recordings carrying the audio gated by hand, bit for bit; a recording at 16 kHz is gated
    at its stored rate, before the resample; without the key nothing changes; both keys are refused"""
    from silent_speech_amd import pipeline
    from tests.test_audio_resample import _batch_recordings, _same_batch
    base = _batch_recordings(np.random.default_rng(17))
    a16 = np.array(_signal(256 * len(base[2]['phonemes']) * 320 // 441 + 1, 16000))
    base[2] = dict(base[2], audio=a16, audio_rate=16000)
    builder = pipeline.DeviceBatchBuilder(dev)
    plain = builder.build(base)
    _same_batch(builder.build([dict(r, noise_gate=None) for r in base]), plain, True)

    def hand(rec):
        return D.reduce_noise_nonstationary(rec['audio'], int(rec.get('audio_rate', 22050))).cpu().numpy()
    # recording 0 (22 050 Hz), the silent one's twin (22 050 Hz) and recording 2 (16 kHz) are gated; the silent recording's own audio is not
    recs = [dict(base[0], noise_gate='nonstationary'), dict(base[1], parallel=dict(base[1]['parallel'], noise_gate='nonstationary')),
            dict(base[2], noise_gate='nonstationary')]
    want = [dict(base[0], audio=hand(base[0])), dict(base[1], parallel=dict(base[1]['parallel'], audio=hand(base[1]['parallel']))),
            dict(base[2], audio=hand(base[2]))]
    got = builder.build(recs)
    _same_batch(got, builder.build(want), True)
    assert not torch.equal(got['audio_features'][0], plain['audio_features'][0]) and not torch.equal(got['audio_features'][2], plain['audio_features'][2])
    prof = D.NoiseProfile.from_noise(base[0]['audio'][:3000], 22050)
    with pytest.raises(ValueError, match='not both'):
        builder.build([dict(base[0], noise_gate='nonstationary', noise_profile=prof)])
    with pytest.raises(ValueError, match="noise_gate: 'nonstationary' or None"):
        builder.build([dict(base[0], noise_gate='stationary')])
