"""Stationary spectral gating (csrc/spectral_gate.hip: data_utils.NoiseProfile / reduce_noise / reduce_noise_batch / clean_session, the loader's
noise_profile) against the float64 restatement tests/spectral_gate_oracle.py, on the emulator tier and on the MI355X.  Every tolerance is derived in
the oracle's docstring from operation counts and the f32 format; none is fitted."""
import functools

import numpy as np
import pytest
import scipy.signal
import torch

from silent_speech_amd import _lib, data_utils as D
from tests import audio_oracle as ao
from tests import spectral_gate_oracle as O
from tests.backend import dev, is_emu  # noqa: F401

LENGTHS = [1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1279, 1280, 1281, 2304, 22050]
INF = float('inf')


@functools.lru_cache(maxsize=None)
def _signal(L, sr=22050, seed=3):
    """a chirp (300 -> 3000 Hz, amplitude 0.3) switched on for the middle half of the signal, over noise of 0.01 RMS; f32"""
    rng = np.random.default_rng(seed + L)
    t = np.arange(L) / sr
    on = (np.arange(L) >= L // 4) & (np.arange(L) < L - L // 4)
    x = 0.3 * np.sin(2 * np.pi * (300 * t + 0.5 * 2700 * t * t / max(L / sr, 1e-3))) * on + 0.01 * rng.standard_normal(L)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _noise_thresh(sr=22050):
    """the f32 threshold table both sides get: the oracle's profile of a 0.25 s clip of the same 0.01 RMS noise"""
    th = O.profile(0.01 * np.random.default_rng(99).standard_normal(sr // 4)).astype(np.float32)
    th.setflags(write=False)
    return th


def _profile(thresh, sr, dev):
    return D.NoiseProfile(torch.from_numpy(np.array(thresh, dtype=np.float32)).to(dev), sr)


def _gate(x, thresh, sr, dev, **kw):
    out, lens, bits = D.reduce_noise_batch([x], _profile(thresh, sr, dev), return_bits=True, **kw)
    assert lens == [len(x)] and tuple(out.shape) == (len(x),) and out.dtype == torch.float32 and tuple(bits.shape) == (O.n_frames(len(x)), 17)
    return out.cpu().numpy().astype(np.float64), O.unpack_bits(bits.cpu().numpy())


NONE = dict(freq_mask_smooth_hz=None, time_mask_smooth_ms=None)


# ------------------------------------------------------------------------------------------------ 1. the oracle itself (CPU only)
@pytest.mark.parametrize('L', [1024, 1025, 2304, 5000, 5120])
def test_oracle_framing_is_scipy_stft_and_istft(L):
    """For L >= 1024 the explicit framing is scipy's: padded=False where L is a multiple of the hop; otherwise padded=False drops the samples behind the
    last whole hop, and F = ceil(L / H) + 1 is what scipy frames once it pads the signal to whole hops (padded=True)."""
    x = _signal(L).astype(np.float64)
    _, _, Z = scipy.signal.stft(x, nfft=1024, nperseg=1024, noverlap=768, padded=L % 256 != 0)
    X = O.stft(x)
    assert Z.shape == X.shape and np.abs(Z - X).max() <= 1e-15
    Y = X * np.random.default_rng(0).uniform(0, 1, X.shape)
    _, y = scipy.signal.istft(Y, nfft=1024, nperseg=1024, noverlap=768)
    assert np.abs(y[:L] - O.istft(Y, L)).max() <= 1e-14


@pytest.mark.parametrize('L', LENGTHS)
def test_oracle_returns_the_signal_when_every_bin_is_open(L):
    x = _signal(L).astype(np.float64)
    y = O.reduce_noise(x, np.full(513, -INF))
    assert y.shape == x.shape and np.abs(y - x).max() <= 1e-12


def test_oracle_pieces():
    assert O.smoothing(22050) == (11, 4) and O.smoothing(16000) == (16, 3) and O.smoothing(22050, None, None) == (0, 0)
    assert np.array_equal(O.tri(0), [1.0]) and np.allclose(O.tri(2), [1 / 3, 2 / 3, 1, 2 / 3, 1 / 3])
    m = np.random.default_rng(1).uniform(0, 1, (513, 7))
    filt = np.outer(O.tri(11), O.tri(4))
    assert np.abs(O.smooth(m, 11, 4) - scipy.signal.fftconvolve(m, filt / filt.sum(), mode='same')).max() <= 1e-12
    assert np.array_equal(O.smooth(m, 0, 0), m)


# the cases of test 4: (name, rate, length, smoothing arguments, p, threshold table or None = the noise clip's profile)
_EDGE_ROWS = np.full(513, INF, dtype=np.float32)
_EDGE_ROWS[[0, 31, 32, 512]] = -INF
CASES = [
    ('default_22050', 22050, 22050, {}, 1.0, None),
    ('default_16000', 16000, 16000, {}, 1.0, None),
    ('no_frequency_taps', 22050, 5000, dict(freq_mask_smooth_hz=None), 1.0, None),
    ('no_time_taps', 22050, 5000, dict(time_mask_smooth_ms=None), 1.0, None),
    ('no_smoothing', 22050, 5000, NONE, 1.0, None),
    ('p_0.8', 22050, 5000, {}, 0.8, None),
    ('frames_le_n_t', 22050, 600, {}, 1.0, None),             # F = 4 = n_t
    ('two_frames', 22050, 200, {}, 1.0, None),                # F = 2
    ('frames_2n_t_plus_1', 22050, 2048, {}, 1.0, None),       # F = 9: the time taps run off both ends in every frame
    ('dword_edges', 22050, 5000, {}, 1.0, _EDGE_ROWS),        # open rows 0, 31, 32, 512 only
]


def _case(case):
    name, sr, L, kw, p, th = case
    n_f, n_t = O.smoothing(sr, kw.get('freq_mask_smooth_hz', 500), kw.get('time_mask_smooth_ms', 50))
    x = _signal(L, sr)
    if name == 'dword_edges':                                  # content in the open rows: an offset, a tone between bins 31 and 32, the Nyquist tone
        n = np.arange(L)
        x = (x + 0.1 + 0.2 * np.sin(2 * np.pi * 31.5 / 1024 * n) + 0.1 * (-1.0) ** n).astype(np.float32)
    return x, (_noise_thresh(sr) if th is None else th), n_f, n_t


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_the_output_bound_discriminates(case):
    """A frame left out of the overlap-add, or the mask moved by one bin, changes the oracle's output by more than 10 x the derived bound: the
    tolerance of test 4 cannot hide the errors the kernel can make."""
    x, th, n_f, n_t = _case(case)
    ref, det = O.reduce_noise(x, th, n_f, n_t, case[4], details=True)
    F = O.n_frames(len(x))
    for wrong in (O.reduce_noise(x, th, n_f, n_t, case[4], skip_frame=F // 2), O.reduce_noise(x, th, n_f, n_t, case[4], shift_mask=1)):
        assert np.abs(wrong - ref).max() > 10 * det['bound'].max()


# ------------------------------------------------------------------------------------------------ 2. closed forms on the device
@pytest.mark.parametrize('L', LENGTHS)
def test_closed_forms(dev, L):
    """thresh = +inf, p = 1 -> exactly 0; p = 0 -> the input; thresh = -inf -> the input; the last two within the round-trip bound, without smoothing
    (with smoothing the pinned definition pads the mask with zeros, so even an all-ones mask attenuates the edge rows and frames: test 4 covers that)."""
    x = _signal(L)
    out, bits = _gate(x, np.full(513, INF), 22050, dev)
    assert not bits.any() and np.array_equal(out, np.zeros(L))
    ref, det = O.reduce_noise(x, np.full(513, -INF), details=True)
    tol = det['bound'] + 1e-12
    out, bits = _gate(x, np.full(513, INF), 22050, dev, prop_decrease=0.0, **NONE)
    assert not bits.any() and (np.abs(out - x) <= tol).all()
    out, bits = _gate(x, np.full(513, -INF), 22050, dev, **NONE)
    assert bits.all() and (np.abs(out - x) <= tol).all()


# ------------------------------------------------------------------------------------------------ 3. gate bits
def _check_bits(x, th, bits, cap=0.005):
    """the kernel's bits equal the oracle's wherever the margin exceeds G 2^-24 S_f; the bins inside it are at most 0.5 % of the case"""
    X, S = O.stft(x), O.frame_sums(x)
    want, open_rows = O.gate(X, th)
    m_bin, m_row = O.margins(X, th, S)
    decided = (m_bin > 0) & ~(open_rows | (m_row <= 0))[:, None]       # a bin of a row that top_db opens (or may open) is decided by the row
    decided |= (open_rows & (m_row > 0))[:, None]
    assert 1.0 - decided.mean() <= cap, 'share of undecided bins %.4f' % (1.0 - decided.mean())
    assert np.array_equal(bits[decided], want[decided])
    return open_rows & (m_row > 0)


@pytest.mark.parametrize('sr', [22050, 16000])
@pytest.mark.parametrize('L', LENGTHS)
def test_gate_bits(dev, L, sr):
    x, th = _signal(L, sr), _noise_thresh(sr)
    _check_bits(x, th, _gate(x, th, sr, dev)[1])


def test_top_db_opens_rows(dev):
    """noise at the 1e-6 level under a tone of amplitude 0.5: every row whose maximum lies more than 80 dB above its threshold is open in EVERY frame.
    The 0.5 % cap on skipped bins cannot hold for THIS input in f32 and is not asserted here (it is on every chirp case of test_gate_bits): in a frame
    that holds the tone G 2^-24 S_f = 32 x 6e-8 x 0.3 = 6e-7, above the threshold amplitude 10^(thresh / 20) ~ 1e-7 of the noise rows itself, so every
    bin of those frames outside the tone's skirt lies inside the margin (24 % of the case's bins); the decided bins and the opened rows are compared."""
    rng = np.random.default_rng(5)
    L, sr = 8000, 22050
    x = (0.5 * np.sin(2 * np.pi * 1000 * np.arange(L) / sr) * (np.arange(L) > 3000) + 1e-6 * rng.standard_normal(L)).astype(np.float32)
    th = O.profile(1e-6 * rng.standard_normal(4000)).astype(np.float32)
    bits = _gate(x, th, sr, dev)[1]
    rows = _check_bits(x, th, bits, cap=1.0)
    assert rows.sum() >= 50 and bits[rows].all()
    assert not O.gate(O.stft(x), th + 80.0)[0][rows].all()            # without the clamp these rows would have closed frames


# ------------------------------------------------------------------------------------------------ 4. the output, given the mask
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_output_given_the_mask(dev, case):
    x, th, n_f, n_t = _case(case)
    out, bits = _gate(x, th, case[1], dev, prop_decrease=case[4], **case[3])
    if case[0] == 'dword_edges':
        assert np.array_equal(np.flatnonzero(bits.all(1)), [0, 31, 32, 512]) and bits.sum() == 4 * bits.shape[1]
    ref, det = O.reduce_noise(x, th, n_f, n_t, case[4], mask=bits, details=True)
    err = np.abs(out - ref)
    print('%s: max err %.3g, bound %.3g .. %.3g' % (case[0], err.max(), det['bound'].min(), det['bound'].max()))
    assert (err <= det['bound']).all()


# ------------------------------------------------------------------------------------------------ 5. the noise profile
@pytest.mark.parametrize('clip', ['1024', '255', '4096', '1s', 'zeros'])
def test_noise_profile(dev, clip):
    rng = np.random.default_rng(8)
    noise = np.zeros(1024, dtype=np.float32) if clip == 'zeros' else (0.01 * rng.standard_normal({'1024': 1024, '255': 255, '4096': 4096, '1s': 22050}[clip])).astype(np.float32)
    prof = D.NoiseProfile.from_noise(noise, 22050, 2.0)
    assert prof.sr == 22050 and prof.n_std == 2.0 and tuple(prof.thresh.shape) == (513,) and prof.thresh.dtype == torch.float32
    want, bound = O.profile_bound(noise, 2.0)
    got = prof.thresh.cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= bound).all()
    if clip == 'zeros':                                                 # std 0: every frame is 20 log10(eps)
        assert np.abs(want - 20 * np.log10(O.EPS)).max() < 1e-9


def test_signal_is_its_own_noise_clip(dev):
    x = _signal(5000)
    a = D.reduce_noise(x, 22050)
    assert torch.equal(a, D.reduce_noise(x, 22050, y_noise=x)) and torch.equal(a, D.reduce_noise(x, 22050, profile=D.NoiseProfile.from_noise(x, 22050)))
    assert tuple(a.shape) == (5000,) and a.dtype == torch.float32
    assert not torch.equal(a, D.reduce_noise(x, 22050, n_std_thresh_stationary=0.5))


# ------------------------------------------------------------------------------------------------ 6. ragged batch
def test_ragged_batch_is_bit_identical_to_single_calls(dev):
    """lengths 1 and 257 among longer signals; +-1e6 right next to every signal and NaN between them in the flat buffer; the batch gives, bit for bit,
    what single calls give, twice; nothing outside the signals is written"""
    from silent_speech_amd import torch_ops  # noqa: F401
    lens, th = [1, 257, 1500, 1, 3000], _noise_thresh()
    sigs = [_signal(n, seed=40 + i) for i, n in enumerate(lens)]
    parts, offs, pos = [], [], 0
    for s in sigs:
        margin = np.array([np.nan, 1e6, np.nan, -1e6], dtype=np.float32)
        parts += [margin, s]
        offs.append(pos + 4)
        pos += 4 + len(s)
    parts.append(np.array([1e6, np.nan], dtype=np.float32))
    flat = torch.from_numpy(np.concatenate(parts)).to(dev)
    frames = [O.n_frames(n) for n in lens]
    fo = np.concatenate([[0], np.cumsum(frames)])
    table = torch.from_numpy(np.stack([offs, lens, fo[:-1], frames], 1).astype(np.int64)).to(dev)
    prof = _profile(th, 22050, dev)
    singles = [D.reduce_noise_batch([s], prof, return_bits=True) for s in sigs]
    runs = []
    for _ in range(2):
        out = torch.full_like(flat, 7.0)
        bits = torch.ops.silent_speech.spectral_gate(flat, out, table, D._gate_windows(flat.device), prof.thresh, int(fo[-1]), 11, 4, 1.0, True)
        runs.append((out.cpu(), bits.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    out, bits = runs[0]
    written = np.zeros(flat.shape[0], dtype=bool)
    for u, (o, n) in enumerate(zip(offs, lens)):
        assert torch.equal(out[o:o + n], singles[u][0].cpu()) and torch.equal(bits[fo[u]:fo[u + 1]], singles[u][2].cpu()), u
        written[o:o + n] = True
    assert torch.isfinite(out).all() and (out.numpy()[~written] == 7.0).all()
    packed = D.reduce_noise_batch(sigs, prof)                          # the public call: the signals back to back
    assert packed[1] == lens and torch.equal(packed[0].cpu(), torch.cat([s[0].cpu() for s in singles]))


# ------------------------------------------------------------------------------------------------ 7. the surface
def test_refusals(dev):
    x = _signal(2000)
    with pytest.raises(NotImplementedError, match='non-stationary gate is out of scope'):
        D.reduce_noise(x, 22050, stationary=False)
    for sr in (0, -22050):
        with pytest.raises(ValueError, match='sample rate must be positive'):
            D.reduce_noise(x, sr)
        with pytest.raises(ValueError, match='sample rate must be positive'):
            D.NoiseProfile.from_noise(x, sr)
    with pytest.raises(ValueError, match='not supported: at most 32 x 8'):
        D.reduce_noise(x, 22050, freq_mask_smooth_hz=1500)              # n_f = 34
    with pytest.raises(ValueError, match='not supported: at most 32 x 8'):
        D.reduce_noise(x, 22050, time_mask_smooth_ms=110)               # n_t = 9
    with pytest.raises(ValueError, match='non-empty'):
        D.reduce_noise(np.zeros(0, dtype=np.float32), 22050)
    with pytest.raises(ValueError, match='non-empty'):
        D.reduce_noise(x, 22050, y_noise=np.zeros(0, dtype=np.float32))
    prof = _profile(_noise_thresh(), 22050, dev)
    with pytest.raises(ValueError, match='empty signal'):
        D.reduce_noise_batch([x, np.zeros(0, dtype=np.float32)], prof)
    with pytest.raises(ValueError, match='prop_decrease'):
        D.reduce_noise_batch([x], prof, prop_decrease=1.5)
    with pytest.raises(TypeError, match='NoiseProfile'):
        D.reduce_noise_batch([x], _noise_thresh())
    lib = _lib.lib()
    import ctypes
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.ss_spectral_gate_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
    assert (a.value, b.value, c.value) == (D.GATE_MAX_NF, D.GATE_MAX_NT, 17) == (32, 8, 17)
    rc = lib.ss_spectral_gate_batch(None, None, None, 1, 2, None, None, 0, 0, 1.0, None, None, None, None, None)
    assert rc != 0 and b'ss_spectral_gate_batch: null pointer' in lib.ss_last_error()
    t = torch.zeros(2048, dtype=torch.float32, device=dev)
    rc = lib.ss_spectral_gate_batch(_lib.ptr(t), _lib.ptr(t), _lib.ptr(t), 1, 2, _lib.ptr(t), _lib.ptr(t), 33, 0, 1.0, _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), None, None)
    assert rc != 0 and b'exceeds the kernel' in lib.ss_last_error()
    rc = lib.ss_spectral_gate_profile(_lib.ptr(t), _lib.ptr(t), 1, _lib.ptr(t), 1.5, _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), None)
    assert rc != 0 and b'empty noise clip' in lib.ss_last_error()


def test_ops_are_registered_with_fakes(dev):
    from silent_speech_amd import torch_ops
    assert 'spectral_gate_profile' in torch_ops.OPS and 'spectral_gate' in torch_ops.OPS
    assert 'Tensor(a1!) out' in str(torch.ops.silent_speech.spectral_gate.default._schema)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        flat, tab, win = torch.empty(1000), torch.empty((2, 4), dtype=torch.int64), torch.empty((3, 1024))
        th = torch.ops.silent_speech.spectral_gate_profile(flat, tab[:1], win, 5, 1.5)
        assert tuple(th.shape) == (513,) and th.dtype == torch.float32
        bits = torch.ops.silent_speech.spectral_gate(flat, torch.empty(1000), tab, win, th, 7, 11, 4, 1.0, True)
        assert tuple(bits.shape) == (7, 17) and bits.dtype == torch.int32
        assert tuple(torch.ops.silent_speech.spectral_gate(flat, torch.empty(1000), tab, win, th, 7, 11, 4, 1.0, False).shape) == (0, 17)


def _session(quiet):
    rng = np.random.default_rng(12)
    sr, out = 16000, [(0.004 * rng.standard_normal(4000)).astype(np.float32)]                       # 0_audio: the silence clip
    for i, n in enumerate((6000, 4500, 7000)):
        t = np.arange(n) / sr
        x = (0.004 if quiet else 0.08 + 0.03 * i) * np.sin(2 * np.pi * (400 + 150 * i) * t) * (np.arange(n) > n // 3) + 0.004 * rng.standard_normal(n)
        if i == 1 and not quiet:
            x[2000:2400] += 0.8 * np.sin(2 * np.pi * 700 * t[2000:2400])                             # a short loud burst: a peak the gain lifts over 0.99
        out.append(x.astype(np.float32))
    return out, sr


@pytest.mark.parametrize('quiet', [False, True], ids=['levelled', 'quiet_run'])
def test_clean_session(dev, quiet):
    """clean_directory from decoded arrays against the oracle composition: gate (given the kernel's own profile table and bits) -> resample_poly ->
    gain 0.2 / smoothed max -> peak rule.  Tolerance: (the gate's bound through the filter's largest phase sum + the resampler's bound) x gain."""
    sigs, sr = _session(quiet)
    flat, lens = D.clean_session(sigs, sr)
    up, down = ao.ratio(sr, 22050)
    assert lens == [ao.out_length(len(s), up, down) for s in sigs] and flat.dtype == torch.float32 and flat.shape[0] == sum(lens)
    got = np.split(flat.cpu().numpy().astype(np.float64), np.cumsum(lens)[:-1])
    rms = [ao.levels(s)[0] for s in sigs]
    gains = []
    for i in range(len(rms)):
        vs = [v for v in rms[max(0, i - 20):i + 21] if v > 0.02]
        gains.append(0.2 / np.mean(vs) if vs else None)
    assert quiet == all(g is None for g in gains[1:])
    if any(g is None for g in gains):
        gains = None                                                    # "long run of quiet audio, skipping volume normalization"
    prof = D.NoiseProfile.from_noise(sigs[0], sr)
    th = prof.thresh.cpu().numpy()
    h, _ = ao.taps(up, down)
    phase_sum = max(float(np.abs(h[ph::up]).sum()) for ph in range(up))
    applied = 0
    for u, s in enumerate(sigs):
        bits = O.unpack_bits(D.reduce_noise_batch([s], prof, return_bits=True)[2].cpu().numpy())
        clean, det = O.reduce_noise(s, th, *O.smoothing(sr), mask=bits, details=True)
        ref = ao.resample(clean, up, down)
        tol = phase_sum * det['bound'].max() + ao.bound(up, down, np.abs(clean).max())
        if gains is not None:
            ref, tol = ref * gains[u], tol * gains[u]
            peak = np.abs(ref).max()
            if peak > 0.99:
                ref, tol, applied = ref / peak * 0.99, tol / peak * 0.99 * (1 + 2 * tol / peak), applied + 1
        tol = tol + 6 * O.U * np.abs(ref).max()                         # the f32 gain, its product, the peak and its scale
        assert np.abs(got[u] - ref).max() <= tol, u
    assert applied == (0 if quiet else 1)


def test_device_batch_builder_gates_recordings_with_a_noise_profile(dev):
    """recordings with noise_profile == gate -> (resample ->) mel done by hand, at the mel bar; without the key the batch is bit for bit what it was"""
    from silent_speech_amd import pipeline
    from tests.test_audio_resample import _batch_recordings, _same_batch
    base = _batch_recordings(np.random.default_rng(17))
    builder = pipeline.DeviceBatchBuilder(dev)
    plain = builder.build(base)
    _same_batch(builder.build([dict(r, noise_profile=None) for r in base]), plain, True)
    src = base + [base[1]['parallel']]
    mel, frames = D.mel_spectrogram_batch([torch.from_numpy(r['audio']).to(dev) for r in src])
    for i, k in enumerate((0, 3, 2)):
        n = plain['audio_feature_lengths'][i]
        assert torch.equal(plain['audio_features'][i], mel[k, :n])
    # recordings 0 and the silent one's twin carry a profile (one each), recording 2 carries none
    p0 = D.NoiseProfile.from_noise(base[0]['audio'][:3000], 22050)
    p1 = D.NoiseProfile.from_noise(base[1]['parallel']['audio'][:2000], 22050, 1.0)
    recs = [dict(base[0], noise_profile=p0), dict(base[1], parallel=dict(base[1]['parallel'], noise_profile=p1)), base[2]]
    got = builder.build(recs)
    hand = [D.reduce_noise(base[0]['audio'], 22050, profile=p0), torch.from_numpy(base[1]['audio']).to(dev), torch.from_numpy(base[2]['audio']).to(dev),
            D.reduce_noise(base[1]['parallel']['audio'], 22050, profile=p1)]
    mel, frames = D.mel_spectrogram_batch(hand)
    for i, k in enumerate((0, 3, 2)):
        n = got['audio_feature_lengths'][i]
        assert n == plain['audio_feature_lengths'][i] and float((got['audio_features'][i] - mel[k, :n]).abs().mean()) < 1e-4
    assert torch.equal(got['audio_features'][2], plain['audio_features'][2]) and not torch.equal(got['audio_features'][0], plain['audio_features'][0])
    # at a stored rate of 16 kHz the gate runs before the resample
    a16 = _signal(256 * len(base[2]['phonemes']) * 320 // 441 + 1, 16000)
    p2 = D.NoiseProfile.from_noise(a16[:2000], 16000)
    got = builder.build([dict(base[2], audio=a16, audio_rate=16000, noise_profile=p2)])
    clean = D.reduce_noise(a16, 16000, profile=p2)
    mel, frames = D.mel_spectrogram_batch(D.resample_audio_batch([clean], 16000, 22050))
    n = got['audio_feature_lengths'][0]
    assert float((got['audio_features'][0] - mel[0, :n]).abs().mean()) < 1e-4
