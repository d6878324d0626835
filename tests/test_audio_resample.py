"""Stored audio on the device (csrc/audio.hip): the band-limited resample and the volume levelling of the reference's load_audio, the loader and
save_output on top of them, against the float64 restatement in tests/audio_oracle.py (scipy.signal.resample_poly is the pinned definition).

The resampler's tolerance is derived, not measured: bound = (taps + 2) 2^-24 max_phase sum |h| max |x| (audio_oracle.bound) -- one f32 rounding
per product of the longest phase plus the rounding of the table and of the input; 3.1e-6 for 441/320 at |x| <= 1."""
import ctypes
import wave

import numpy as np
import pytest
import torch

from silent_speech_amd import _lib, data_utils as D
from tests import audio_oracle as ao
from tests.backend import dev, is_emu  # noqa: F401

T, SPAN = D.RESAMPLE_TILE, D.RESAMPLE_SPAN
RATIOS = [(441, 320), (320, 441), (2, 1), (1, 2)]          # (up, down): 16 000 -> 22 050 Hz, back, and the two octave steps
U24 = 2.0 ** -24


def _resample(x, up, down, dev, **kw):
    flat, lens = D.resample_audio_batch([torch.from_numpy(np.asarray(x, dtype=np.float32)).to(dev)], down, up, **kw)
    assert lens == [int(flat.shape[0])] and flat.dtype == torch.float32 and flat.device.type == dev.type
    return flat.cpu().numpy()


def _n_for(n_out, up, down):
    """the shortest signal with at least n_out outputs"""
    n = n_out * down // up
    while ao.out_length(n, up, down) < n_out:
        n += 1
    while n > 1 and ao.out_length(n - 1, up, down) >= n_out:
        n -= 1
    return n


def test_limits_are_the_kernels(dev):
    t, s, f = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.lib().ss_audio_resample_limits(ctypes.byref(t), ctypes.byref(s), ctypes.byref(f))
    assert (t.value, s.value, f.value) == (T, SPAN, D.RESAMPLE_TABLE_FLOATS)
    for orig, target in [(16000, 22050), (22050, 16000), (48000, 22050), (44100, 16000), (32000, 16000), (8000, 16000)]:
        D._resample_table(*D._rate_ratio(orig, target), dev)


@pytest.mark.parametrize('up,down', RATIOS + [(3, 2)])
def test_oracle_closed_form_is_resample_poly(up, down):
    rng = np.random.default_rng(up)
    for n in (1, 2, 21, 29, 100, 333):
        x = rng.uniform(-1, 1, n)
        want = ao.resample(x, up, down)
        assert want.shape == (ao.out_length(n, up, down),)
        assert np.abs(ao.resample_closed_form(x, up, down) - want).max() < 1e-12
    h, half = ao.taps(up, down)
    mine, half2 = D.resample_filter(up, down)
    assert half2 == half and np.abs(mine - h).max() < 1e-14


@pytest.mark.parametrize('up,down', RATIOS)
def test_impulse_reads_the_filter_back(dev, up, down):
    """1. closed form: an impulse at j gives float32(h) at stride `down`, bit for bit, and zeros elsewhere"""
    h, half = ao.taps(up, down)
    n = 50
    for j in (0, 1, n - 1, 23):
        x = np.zeros(n, dtype=np.float32)
        x[j] = 1.0
        got = _resample(x, up, down, dev)
        k = np.arange(ao.out_length(n, up, down)) * down + half - j * up
        want = np.where((k >= 0) & (k <= 2 * half), h[np.clip(k, 0, 2 * half)], 0.0).astype(np.float32)
        assert got.shape == want.shape and np.array_equal(got, want), (up, down, j)


@pytest.mark.parametrize('up,down', RATIOS)
def test_every_length_edge(dev, up, down):
    """2. lengths around the 21 / 28 products of an output, and around the output tile: within the bound of scipy, exact output length"""
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, 2 * SPAN + 64).astype(np.float32)
    lengths = [1, 2, 19, 20, 21, 22, 27, 28, 29]
    tile_edges = [T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1]           # T + 1, 2 T + 1: the last tile holds a single output
    lengths += [_n_for(e, up, down) for e in tile_edges]
    if up <= down:
        assert [ao.out_length(n, up, down) for n in lengths[9:]] == tile_edges       # every output count is reachable when downsampling
    bound = ao.bound(up, down, 1.0)
    if (up, down) == (441, 320):
        assert 3.0e-6 < bound < 3.2e-6
    for n in lengths:
        got, want = _resample(x[:n], up, down, dev), ao.resample(x[:n], up, down)
        assert got.shape == (ao.out_length(n, up, down),) == want.shape, n
        err = float(np.abs(got - want).max())
        assert err <= bound, (n, err, bound)


def test_copy_when_the_rates_agree(dev):
    x = np.random.default_rng(0).standard_normal(1031).astype(np.float32)
    assert np.array_equal(_resample(x, 1, 1, dev), x)
    assert np.array_equal(D.resample_audio(x, 22050, 22050).cpu().numpy(), x)
    assert np.array_equal(D.resample_audio(x, 22050, 22050, clip=True).cpu().numpy(), np.clip(x, -1, 1))


def _raw_call(dev, x_flat, rows, up, down, margin, gains=None, flags=0):
    """ss_audio_resample_batch on caller-made buffers: the outputs packed behind `margin` NaNs, `margin` NaNs behind them"""
    coef, half, tpp = D._resample_table(up, down, dev)
    total = sum(r[3] for r in rows)
    out = torch.full((total + 2 * margin,), float('nan'), dtype=torch.float32, device=dev)
    table = torch.tensor(rows, dtype=torch.int64).to(dev)
    x = torch.from_numpy(x_flat).to(dev)
    g = None if gains is None else torch.tensor(gains, dtype=torch.float32).to(dev)
    rc = _lib.lib().ss_audio_resample_batch(_lib.ptr(x), ctypes.c_void_p(out.data_ptr() + 4 * margin), _lib.ptr(table), len(rows), up, down, half, tpp,
                                            _lib.ptr(coef), _lib.ptr(g), flags, total, _lib.stream_of(x))
    _lib.check(rc, 'ss_audio_resample_batch')
    return out.cpu().numpy()


@pytest.mark.parametrize('up,down', [(441, 320), (320, 441)])
def test_ragged_batch_keeps_utterances_apart(dev, up, down):
    """3. five utterances in one call, +-1e6 blocks between them in the input, NaN margins around the packed output: bit-identical to the
    one-utterance calls, margins untouched -- for the LDS-table and the cached-table variant of the kernel, and at a misaligned output address"""
    rng = np.random.default_rng(11)
    lens = [1, 21, _n_for(T + 1, up, down), 0, 1500]
    sigs = [rng.uniform(-1, 1, n).astype(np.float32) for n in lens]
    singles = [_resample(s, up, down, dev) if len(s) else np.zeros(0, dtype=np.float32) for s in sigs]
    guard, parts, rows, o = 64, [], [], 0
    at = 0
    for u, s in enumerate(sigs):
        parts.append(np.full(guard, 1e6 if u % 2 else -1e6, dtype=np.float32))
        at += guard
        rows.append((at, len(s), o, ao.out_length(len(s), up, down)))
        parts.append(s)
        at += len(s)
        o += rows[-1][3]
    parts.append(np.full(guard, 1e6, dtype=np.float32))
    x_flat = np.concatenate(parts)
    for margin, flags in ((8, 0), (7, 0), (8, 2)):
        out = _raw_call(dev, x_flat, rows, up, down, margin, flags=flags)
        assert np.isnan(out[:margin]).all() and np.isnan(out[len(out) - margin:]).all()
        for (_, _, oo, n_out), want in zip(rows, singles):
            assert np.array_equal(out[margin + oo:margin + oo + n_out], want)
    # the public batch call: same values, lengths reported
    flat, out_lens = D.resample_audio_batch([torch.from_numpy(s).to(dev) for s in sigs], down, up)
    assert out_lens == [r[3] for r in rows] and np.array_equal(flat.cpu().numpy(), np.concatenate(singles))
    packed = (torch.from_numpy(np.concatenate(sigs)).to(dev), lens)
    assert torch.equal(D.resample_audio_batch(packed, down, up)[0], flat)


def test_gain_and_clip(dev):
    """4. a +-1 square wave overshoots: clip=True is np.clip of the oracle; per-utterance gains scale before the clip.  With a gain g the bound scales
    by g and the product adds one rounding: half an ulp of the result, 2^-24 below 1 (all that survives the clip), 2^-23 for values in [2, 4)."""
    up, down = 441, 320
    sq = np.where((np.arange(700) // 25) % 2 == 0, 1.0, -1.0).astype(np.float32)
    want = ao.resample(sq, up, down)
    assert want.max() > 1.05                                                   # the overshoot is there
    bound = ao.bound(up, down, 1.0)
    got = _resample(sq, up, down, dev, clip=True)
    assert np.abs(got).max() <= 1.0 and np.abs(got - np.clip(want, -1, 1)).max() <= bound
    gains = [0.5, 2.0]
    flat, lens = D.resample_audio_batch([torch.from_numpy(sq).to(dev)] * 2, 320, 441, gains=gains, clip=True)
    flat = flat.cpu().numpy()
    for u, g in enumerate(gains):
        assert np.abs(flat[u * lens[0]:(u + 1) * lens[0]] - np.clip(g * want, -1, 1)).max() <= g * bound + U24
    assert np.abs(flat[:lens[0]]).max() < 0.7 and np.abs(flat[lens[0]:]).max() == 1.0
    unclipped = D.resample_audio_batch([torch.from_numpy(sq).to(dev)], 320, 441, gains=torch.tensor([2.0]))[0].cpu().numpy()
    assert np.abs(unclipped - 2.0 * want).max() <= 2.0 * bound + 2 * U24


def test_level_kernel(dev):
    """5. max frame RMS within 2048 2^-24 (relative; any f32 summation order over a frame), max |x| exact, the two gain cases"""
    rng = np.random.default_rng(5)
    lens = [1, 511, 512, 513, 2047, 2048, 2049, 5000, 0]
    sigs = [(rng.standard_normal(n) * 0.05).astype(np.float32) for n in lens]
    sigs[7][1234] = 0.9                                                          # a full-scale spike in near-silence
    sigs[7][:1000] *= 0.01
    level, gains = D.volume_levels([torch.from_numpy(s).to(dev) for s in sigs])
    level, gains = level.cpu().numpy(), gains.cpu().numpy()
    rtol = 2048 * U24
    for u, s in enumerate(sigs):
        rms, peak = ao.levels(s)
        assert abs(level[u, 0] - rms) <= rtol * rms + 1e-30, (lens[u], level[u, 0], rms)
        assert level[u, 1] == np.float32(peak)
        want = ao.volume_gain(s) if len(s) else 20.0
        assert abs(gains[u] - want) <= (rtol + 4 * U24) * want, (lens[u], gains[u], want)
    rms5, peak5 = ao.levels(sigs[5])
    assert 0.2 / (rms5 + 0.01) * peak5 <= 1.0 and abs(gains[5] - 0.2 / (rms5 + 0.01)) <= (rtol + 4 * U24) * gains[5]     # quiet: the RMS rule
    rms7, peak7 = ao.levels(sigs[7])
    assert 0.2 / (rms7 + 0.01) * peak7 > 1.0 and abs(gains[7] - 1.0 / 0.9) <= 2 * U24 * gains[7]                         # peak: 1 / max |x|
    assert torch.equal(D.volume_gains([torch.from_numpy(sigs[7]).to(dev)]).cpu(), torch.from_numpy(gains[7:8]))           # alone = in the batch
    y = D.normalize_volume(sigs[4])
    assert np.abs(y.cpu().numpy() - ao.normalize_volume(sigs[4])).max() <= (rtol + 8 * U24) * np.abs(ao.normalize_volume(sigs[4])).max()


def _noise16k(seed=21, seconds=1.0, channels=None):
    rng = np.random.default_rng(seed)
    shape = (int(16000 * seconds),) if channels is None else (int(16000 * seconds), channels)
    return rng.uniform(-0.3, 0.3, shape).astype(np.float32)


@pytest.mark.parametrize('case', ['plain', 'renormalize', 'slice', 'max_frames', 'stereo', 'at_22050'])
def test_load_audio(dev, case):
    """6. load_audio from an array in memory against the float64 restatement, at the project's mel bar (mean |d| < 1e-4), frame count exact"""
    x, rate = _noise16k(), 16000
    kw = {}
    if case == 'renormalize':
        kw = dict(renormalize_volume=True)
    elif case == 'slice':
        kw = dict(start=1000, end=12345, renormalize_volume=True)
    elif case == 'max_frames':
        kw = dict(max_frames=40)
    elif case == 'stereo':
        x = _noise16k(channels=2)
    elif case == 'at_22050':
        rate, kw = 22050, dict(renormalize_volume=True)
    src = torch.from_numpy(x).to(dev) if case in ('slice', 'stereo') else x          # tensors on the device and host arrays
    got = D.load_audio(src, rate, **kw)
    want = ao.load_audio(x, rate, **kw)
    assert torch.is_tensor(got) and got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.shape[1] == 80
    if case == 'max_frames':
        assert got.shape[0] == 40
    assert float(np.abs(got.cpu().numpy() - want).mean()) < 1e-4


def _batch_recordings(rng):
    from tests.test_pipeline import _recording
    recs = [_recording(rng, 260, 10), _recording(rng, 300, 14, silent=True, context=False), _recording(rng, 250, 9)]
    recs[1]['parallel'] = _recording(rng, 280, 12)
    return recs


def _with_16k_audio(recs, rng, as_oracle, dev=None):
    """the same recordings carrying 16 kHz audio + audio_rate (as_oracle=False) or the oracle's resampled, clipped f32 audio at 22 050 Hz and no rate"""
    out = []
    for r in recs:
        r = dict(r)
        frames = len(r['phonemes'])
        n16 = 256 * frames * 320 // 441 + 1                                         # ceil(n16 441 / 320) // 256 == frames
        a16 = np.clip(rng.standard_normal(n16).astype(np.float32) * 0.4, -1.2, 1.2)
        if as_oracle:
            r['audio'] = np.clip(ao.resample(a16, 441, 320), -1, 1).astype(np.float32)
            assert len(r['audio']) // 256 == frames
        else:
            r['audio'], r['audio_rate'] = a16, 16000
        if dev is not None:
            r['audio'] = torch.from_numpy(r['audio']).to(dev)
        if 'parallel' in r:
            r['parallel'] = _with_16k_audio([r['parallel']], rng, as_oracle, dev)[0]
        out.append(r)
    return out


def _same_batch(a, b, exact_audio):
    assert set(a) == set(b)
    for k in a:
        assert len(a[k]) == len(b[k]), k
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            if torch.is_tensor(x):
                assert torch.is_tensor(y) and x.shape == y.shape and x.dtype == y.dtype, (k, i)
                if k == 'audio_features' and not (exact_audio is True or i in exact_audio):
                    assert float((x - y).abs().mean()) < 1e-4, (k, i)
                else:
                    assert torch.equal(x, y), (k, i)
            elif isinstance(x, np.ndarray):
                assert np.array_equal(x, y), (k, i)
            else:
                assert x == y, (k, i)


def test_device_batch_builder_resamples_stored_audio(dev):
    """7. recordings at 16 kHz with audio_rate=16000 == the same recordings carrying the oracle's 22 050 Hz audio: every length and list identical,
    mel targets within the mel bar; from host arrays and from device tensors; mixed rates keep their order; without audio_rate nothing changes"""
    from silent_speech_amd import pipeline
    from silent_speech_amd.data_utils import FeatureNormalizer
    norm = FeatureNormalizer([np.zeros((2, 80), dtype=np.float32)], share_scale=True)
    norm.feature_means = np.linspace(-6, -3, 80, dtype=np.float32)[None]
    norm.feature_stddevs = np.float32(2.5)
    base = _batch_recordings(np.random.default_rng(17))
    builder = pipeline.DeviceBatchBuilder(dev, mfcc_norm=norm)
    want = builder.build(_with_16k_audio(base, np.random.default_rng(1), True))
    _same_batch(builder.build(_with_16k_audio(base, np.random.default_rng(1), False)), want, ())                    # host arrays: one pinned upload
    _same_batch(builder.build(_with_16k_audio(base, np.random.default_rng(1), False, dev)), want, ())               # device tensors
    # mixed rates: recording 1 (and its twin) stay at 22 050 Hz, in place
    mixed, stored = _with_16k_audio(base, np.random.default_rng(1), False), _with_16k_audio(base, np.random.default_rng(1), True)
    mixed[1] = stored[1]
    _same_batch(builder.build(mixed), want, (1,))
    # no audio_rate: the 22 050 Hz path, bit for bit -- equal to an explicit 22 050 and to the mel launch the builder has always made
    plain = builder.build(base)
    _same_batch(builder.build([dict(r, audio_rate=22050) for r in base]), plain, True)
    src = base + [base[1]['parallel']]
    mel, frames = D.mel_spectrogram_batch([torch.from_numpy(r['audio']).to(dev) for r in src])
    mean, std = pipeline._normalizer_tensors(norm, 80, dev)
    pipeline._soft_clip(mel, mel, 80, mean, std, 1.0, 0.0)
    for i, k in enumerate((0, 3, 2)):
        n = plain['audio_feature_lengths'][i]
        assert n <= frames[k] and torch.equal(plain['audio_features'][i], mel[k, :n])


def test_errors(dev):
    """8. unsupported ratios and bad rates are ValueErrors, a filename is refused with the documented message, the C entries check their pointers"""
    x = np.zeros(100, dtype=np.float32)
    with pytest.raises(ValueError, match='not supported'):
        D.resample_audio(x, 16000, 22051)
    with pytest.raises(ValueError, match='not supported'):
        D.resample_audio_batch([x], 11025, 16000)                   # 640/441: a 15 360-float table
    for bad in (0, -16000, 22050.5):
        with pytest.raises(ValueError, match='positive integers'):
            D.resample_audio(x, bad, 22050)
        with pytest.raises(ValueError, match='positive integers'):
            D.resample_audio(x, 16000, bad)
    with pytest.raises(TypeError, match='decoding an audio file is out of scope'):
        D.load_audio('utterance.flac', 16000)
    lib = _lib.lib()
    assert not lib.ss_audio_resample_supported(640, 441, 6400, 24) and lib.ss_audio_resample_supported(441, 320, 4410, 24)
    rc = lib.ss_audio_resample_batch(None, None, None, 1, 441, 320, 4410, 24, None, None, 0, 10, None)
    assert rc != 0 and b'ss_audio_resample_batch: null pointer' in lib.ss_last_error()
    t = torch.zeros(16, dtype=torch.float32, device=dev)
    tab = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    rc = lib.ss_audio_resample_batch(_lib.ptr(t), _lib.ptr(t), _lib.ptr(tab), 1, 640, 441, 6400, 24, _lib.ptr(t), None, 0, 0, None)
    assert rc != 0 and b'not supported' in lib.ss_last_error()
    rc = lib.ss_audio_resample_batch(_lib.ptr(t), _lib.ptr(t), _lib.ptr(tab), 0, 441, 320, 4410, 24, _lib.ptr(t), None, 0, 0, None)
    assert rc != 0 and b'bad sizes' in lib.ss_last_error()
    rc = lib.ss_audio_level_batch(None, None, 1, 0, None, 0, None, None, None)
    assert rc != 0 and b'ss_audio_level_batch: null pointer' in lib.ss_last_error()
    rc = lib.ss_audio_level_batch(_lib.ptr(t), _lib.ptr(tab), 1, 4, _lib.ptr(t), 7, _lib.ptr(t), None, None)
    assert rc != 0 and b'workspace too small' in lib.ss_last_error()


def test_ops_are_registered_with_fakes(dev):
    from silent_speech_amd import torch_ops
    assert 'audio_resample' in torch_ops.OPS and 'audio_level' in torch_ops.OPS
    assert 'Tensor(a1!) out' in str(torch.ops.silent_speech.audio_resample.default._schema)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        level, gains = torch.ops.silent_speech.audio_level(torch.empty(100), torch.empty((3, 3), dtype=torch.int64), 3)
        assert tuple(level.shape) == (3, 2) and tuple(gains.shape) == (3,) and gains.dtype == torch.float32


def test_save_output_at_16_khz(dev, tmp_path, monkeypatch):
    """9. save_output(..., sampling_rate=16000): the vocoder's output resampled on the device -- ceil(L 320 / 441) samples within the 320/441 bound"""
    from silent_speech_amd import transduction_model as tm
    from silent_speech_amd.architecture import Model
    from silent_speech_amd.data_utils import FeatureNormalizer
    from tests import hifigan_oracle as ho
    from tests.test_vocoder import _vocoder
    torch.manual_seed(0)
    model = Model(112, 80, 48, model_size=16, num_layers=1, dropout=0.0, compute_dtype=torch.float32).to(dev)
    n_frames = 8
    g = torch.Generator().manual_seed(2)
    dp = dict(raw_emg=50.0 * torch.tanh(torch.randn(8 * n_frames, 8, generator=g) * 0.1), emg=torch.zeros(n_frames, 112),
              session_ids=torch.zeros(n_frames, dtype=torch.long))
    norm = FeatureNormalizer([np.random.default_rng(0).standard_normal((50, 80)).astype(np.float32) * 2.0 + 0.5])
    voc = _vocoder('S3', dev, 'bf16x3')
    L = n_frames * ho.hop(ho.CONFIGS['S3'])
    seen, predict, written, write = [], tm.predict_utterance, [], tm.write_wav
    monkeypatch.setattr(tm, 'predict_utterance', lambda *a: seen.append(predict(*a)) or seen[-1])
    monkeypatch.setattr(tm, 'write_wav', lambda f, a, sr=22050: written.append(np.asarray(a)) or write(f, a, sr))
    path = str(tmp_path / 'out16.wav')
    tm.save_output(model, dp, path, dev, norm, voc, sampling_rate=16000)
    mel = seen[0] * torch.from_numpy(norm.feature_stddevs).float().to(dev) + torch.from_numpy(norm.feature_means).float().to(dev)
    audio = voc(mel).cpu().numpy().astype(np.float64).reshape(-1)
    want = ao.resample(audio, 320, 441)
    assert len(audio) == L and want.shape == (ao.out_length(L, 320, 441),)
    with wave.open(path, 'rb') as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 16000, len(want))
    assert written[0].shape == want.shape and np.abs(written[0] - want).max() <= ao.bound(320, 441, np.abs(audio).max())
    if is_emu(dev):                                            # the batched path doubles the model / vocoder work: on the GPU tier only
        return
    tm.save_outputs(model, [dp, dp], [str(tmp_path / 'a.wav'), str(tmp_path / 'b.wav')], dev, norm, voc, sampling_rate=16000)
    for k, name in ((1, 'a.wav'), (2, 'b.wav')):               # the batched model / vocoder path has its own tests: here the rate, the length, the same signal
        with wave.open(str(tmp_path / name), 'rb') as f:
            assert (f.getframerate(), f.getnframes()) == (16000, len(want))
        assert written[k].shape == want.shape and np.abs(written[k] - written[0]).max() < 1e-3
