"""The 112-d hand-crafted EMG features (data_utils.py:85-136, csrc/emg_features.hip): the numpy restatement and the device kernel vs the
reference's own get_emg_features (tests/golden/emg_features.npz, make_golden_emg_features.py), the ragged batch vs per-recording calls, the
drop-in / dispatcher surface, and DeviceBatchBuilder(emg_features=True) vs load_utterance + EMGDataset.__getitem__ restated per utterance.

Tolerances: the zero-crossing columns are multiples of 1/16 and must agree exactly; every other column within 1e-5 of that column's largest
magnitude (librosa 0.10 forms the RMS power in float32 -- the golden values carry that rounding -- and releases differ in how stft rounds)."""
import os

import numpy as np
import pytest
import torch

from oracle import filter_ref
from silent_speech_amd import data_utils, pipeline, read_emg
from silent_speech_amd.data_utils import FeatureNormalizer
from tests.backend import dev, is_emu  # noqa: F401  (fixture: host emulator on the CPU tier, libsilent_speech_hip.so on the gpu tier)

GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'emg_features.npz'))
TAGS = ('short', 'mid', 'context', 'n16', 'n21', 'n22', 'n4000')
ZP = slice(3, None, 14)                     # the zero-crossing-rate column of every channel


# ------------------------------------------------------------------ numpy restatement of data_utils.get_emg_features (librosa 0.10 semantics)
def features_ref(emg):
    """(n, C) -> (1 + (n - 16) // 6, 14 C) float32, vectorised over frames and channels."""
    emg = np.asarray(emg, dtype=np.float64)
    n, C = emg.shape
    F = 1 + (n - 16) // 6
    xs = emg - emg.mean(axis=0, keepdims=True)
    box = np.ones(9) / 9.0
    idx = 6 * np.arange(F)[:, None] + np.arange(16)[None, :]                 # librosa.util.frame(16, 6): (F, 16) sample indices
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(16) / 16)                 # periodic Hann
    cols = []
    for c in range(C):
        x = xs[:, c]
        w = np.convolve(np.convolve(x, box, 'same'), box, 'same')
        p = x - w
        r = np.abs(p)
        W, P, Rf, X = w[idx], p[idx], r[idx], x[idx]
        s = np.signbit(np.where(np.abs(P) <= 1e-10, 0.0, P))
        z = (s[:, 1:] != s[:, :-1]).sum(1) / 16.0
        cols.append(np.stack([W.mean(1), np.sqrt((W ** 2).mean(1)), np.sqrt((Rf ** 2).mean(1)), z, Rf.mean(1)], 1))
        cols.append(np.abs(np.fft.rfft(win[None] * X, axis=1)))
    return np.concatenate(cols, 1).astype(np.float32)


def _check_golden(got, want):
    assert got.shape == want.shape and got.dtype == np.float32, (got.shape, want.shape, got.dtype)
    assert np.array_equal(got[:, ZP], want[:, ZP])
    err = np.abs(got.astype(np.float64) - want).max(0)
    scale = np.abs(want).max(0).astype(np.float64)
    bad = err > 1e-5 * scale
    assert not bad.any(), [(int(j), float(err[j]), float(scale[j])) for j in np.nonzero(bad)[0][:8]]


def test_restatement_matches_the_reference():
    for tag in TAGS:
        _check_golden(features_ref(GOLD[tag + '/x']), GOLD[tag + '/features'])
    f = GOLD['n4000/features']
    assert float(np.abs(f[:, 5 * 14:6 * 14]).max()) == 0.0                    # the zeroed column: zero RMS, zero crossings, zero spectrum


# ------------------------------------------------------------------ the device kernel
def test_kernel_matches_the_reference(dev):
    sigs = [torch.from_numpy(GOLD[tag + '/x']).to(dev) for tag in TAGS]
    got = read_emg.emg_features_batch(sigs)                                     # all seven recordings in one launch
    for tag, g in zip(TAGS, got):
        _check_golden(g.cpu().numpy(), GOLD[tag + '/features'])
    for tag in TAGS:                                                            # the drop-in, numpy in / numpy out
        _check_golden(data_utils.get_emg_features(GOLD[tag + '/x']), GOLD[tag + '/features'])


def test_ragged_batch_equals_per_recording_calls(dev):
    rng = np.random.default_rng(5)
    lens = (15, 16, 21, 22, 3997, 40)
    xs = [rng.standard_normal((n, 8)) * 30.0 + rng.uniform(-500, 500, (1, 8)) for n in lens]
    xs[5][:, 2] = 0.0                                                           # a removed channel
    packed = torch.from_numpy(np.concatenate(xs, 0)).to(dev)
    offs = np.concatenate([[0], np.cumsum(lens)])
    views = [packed[offs[u]:offs[u + 1]] for u in range(len(lens))]             # back to back in one buffer: read in place
    batch = read_emg.emg_features_batch(views)
    assert [tuple(b.shape) for b in batch] == [(0 if n < 16 else 1 + (n - 16) // 6, 112) for n in lens]
    assert batch[1]._base is batch[4]._base                                     # one packed output buffer
    for u, n in enumerate(lens):
        if n < 16:
            continue
        one = read_emg.emg_features_batch([torch.from_numpy(xs[u]).to(dev)])[0]
        assert torch.equal(batch[u].cpu(), one.cpu()), u
    assert float(batch[5][:, 2 * 14:3 * 14].abs().max()) == 0.0
    _check_golden(batch[4].cpu().numpy(), features_ref(xs[4]))
    # views that are NOT back to back (every other recording) take the copying path and give the same rows
    again = read_emg.emg_features_batch([views[4], views[1]])
    assert torch.equal(again[0].cpu(), batch[4].cpu()) and torch.equal(again[1].cpu(), batch[1].cpu())


def test_drop_in_and_dispatcher_op(dev):
    rng = np.random.default_rng(6)
    x = rng.standard_normal((100, 8)) * 20.0
    y = data_utils.get_emg_features(x)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == (1 + (100 - 16) // 6, 112)
    t = torch.from_numpy(x).to(dev)
    yt = data_utils.get_emg_features(t)
    assert torch.is_tensor(yt) and yt.device == t.device and yt.dtype == torch.float32 and tuple(yt.shape) == y.shape
    assert np.array_equal(yt.cpu().numpy(), y)
    assert tuple(data_utils.get_emg_features(x[:16, :3]).shape) == (1, 42)
    for n in (0, 1, 15):
        with pytest.raises(ValueError):
            data_utils.get_emg_features(x[:n])
    with pytest.raises(NotImplementedError):
        data_utils.get_emg_features(x, debug=True)
    op = torch.ops.silent_speech.emg_features
    assert np.array_equal(op(t).cpu().numpy(), y)
    torch.library.opcheck(op.default, (t,), test_utils=('test_schema', 'test_faketensor'))
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = op(torch.empty(4000, 8, dtype=torch.float64))
        assert tuple(f.shape) == (1 + (4000 - 16) // 6, 112) and f.dtype == torch.float32


# ------------------------------------------------------------------ DeviceBatchBuilder(emg_features=True)
def _recording(rng, n_1k, audio_frames, silent=False, context=True):
    t = np.arange(n_1k + 400) / 1000.0
    walk = np.cumsum(rng.standard_normal((n_1k + 400, 8)), 0) * 2.0
    hum = 40.0 * np.sin(2 * np.pi * 60.0 * t)[:, None] * rng.uniform(0.5, 1.5, 8)[None]
    x = walk + hum + rng.standard_normal((n_1k + 400, 8)) * 30.0
    rec = {'raw_emg': x[200:200 + n_1k].copy(), 'silent': silent, 'session_index': 3,
           'audio': np.clip(rng.standard_normal(256 * audio_frames).astype(np.float32) * 0.4, -1.2, 1.2),
           'text_int': rng.integers(0, 37, 5).astype(np.int64), 'phonemes': rng.integers(0, 48, audio_frames).astype(np.int64)}
    if context:
        rec['raw_emg_before'], rec['raw_emg_after'] = x[:200].copy(), x[200 + n_1k:].copy()
    return rec


def _emg_norm():
    z = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'normalizers.npz'))
    norm = FeatureNormalizer([np.zeros((2, 112), dtype=np.float32)])
    norm.feature_means, norm.feature_stddevs = z['emg_means'], z['emg_stds']
    return norm


def _expected(rec, n, norm, remove_channels=()):
    """load_utterance (read_emg.py:65-83) + EMGDataset.__getitem__ (:230-233) for the `emg` key, restated with the oracle's filters."""
    _, e516 = filter_ref.condition(rec['raw_emg'], rec.get('raw_emg_before'), rec.get('raw_emg_after'))
    for c in remove_channels:
        e516[:, c] = 0
    f = features_ref(e516)[:n]
    if norm is not None:
        f = norm.normalize(f.copy())
        f = 8 * np.tanh(f / 8.)
    return f


def _check_batch(b, recs, norm, remove_channels=()):
    for i, r in enumerate(recs):
        n = b['lengths'][i]
        want = _expected(r, n, norm, remove_channels)
        got = b['emg'][i].cpu().numpy()
        assert got.shape == (n, 112) and float(np.abs(got - want).max()) < 1e-4, (i, float(np.abs(got - want).max()))
        pv = b['parallel_voiced_emg'][i]
        if r['silent']:
            nt = b['audio_feature_lengths'][i]                                  # the twin's own frame count
            want = _expected(r['parallel'], nt, norm, remove_channels)
            got = pv.cpu().numpy()
            assert got.shape == (nt, 112) and float(np.abs(got - want).max()) < 1e-4, (i, float(np.abs(got - want).max()))
        else:
            assert isinstance(pv, np.ndarray) and pv.shape == (1,) and not pv.any()


def _small_batch(rng):
    recs = [_recording(rng, 260, 10), _recording(rng, 300, 14, silent=True, context=False), _recording(rng, 240, 12)]
    recs[1]['parallel'] = _recording(rng, 280, 9)                               # the twin's mel frames (9) truncate its features
    return recs


def test_builder_computes_the_features(dev):
    recs = _small_batch(np.random.default_rng(17))
    norm = _emg_norm()
    b = pipeline.DeviceBatchBuilder(dev, emg_norm=norm, emg_features=True).build(recs)
    _check_batch(b, recs, norm)
    assert b['emg'][0]._base is not None and b['emg'][0]._base is b['parallel_voiced_emg'][1]._base     # one packed buffer
    b = pipeline.DeviceBatchBuilder(dev, emg_features=True).build(recs)         # no emg_norm: the raw features
    _check_batch(b, recs, None)
    b = pipeline.DeviceBatchBuilder(dev, emg_norm=norm, emg_features=True, remove_channels=(2, 5)).build(recs)
    _check_batch(b, recs, norm, (2, 5))
    b = pipeline.DeviceBatchBuilder(dev, emg_features=True, remove_channels=(2, 5)).build(recs)
    for e in (b['emg'][0], b['emg'][2], b['parallel_voiced_emg'][1]):       # a zeroed electrode has all-zero features
        assert float(e[:, 2 * 14:3 * 14].abs().max()) == 0.0 and float(e[:, 5 * 14:6 * 14].abs().max()) == 0.0
        assert float(e[:, 3 * 14:4 * 14].abs().max()) > 0.0


def test_builder_pass_through_and_default(dev):
    rng = np.random.default_rng(18)
    recs = _small_batch(rng)
    norm = _emg_norm()
    b0 = pipeline.DeviceBatchBuilder(dev, emg_norm=norm).build(recs)            # default: zeros, as before
    assert all(float(e.abs().max()) == 0.0 for e in b0['emg'] if e.numel())
    assert isinstance(b0['parallel_voiced_emg'][1], np.ndarray)
    n0 = b0['lengths'][0]
    recs[0]['emg_features'] = np.full((n0 + 3, 112), 2.0, dtype=np.float32)
    recs[1]['parallel']['emg_features'] = np.full((b0['audio_feature_lengths'][1], 112), 3.0, dtype=np.float32)
    b = pipeline.DeviceBatchBuilder(dev, emg_norm=norm, emg_features=True).build(recs)
    mean, std = norm.feature_means.reshape(-1), norm.feature_stddevs.reshape(-1)
    want0 = 8 * np.tanh(((2.0 - mean) / std) / 8.)
    assert np.abs(b['emg'][0].cpu().numpy() - want0[None]).max() < 1e-5 and tuple(b['emg'][0].shape) == (n0, 112)
    want1 = 8 * np.tanh(((3.0 - mean) / std) / 8.)
    assert np.abs(b['parallel_voiced_emg'][1].cpu().numpy() - want1[None]).max() < 1e-5
    want2 = _expected(recs[2], b['lengths'][2], norm)                           # the others are still computed
    assert np.abs(b['emg'][2].cpu().numpy() - want2).max() < 1e-4
    for k in ('raw_emg', 'audio_features', 'phonemes'):                         # nothing else moves
        for i in range(len(recs)):
            assert torch.equal(b[k][i].cpu(), b0[k][i].cpu()), (k, i)


# ------------------------------------------------------------------ the MI355X at the loader's shape
def _loader_batch(rng, n):
    recs = []
    for i in range(n):
        n_1k = int(rng.integers(3000, 6000))
        silent = i % 5 == 1
        recs.append(_recording(rng, n_1k, n_1k * 22050 // 1000 // 256, silent=silent, context=i % 3 != 2))
        if silent:
            m = int(rng.integers(3000, 6000))
            recs[-1]['parallel'] = _recording(rng, m, m * 22050 // 1000 // 256)
    return recs


@pytest.mark.gpu
def test_builder_at_the_loader_shape():
    from silent_speech_amd import _lib
    _lib.load()
    dev = torch.device('cuda')
    recs = _loader_batch(np.random.default_rng(19), 40)
    norm = _emg_norm()
    b = pipeline.DeviceBatchBuilder(dev, emg_norm=norm, emg_features=True, remove_channels=(4,)).build(recs)
    _check_batch(b, recs, norm, (4,))


@pytest.mark.gpu
def test_training_step_runs_from_a_batch_with_features():
    from silent_speech_amd import _lib
    from silent_speech_amd.architecture import Model
    from silent_speech_amd.transduction_model import _pack_batch, dtw_loss
    _lib.load()
    dev = torch.device('cuda')
    rng = np.random.default_rng(2)
    recs = [_recording(rng, 3000, 300), _recording(rng, 3500, 320, silent=True), _recording(rng, 2800, 200)]
    recs[1]['parallel'] = _recording(rng, 3300, 290)
    batch = pipeline.DeviceBatchBuilder(dev, emg_norm=_emg_norm(), emg_features=True).build(recs)
    assert all(float(e.abs().max()) > 0 for e in batch['emg'])
    torch.manual_seed(0)
    m = Model(112, 80, 48, model_size=64, num_layers=1, dropout=0.1).to(dev)
    m.train()
    X, X_raw, sess = _pack_batch(batch, dev)
    assert tuple(X.shape)[-1] == 112 and float(X.abs().max()) > 0
    pred, aux = m(X, X_raw, sess)
    loss, _ = dtw_loss(pred, aux, batch, phoneme_loss_weight=0.5)
    loss.backward()
    assert torch.isfinite(loss).item() and float(m.w_out.weight.grad.abs().max()) > 0
