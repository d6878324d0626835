"""HiFi-GAN generator on the device (silent_speech_amd/vocoder.py, csrc/vocoder.hip) against the float64 torch oracle of
tests/hifigan_oracle.py.

Tolerance, from the oracle alone: for a configuration and an arithmetic mode, e_max / e_mean are the max / mean of
|oracle_f32(operands rounded like the kernel's) - oracle_f64| at the configuration's longest length; the kernel passes at every length when
its max error against oracle_f64 is <= 4 e_max + 2e-6 and its mean error <= 4 e_mean + 5e-7.  (4 x: the emulation shares the dominant error,
operand rounding, with the kernel but accumulates in torch's order and keeps the lo * lo term the kernel drops; the max over a few hundred
samples fluctuates.)  A wrong tap, edge, slope or average moves the output by 0.1 - 1."""
import functools
import json
import os
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import hifigan_oracle as ho
from tests.backend import dev, is_emu  # noqa: F401

LENGTHS = {'S1': [1, 37], 'S2': [1, 23], 'S3': [70], 'V1': [3, 12]}
ROUNDING = {'bf16': ho.round_bf16, 'bf16x3': ho.round_bf16x2}
SEED = 0


@functools.lru_cache(maxsize=None)
def _generator(name, T=None):
    """The seeded weights of a configuration, conv_post scaled on the seeded mel of T frames (default: the configuration's longest length)."""
    return ho.random_generator(ho.CONFIGS[name], SEED, T or max(LENGTHS[name]))


@functools.lru_cache(maxsize=None)
def _oracle(name, T):
    """float64 audio of the seeded mel of T frames; also checks that the signal neither vanished nor saturated."""
    cfg = ho.CONFIGS[name]
    return ho.forward(cfg, _generator(name, T), ho.random_mel(cfg, SEED, T))


def _check_signal(y):
    rms = float(y.pow(2).mean().sqrt())
    assert 0.2 <= rms <= 0.6, 'oracle audio rms %g outside [0.2, 0.6]' % rms
    assert float((y.abs() > 0.99).double().mean()) < 0.01, 'oracle audio saturates'


@functools.lru_cache(maxsize=None)
def _tolerance(name, mode):
    cfg, T = ho.CONFIGS[name], max(LENGTHS[name])
    emu = ho.forward(cfg, _generator(name), ho.random_mel(cfg, SEED, T), rounding=ROUNDING[mode], dtype=torch.float32).double()
    err = (emu - _oracle(name, T)).abs()
    return float(err.max()), float(err.mean())


def _assert_within(got, want, e_max, e_mean, what):
    err = (got.detach().cpu().double() - want).abs()
    mx, mn = float(err.max()), float(err.mean())
    print('%s: max err %.3e (bound %.3e), mean err %.3e (bound %.3e)' % (what, mx, 4 * e_max + 2e-6, mn, 4 * e_mean + 5e-7))
    assert mx <= 4 * e_max + 2e-6, '%s: max error %g > 4 * %g + 2e-6' % (what, mx, e_max)
    assert mn <= 4 * e_mean + 5e-7, '%s: mean error %g > 4 * %g + 5e-7' % (what, mn, e_mean)


def _vocoder(name, dev, mode, T=None):
    from silent_speech_amd.vocoder import Vocoder
    return Vocoder(dev, config=ho.CONFIGS[name], state_dict=_generator(name, T), matmul=mode)


def _run_case(name, T, mode, dev):
    cfg = ho.CONFIGS[name]
    want = _oracle(name, T)
    _check_signal(want)
    got = _vocoder(name, dev, mode, T)(ho.random_mel(cfg, SEED, T).float().to(dev))
    assert got.shape == (T * ho.hop(cfg),) and got.dtype == torch.float32 and got.device.type == dev.type
    _assert_within(got, want, *_tolerance(name, mode), what='%s T=%d %s' % (name, T, mode))


SMALL = [(n, T) for n in ('S1', 'S2', 'S3') for T in LENGTHS[n]]


@pytest.mark.parametrize('mode', ['bf16x3', 'bf16'])
@pytest.mark.parametrize('name,T', SMALL)
def test_generator_matches_oracle(dev, name, T, mode):
    _run_case(name, T, mode, dev)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['bf16x3', 'bf16'])
@pytest.mark.parametrize('T', LENGTHS['V1'])
def test_v1_generator_matches_oracle(T, mode):
    from silent_speech_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), 'gpu-marked test needs an MI355X'
    _run_case('V1', T, mode, torch.device('cuda'))


# ------------------------------------------------------------------------------------------------ component ops
def _rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _component_bounds(ref_fn, x, w):
    """ref_fn(x, w, dtype) -> output; (want_f64, {mode: (e_max, e_mean)})"""
    want = ref_fn(x, w, torch.float64)
    tol = {}
    for mode, rnd in ROUNDING.items():
        err = (ref_fn(rnd(x), rnd(w), torch.float32).double() - want).abs()
        tol[mode] = (float(err.max()), float(err.mean()))
    return want, tol


CONV_CASES = [  # c_in, c_out, k, d, L, slope, residual
    (32, 32, 11, 5, 7, 0.1, False),       # shorter than the 25-step halo
    (32, 32, 11, 5, 130, 0.1, True),
    (80, 64, 7, 1, 37, 1.0, False),       # conv_pre: K = 80 * 7, no activation
]
CONVT_CASES = [(64, 32, 16, 8, 5), (32, 16, 4, 2, 33)]   # c_in, c_out, k, u, L


def _conv_case(case, seed=3):
    c_in, c_out, k, d, L, slope, with_res = case
    g = torch.Generator().manual_seed(seed)
    x, w, b = _rand(g, L, c_in), _rand(g, c_out, c_in, k, scale=(c_in * k) ** -0.5), _rand(g, c_out, scale=0.05)
    res = _rand(g, L, c_out) if with_res else None

    def ref(xx, ww, dtype):
        # leaky_relu commutes with the operand rounding for slope 1; for slope 0.1 the kernel rounds AFTER the activation, like the generator oracle
        y = F.conv1d(xx.to(dtype).T[None], ww.to(dtype), b.to(dtype), dilation=d, padding=(k - 1) * d // 2)[0].T
        return y + res.to(dtype) if with_res else y
    act = F.leaky_relu(x, slope)
    want, tol = _component_bounds(ref, act, w)
    return x, w, b, res, want, tol


def _convt_case(case, seed=4):
    c_in, c_out, k, u, L = case
    g = torch.Generator().manual_seed(seed)
    x, w, b = _rand(g, L, c_in), _rand(g, c_in, c_out, k, scale=(u / (c_in * k)) ** 0.5), _rand(g, c_out, scale=0.05)

    def ref(xx, ww, dtype):
        return F.conv_transpose1d(xx.to(dtype).T[None], ww.to(dtype), b.to(dtype), stride=u, padding=(k - u) // 2)[0].T
    want, tol = _component_bounds(ref, F.leaky_relu(x, 0.1), w)
    return x, w, b, want, tol


@pytest.mark.parametrize('mode', ['bf16x3', 'bf16'])
@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: 'c%dto%d_k%d_d%d_L%d' % c[:5])
def test_vocoder_conv1d_op(dev, case, mode):
    from silent_speech_amd import vocoder
    c_in, c_out, k, d, L, slope, with_res = case
    x, w, b, res, want, tol = _conv_case(case)
    got = torch.ops.silent_speech.vocoder_conv1d(x.float().to(dev), vocoder.conv_blob(w, b).to(dev), c_out, k, d, slope,
                                                 res.float().to(dev) if with_res else None, mode == 'bf16x3')
    assert got.shape == (L, c_out)
    _assert_within(got, want, *tol[mode], what='conv1d %s %s' % (case, mode))


@pytest.mark.parametrize('mode', ['bf16x3', 'bf16'])
@pytest.mark.parametrize('case', CONVT_CASES, ids=lambda c: 'c%dto%d_k%d_u%d_L%d' % c)
def test_vocoder_conv_transpose1d_op(dev, case, mode):
    from silent_speech_amd import vocoder
    c_in, c_out, k, u, L = case
    x, w, b, want, tol = _convt_case(case)
    got = torch.ops.silent_speech.vocoder_conv_transpose1d(x.float().to(dev), vocoder.conv_transpose_blob(w, b, u).to(dev), c_out, k, u, 0.1,
                                                           mode == 'bf16x3')
    assert got.shape == (L * u, c_out)
    _assert_within(got, want, *tol[mode], what='conv_transpose1d %s %s' % (case, mode))


def test_vocoder_ops_pass_opcheck(dev):
    from silent_speech_amd import torch_ops, vocoder  # noqa: F401
    utils = ('test_schema', 'test_faketensor')
    for case in CONV_CASES:
        c_in, c_out, k, d, L, slope, with_res = case
        x, w, b, res, _, _ = _conv_case(case)
        args = (x.float().to(dev), vocoder.conv_blob(w, b).to(dev), c_out, k, d, slope, res.float().to(dev) if with_res else None, True)
        torch.library.opcheck(torch.ops.silent_speech.vocoder_conv1d.default, args, test_utils=utils)
    for case in CONVT_CASES:
        c_in, c_out, k, u, L = case
        x, w, b, _, _ = _convt_case(case)
        args = (x.float().to(dev), vocoder.conv_transpose_blob(w, b, u).to(dev), c_out, k, u, 0.1, True)
        torch.library.opcheck(torch.ops.silent_speech.vocoder_conv_transpose1d.default, args, test_utils=utils)
    g = torch.Generator().manual_seed(6)
    x, w, b = _rand(g, 37, 16), _rand(g, 1, 16, 7, scale=0.1), _rand(g, 1, scale=0.05)
    args = (x.float().to(dev), vocoder.tail_weights(w, b).to(dev), 7, 0.01)
    torch.library.opcheck(torch.ops.silent_speech.vocoder_tail.default, args, test_utils=utils)
    got = torch.ops.silent_speech.vocoder_tail(*args)
    want = torch.tanh(F.conv1d(F.leaky_relu(x, 0.01).T[None], w, b, padding=3)).reshape(-1)
    assert float((got.cpu().double() - want).abs().max()) < 2e-6          # exact-f32 kernel: f32 rounding of x, w and a 112-term sum of O(1) terms


# ------------------------------------------------------------------------------------------------ ragged batch
@pytest.mark.parametrize('mode', ['bf16x3', 'bf16'])
def test_batch_keeps_utterances_apart(dev, mode):
    """Packed utterances of 5, 37 and 1 frames: each equals the oracle of that utterance ALONE (own zero edges, nothing leaks across)."""
    cfg, sd = ho.CONFIGS['S1'], _generator('S1')
    _check_signal(_oracle('S1', 37))
    g = torch.Generator().manual_seed(11)
    mels = [torch.randn(T, 80, generator=g, dtype=torch.float64) for T in (5, 37, 1)]
    outs = _vocoder('S1', dev, mode).batch([m.float().to(dev) for m in mels])
    assert len(outs) == 3
    for m, got in zip(mels, outs):
        assert got.shape == (m.shape[0] * ho.hop(cfg),)
        _assert_within(got, ho.forward(cfg, sd, m), *_tolerance('S1', mode), what='batch T=%d %s' % (m.shape[0], mode))


# ------------------------------------------------------------------------------------------------ checkpoint forms
def test_checkpoint_forms(dev, tmp_path):
    from silent_speech_amd.vocoder import Vocoder
    cfg, sd = ho.CONFIGS['S3'], _generator('S3')
    T = 9
    mel = ho.random_mel(cfg, SEED, T)
    normed = ho.weight_normed(sd, SEED)
    assert any(k.endswith('.weight_g') for k in normed) and not any(k.endswith('.weight') for k in normed)
    d1, d2 = tmp_path / 'wn', tmp_path / 'plain'
    for d, state in ((d1, normed), (d2, sd)):
        d.mkdir()
        torch.save({'generator': {k: v.float() if d is d2 else v for k, v in state.items()}}, str(d / 'g_00000001'))
        with open(str(d / 'config.json'), 'w') as f:
            json.dump(cfg, f)
    v1 = Vocoder(dev, checkpoint_file=str(d1 / 'g_00000001'))
    assert v1.matmul == 'bf16x3'
    got = v1(mel.float().to(dev))
    _assert_within(got, ho.forward(cfg, sd, mel), *_tolerance('S3', 'bf16x3'), what='weight-normed checkpoint')
    got_plain = Vocoder(dev, checkpoint_file=str(d2 / 'g_00000001'))(mel.float().to(dev))
    assert torch.equal(got, got_plain)
    # through the flags shim, like the reference's Vocoder(device)
    from silent_speech_amd.flags import FLAGS
    FLAGS.hifigan_checkpoint = str(d2 / 'g_00000001')
    try:
        assert torch.equal(Vocoder(dev)(mel.float().to(dev)), got)
    finally:
        FLAGS._over.pop('hifigan_checkpoint', None)
    bad = dict(cfg, upsample_kernel_sizes=[5, 4])
    with pytest.raises(ValueError):
        Vocoder(dev, config=bad, state_dict=sd)


# ------------------------------------------------------------------------------------------------ save_output
def test_save_output_writes_the_vocoded_wav(dev, tmp_path, monkeypatch):
    from silent_speech_amd import transduction_model as tm
    from silent_speech_amd.architecture import Model
    from silent_speech_amd.data_utils import FeatureNormalizer
    torch.manual_seed(0)
    model = Model(112, 80, 48, model_size=16, num_layers=1, dropout=0.0, compute_dtype=torch.float32).to(dev)
    T = 8
    g = torch.Generator().manual_seed(2)
    dp = dict(raw_emg=50.0 * torch.tanh(torch.randn(8 * T, 8, generator=g) * 0.1), emg=torch.zeros(T, 112), session_ids=torch.zeros(T, dtype=torch.long))
    norm = FeatureNormalizer([np.random.default_rng(0).standard_normal((50, 80)).astype(np.float32) * 2.0 + 0.5])
    voc = _vocoder('S3', dev, 'bf16x3')
    hop = ho.hop(ho.CONFIGS['S3'])
    model.train()                        # the state the reference's save_output does NOT restore (it always leaves train mode); eval is the trivial one
    path = str(tmp_path / 'out.wav')
    seen, predict = [], tm.predict_utterance
    monkeypatch.setattr(tm, 'predict_utterance', lambda *a: seen.append(predict(*a)) or seen[-1])      # the model's forward is the slow part: keep its result
    tm.save_output(model, dp, path, dev, norm, voc)
    assert model.training and len(seen) == 1 and seen[0].shape == (T, 80)
    with wave.open(path, 'rb') as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 22050, T * hop)
        pcm = np.frombuffer(f.readframes(f.getnframes()), dtype='<i2')
    mel = seen[0] * torch.from_numpy(norm.feature_stddevs).float().to(dev) + torch.from_numpy(norm.feature_means).float().to(dev)
    audio = voc(mel).cpu().numpy().astype(np.float64)
    assert np.array_equal(pcm, np.rint(32767.0 * np.clip(audio, -1.0, 1.0)).astype(np.int16))
    assert pcm.std() > 0
