"""Whole-utterance inference as ragged batches: N utterances of different lengths through ONE plan call (Model.forward_utterances,
torch.ops.silent_speech.model_forward_ragged), each equal to the eval-mode forward of that utterance ALONE -- the oracle everywhere is
model_ref.model_forward(sd, raw[None], training=False) per utterance, with the project's whole-utterance error bars.  A zero-padded batch
without the length masks misses those bars by three orders of magnitude (padding leaks through the right tap of every stride-1 convolution
and through every in-band padded key)."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import model_ref
from silent_speech_amd import recognition_model as rm
from silent_speech_amd import torch_ops
from silent_speech_amd import transduction_model as tm
from silent_speech_amd.architecture import Model
from tests.backend import dev, is_emu  # noqa: F401
from tests.util import assert_close_robust

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
SHORT = [53, 17, 16, 8]                       # emulator tier: ~10 s per plan call + ~0.1 s per frame
FULL = [230, 121, 53, 17, 16, 8]              # + out-of-band keys (230 > 199) and a length (121) that ends inside other queries' bands
LONG = [1003, 640, 333, 200, 199, 24]


def _raw(T, seed):
    g = torch.Generator().manual_seed(seed)
    return 50.0 * torch.tanh(torch.randn(8 * T, 8, generator=g) * 5.0 / 50.0)


def _raws(lengths):
    return [_raw(T, 10 + i) for i, T in enumerate(lengths)]


def _datapoint(raw):
    T = raw.shape[0] // 8
    return dict(raw_emg=raw, emg=torch.zeros(T, 112), session_ids=torch.zeros(T, dtype=torch.long), silent=False)


def _tiny_sd(seed_shift=0.0):
    z = np.load(os.path.join(GOLD, 'model_d16_L1_train_r3_T40.npz'))
    sd = {k[3:]: torch.from_numpy(z[k]).clone() for k in z.files if k.startswith('sd/')}
    if seed_shift:
        g = torch.Generator().manual_seed(5)
        for k in sd:
            if sd[k].dtype == torch.float32 and 'running_var' not in k and 'relative_positional' not in k:
                sd[k] = sd[k] + seed_shift * torch.randn(sd[k].shape, generator=g)
    return sd


def _model(dev, seed_shift=0.0, **kw):
    sd = _tiny_sd(seed_shift)
    kw.setdefault('compute_dtype', torch.float32)
    m = Model(112, 80, 48, model_size=16, num_layers=1, dropout=0.0, **kw)
    m.load_state_dict(sd, strict=True)
    return m.to(dev), sd


_ORACLE = {}


def _oracle(tag, sd, lengths):
    """Every utterance alone through the oracle; computed once per (weights, lengths) and shared, never modified."""
    key = (tag, tuple(lengths))
    if key not in _ORACLE:
        outs = []
        for raw in _raws(lengths):
            with torch.no_grad():
                o = model_ref.model_forward(sd, raw[None].clone(), training=False)
            outs.append(tuple(t[0] for t in o) if isinstance(o, tuple) else (o[0],))
        _ORACLE[key] = outs
    return _ORACLE[key]


def _check_each(preds, auxs, want, lengths, tol, frac=0):
    assert len(preds) == len(lengths) and (auxs is None or len(auxs) == len(lengths))
    for i, T in enumerate(lengths):                       # input order: utterance i has its own length and its own values
        assert tuple(preds[i].shape) == (T, want[i][0].shape[1])
        print('utterance %d (T=%d): pred err/scale %.3e' % (i, T, assert_close_robust(preds[i], want[i][0], tol, name='pred[%d] T=%d' % (i, T), max_outlier_frac=frac)))
        if auxs is not None:
            assert tuple(auxs[i].shape) == (T, want[i][1].shape[1])
            print('utterance %d (T=%d): aux err/scale %.3e' % (i, T, assert_close_robust(auxs[i], want[i][1], tol, name='aux[%d] T=%d' % (i, T), max_outlier_frac=frac)))


# ---------------------------------------------------------------------------------------------- 1. each utterance equals itself alone
def test_each_utterance_equals_itself_alone(dev):
    lengths = SHORT if is_emu(dev) else FULL
    m, sd = _model(dev)
    m.eval()
    preds, auxs = m.forward_utterances([r.to(dev) for r in _raws(lengths)])
    assert not m.training
    _check_each(preds, auxs, _oracle('tiny', sd, lengths), lengths, 2e-4)
    m.train()
    out = tm.predict_utterances(m, [_datapoint(r) for r in _raws(lengths)], dev)
    assert m.training                                      # returned to the mode it was in
    _check_each(out, None, _oracle('tiny', sd, lengths), lengths, 2e-4)


# ---------------------------------------------------------------------------------------------- 2. arithmetic modes
@pytest.mark.gpu
@pytest.mark.parametrize('kw,tol,frac', [(dict(compute_dtype=torch.float32), 2e-4, 0), (dict(compute_dtype=torch.float32, f32_matmul='bf16x3'), 2e-4, 0),
                                         (dict(compute_dtype=torch.bfloat16), 8e-2, 1e-3)], ids=['f32', 'bf16x3', 'bf16'])
def test_arithmetic_modes_gpu(kw, tol, frac):
    from silent_speech_amd import _lib
    _lib.load()
    m, sd = _model('cuda', **kw)
    m.eval()
    preds, auxs = m.forward_utterances([r.to('cuda') for r in _raws(FULL)])
    _check_each(preds, auxs, _oracle('tiny', sd, FULL), FULL, tol, frac)


WIDE = [230, 121, 16, 5]


@pytest.mark.gpu
@pytest.mark.parametrize('kw,tol,frac', [(dict(compute_dtype=torch.float32), 2e-4, 0), (dict(compute_dtype=torch.float32, f32_matmul='bf16x3'), 2e-4, 0),
                                         (dict(compute_dtype=torch.bfloat16), 8e-2, 1e-3)], ids=['f32', 'bf16x3', 'bf16'])
def test_product_width_gpu(kw, tol, frac):
    """The product's width, one layer: d_head 96 runs attn_fwd_ragged_kernel<.., 3> inside the plan, and C = 768 puts every BatchNorm apply of the first
    ResBlock (4 x 922 rows of 96 chunks > 768 x 256 threads) on the multi-trip RowWalk form, across slot boundaries."""
    from silent_speech_amd import _lib
    _lib.load()
    sd = model_ref.init_state_dict(d_model=768, num_layers=1, seed=4)
    m = Model(112, 80, 48, model_size=768, num_layers=1, dropout=0.0, **kw)
    m.load_state_dict(sd, strict=True)
    m.to('cuda').eval()
    preds, auxs = m.forward_utterances([r.to('cuda') for r in _raws(WIDE)])
    _check_each(preds, auxs, _oracle('d768', sd, WIDE), WIDE, tol, frac)


# ---------------------------------------------------------------------------------------------- 2b. recycled workspace
def test_valid_rows_do_not_depend_on_what_the_workspace_held(dev, monkeypatch):
    """engine.forward_ragged takes its workspace from torch.empty, i.e. recycled memory.  Here it arrives filled with 0xFF bytes -- NaN as f32 and as bf16:
    every row the plan does not store (attention output rows behind an utterance's end, and what the row-wise kernels make of them) is then
    non-finite, and the valid rows still meet the bar only because K rows, V^T fragments and BatchNorm inputs behind the end are discarded by select,
    never multiplied by 0."""
    lengths = [17, 9, 16] if is_emu(dev) else FULL
    m, sd = _model(dev)
    m.eval()
    raws = [r.to(dev) for r in _raws(lengths)]
    filled = []
    real_empty = torch.empty
    with monkeypatch.context() as mp:
        def poisoned_empty(*a, **k):
            t = real_empty(*a, **k)
            if k.get('dtype') is torch.uint8:
                t.fill_(0xFF)
                filled.append(t.numel())
            return t
        mp.setattr(torch, 'empty', poisoned_empty)
        preds, auxs = m.forward_utterances(raws)
    assert torch.empty is real_empty
    assert filled and max(filled) > 0                      # the wrapper saw (at least) the workspace
    head = preds[0]._base.float().cpu().view(len(lengths), max(lengths), -1)
    filler = torch.cat([head[b, T:] for b, T in enumerate(lengths)])
    assert filler.shape[0] > 0 and not torch.isfinite(filler).all(), 'the poison never reached a filler row: this run proves nothing'
    _check_each(preds, auxs, _oracle('tiny', sd, lengths), lengths, 2e-4)


# ---------------------------------------------------------------------------------------------- 3. long utterances through the grouper
@pytest.mark.gpu
@pytest.mark.parametrize('dt,tol', [(torch.float32, 3e-4), (torch.bfloat16, 8e-2)])
def test_long_utterances_through_the_grouper_gpu(dt, tol):
    from silent_speech_amd import _lib
    _lib.load()
    groups = tm.plan_ragged_groups(LONG, 1400, 0.25)
    assert len(groups) >= 2 and sorted(i for g in groups for i in g) == list(range(len(LONG)))
    sd = model_ref.init_state_dict(d_model=64, num_layers=2, seed=3)
    m = Model(112, 80, 48, model_size=64, num_layers=2, dropout=0.0, compute_dtype=dt)
    m.load_state_dict(sd, strict=True)
    m.to('cuda')
    out = tm.predict_utterances(m, [_datapoint(r) for r in _raws(LONG)], 'cuda', max_slot_frames=1400)
    assert m.training
    _check_each(out, None, _oracle('d64', sd, LONG), LONG, tol, 0 if dt == torch.float32 else 1e-3)


# ---------------------------------------------------------------------------------------------- 4. one utterance
def test_one_utterance_equals_predict_utterance(dev):
    """Same kernel family on both sides (per-tile attention) and no masking in play: the slot is the utterance."""
    m, sd = _model(dev)
    raw = _raw(17, 10)
    want = tm.predict_utterance(m, _datapoint(raw), dev)
    m.eval()
    preds, auxs = m.forward_utterances([raw.to(dev)])
    assert len(preds) == 1 and len(auxs) == 1 and tuple(auxs[0].shape) == (17, 48)
    assert_close_robust(preds[0], want, 1e-5, atol_frac=0, name='one utterance', max_outlier_frac=0)


# ---------------------------------------------------------------------------------------------- 5. recognition model, no aux head
def _recog(dev):
    z = np.load(os.path.join(GOLD, 'recog_d16_L1_T40.npz'))
    sd = {k[3:]: torch.from_numpy(z[k]).clone() for k in z.files if k.startswith('sd/')}
    m = Model(112, 38, model_size=16, num_layers=1, dropout=0.0, compute_dtype=torch.float32)
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval(), sd


def test_recognition_logits_and_argmax_path(dev):
    lengths = SHORT if is_emu(dev) else FULL
    m, sd = _recog(dev)
    logits = m.forward_utterances([r.to(dev) for r in _raws(lengths)])
    assert isinstance(logits, list)                       # no aux head: just the predictions
    want = _oracle('recog', sd, lengths)
    _check_each(logits, None, want, lengths, 2e-4)
    # the per-frame arg-max over the slots (one launch, one read-back) against the oracle's, on every frame whose top-2 margin is decidable
    V = want[0][0].shape[1]
    lse = torch.empty(len(lengths) * max(lengths), dtype=torch.float32, device=dev)
    amax = torch.empty(len(lengths) * max(lengths), dtype=torch.int32, device=dev)
    head = logits[0]._base
    from silent_speech_amd import _lib
    _lib.check(_lib.lib().ss_frame_lse(_lib.ptr(head), head.shape[1], 0, V, head.shape[0], _lib.ptr(lse), _lib.ptr(amax), _lib.stream_of(head)), 'ss_frame_lse')
    path = amax.cpu().numpy().reshape(len(lengths), max(lengths))
    scale = max(float(w[0].abs().max()) for w in want)
    frames = left_out = 0
    classes = set()
    for b, T in enumerate(lengths):
        top2 = want[b][0].topk(2, dim=1).values
        decidable = ((top2[:, 0] - top2[:, 1]) >= 1e-3 * scale).numpy()
        ref = want[b][0].argmax(1).numpy()
        frames += T
        left_out += int((~decidable).sum())
        classes.update(ref.tolist())
        assert np.array_equal(path[b, :T][decidable], ref[decidable]), 'utterance %d' % b
    assert left_out <= 0.02 * frames, (left_out, frames)   # a cap on the ORACLE: the comparison may not be hollowed out by near-ties
    assert len(classes) > 1
    # and the decode built on it collapses each utterance over its own frames only
    decoded = rm.greedy_decode_utterances(logits)
    for b, T in enumerate(lengths):
        assert decoded[b] == rm._collapse(path[b, :T], V - 1)


def test_recognition_test_whole_utterances(dev, monkeypatch):
    from silent_speech_amd.synthetic import SyntheticEMGDataset
    n = 3 if is_emu(dev) else 9
    ds = SyntheticEMGDataset(n, seed=2, min_frames=8, max_frames=24 if is_emu(dev) else 60, silent_fraction=0.0)
    m = Model(ds.num_features, len(ds.text_transform.chars) + 1, model_size=16, num_layers=1, dropout=0.0, compute_dtype=torch.float32).to(dev)
    calls = []
    real = Model.forward_utterances

    def counting(self, raws):
        calls.append(len(raws))
        return real(self, raws)
    monkeypatch.setattr(Model, 'forward_utterances', counting)
    w = rm.test(m, ds, dev, batch_size=4, whole_utterances=True)
    assert isinstance(w, float) and 0.0 <= w < float('inf')
    assert len(calls) == math.ceil(n / 4) and sum(calls) == n and max(calls) <= 4


# ---------------------------------------------------------------------------------------------- 6. ensemble
def test_ensemble_forward_utterances(dev):
    lengths = [24, 9]
    m1, sd1 = _model(dev)
    m2, sd2 = _model(dev, seed_shift=0.02)
    ens = tm.EnsembleModel([m1, m2]).eval()
    ys, ps = ens.forward_utterances([r.to(dev) for r in _raws(lengths)])
    w1, w2 = _oracle('tiny', sd1, lengths), _oracle('tiny+0.02', sd2, lengths)
    want = [(0.5 * (a[0] + b[0]), 0.5 * (a[1] + b[1])) for a, b in zip(w1, w2)]
    _check_each(ys, ps, want, lengths, 2e-4)


# ---------------------------------------------------------------------------------------------- 7. host logic and errors (no device)
def test_plan_ragged_groups_partitions_within_both_caps():
    rng = np.random.default_rng(0)
    assert tm.plan_ragged_groups([]) == []
    assert tm.plan_ragged_groups([5000], 100, 0.0) == [[0]]            # a single utterance is always a valid group
    for trial in range(20):
        lengths = rng.integers(1, 1200, size=int(rng.integers(1, 40))).tolist()
        cap, pad = int(rng.integers(200, 30000)), float(rng.choice([0.0, 0.1, 0.25, 0.5]))
        groups = tm.plan_ragged_groups(lengths, cap, pad)
        assert groups == tm.plan_ragged_groups(list(lengths), cap, pad)                    # deterministic
        assert sorted(i for g in groups for i in g) == list(range(len(lengths)))           # a partition
        for g in groups:
            if len(g) > 1:
                slots = len(g) * max(lengths[i] for i in g)
                assert slots <= cap
                assert (slots - sum(lengths[i] for i in g)) / slots <= pad + 1e-12
    d = tm.plan_ragged_groups(LONG)                                     # the defaults: 22 050 slot frames, a quarter of them filler at the most
    assert sorted(i for g in d for i in g) == list(range(len(LONG)))
    assert tm.plan_ragged_groups([100] * 300) == [list(range(i, min(i + 220, 300))) for i in range(0, 300, 220)]


def test_forward_utterances_refuses_training_mode_and_odd_lengths():
    m = Model(112, 80, 48, model_size=16, num_layers=1, dropout=0.0, compute_dtype=torch.float32)
    m.train()
    with pytest.raises(RuntimeError, match='eval'):
        m.forward_utterances([_raw(8, 1)])
    m.eval()
    with pytest.raises(ValueError, match='multiple of 8'):
        m.forward_utterances([_raw(8, 1), torch.zeros(8 * 5 + 3, 8)])
    assert m.forward_utterances([]) == ([], [])
    assert Model(112, 38, model_size=16, num_layers=1).eval().forward_utterances([]) == []


def test_model_forward_ragged_has_a_fake_implementation():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'model_forward_ragged' in torch_ops.OPS
    m = Model(112, 80, 48, model_size=16, num_layers=1, dropout=0.0, compute_dtype=torch.float32)
    h = torch_ops.model_handle(m)
    with FakeTensorMode():
        out = torch.ops.silent_speech.model_forward_ragged(torch.empty(3, 8 * 21, 8), torch.empty(3, dtype=torch.int32), h)
    assert tuple(out.shape) == (3 * 21, 128) and out.dtype == torch.float32
