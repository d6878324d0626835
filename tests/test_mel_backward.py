"""The gradient of the log-mel spectrogram with respect to the audio (csrc/mel_bwd.hip, torch.ops.silent_speech.stft_logmel{,_ragged}{,_backward}),
on the emulator tier and, marked gpu, on the MI355X.

REFERENCE.  torch autograd in float64 on the CPU of a restatement of the forward (_restate: reflect pad, unfold(1024, hop), the f32 Hann window and the f32
Slaney basis of oracle/mel_ref.py, torch.fft.rfft, sqrt(. + 1e-9), log(clamp(., 1e-5))).  test_restatement_is_pinned_to_the_oracle holds its forward to
oracle.mel_ref.mel_spectrogram_ref within 1e-5 absolute on the cases of this file.

TOLERANCE.  No constant.  Per case E_max = max|g - g64| / max|g64| and E_2 = |g - g64| / |g64|; the yardstick is the same restatement evaluated by torch in
float32 on the CPU (e_max, e_2).  The kernel passes when E_max <= 4 e_max + floor and E_2 <= 4 e_2 + floor, floor = the median of that measure over the
cases of this file (the factor 4: tests/test_vocoder.py's convention -- the same roundings in another summation order, and a maximum over few samples
fluctuates).  A wrong tap, fold, weight or gate moves the result by order 1.  Every test prints its figures.

THE CLAMP.  log(clamp) has a kink: (frame, band) pairs whose float64 mel lies within a relative 1e-3 of 1e-5 are undecided and get a ZERO upstream gradient
(at most 1 % of a case's pairs; the clamp cases have at least 10 % of their pairs on each side).

What the f32 error depends on: G[k] = g_mag[k] X[k] / |X[k]| is a unit phasor, so an absolute error d of X[k] (about 1e-7 of the frame's typical |X|, for any
f32 FFT) turns into d / |X[k]| -- a bin that happens to be 400 times smaller than its neighbours carries a 4e-5 error of its own share.  The maximum over a
case's samples therefore fluctuates with the data by a few times, for the kernel and for the yardstick alike and not at the same bins."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle import mel_ref
from silent_speech_amd import _lib, data_utils, torch_ops  # noqa: F401
from tests.backend import dev, is_emu  # noqa: F401

MEL = (1024, 80, 22050)            # n_fft, bands, rate; hop / win / fmin / fmax follow per call
CLAMP = 1e-5


def _mel(y, hop=256, center=False, n_fft=1024, win=1024):
    return data_utils.mel_spectrogram(y, n_fft, 80, 22050, hop, win, 0, 8000, center=center)


def _restate(y, hop, clip=False, log=True):
    """(B, L) -> (B, 80, F) in y's dtype: the forward, restated in torch."""
    dt = y.dtype
    pad = (1024 - hop) // 2
    if clip:
        y = torch.clamp(y, -1.0, 1.0)
    yp = Fn.pad(y.unsqueeze(1), (pad, pad), mode='reflect').squeeze(1)
    fr = yp.unfold(1, 1024, hop)
    w = torch.from_numpy(np.asarray(mel_ref.hann_periodic(1024), dtype=np.float32)).to(dt)
    X = torch.fft.rfft(fr * w, dim=-1)
    mag = torch.sqrt(X.real ** 2 + X.imag ** 2 + 1e-9)
    basis = torch.from_numpy(np.asarray(mel_ref.slaney_mel_basis(22050, 1024, 80, 0, 8000), dtype=np.float32)).to(dt)
    mel = (mag @ basis.T).transpose(1, 2)
    return torch.log(torch.clamp(mel, min=CLAMP)) if log else mel


def _noise(seed, B, L, amp):
    return (amp * np.random.default_rng(seed).standard_normal((B, L))).astype(np.float32)


def _frames(L, hop):
    return 1 + (L + (1024 - hop) // 2 * 2 - 1024) // hop


class Case:
    """One (signals, upstream gradient) pair with its float64 gradient and the float32 yardstick, computed once on the CPU and shared."""

    def __init__(self, name, y, hop=256, clip=False, seed=0, l1_target=None, subset=None):
        self.name, self.y, self.hop, self.clip, self.l1_target, self.subset = name, y, hop, clip, l1_target, subset
        B, L = y.shape
        with torch.no_grad():
            mel64 = _restate(torch.from_numpy(y).double(), hop, clip, log=False)
        undecided = (mel64 - CLAMP).abs() <= 1e-3 * CLAMP
        self.undecided = float(undecided.double().mean())
        self.above = float(((mel64 > CLAMP) & ~undecided).double().mean())
        self.below = float(((mel64 < CLAMP) & ~undecided).double().mean())
        if l1_target is None:
            g = np.random.default_rng(1000 + seed).standard_normal(tuple(mel64.shape)).astype(np.float32)
            g[undecided.numpy()] = 0.0
            self.g = g                                              # d loss / d mel, (B, 80, F) f32
            self.mask = None
        else:                                                       # 45 L1(mel(y^), mel(y)): pairs with |delta| < 1e-4 in float64 get their sign zeroed
            with torch.no_grad():
                d = _restate(torch.from_numpy(y).double(), hop) - _restate(torch.from_numpy(l1_target).double(), hop)
            small = (d.abs() < 1e-4) | undecided
            self.small = float(small.double().mean())
            self.mask = (~small).float()
            self.g = None
        self.g64 = self._grad(torch.float64)
        g32 = self._grad(torch.float32).double()
        self.e_max, self.e_2 = self.errors(g32)

    def loss(self, mel_of, y):
        """The case's scalar loss of the (B, 80, F) log-mel that mel_of(y) returns."""
        m = mel_of(y)
        if self.l1_target is None:
            return (m * torch.from_numpy(self.g).to(device=m.device, dtype=m.dtype)).sum()
        mask = self.mask.to(device=m.device, dtype=m.dtype)
        tgt = mel_of(torch.from_numpy(self.l1_target).to(device=y.device, dtype=y.dtype)).detach()
        return 45 * Fn.l1_loss(m * mask, tgt * mask)

    def _grad(self, dt):
        y = torch.from_numpy(self.y).to(dt).requires_grad_()
        self.loss(lambda t: _restate(t, self.hop, self.clip), y).backward()
        return y.grad.detach()

    def errors(self, g):
        g, ref = g.double().cpu(), self.g64
        if self.subset is not None:
            g, ref = g[:, self.subset], ref[:, self.subset]
        return float((g - ref).abs().max() / ref.abs().max()), float((g - ref).norm() / ref.norm())


_cases = {}
FRAMING = (385, 640, 1023, 1024, 1025, 1279, 1280, 2304)
RAGGED = (385, 2304, 1025, 640)


def _tones(seed, B, L):
    t = np.arange(L) / 22050.0
    rng = np.random.default_rng(seed)
    return (0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 3000.0 * t))[None, :].repeat(B, 0).astype(np.float32) + \
        (0.01 * rng.standard_normal((B, L))).astype(np.float32)


def _subset_8():
    rng = np.random.default_rng(8)
    L = 65536
    return np.unique(np.concatenate([np.arange(1024), np.arange(L - 1024, L), rng.choice(L, 4096, replace=False)]))


def _build(name):
    if name.startswith('framing'):
        L = int(name.split('-')[1])
        return Case(name, _noise(L, 2, L, 0.1), seed=L)
    if name.startswith('quiet'):
        amp = {'quiet-1e-5': 1e-5, 'quiet-2e-5': 2e-5}[name]
        return Case(name, _noise(31, 1, 4096, amp), seed=31)
    if name == 'half-silent':
        y = _noise(32, 1, 4096, 0.1)
        y[:, :2048] = 0.0
        return Case(name, y, seed=32)
    if name in ('clip-on', 'clip-off'):
        return Case(name, _noise(41, 1, 2304, 0.8), clip=name == 'clip-on', seed=41)
    if name.startswith('ragged'):
        b = int(name.split('-')[1])
        return Case(name, _noise(50 + b, 1, RAGGED[b], 0.1), seed=50 + b)
    if name == 'layout':
        return Case(name, _noise(61, 2, 2304, 0.1), seed=61)
    if name.startswith('hop'):
        return Case(name, _noise(71, 2, 2304, 0.1), hop=int(name.split('-')[1]), seed=71)
    if name == 'grid-stride':
        return Case(name, _noise(81, 13, 65536, 0.1), seed=81, subset=_subset_8())
    if name == 'l1':
        y = _tones(91, 2, 8192)
        yhat = y + _noise(92, 2, 8192, 0.05)
        return Case(name, yhat, l1_target=y)
    raise KeyError(name)


ALL = ['framing-%d' % L for L in FRAMING] + ['quiet-1e-5', 'quiet-2e-5', 'half-silent', 'clip-on', 'clip-off'] + ['ragged-%d' % b for b in range(4)] + \
    ['layout', 'hop-128', 'hop-512', 'grid-stride', 'l1']


def case(name):
    if name not in _cases:
        _cases[name] = _build(name)
    return _cases[name]


_floor = {}


def floors():
    if not _floor:
        cs = [case(n) for n in ALL]
        _floor['max'] = float(np.median([c.e_max for c in cs]))
        _floor['2'] = float(np.median([c.e_2 for c in cs]))
    return _floor['max'], _floor['2']


def check(c, g, what=''):
    E_max, E_2 = c.errors(g)
    f_max, f_2 = floors()
    print('%s%s: E_max %.3g (yardstick e_max %.3g, bound %.3g)  E_2 %.3g (e_2 %.3g, bound %.3g)  undecided pairs %.2f %%'
          % (c.name, what, E_max, c.e_max, 4 * c.e_max + f_max, E_2, c.e_2, 4 * c.e_2 + f_2, 100 * c.undecided))
    assert c.undecided <= 0.01
    assert E_max <= 4 * c.e_max + f_max, (c.name, E_max, c.e_max, f_max)
    assert E_2 <= 4 * c.e_2 + f_2, (c.name, E_2, c.e_2, f_2)


def kernel_grad(c, dev, mel_of=None):
    y = torch.from_numpy(c.y).to(dev).requires_grad_()
    c.loss(mel_of or (lambda t: _mel(t, c.hop)), y).backward()
    return y.grad


def ragged_layout(lens, dev, guard=64, sentinel=7.0):
    """A flat buffer with a stretch of sentinel samples in front of, between and behind the signals: (flat, offsets, lengths, signals)."""
    sigs = [case('ragged-%d' % b).y[0] for b in range(len(lens))]
    parts, offs, pos = [], [], 0
    for s in sigs:
        parts.append(np.full(guard, sentinel, dtype=np.float32)); pos += guard
        offs.append(pos); parts.append(s); pos += len(s)
    parts.append(np.full(guard, sentinel, dtype=np.float32))
    flat = torch.from_numpy(np.concatenate(parts)).to(dev)
    return flat, torch.tensor(offs, dtype=torch.int64).to(dev), torch.tensor(lens, dtype=torch.int32).to(dev), sigs


def ragged_op(flat, offs, lens, F, clip, hop=256):
    return torch.ops.silent_speech.stft_logmel_ragged(flat, offs, lens, F, clip, 1024, 80, 22050, hop, 1024, 0, 8000)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_restatement_is_pinned_to_the_oracle():
    worst = 0.0
    for n in ALL:
        if n in ('grid-stride', 'clip-on'):                        # (13 x 65536 through the numpy oracle takes seconds; the oracle has no clip)
            continue
        c = case(n)
        with torch.no_grad():
            got = _restate(torch.from_numpy(c.y).double(), c.hop).numpy()
        want = mel_ref.mel_spectrogram_ref(c.y, hop_size=c.hop)
        d = float(np.abs(got - want).max())
        worst = max(worst, d)
        assert got.shape == want.shape and d <= 1e-5, (n, d)
    print('restatement vs oracle.mel_ref: largest difference %.3g' % worst)


def test_clamp_cases_meet_their_conditions():
    for n in ('quiet-1e-5', 'quiet-2e-5'):
        c = case(n)
        print('%s: %.1f %% above the clamp, %.1f %% below, %.2f %% undecided' % (n, 100 * c.above, 100 * c.below, 100 * c.undecided))
        assert c.above >= 0.10 and c.below >= 0.10 and c.undecided <= 0.01
    assert case('l1').small <= 0.01


# ------------------------------------------------------------------------------------------------ 1. fails without the feature
def test_backward_exists_and_the_forward_value_does_not_move(dev):
    c = case('framing-2304')
    y = torch.from_numpy(c.y).to(dev)
    plain = _mel(y)
    yg = y.clone().requires_grad_()
    m = _mel(yg)
    assert m.grad_fn is not None and 'stft_logmel' in type(m.grad_fn).__name__
    assert torch.equal(m.detach(), plain)
    (m * torch.from_numpy(c.g).to(dev)).sum().backward()
    assert yg.grad is not None and yg.grad.shape == y.shape and bool(torch.isfinite(yg.grad).all())
    assert float(yg.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 2. framing edges
@pytest.mark.parametrize('L', FRAMING)
def test_framing_edges(dev, L):
    """385: one frame, reflected at both ends (a sample receives direct, left and right contributions); 1023 / 1025 / 1279: padded tails no frame covers."""
    c = case('framing-%d' % L)
    check(c, kernel_grad(c, dev))


# ------------------------------------------------------------------------------------------------ 3. clamp gate
@pytest.mark.parametrize('name', ['quiet-1e-5', 'quiet-2e-5'])
def test_clamp_gate(dev, name):
    c = case(name)
    check(c, kernel_grad(c, dev))


def test_silence_has_an_exactly_zero_gradient(dev):
    y = torch.zeros(1, 4096).to(dev).requires_grad_()
    m = _mel(y)
    (m * torch.from_numpy(case('half-silent').g).to(dev)).sum().backward()
    assert bool((y.grad == 0).all())
    c = case('half-silent')
    g = kernel_grad(c, dev)
    silent = (c.g64[0] == 0).numpy()                                # samples all of whose covering frames are silent (or that sit on a zero of the window)
    print('half-silent: %d samples with an exactly zero float64 gradient' % int(silent.sum()))
    assert int(silent.sum()) == 1153
    assert bool((g[0].cpu()[torch.from_numpy(silent)] == 0).all())
    check(c, g)


# ------------------------------------------------------------------------------------------------ 4. clip gate (ragged op)
def test_clip_gate(dev):
    on, off = case('clip-on'), case('clip-off')
    beyond = np.abs(on.y[0]) > 1.0
    print('clip: %.1f %% of the samples beyond +-1' % (100 * beyond.mean()))
    assert 0.15 < beyond.mean() < 0.25
    offs, lens = torch.zeros(1, dtype=torch.int64).to(dev), torch.tensor([on.y.shape[1]], dtype=torch.int32).to(dev)
    F = _frames(on.y.shape[1], 256)
    for c in (on, off):
        g = kernel_grad(c, dev, lambda t: ragged_op(t.reshape(-1), offs, lens, F, c.clip).transpose(1, 2))
        at = g[0].cpu()[torch.from_numpy(beyond)]
        if c.clip:
            assert bool((at == 0).all())
        else:
            assert float((at != 0).float().mean()) > 0.99
        check(c, g)


# ------------------------------------------------------------------------------------------------ 5. / 10. ragged batch, determinism
def _ragged_run(dev):
    flat, offs, lens, sigs = ragged_layout(list(RAGGED), dev)
    fr = [_frames(L, 256) for L in RAGGED]
    F = max(fr)
    G = torch.full((len(RAGGED), F, 80), float('nan'))
    for b in range(len(RAGGED)):
        G[b, :fr[b]] = torch.from_numpy(case('ragged-%d' % b).g[0].T)
    flat.requires_grad_()
    buf = ragged_op(flat, offs, lens, F, False)
    buf.backward(G.to(dev))
    return flat.grad, offs, fr


def test_ragged_batch_filler_rows_guards_and_uniform_rows(dev):
    """Upstream NaN in every filler row f >= frames[b], sentinel samples between the signals.  The ragged and the uniform-row call run the SAME two kernels
    with the same per-sample order of additions: the gradients are compared BITWISE."""
    grad, offs, fr = _ragged_run(dev)
    assert bool(torch.isfinite(grad).all())
    inside = torch.zeros(grad.shape[0], dtype=torch.bool)
    for b, L in enumerate(RAGGED):
        c = case('ragged-%d' % b)
        o = int(offs[b])
        inside[o:o + L] = True
        alone = kernel_grad(c, dev)
        assert torch.equal(grad[o:o + L].cpu(), alone[0].cpu()), b
        check(c, alone)
    assert bool((grad.cpu()[~inside] == 0).all())                   # the guard stretches belong to no signal
    again, _, _ = _ragged_run(dev)
    assert torch.equal(grad.cpu(), again.cpu())                     # 10. two runs, bitwise


def test_packed_and_list_inputs_give_the_same_gradient(dev):
    sigs = [torch.from_numpy(case('ragged-%d' % b).y[0]).to(dev) for b in range(len(RAGGED))]
    fr = [_frames(L, 256) for L in RAGGED]
    G = torch.from_numpy(np.random.default_rng(55).standard_normal((len(RAGGED), max(fr), 80)).astype(np.float32)).to(dev)
    flat = torch.cat(sigs).requires_grad_()
    buf, frames = data_utils.mel_spectrogram_batch((flat, list(RAGGED)))
    assert frames == fr and buf.grad_fn is not None
    buf.backward(G)
    leaves = [s.clone().requires_grad_() for s in sigs]
    buf2, _ = data_utils.mel_spectrogram_batch(leaves)
    assert buf2.grad_fn is not None and torch.equal(buf2.detach(), buf.detach())
    buf2.backward(G)
    assert torch.equal(torch.cat([t.grad for t in leaves]), flat.grad)
    with torch.no_grad():                                           # no grad asked for: the loader's path, the same values
        buf3, _ = data_utils.mel_spectrogram_batch(leaves)
    assert buf3.grad_fn is None and torch.equal(buf3, buf.detach())


# ------------------------------------------------------------------------------------------------ 6. upstream layouts
def test_upstream_layouts(dev):
    c = case('layout')
    y = torch.from_numpy(c.y).to(dev).requires_grad_()
    gT = torch.from_numpy(np.ascontiguousarray(c.g.transpose(0, 2, 1))).to(dev)
    seen = []
    m = _mel(y)
    m.register_hook(lambda g: seen.append(g.is_contiguous()))
    (m.transpose(1, 2) * gT).sum().backward()                        # d loss / d mel arrives as a transposed view
    print('upstream of the transposed loss contiguous:', seen)
    check(c, y.grad, ' (transposed)')
    # a loss on every second band
    half = Case('layout-slice', c.y, seed=61)
    half.g[:, 1::2, :] = 0.0
    half.g64 = half._grad(torch.float64)
    half.e_max, half.e_2 = half.errors(half._grad(torch.float32))
    y2 = torch.from_numpy(c.y).to(dev).requires_grad_()
    (_mel(y2)[:, ::2, :] * torch.from_numpy(half.g[:, ::2, :].copy()).to(dev)).sum().backward()
    check(half, y2.grad, ' (strided slice)')
    # the backward op itself on a strided view: band stride 2 F
    wide = torch.zeros(c.g.shape[0], 160, c.g.shape[2])
    wide[:, ::2, :] = torch.from_numpy(c.g)
    view = wide.to(dev)[:, ::2, :]
    assert not view.is_contiguous()
    g = torch.ops.silent_speech.stft_logmel_backward(view, torch.from_numpy(c.y).to(dev), 1024, 80, 22050, 256, 1024, 0, 8000, False)
    check(c, g, ' (backward op on a strided view)')


# ------------------------------------------------------------------------------------------------ 7. other hops
@pytest.mark.parametrize('hop', [128, 512])
def test_other_hops(dev, hop):
    """hop 128: 8 covering frames, 448 reflected samples; hop 512: 2 and 256."""
    c = case('hop-%d' % hop)
    check(c, kernel_grad(c, dev))


# ------------------------------------------------------------------------------------------------ 8. grid-stride loop
@pytest.mark.gpu
def test_more_frames_than_the_grid_holds():
    """13 x 65 536 samples = 3328 frames, more than the 2 x 256 workgroups of 4 waves (2048 waves) the launcher starts at most -- and more than the 3 per CU of
    the forward's launcher --: waves walk several frames.  On the emulator tier the launcher pretends 2 CUs (16 waves), so the ragged batch (36 frame slots),
    hop 128 (36 frames) and the L1 case (64) already walk the loop there."""
    _lib.load()
    c = case('grid-stride')
    check(c, kernel_grad(c, torch.device('cuda')))


# ------------------------------------------------------------------------------------------------ 9. the loss it is for
def test_generator_mel_loss(dev):
    c = case('l1')
    print('l1: %.2f %% of the pairs with |delta| < 1e-4 or undecided' % (100 * c.small))
    check(c, kernel_grad(c, dev))


# ------------------------------------------------------------------------------------------------ 11. op hygiene
def test_op_hygiene(dev):
    c = case('framing-1280')
    y = torch.from_numpy(c.y).to(dev).requires_grad_()
    utils = ('test_schema', 'test_faketensor', 'test_autograd_registration')
    torch.library.opcheck(torch.ops.silent_speech.stft_logmel.default, (y, 1024, 80, 22050, 256, 1024, 0, 8000, False), test_utils=utils)
    flat = torch.from_numpy(np.concatenate([c.y[0], c.y[1, :700]])).to(dev).requires_grad_()
    offs, lens = torch.tensor([0, 1280], dtype=torch.int64).to(dev), torch.tensor([1280, 700], dtype=torch.int32).to(dev)
    torch.library.opcheck(torch.ops.silent_speech.stft_logmel_ragged.default, (flat, offs, lens, 5, True, 1024, 80, 22050, 256, 1024, 0, 8000), test_utils=utils)
    for name in ('stft_logmel_backward', 'stft_logmel_ragged', 'stft_logmel_ragged_backward'):
        assert name in torch_ops.OPS
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        g = torch.ops.silent_speech.stft_logmel_backward(torch.empty(3, 80, 16), torch.empty(3, 4096), 1024, 80, 22050, 256, 1024, 0, 8000, False)
        assert tuple(g.shape) == (3, 4096) and g.dtype == torch.float32
        o, n = torch.empty(3, dtype=torch.int64), torch.empty(3, dtype=torch.int32)
        b = torch.ops.silent_speech.stft_logmel_ragged(torch.empty(9000), o, n, 12, True, 1024, 80, 22050, 256, 1024, 0, 8000)
        assert tuple(b.shape) == (3, 12, 80)
        g = torch.ops.silent_speech.stft_logmel_ragged_backward(torch.empty(3, 12, 80), torch.empty(9000), o, n, True, 1024, 80, 22050, 256, 1024, 0, 8000)
        assert tuple(g.shape) == (9000,)
    m = _mel(y)
    m.sum().backward()
    with pytest.raises(RuntimeError):                                # the graph's saved tensors are gone
        m.sum().backward()


# ------------------------------------------------------------------------------------------------ 12. refusals
def test_configurations_without_a_gradient_refuse_at_the_call(dev):
    y = torch.from_numpy(_noise(12, 1, 512, 0.1)).to(dev)
    today_c = _mel(y, center=True)
    today_512 = _mel(y, hop=128, n_fft=512, win=512)
    want = mel_ref.mel_spectrogram_ref(y.cpu().numpy(), n_fft=512, hop_size=128, win_size=512)
    assert float(np.abs(today_512.cpu().numpy() - want).max()) < 2e-3
    yg = y.clone().requires_grad_()
    with pytest.raises(ValueError, match='center=True.*only the n_fft = 1024, center=False path'):
        _mel(yg, center=True)
    with pytest.raises(ValueError, match='n_fft = 512.*only the n_fft = 1024, center=False path'):
        _mel(yg, hop=128, n_fft=512, win=512)
    with pytest.raises(ValueError, match='only the n_fft = 1024'):
        data_utils.mel_spectrogram_batch([yg[0]], n_fft=512, hop_size=128, win_size=512)
    with torch.no_grad():                                           # nobody asks for a gradient: today's results
        assert torch.equal(_mel(yg, center=True), today_c)
        assert torch.equal(_mel(yg, hop=128, n_fft=512, win=512), today_512)


# ------------------------------------------------------------------------------------------------ 13. ABI
def test_abi_entry_points_validate_before_any_launch(dev):
    lib = _lib.lib()
    P = ctypes.c_void_p
    one = P(16)                                                      # never dereferenced: validation comes first
    def call(y, n_fft):
        return lib.ss_stft_logmel_fft_backward(y, None, None, 2048, 2048, 1, 5, 384, 0, n_fft, 256, one, one, one, one, one, one, 80, 900, one, one, 2, 1e-5,
                                               one, 400, 1, 5, one, 1 << 20, one, None)
    assert call(None, 1024) != 0 and b'null pointer' in lib.ss_last_error()
    assert call(one, 512) != 0 and b'n_fft must be 1024' in lib.ss_last_error()
    assert lib.ss_stft_logmel_fft_backward_workspace_bytes(3, 7) == 3 * 7 * 4096
    rc = lib.ss_stft_logmel_fft_backward(one, None, None, 2048, 2048, 1, 5, 384, 0, 1024, 256, one, one, one, one, one, one, 80, 900, one, one, 3, 1e-5,
                                         one, 400, 1, 5, one, 1 << 20, one, None)
    assert rc != 0 and b'bands over one bin' in lib.ss_last_error()
    rc = lib.ss_stft_logmel_fft_backward(one, None, None, 300, 300, 1, 1, 384, 0, 1024, 256, one, one, one, one, one, one, 80, 900, one, one, 2, 1e-5,
                                         one, 400, 1, 5, one, 1 << 20, one, None)
    assert rc != 0 and b'pad < length' in lib.ss_last_error()
