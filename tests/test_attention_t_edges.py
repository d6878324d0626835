"""The transposed-score attention kernels (csrc/attention_t.hip: attn_t_fwd / attn_t_bwd_q / attn_t_bwd_kv and their x3 plane twins) at the edges
where their unrolled instances differ: every (d_head / 32, tiles) instance, the band limits at which a whole 32-key block holds one in-band pair,
the persistent pair loop with more pairs than workgroups, and the last-tile / LDS-capacity limits.

Every launch is compared with the closed form in float64 on inputs that are exact in the storage type (bf16, resp. f32 for the plane kernels), runs
TWICE on fresh buffers (bit-equal results: a race between the loader wave and the compute waves would differ) and writes into buffers that carry
32 guard rows of a sentinel behind them (out, lse, dqkv, the D' scratch, the probability image), which must come back untouched.

Two adversarial inputs besides the random one put the probability mass where a band mistake shows:
  'spike': k_j = c (q^_{j-(D-1)} + q^_{j+(D-1)}), q^ the normalised query -- the keys at distance exactly D - 1 (the last ones inside the band) hold
           most of every row, so a skipped edge block or a band one too narrow moves O by about max|O|;
  'leak' : the same at distance D, just outside the band -- a key that slips through the mask takes the row.
The self-check of each (on the reference alone, `_self_check`) asserts that the closed form with the band off by one differs from the true one by
>= 10 x the bar of the test on >= half of the queries that have such a key.

Bars: the project's own (bf16: 2e-2 forward, 3e-2 gradients; x3: 1e-4, 3e-4; of max|want|, no outliers).  Two are derived, from the reference and
the number format alone (`_bars`):
  * bf16 on the spike / leak inputs: dQ and dK are what is left of cancelling terms many times their size, and the bf16 rounding of dS' (with that
    of P, of the table E / scale and of the stored O) is a larger share of them than 3e-2.  The float64 reference restated with these four roundings
    (`_restated_bf16`) differs from the exact one by up to 2.1e-2 (dQ, emulator shapes) / 1.1e-1 (dQ), 2.6e-2 (dK), 5.3e-3 (lse) at the GPU shapes; the
    bar is 4 x that per case where it exceeds the inherited one: at worst 8.2e-2 (emulator) and 4.5e-1 / 1.0e-1 / 2.1e-2 for dQ / dK / lse (GPU).  The
    kernels use at most 0.29 of a derived bar (measured on an MI355X);
  * D = 1 or T = 1: one key per query, dQ = dK = 0 identically; the bar is 3e-2 (3e-4) of the two terms that cancel (measured <= 4.1e-3 of them)."""
import functools
import math

import pytest
import torch

from oracle import dropout_ref
from silent_speech_amd import ops
from tests.backend import dev, is_emu  # noqa: F401
from tests.test_attention import _pack, _reference
from tests.util import assert_close_robust

BARS = {'bf16': (2e-2, 3e-2), 'x3': (1e-4, 3e-4)}          # (O and lse, gradients) of max|want|
GUARD = 32                                                 # guard rows behind every output
SENT = 7.0                                                 # sentinel of the float buffers (bf16 0x40E0)
SENT_IMG = 0x5A                                            # sentinel of the probability image
SPIKE_C = 6.0                                              # k = SPIKE_C * sqrt(dh) * (normalised queries)
DROP_STREAM = 8


# ------------------------------------------------------------------ inputs and the closed form
def _inputs(kind, B, H, T, dh, D, seed, mode):
    """q, k, v, dO (B,H,T,dh) and E (H,2D-1,dh) as float64 tensors whose values are exact in the storage type of `mode`."""
    st = torch.bfloat16 if mode == 'bf16' else torch.float32
    g = torch.Generator().manual_seed(seed)
    q, k, v = [(torch.randn(B, H, T, dh, generator=g) * 0.8).to(st).double() for _ in range(3)]
    E = (torch.randn(H, 2 * D - 1, dh, generator=g) * dh ** -0.5).to(st).double()
    dO = torch.randn(B, H, T, dh, generator=g).to(st).double()
    if kind != 'random':
        d = D - 1 if kind == 'spike' else D
        qn = q / q.norm(dim=-1, keepdim=True)
        k = torch.zeros_like(q)
        if d < T:
            k[:, :, d:] += qn[:, :, :T - d]                   # q^_{j-d}
            if d > 0:
                k[:, :, :T - d] += qn[:, :, d:]               # q^_{j+d}  (d = 0: one term, the key of the query itself)
            else:
                k *= 2.0
        k = (k * (SPIKE_C * math.sqrt(dh))).to(st).double()
    return dict(q=q, k=k, v=v, E=E, dO=dO)


def _closed_form(q, k, v, E, D, dh, band):
    """The closed form (no dropout) with the band limit moved: |k - q| <= band - 1 is kept.  band = D is the kernels' contract; band = D - 1 drops the
    keys at distance D - 1; band = D + 1 lets the keys at distance D in with their plain q.k logit (there is no embedding row for them)."""
    T = q.shape[2]
    dist = (torch.arange(T)[None, :] - torch.arange(T)[:, None])
    logits = torch.einsum('bhqa,bhka->bhqk', q, k) / math.sqrt(dh)
    rel = torch.einsum('bhqa,hma->bhqm', q, E)
    pos = torch.gather(rel, 3, (dist + D - 1).clamp(0, 2 * D - 2)[None, None].expand_as(logits))
    logits = logits + torch.where(dist.abs() <= D - 1, pos, torch.zeros_like(pos))
    logits = logits.masked_fill((dist.abs() > band - 1)[None, None], -1e8)
    return torch.einsum('bhqk,bhka->bhqa', torch.softmax(logits, -1), v)


@functools.lru_cache(maxsize=None)
def _problem(kind, B, H, T, dh, D, seed, mode, p):
    """Inputs, keep mask and the float64 reference (O, lse, dQ, dK, dV): computed once per case, shared by the two launches and never modified."""
    x = _inputs(kind, B, H, T, dh, D, seed, mode)
    q, k, v = [x[n].clone().requires_grad_(True) for n in 'qkv']
    drop = None
    if p > 0:
        drop = torch.from_numpy(dropout_ref.attention_mask(2, seed + 1000, DROP_STREAM, B, H, T, p)).double() / (1.0 - p)
    O, lse = _reference(q, k, v, x['E'], D, dh, drop=drop)
    O.backward(x['dO'])
    x.update(O=O.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad, dv=v.grad, shape=(B, H, T, dh, D), kind=kind, seed=seed, p=p, mode=mode)
    return x


def _bf(x):
    return x.float().to(torch.bfloat16).double()


def _restated_bf16(x):
    """The closed form in float64 with the roundings the bf16 kernels make BY DESIGN restated: the table E' = bf16(E / scale), the saved
    probabilities bf16(P) (which are also the operand of P.V and of the backward), O stored as bf16 (it enters D = rowsum(dO * O)) and
    dS' = bf16(max(pf, 0) dP - |pf| D') (the operand of the dQ and dK products).  Everything else stays exact.  -> O, lse, dq, dk, dv"""
    B, H, T, dh, D = x['shape']
    p = x['p']
    s, scale = 1.0 / (1.0 - p), 1.0 / math.sqrt(dh)
    q, k, v, dO = x['q'], x['k'], x['v'], x['dO']
    keep = torch.ones(B, H, T, T, dtype=torch.float64)
    if p > 0:
        keep = torch.from_numpy(dropout_ref.attention_mask(2, x['seed'] + 1000, DROP_STREAM, B, H, T, p)).double()
    Es = _bf(x['E'] / scale)
    dist = torch.arange(T)[None, :] - torch.arange(T)[:, None]
    inband = (dist.abs() <= D - 1)[None, None]
    idx = (dist + D - 1).clamp(0, 2 * D - 2)[None, None].expand(B, H, T, T)
    logits = (torch.einsum('bhqa,bhka->bhqk', q, k) + torch.gather(torch.einsum('bhqa,hma->bhqm', q, Es), 3, idx)) * scale
    logits = logits.masked_fill(~inband, -1e8)
    Pb = _bf(torch.softmax(logits, -1))
    Pk = Pb * keep
    O = s * torch.einsum('bhqk,bhka->bhqa', Pk, v)
    dP = torch.einsum('bhqa,bhka->bhqk', dO, v)
    Dp = (dO * _bf(O)).sum(-1, keepdim=True) / s
    dS = _bf(Pk * dP - Pb * Dp) * inband
    dR = torch.zeros(B, H, T, 2 * D - 1, dtype=torch.float64).scatter_add_(3, idx, dS)
    dq = scale * s * (torch.einsum('bhqk,bhka->bhqa', dS, k) + torch.einsum('bhqm,hma->bhqa', dR, Es))
    dk = scale * s * torch.einsum('bhqk,bhqa->bhka', dS, q)
    dv = s * torch.einsum('bhqk,bhqa->bhka', Pk, dO)
    return dict(O=O, lse=torch.logsumexp(logits, -1), dq=dq, dk=dk, dv=dv)


def _bars(x):
    """The bar of every output of the case (a fraction of max|want|).  The project's own, except for the bf16 kernels on the spike / leak inputs:
    there K is ~ 6 sqrt(dh) long, the rows of dS' sum to zero and dQ = scale dS' K + dS' E' is what is left of terms many times its size, so the
    rounding of dS' (and of P, E', O) to bf16 -- 2^-9 of the TERMS -- is a larger fraction of the result than the inherited 3e-2 allows for.
    The bar is then 4 x (restated reference - exact reference) / max|exact| where that is wider: a property of the inputs and of the number
    format, computed from the reference alone.  Worst derived bars: the module docstring and DESIGN.md (section 7, N2b)."""
    tol_f, tol_b = BARS[x['mode']]
    bars = dict(O=tol_f, lse=tol_f, dq=tol_b, dk=tol_b, dv=tol_b)
    if x['mode'] == 'bf16' and x['kind'] != 'random':
        r = _restated_bf16(x)
        for n in bars:
            derived = 4.0 * float((r[n] - x[n]).abs().max()) / (float(x[n].abs().max()) + 1e-12)
            if derived > bars[n] and float(x[n].abs().max()) > 1e-9:
                print('    %-4s bar derived from the restated roundings: %.3e (inherited %.1e)' % (n, derived, bars[n]))
                bars[n] = derived
    B, H, T, dh, D = x['shape']
    floors = {}
    if D == 1 or T == 1:
        # One key per query: P = 1, dS = P (dP - D) = 0, so dQ and dK are identically zero and a bar relative to max|want| has no scale.  The kernels
        # form dP - D from dP = dO . V (f32) and D = dO . bf16(O): the bar is taken of the size of the two terms that cancel,
        # max|dO . V| / (1 - p) times the largest factor it meets (scale |K| + |E| for dQ, scale |Q| for dK).
        G = float(torch.einsum('bhqa,bhka->bhqk', x['dO'], x['v']).abs().max()) / (1.0 - x['p'])
        scale = 1.0 / math.sqrt(dh)
        floors = dict(dq=G * (scale * float(x['k'].abs().max()) + float(x['E'].abs().max())), dk=G * scale * float(x['q'].abs().max()))
        assert float(x['dq'].abs().max()) < 1e-9 and float(x['dk'].abs().max()) < 1e-9
    return bars, floors


def _self_check(kind, B, H, T, dh, D, seed, mode):
    """On the reference alone: the band off by one (D - 2 for the spike, D for the leak probe) moves O by >= 10 x the forward bar (of max|O|) on at
    least half of the queries that have a key at the probed distance.  Returns the fraction (None: no query has such a key)."""
    x = _problem(kind, B, H, T, dh, D, seed, mode, 0.0)
    d = D - 1 if kind == 'spike' else D
    if d >= T:
        return None
    true = _closed_form(x['q'], x['k'], x['v'], x['E'], D, dh, D)
    assert float((true - x['O']).abs().max()) <= 1e-9 * float(x['O'].abs().max())          # the same closed form as tests.test_attention._reference
    wrong = _closed_form(x['q'], x['k'], x['v'], x['E'], D, dh, D - 1 if kind == 'spike' else D + 1)
    t = torch.arange(T)
    has = (t - d >= 0) | (t + d < T)
    moved = (wrong - true).abs().amax(-1)[:, :, has] >= 10 * BARS[mode][0] * float(true.abs().max())
    frac = float(moved.double().mean())
    print('self-check %s %s T=%d dh=%d D=%d: band off by one moves O by %.2f x max on the worst query, >= 10 x bar on %.0f %% of %d queries'
          % (kind, mode, T, dh, D, float((wrong - true).abs().max() / true.abs().max()), 100 * frac, int(has.sum())))
    assert frac >= 0.5, (kind, mode, T, dh, D, frac)
    return frac


# ------------------------------------------------------------------ guarded buffers
class _Guarded(object):
    """`rows` live rows of `cols` elements with GUARD more behind them, everything filled with a sentinel."""

    def __init__(self, rows, cols, dtype, fill, device):
        self.fill, self.n = fill, rows * cols
        self.full = torch.full(((rows + GUARD) * cols,), fill, dtype=dtype, device=device)
        self.live = self.full[:self.n].view(rows, cols)

    def guard_untouched(self):
        return bool((self.full[self.n:] == self.fill).all())


def _rows(x, dp):          # (B,H,T,dh) f64 -> (B*T, H*dp) f32, head dims zero padded
    B, H, T, _ = x.shape
    return _pack(x.float(), dp).reshape(B * T, H * dp).contiguous()


def _launch(dev, x):
    """One forward + backward of the case on fresh sentinel buffers -> the live parts as CPU tensors (float outputs as f32, plane pairs summed)."""
    B, H, T, dh, D = x['shape']
    mode, p = x['mode'], x['p']
    dp, Tp, nt = (dh + 31) // 32 * 32, (T + 7) // 8 * 8, (T + 31) // 32
    scale = 1.0 / math.sqrt(dh)
    bf = torch.bfloat16
    kw = dict(p=p, seed=x['seed'] + 1000, rng_stream=DROP_STREAM) if p > 0 else {}
    qkv = torch.cat([_rows(x[n], dp) for n in 'qkv'], 1).contiguous().to(dev)
    dO = _rows(x['dO'], dp).to(dev)
    lse = _Guarded(B * H, T, torch.float32, SENT, dev)
    dsc = _Guarded(B * H, T, torch.float32, SENT, dev)
    nplanes = 1 if mode == 'bf16' else 2
    out = [_Guarded(B * T, H * dp, bf, SENT, dev) for _ in range(nplanes)]
    dqkv = [_Guarded(B * T, 3 * H * dp, bf, SENT, dev) for _ in range(nplanes)]
    nimg = B * H * nt * nt * 2048 * nplanes
    img = _Guarded(nimg // 64, 64, torch.uint8, SENT_IMG, dev)
    saved = img.live.view(-1)
    lse_v = lse.live.view(B, H, T)
    if mode == 'bf16':
        assert ops.relpos_attention_family(bf, T, dp, D) == 2
        assert ops.relpos_attention_saved_bytes(bf, B, H, T, dp, D) == nimg
        tab = ops.relpos_attention_tables(x['E'].float().to(dev), dp, scale)
        qkv = qkv.to(bf)
        ops.relpos_attention_forward(qkv, None, None, out[0].live, lse_v, B, H, T, Tp, dp, D, scale, saved=saved, tab=tab, **kw)
        ops.relpos_attention_backward(qkv, None, None, None, out[0].live, lse_v, dO.to(bf), None, dsc.live, dqkv[0].live, B, H, T, Tp, dp, D, scale,
                                      saved=saved, tab=tab, **kw)
    else:
        assert ops.relpos_attention_x3_supported(T, dp, D)
        assert ops.relpos_attention_x3_saved_bytes(B, H, T, dp, D) == nimg
        tab = ops.relpos_attention_x3_tables(x['E'].float().to(dev), dp, scale)
        qkv_p = ops.split_planes(qkv)
        out_p, dqkv_p = [o.live for o in out], [o.live for o in dqkv]
        ops.relpos_attention_x3_forward(qkv_p, tab, out_p, lse_v, B, H, T, dp, D, scale, saved=saved, **kw)
        ops.relpos_attention_x3_backward(qkv_p, tab, out_p, ops.split_planes(dO), dsc.live, dqkv_p, saved, B, H, T, dp, D, scale, **kw)
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    for name, bufs in (('out', out), ('lse', [lse]), ("D' scratch", [dsc]), ('dqkv', dqkv), ('image', [img])):
        for b in bufs:
            assert b.guard_untouched(), '%s: the guard rows behind the buffer were written' % name
    res = dict(lse=lse.live.cpu().view(B, H, T), dsc=dsc.live.cpu(), img=img.live.cpu())
    for name, bufs in (('out', out), ('dqkv', dqkv)):
        planes = [b.live.cpu() for b in bufs]
        # a live element that still holds the sentinel: the bf16 kernels leave 7.0 only where that is the result (checked against the reference
        # in _compare); a plane pair can never legitimately hold 7.0 in BOTH planes
        res[name + '_stale'] = planes[0] == SENT if nplanes == 1 else (planes[0] == SENT) & (planes[1] == SENT)
        res[name + '_planes'] = planes
        res[name] = planes[0].float() if nplanes == 1 else planes[0].float() + planes[1].float()
    return res


def _figure(got, want, tol, name, floor=None):
    if floor is not None:                                                # want is identically zero: the bar is a fraction of `floor` (see _bars)
        err = float((got.double() - want.double()).abs().max()) / floor
        print('    %-4s %.3e of the cancelling terms (bar %.1e)' % (name, err, tol))
        assert bool(torch.isfinite(got).all()) and err <= tol, '%s: %.3e of the cancelling terms (bar %.1e)' % (name, err, tol)
        return
    err = float((got.double() - want.double()).abs().max()) / (float(want.abs().max()) + 1e-12)
    print('    %-4s %.3e of max (bar %.3e)' % (name, err, tol))
    assert_close_robust(got, want.float(), tol, name=name, max_outlier_frac=0)


def _compare(res, x, tag):
    B, H, T, dh, D = x['shape']
    dp = (dh + 31) // 32 * 32
    bars, floors = _bars(x)
    print('%s %s %s p=%g B=%d H=%d T=%d dh=%d D=%d' % (tag, x['mode'], x['kind'], x['p'], B, H, T, dh, D))
    out, dqkv = res['out'].view(B, T, H, dp), res['dqkv'].view(B, T, 3, H, dp)
    want_out = _pack(x['O'].float(), dp)
    want_dqkv = torch.stack([_pack(x[n].float(), dp) for n in ('dq', 'dk', 'dv')], 2)
    for name, stale, want in (('out', res['out_stale'].view_as(want_out), want_out), ('dqkv', res['dqkv_stale'].view_as(want_dqkv), want_dqkv)):
        left = stale & ((want - SENT).abs() > 0.5)
        assert not bool(left.any()), '%s: %d live elements still hold the sentinel' % (name, int(left.sum()))
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(res['lse']).all())
    _figure(out[..., :dh].permute(0, 2, 1, 3), x['O'], bars['O'], 'O')
    _figure(res['lse'], x['lse'], bars['lse'], 'lse')
    for i, n in enumerate(('dq', 'dk', 'dv')):
        _figure(dqkv[:, :, i, :, :dh].permute(0, 2, 1, 3), x[n], bars[n], n, floor=floors.get(n))
    if dp > dh:                                                          # padded head columns stay exactly zero
        assert float(out[..., dh:].abs().max()) == 0.0 and float(dqkv[..., dh:].abs().max()) == 0.0


def _case(dev, kind, B, H, T, dh, D, seed, mode, p, tag=''):
    """Run the case twice on fresh buffers, demand bit-equal results, compare the first with the float64 closed form."""
    x = _problem(kind, B, H, T, dh, D, seed, mode, p)
    a, b = _launch(dev, x), _launch(dev, x)
    for n in ('out_planes', 'dqkv_planes'):
        for pa, pb in zip(a[n], b[n]):
            assert torch.equal(pa.view(torch.int16), pb.view(torch.int16)), '%s differs between two runs of the same launch' % n
    for n in ('lse', 'dsc', 'img'):
        assert torch.equal(a[n], b[n]), '%s differs between two runs of the same launch' % n
    _compare(a, x, tag)


@functools.lru_cache(maxsize=None)
def _x3_tmax(dp, D=100):
    """The longest row the plane kernels take at this head width: found by scanning the support predicate (which must not have holes below it)."""
    ok = [bool(ops.relpos_attention_x3_supported(T, dp, D)) for T in range(1, 260)]
    tmax = max(T for T, o in zip(range(1, 260), ok) if o)
    assert all(ok[:tmax])
    return tmax


def _modes(T, dp, D):
    return ['bf16'] + (['x3'] if ops.relpos_attention_x3_supported(T, dp, D) else [])


# ------------------------------------------------------------------ a. every (DPK, NT) instance
def _sweep_params():
    out = []
    for dpk in (1, 2, 3):
        for nt in range(1, 8):
            # the emulator tier: one (T, mode) of the instance per case keeps a case at ~3 s; NT = 7 (4 s per case) runs on the GPU only
            if (dpk == 1 and nt <= 6) or nt <= 2:
                out += [pytest.param('emu', dpk, nt, ti, mode, id='emu-dpk%d-nt%d-T%d-%s' % (dpk, nt, ti, mode)) for ti in range(3) for mode in ('bf16', 'x3')]
            out.append(pytest.param('hip', dpk, nt, None, None, marks=pytest.mark.gpu, id='hip-dpk%d-nt%d' % (dpk, nt)))
    return out


@pytest.mark.parametrize('dev,dpk,nt,only_t,only_mode', _sweep_params(), indirect=['dev'])
def test_instance_sweep(dev, dpk, nt, only_t, only_mode):
    """Each of the 21 (d_head / 32, tiles) instances of the six kernels, forward with and without dropout: T = 32 NT (no ragged tile), 32 (NT - 1) + 1
    (one live row in the last tile) and 32 (NT - 1) + 13; padded head dim (32 DPK - 8); D = 34 (one in-band pair in the block pair at distance 2)
    from three tiles on, else D = 2 (the same at distance 1).  GPU: all 21, B = H = 2.  Emulator: NT <= 6 at DPK = 1 and NT <= 2 at DPK = 2, 3, B = H = 1
    (`dev` is parametrised here case by case: the emulator tier runs fewer instances, and one (T, mode) of an instance per case)."""
    dh, D = 32 * dpk - 8, (34 if nt >= 3 else 2)
    BH = 1 if is_emu(dev) else 2
    nx3 = 0
    for ti, T in enumerate((32 * nt, 32 * (nt - 1) + 1, 32 * (nt - 1) + 13)):
        if only_t is not None and ti != only_t:
            continue
        assert (T + 31) // 32 == nt and ops.relpos_attention_family(torch.bfloat16, T, 32 * dpk, D) == 2
        # the plane kernels hold four K / V plane tables in LDS: every shape but the longest rows of d_head 96 (the count below pins which)
        assert ops.relpos_attention_x3_supported(T, 32 * dpk, D) == (T <= _x3_tmax(32 * dpk))
        for mode in _modes(T, 32 * dpk, D):
            if only_mode is not None and mode != only_mode:
                continue
            nx3 += mode == 'x3'
            if T > D - 1:
                _self_check('spike', BH, BH, T, dh, D, 100 * dpk + nt, mode)
            for kind in ('random', 'spike'):
                for p in (0.0, 0.25):
                    _case(dev, kind, BH, BH, T, dh, D, 100 * dpk + nt, mode, p, tag='sweep')
    if only_t is None:
        assert nx3 == (1 if (dpk, nt) == (3, 7) else 3)


# ------------------------------------------------------------------ b. band edges
def _band_params():
    out = [pytest.param('emu', D, id='emu-D%d' % D) for D in (1, 2, 33, 34)]
    return out + [pytest.param('hip', D, marks=pytest.mark.gpu, id='hip-D%d' % D) for D in (1, 2, 33, 34, 65, 66, 97, 98, 100)]


@pytest.mark.parametrize('dev,D', _band_params(), indirect=['dev'])
def test_band_edges(dev, D):
    """D - 1 = 32 u + 1 (D = 2, 34, 66, 98): the block pair at distance u + 1 holds exactly ONE in-band (query, key) pair per tile, and the spike input
    puts most of that query's mass on it; D - 1 = 32 u (33, 65, 97): that block pair is skipped, and the leak probe puts the mass on the first key
    behind the band; D = 1: the diagonal alone; D = 100: the model's.  T leaves room for block pairs at distance ceil((D - 1) / 32) + 1."""
    if is_emu(dev):
        B = H = 1
        T, dh = 97, 8
    else:
        B = H = 2
        T, dh = (131, 88) if D <= 66 else (224, 56)
    dp = (dh + 31) // 32 * 32
    assert _modes(T, dp, D) == ['bf16', 'x3']
    for mode in ('bf16', 'x3'):
        for kind in ('spike', 'leak'):
            assert _self_check(kind, B, H, T, dh, D, 200 + D, mode) is not None
            for p in (0.0, 0.25):
                _case(dev, kind, B, H, T, dh, D, 200 + D, mode, p, tag='band')


@pytest.mark.parametrize('mode', ['bf16', 'x3'])
@pytest.mark.parametrize('T,D', [(20, 34), (34, 34), (33, 34)])
def test_band_wider_than_the_sequence(dev, T, D, mode):
    """D > T (no masking at all, one tile), D - 1 = T - 1 (the band ends on the last key of the first query) and D - 1 = T (it ends one behind it)."""
    for kind in ('random', 'spike', 'leak'):
        _self_check(kind, 1, 2, T, 8, D, 300 + T, mode)
        for p in (0.0, 0.25):
            _case(dev, kind, 1, 2, T, 8, D, 300 + T, mode, p, tag='wide band')


# ------------------------------------------------------------------ c. the persistent pair loop
def _pair_loop_cases():
    out = [pytest.param('emu', B, H, 37, 8, 9, id='emu-B%d-H%d' % (B, H)) for B, H in ((3, 2), (3, 3), (2, 5))]
    for H in (8, 3):
        for T, dh, D in ((40, 32, 9), (70, 64, 34)):
            out.append(pytest.param('hip', None, H, T, dh, D, marks=pytest.mark.gpu, id='hip-H%d-T%d' % (H, T)))
    return out


@pytest.mark.parametrize('mode', ['bf16', 'x3'])
@pytest.mark.parametrize('dev,B,H,T,dh,D', _pair_loop_cases(), indirect=['dev'])
def test_persistent_pair_loop(dev, B, H, T, dh, D, mode):
    """More (sequence, head) pairs than workgroups: the forward and the query-major backward launch min(CUs / H * H, B H) workgroups that walk the
    pairs blockIdx.x, + gridDim.x, ..., the loader wave fetching K of the next pair under the softmax and P.V of this one.  Every pair has its own
    inputs and its own reference, so a stale K or V table shows.  Emulator (4 CUs): (B, H) = (3, 2) -- two workgroups take two pairs, two take one;
    (3, 3) -- a grid of 3; (2, 5) -- more heads than CUs.  GPU: H = 8 and H = 3 (grid 255 on 256 CUs) with B giving two full rounds and a partial one."""
    if B is None:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        grid = max(cus // H * H, H)
        B = (2 * grid + grid // 2 + H - 1) // H
        assert 2 * grid < B * H < 3 * grid
    else:
        grid = max(4 // H * H, H)
        assert B * H > grid
    for p in (0.0, 0.25):
        _case(dev, 'random', B, H, T, dh, D, 400 + H, mode, p, tag='pair loop (grid %d)' % grid)


# ------------------------------------------------------------------ d. capacity and dispatch edges
@pytest.mark.parametrize('T', [1, 2])
def test_shortest_sequences(dev, T):
    for D in (1, 9):
        for mode in ('bf16', 'x3'):
            for p in (0.0, 0.25):
                _case(dev, 'random', 2, 2, T, 24, D, 500 + T, mode, p, tag='short')


@pytest.mark.gpu
def test_last_family_2_shape_and_the_hand_over():
    """bf16 at (T, dp) = (224, 96): the last shape of the transposed-score kernels (with dropout); (225, 96) goes to the per-tile family."""
    from silent_speech_amd import _lib
    from tests.test_attention import _run
    _lib.load()
    dev = torch.device('cuda')
    assert ops.relpos_attention_family(torch.bfloat16, 224, 96, 100) == 2
    for kind in ('random', 'spike'):
        _case(dev, kind, 2, 2, 224, 96, 100, 600, 'bf16', 0.25, tag='capacity')
    assert ops.relpos_attention_family(torch.bfloat16, 225, 96, 100) == 0
    _run(dev, torch.bfloat16, B=2, H=2, T=225, dh=96, D=100, seed=601, tol_f=2e-2, tol_b=3e-2, p=0.25)


@pytest.mark.gpu
@pytest.mark.parametrize('dp', [32, 64, 96])
def test_x3_capacity_limit(dp):
    """The longest row the plane kernels take at each head width (found by scanning the support predicate) runs; one row more is refused by
    ss_relpos_attention_x3_forward with its own message, not run."""
    from silent_speech_amd import _lib
    _lib.load()
    dev = torch.device('cuda')
    D = 100
    Tmax = _x3_tmax(dp, D)
    assert Tmax == 224 if dp < 96 else 192 < Tmax < 224          # d_head 96: the training rows (200) fit, the last family-2 shape does not
    for p in (0.0, 0.25):
        _case(dev, 'random', 2, 2, Tmax, dp - 8, D, 700 + dp, 'x3', p, tag='x3 capacity')
    B, H, T = 1, 1, Tmax + 1
    bf = torch.bfloat16
    qkv_p = [torch.zeros(B * T, 3 * H * dp, dtype=bf, device=dev) for _ in range(2)]
    tab = ops.relpos_attention_x3_tables(torch.zeros(H, 2 * D - 1, dp - 8, device=dev), dp, 1.0)
    out_p = [torch.full((B * T, H * dp), SENT, dtype=bf, device=dev) for _ in range(2)]
    lse = torch.full((B, H, T), SENT, device=dev)
    with pytest.raises(RuntimeError, match='does not run the plane kernels'):
        ops.relpos_attention_x3_forward(qkv_p, tab, out_p, lse, B, H, T, dp, D, 1.0)
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in out_p) and bool((lse == SENT).all())
