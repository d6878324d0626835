"""The two kernels that take per-utterance lengths, each alone against float64: attn_fwd_ragged_kernel (ss_relpos_attention_forward_ragged,
csrc/attention.hip) and the RAGGED instantiation of bn_apply_kernel (ss_bn_apply_ragged, csrc/norm.hip).  End to end (test_ragged_inference.py) they
only ever ran at d_head 2 and 8 and at C = 16 and 64; here they run at every head width the dispatch has (dp / 32 = 1 .. 4), in the three arithmetic
modes, and on the three paths of the BatchNorm apply (per-chunk fallback, RowWalk with one trip, RowWalk with several trips across slot boundaries).
Everything behind an utterance's end is poisoned with NaN: a valid row may depend on it only through a select, never through arithmetic."""
import math

import pytest
import torch

from silent_speech_amd import _lib, ops
from tests.backend import dev, is_emu  # noqa: F401
from tests.test_attention import _pack, _reference
from tests.util import assert_close_robust

SENTINEL = -777.0          # what out / y hold before the launch (compared with a tensor filled the same way, so its bf16 rounding does not matter)
GUARD = 64                 # rows behind the last slot: one workgroup's worth of query rows
# oracle-relative bars of the same arithmetic in tests/test_attention.py: exact f32, f32 storage with bf16 x 3 products, bf16
MODES = {'f32': (torch.float32, 'exact', 2e-5), 'bf16x3': (torch.float32, 'bf16x3', 2e-4), 'bf16': (torch.bfloat16, 'exact', 2e-2)}
EMU_LENS = [41, 33, 32, 17, 16, 1, 0, 50]
GPU_LENS = [250, 249, 225, 224, 200, 199, 121, 100, 99, 65, 64, 33, 32, 31, 17, 16, 15, 1, 0, 300]


# =========================================================================================================== attention
_ATTN = {}


def _attn_problem(dt, H, T, dh, D, lens, seed):
    """Operands (rounded to the storage type) and the float64 oracle of every utterance ALONE; made once per shape, shared, never modified."""
    key = (dt, H, T, dh, D, tuple(lens), seed)
    if key not in _ATTN:
        B = len(lens)
        g = torch.Generator().manual_seed(seed)
        q, k, v = [(torch.randn(B, H, T, dh, generator=g) * 0.8).to(dt).float() for _ in range(3)]
        E = (torch.randn(H, 2 * D - 1, dh, generator=g) * dh ** -0.5).to(dt).float()
        want = []
        for b, n in enumerate(lens):
            L = min(max(n, 0), T)
            want.append(_reference(q[b:b + 1, :, :L].double(), k[b:b + 1, :, :L].double(), v[b:b + 1, :, :L].double(), E.double(), D, dh)[0][0] if L else None)
        _ATTN[key] = (q, k, v, E, want)
    return _ATTN[key]


def _attn_device_operands(dev, dt, q, k, v, E, H, T, dh, D, lens=None):
    """qkv [B T][3 H dp], qkvT [B][3 H dp][Tp], E [H][2D-1][dp] as _run of tests/test_attention.py builds them; with lens, everything behind an
    utterance's end is NaN: rows t >= L_b of Q, K and V, columns t >= L_b of qkvT up to Tp (L_b clamped to [0, T])."""
    B = q.shape[0]
    dp, Tp = (dh + 31) // 32 * 32, (T + 7) // 8 * 8
    qkv = torch.cat([_pack(t, dp).reshape(B * T, H * dp) for t in (q, k, v)], 1).to(dt).contiguous()
    qkvT = torch.zeros(B, 3 * H * dp, Tp, dtype=dt)
    qkvT[:, :, :T] = qkv.view(B, T, 3 * H * dp).transpose(1, 2)
    if lens is not None:
        for b, n in enumerate(lens):
            L = min(max(n, 0), T)
            qkv.view(B, T, 3 * H * dp)[b, L:] = float('nan')
            qkvT[b, :, L:] = float('nan')
    Ed = torch.zeros(H, 2 * D - 1, dp, dtype=dt)
    Ed[..., :dh] = E.to(dt)
    return qkv.to(dev), qkvT.to(dev), Ed.to(dev), dp, Tp


def _run_ragged(dev, mode, H, T, dh, D, lens, seed):
    dt, f32_math, tol = MODES[mode]
    B = len(lens)
    q, k, v, E, want = _attn_problem(dt, H, T, dh, D, lens, seed)
    qkv, qkvT, Ed, dp, Tp = _attn_device_operands(dev, dt, q, k, v, E, H, T, dh, D, lens)
    out = torch.full((B * T + GUARD, H * dp), SENTINEL, dtype=dt, device=dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    ops.relpos_attention_forward_ragged(qkv, qkvT, Ed, out, lens_d, B, H, T, Tp, dp, D, 1.0 / math.sqrt(dh), f32_math=f32_math)
    got = out.cpu()
    assert torch.equal(got[B * T:], torch.full((GUARD, H * dp), SENTINEL, dtype=dt)), 'rows behind the last slot were written'
    got = got[:B * T].float().view(B, T, H, dp)
    worst = 0.0
    for b, n in enumerate(lens):
        L = min(max(n, 0), T)
        if not L:
            continue                                       # nothing is promised about a slot without a valid row
        e = assert_close_robust(got[b, :L, :, :dh].permute(1, 0, 2), want[b], tol, name='O[%d] L=%d' % (b, n), max_outlier_frac=0)     # finite, too
        worst = max(worst, e)
        if dp > dh:
            assert float(got[b, :L, :, dh:].abs().max()) == 0.0, 'padded head columns of utterance %d' % b
    print('ragged attention %s H=%d T=%d dh=%d (DPK %d) D=%d: worst err/scale over %d utterances %.3e (bar %.0e)' % (mode, H, T, dh, dp // 32, D, B, worst, tol))


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('dpk', [1, 2, 3, 4])
def test_ragged_attention_each_utterance_alone(dev, dpk, mode):
    """First execution of attn_fwd_ragged_kernel<float | x3_t | bf16_t, DPK> for DPK = 2, 3, 4 (and of DPK = 1 outside the model).  Emulator: d_head
    8, 40, 96, 100 (DPK 1 .. 4); GPU: 24, 64, 96, 128 (DPK 1 .. 4).  Lengths: 0 (every tile exits), above T (behaves as T), both sides of the 16-row
    query tile and of the 32-row alignment of kstart, both sides of D - 1 and D, ends inside the band of other slots' queries.  Of the kernel's three uses of the length on the key side, the k < L test
    of the logits and the zeroing of the V^T fragments are each pinned by these cases (either one bounded by T instead fails all of them); the row bound
    of the K loads is not observable from outside while the logits test stands -- a K row behind the end only reaches logit columns k >= L, which that
    select discards -- so no case here can tell it from a bound of T."""
    if is_emu(dev):
        _run_ragged(dev, mode, H=2, T=41, dh={1: 8, 2: 40, 3: 96, 4: 100}[dpk], D=9, lens=EMU_LENS, seed=dpk)
    else:
        _run_ragged(dev, mode, H=8, T=250, dh={1: 24, 2: 64, 3: 96, 4: 128}[dpk], D=100, lens=GPU_LENS, seed=dpk)


@pytest.mark.parametrize('mode', list(MODES))
def test_ragged_attention_workgroup_count_not_a_multiple_of_8(dev, mode):
    """H = 3 and an odd B: gx * H * B is 60 on the GPU (gx = 4, B = 5) and 9 on the emulator (gx = 1, B = 3), so nwg & 7 != 0 and the remainder
    branch of attn_block_coord maps the last workgroups; a wrong map computes some (slot, head, tile) twice and another never (sentinel left)."""
    if is_emu(dev):
        _run_ragged(dev, mode, H=3, T=41, dh=96, D=9, lens=[41, 20, 7], seed=7)
    else:
        _run_ragged(dev, mode, H=3, T=250, dh=96, D=100, lens=[250, 121, 33, 0, 300], seed=7)


@pytest.mark.parametrize('mode', list(MODES))
def test_ragged_attention_with_full_lengths_equals_dense(dev, mode):
    """Every length equal to T: the ragged kernel against attn_fwd_kernel (per-tile family, asserted) on the same operands.  bf16 needs a shape the
    transposed-score kernels do not take: T = 250 > 224 on the GPU, d_head 100 (dp 128) on the emulator."""
    dt, f32_math, tol = MODES[mode]
    B, H, T, D = (2, 2, 41, 9) if is_emu(dev) else (2, 8, 250, 100)
    dh = (100 if mode == 'bf16' else 40) if is_emu(dev) else 96
    q, k, v, E, _ = _attn_problem(dt, H, T, dh, D, [T] * B, 21)
    qkv, qkvT, Ed, dp, Tp = _attn_device_operands(dev, dt, q, k, v, E, H, T, dh, D)
    assert ops.relpos_attention_family(_lib.SS_F32X3 if f32_math == 'bf16x3' else dt, T, dp, D) == 0
    scale = 1.0 / math.sqrt(dh)
    dense = torch.full((B * T, H * dp), SENTINEL, dtype=dt, device=dev)
    lse = torch.zeros(B, H, T, device=dev)
    ops.relpos_attention_forward(qkv, qkvT, Ed, dense, lse, B, H, T, Tp, dp, D, scale, f32_math=f32_math)
    ragged = torch.full((B * T, H * dp), SENTINEL, dtype=dt, device=dev)
    ops.relpos_attention_forward_ragged(qkv, qkvT, Ed, ragged, torch.full((B,), T, dtype=torch.int32, device=dev), B, H, T, Tp, dp, D, scale, f32_math=f32_math)
    e = assert_close_robust(ragged, dense, tol, name='ragged vs dense', max_outlier_frac=0)
    print('ragged vs dense %s T=%d dh=%d: err/scale %.3e, bit-equal %s' % (mode, T, dh, e, torch.equal(ragged, dense)))


# =========================================================================================================== BatchNorm apply
def _run_bn(dev, dt, C, B, T, len_mul, lens, two):
    """two = False: one branch into a y with halo rows (pad_y = 1: h1 of a ResBlock); True: bn2(xa) + res_norm(xb), pad_y = 0 (the block's output).
    Three launches on the same operands.  (ReLU, NaN behind every end) is the plan's call on the poison that shows a mask by arithmetic -- but the kernel's
    fmaxf(NaN, 0) is 0, exactly what a filler row must hold, so under ReLU a NaN that got through is laundered.  (no ReLU, NaN) lets it show, and (ReLU,
    a large finite value) shows an input row behind the end that was read and normalised."""
    pad_y = 0 if two else 1
    TP = T + 2 * pad_y
    g = torch.Generator().manual_seed(C + T)
    xs = [(torch.randn(B, T, C, generator=g) * 2 + 0.5).to(dt) for _ in range(2 if two else 1)]
    st = [(torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)) for _ in xs]      # mean, invstd, gamma, beta
    pre = sum((x.double() - m.double()) * (ga.double() * i.double()) + be.double() for x, (m, i, ga, be) in zip(xs, st))
    rows = [min(max(n * len_mul, 0), T) for n in lens]
    valid = torch.zeros(B, TP, dtype=torch.bool)
    for b, n in enumerate(rows):
        valid[b, pad_y:pad_y + n] = True
    sd = [tuple(t.to(dev) for t in s) for s in st]
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    tol = 2e-5 if dt == torch.float32 else 2e-2
    for relu, poison in ((True, float('nan')), (False, float('nan')), (True, 3e4)):
        want = torch.zeros(B, TP, C, dtype=torch.float64)
        xd = []
        for b, n in enumerate(rows):
            want[b, pad_y:pad_y + n] = torch.relu(pre[b, :n]) if relu else pre[b, :n]
        for x in xs:
            x = x.clone()
            for b, n in enumerate(rows):
                x[b, n:] = poison                          # inputs behind the utterance's end
            xd.append(x.to(dev))
        y = torch.full((B * TP + 8, C), SENTINEL, dtype=dt, device=dev)
        if two:
            ops.bn_apply_ragged(xd[0], sd[0], 0, y, pad_y, B, T, C, relu, lens_d, len_mul, xb=xd[1], sb=sd[1], pad_xb=0)
        else:
            ops.bn_apply_ragged(xd[0], sd[0], 0, y, pad_y, B, T, C, relu, lens_d, len_mul)
        got = y.cpu()
        tag = 'relu=%d poison=%g' % (relu, poison)
        assert torch.equal(got[B * TP:], torch.full((8, C), SENTINEL, dtype=dt)), tag + ': rows behind the last slot were written'
        got = got[:B * TP].float().view(B, TP, C)
        assert torch.isfinite(got).all(), tag + ': non-finite rows in y'
        assert float(got[~valid].abs().max()) == 0.0, tag + ': filler / halo rows are not exact zeros'
        e = assert_close_robust(got, want, tol, name='y (%s)' % tag, max_outlier_frac=0)
        print('ragged bn_apply %s C=%d B=%d T=%d len_mul=%d %s %s: err/scale %.3e' % (str(dt)[6:], C, B, T, len_mul, 'two branches pad_y=0' if two else 'one branch pad_y=1', tag, e))


DTS = [torch.float32, torch.bfloat16]
TWO = [pytest.param(False, id='one-pad1'), pytest.param(True, id='two-pad0')]


@pytest.mark.parametrize('two', TWO)
@pytest.mark.parametrize('dt', DTS, ids=['f32', 'bf16'])
@pytest.mark.parametrize('len_mul', [4, 2, 1])
def test_ragged_bn_apply_per_chunk_fallback_c24(dev, len_mul, dt, two):
    """Per-chunk fallback.  C = 24: CV = C / 8 = 3, B (T + 2 pad_y) CV is 105 .. 330 chunks, so ew_grid gives 1 or 2 workgroups of 256 (less than
    4 m = 12, m = CV / gcd(CV, 256) = 3: no rounding to a multiple of m); step32 = 256 or 512, step32 % 3 != 0 -> the loop behind the RowWalk form."""
    _run_bn(dev, dt, 24, 5, 5 * len_mul, len_mul, [5, 3, 0, 1, 9], two)


@pytest.mark.parametrize('two', TWO)
@pytest.mark.parametrize('dt', DTS, ids=['f32', 'bf16'])
def test_ragged_bn_apply_per_chunk_fallback_c768(dev, dt, two):
    """Per-chunk fallback at the product width.  C = 768: CV = 96, m = 96 / gcd(96, 256) = 3.  27 rows (pad_y = 1) are 2592 chunks -> 11 workgroups,
    21 rows (pad_y = 0) are 2016 -> 8; both below 4 m = 12, so neither is rounded to a multiple of 3, and 11 * 256 % 96 = 8 * 256 % 96 = 32 != 0."""
    _run_bn(dev, dt, 768, 3, 7, 1, [7, 2, 5], two)


@pytest.mark.parametrize('two', TWO)
@pytest.mark.parametrize('dt', DTS, ids=['f32', 'bf16'])
@pytest.mark.parametrize('len_mul', [4, 2, 1])
def test_ragged_bn_apply_row_walk_single_trip(dev, len_mul, dt, two):
    """RowWalk, one trip.  C = 16: CV = 2 divides every thread count, at most 110 rows x 2 chunks = 220 < 256 -> one workgroup, every thread at most one
    row: the prefetch of a next row never happens."""
    _run_bn(dev, dt, 16, 5, 5 * len_mul, len_mul, [5, 3, 0, 1, 9], two)


@pytest.mark.parametrize('two', TWO)
@pytest.mark.parametrize('dt', DTS, ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', [(768, 5, 480, 4, [120, 77, 0, 1, 119]), (256, 7, 1000, 2, [500, 499, 1, 250, 0, 333, 77])], ids=['c768', 'c256'])
def test_ragged_bn_apply_row_walk_multi_trip(dev, shape, dt, two):
    """RowWalk, several trips: a thread requests the chunks of its NEXT row (rows_of of the next slot) before it stores the current one (rows_of of this
    slot).  ew_grid caps the grid at 768 workgroups = 196 608 threads (SS_BN_GRID unset).  C = 768: CV = 96, m = 3, 768 is a multiple of 3 and
    196 608 % 96 = 0; 2410 (pad_y = 1) or 2400 rows x 96 chunks > 196 608, a thread steps 2048 rows = 4 slots of 482 (480) + 120, so the threads of
    slot 0 (480 valid rows) walk on into slot 4 (476).  C = 256: CV = 32, m = 1, 7014 or 7000 rows x 32 chunks > 196 608, a step is 6144 rows = 6
    slots + 132: slot 0 (1000 valid rows) into slot 6 (154)."""
    C, B, T, len_mul, lens = shape
    _run_bn(dev, dt, C, B, T, len_mul, lens, two)
