"""Parity AT THE SIZE THE BENCH RUNS (BASELINE.json configs[1]: 768-d / 6-layer model, one reference-size batch of
~22 000 frames = 110 packed rows).  The golden-vector tests pin the math at d <= 64; here the SAME kernels the benchmark
launches (8-wave / 2-wave / direct-to-LDS GEMM variants on 22 000 .. 88 000-row operands, the grouped weight-gradient
kernel over 22 000 frames, the LDS-resident attention with its half-workgroup tail at 880 (sequence, head) pairs) are
compared with the CPU oracle / a torch fp32 matmul on the real shapes, and `ss_gemm_last_kernel()` is asserted so that
every variant is known to have run.  GPU only; the oracle step runs once per module on the host (tens of seconds)."""
import json
import os

import numpy as np
import pytest
import torch

from silent_speech_amd import _lib, ops
from silent_speech_amd._lib import OP_OC
from tests.util import assert_close_robust, rel_l2_cos

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


class _FixedShift(object):
    @staticmethod
    def randrange(n):
        return 3


@pytest.fixture(scope='module')
def cuda():
    _lib.load()
    assert not _lib.is_emulator() and torch.cuda.is_available()
    return torch.device('cuda')


DROP_P = 0.2            # BASELINE configs[1] / the bench: FLAGS.dropout of the reference (architecture.py:13)
SEED_BASE = 0xBE7C


@pytest.fixture(scope='module')
def cfg2(cuda):
    """Weights and batch of the full-size step, plus a cache of oracle runs keyed by (dropout p, attention hash family, storage):
    forward / loss / gradients of `oracle/model_ref` on the SAME dropout masks the kernels draw (`oracle/dropout_ref`)."""
    from silent_speech_amd.architecture import Model
    from silent_speech_amd.synthetic import reference_size_batch
    torch.manual_seed(0)
    m = Model(112, 80, 48, model_size=768, num_layers=6, dropout=0.0, compute_dtype=torch.float32)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    return dict(sd=sd, batch=reference_size_batch(seed=0), runs={})


def _oracle(cfg2, p, resident, seed, storage=False):
    from oracle import dropout_ref, loss_ref, model_ref
    key = (p, int(resident) if p > 0 else None, seed if p > 0 else None, storage)
    if key in cfg2['runs']:
        return cfg2['runs'][key]
    ref = {k: v.clone() for k, v in cfg2['sd'].items()}
    for v in ref.values():
        if v.dtype == torch.float32:
            v.requires_grad_(True)
    batch = cfg2['batch']
    xr = loss_ref.combine_fixed_length(batch['raw_emg'], 1600)
    masks = dropout_ref.layer_masks(seed, 6, xr.shape[0], 200, 768, 8, 3072, p, resident) if p > 0 else None

    def run():
        pr, ar = model_ref.model_forward(ref, xr, training=True, shift_r=3, running_out={}, layer_masks=masks, dropout_p=p)
        lref, _ = loss_ref.dtw_loss_ref(pr, ar, batch)
        lref.backward()
        return pr, ar, lref
    if storage:
        with model_ref.bf16_storage():
            pr, ar, lref = run()
    else:
        pr, ar, lref = run()
    out = dict(pred=pr.detach(), aux=ar.detach(), loss=float(lref),
               grads={k: v.grad for k, v in ref.items() if v.dtype == torch.float32 and v.grad is not None})
    cfg2['runs'][key] = out
    return out


def _step(cfg2, dt, dev, p=0.0, f32_matmul='exact'):
    from silent_speech_amd.architecture import Model
    from silent_speech_amd.transduction_model import _pack_batch, dtw_loss
    m = Model(112, 80, 48, model_size=768, num_layers=6, dropout=p, compute_dtype=dt, f32_matmul=f32_matmul)
    m.load_state_dict(cfg2['sd'], strict=True)
    m.to(dev)
    m.shift_rng = _FixedShift
    m.set_seed(SEED_BASE)
    m.train()
    batch = cfg2['batch']
    X, X_raw, sess = _pack_batch(batch, dev)
    assert X_raw.shape[0] >= 100, 'reference-size batch expected (~110 rows), got %d' % X_raw.shape[0]
    pred, aux = m(X, X_raw, sess)
    loss, _ = dtw_loss(pred, aux, batch, phoneme_loss_weight=0.5)
    loss.backward()
    torch.cuda.synchronize()
    return m, pred.detach().float().cpu(), aux.detach().float().cpu(), float(loss)


def _record(name, payload):
    out = os.path.join(ROOT, 'gpurun_out')
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, 'fullsize_parity.json')
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[name] = payload
    json.dump(data, open(path, 'w'), indent=1, sort_keys=True)
    short = {k: v for k, v in payload.items() if k != 'per_tensor'}
    print('fullsize parity %s: %s' % (name, json.dumps(short)))


def _skip_grad(n):
    # conv biases feed training-mode BatchNorm: identically zero gradient (the reference holds rounding noise)
    return 'relative_positional' in n or (n.endswith('.bias') and ('conv1' in n or 'conv2' in n or 'residual_path' in n))


def _grad_figures(m, want, yard=None):
    """Per tensor: relative L2 error, cosine, max error over max (and the same for the bf16-storage yardstick)."""
    from tests.test_dropout_parity import yardstick_levels
    names = [n for n, _ in m.named_parameters() if not _skip_grad(n)]
    ylev = yardstick_levels(yard, want, names) if yard is not None else None
    rows = {}
    for n, p in m.named_parameters():
        if 'relative_positional' in n:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0
        if n not in names:
            continue
        rl2, cos = rel_l2_cos(p.grad, want[n])
        g, w = p.grad.detach().float().cpu(), want[n]
        rows[n] = {'rel_l2': rl2, 'cos': cos, 'max_err_over_max': float((g - w).abs().max() / (w.abs().max() + 1e-30))}
        if yard is not None:
            y2, yc = rel_l2_cos(yard[n], want[n])
            rows[n].update(yard_rel_l2=y2, yard_cos=yc, yard_level=ylev[n],
                           yard_max_err_over_max=float((yard[n] - w).abs().max() / (w.abs().max() + 1e-30)))
    return rows


def _full_step_check(cfg2, cuda, dt, p, tag, f32_matmul='exact'):
    """fp32 kernels: north_star's bar (mel-L1 of `pred` < 1e-4 vs the reference function), loss 1e-4 relative, every gradient tensor
    within 2e-3 relative L2 and cosine >= 0.99999.  bf16 kernels (the bench dtype): recorded, and bounded tensor by tensor by twice
    the deviation of the oracle itself under bf16 storage (the yardstick; see tests/test_dropout_parity.py)."""
    f32 = dt == torch.float32
    m, pred, aux, loss = _step(cfg2, dt, cuda, p, f32_matmul)
    resident = m.attention_mask_family(200)       # 0 per-tile, 2 transposed 32 x 32: selects the mask restatement
    ref = _oracle(cfg2, p, resident, m.last_seed)
    yard = None if f32 else _oracle(cfg2, p, resident, m.last_seed, storage=True)
    l1 = float((pred - ref['pred']).abs().mean())
    rows = _grad_figures(m, ref['grads'], None if f32 else yard['grads'])
    worst = max(rows, key=lambda n: rows[n]['rel_l2'])
    payload = {'dropout': p, 'mel_l1': l1, 'loss': loss, 'loss_oracle': ref['loss'], 'rows': int(ref['pred'].shape[0]),
               'worst_grad': worst, 'worst_rel_l2': rows[worst]['rel_l2'], 'min_cos': min(r['cos'] for r in rows.values()),
               'median_rel_l2': float(np.median([r['rel_l2'] for r in rows.values()])),
               'worst_max_err_over_max': max(r['max_err_over_max'] for r in rows.values()), 'per_tensor': rows}
    if not f32:
        payload.update(yard_mel_l1=float((yard['pred'] - ref['pred']).abs().mean()), yard_loss=yard['loss'],
                       yard_worst_rel_l2=max(r['yard_rel_l2'] for r in rows.values()),
                       yard_worst_max_err_over_max=max(r['yard_max_err_over_max'] for r in rows.values()))
    _record(tag, payload)
    g_l2, g_cos = (2e-3, 0.99999) if f32_matmul == 'exact' else (1e-2, 0.9999)
    if f32:
        assert l1 < 1e-4, 'mel-L1 %g' % l1
        assert_close_robust(pred, ref['pred'], 2e-4, name='pred', max_outlier_frac=0)
        assert_close_robust(aux, ref['aux'], 2e-4, name='aux', max_outlier_frac=0)
        assert abs(loss - ref['loss']) < 1e-4 * abs(ref['loss']), (loss, ref['loss'])
        for n, r in rows.items():
            assert r['rel_l2'] <= g_l2 and r['cos'] >= g_cos, (n, r)
    else:
        assert l1 <= 2.0 * payload['yard_mel_l1'] + 1e-3, (l1, payload['yard_mel_l1'])
        assert_close_robust(pred, ref['pred'], 6e-2, name='pred', max_outlier_frac=1e-3)
        assert abs(loss - ref['loss']) < 2e-2 * abs(ref['loss']), (loss, ref['loss'])
        for n, r in rows.items():
            assert r['rel_l2'] <= 2.0 * r['yard_level'] + 1e-2, (n, r)


def test_full_step_fp32_vs_oracle(cfg2, cuda):
    """north_star: mel-L1 within 1e-4 of the reference, at the benchmarked size, exact-f32 kernels, dropout off."""
    _full_step_check(cfg2, cuda, torch.float32, 0.0, 'fp32')


def test_full_step_fp32_dropout_vs_oracle(cfg2, cuda):
    """The benchmarked mode (dropout 0.2) in exact-f32 kernels: same bars, masks restated by oracle/dropout_ref.py."""
    _full_step_check(cfg2, cuda, torch.float32, DROP_P, 'fp32_dropout')


def test_full_step_fp32_storage_bf16x3_matmul_vs_oracle(cfg2, cuda):
    """The parity-grade FAST mode (f32 storage between the kernels, every GEMM / attention product on three bf16 MFMAs, f32 accumulate;
    Model(f32_matmul='bf16x3')): held to north_star's bar like the exact-f32 kernels -- mel-L1 < 1e-4, pred 2e-4, loss 1e-4 -- and every gradient
    tensor within 1e-2 relative L2 / cosine 0.9999.  Measured: mel-L1 7.9e-6 (exact f32 9e-7, bf16 5.7e-3), median gradient tensor 3.9e-5
    (1.3e-5 / 4e-3), worst tensor conv_blocks.0.conv1.weight 5.1e-3 (1.5e-3 / 0.15): the 2^-17 operand rounding is amplified by the same
    path (three BatchNorms, the DTW alignment) that amplifies the f32 rounding of the exact kernels to 1.5e-3."""
    _full_step_check(cfg2, cuda, torch.float32, 0.0, 'fp32_bf16x3', f32_matmul='bf16x3')


def test_full_step_fp32_storage_bf16x3_matmul_dropout_vs_oracle(cfg2, cuda):
    _full_step_check(cfg2, cuda, torch.float32, DROP_P, 'fp32_bf16x3_dropout', f32_matmul='bf16x3')


def test_full_step_bf16_dropout_vs_oracle(cfg2, cuda):
    """THE benchmarked configuration: bf16 kernels, dropout 0.2, 110 rows: LDS-resident attention writing the probability image with
    the dropout decision in the sign bit, backward from it, GEMM-epilogue dropout + gate, add_dropout_ln."""
    _full_step_check(cfg2, cuda, torch.bfloat16, DROP_P, 'bf16_dropout')


def test_full_step_bf16_vs_oracle(cfg2, cuda):
    """bf16 kernels with dropout off (mel-L1 of the bench line's `parity` object)."""
    _full_step_check(cfg2, cuda, torch.bfloat16, 0.0, 'bf16')


# ------------------------------------------------------------------ GEMM shape classes of the step, every kernel variant
VARIANTS = [          # (name, {option: value}, expected ss_gemm_last_kernel)
    ('glds-128', {ops.GEMM_OPT_G8: 0, ops.GEMM_OPT_W2: 0}, 1),
    ('w2-128', {ops.GEMM_OPT_G8: 0, ops.GEMM_OPT_W2: 2, ops.GEMM_OPT_W2_BM: 128}, 2),
    ('w2-144', {ops.GEMM_OPT_G8: 0, ops.GEMM_OPT_W2: 2, ops.GEMM_OPT_W2_BM: 144}, 2),
    ('gemm8-256-burst', {ops.GEMM_OPT_G8: 2, ops.GEMM_OPT_G8_NI: 8, ops.GEMM_OPT_G8_PIN: 0}, 3),
    ('gemm8-256-spread', {ops.GEMM_OPT_G8: 2, ops.GEMM_OPT_G8_NI: 8, ops.GEMM_OPT_G8_PIN: 1}, 3),
    ('gemm8-288-burst', {ops.GEMM_OPT_G8: 2, ops.GEMM_OPT_G8_NI: 9, ops.GEMM_OPT_G8_PIN: 0}, 4),
    ('gemm8-288-spread', {ops.GEMM_OPT_G8: 2, ops.GEMM_OPT_G8_NI: 9, ops.GEMM_OPT_G8_PIN: 1}, 4),
]


@pytest.fixture
def knobs():
    yield
    for what in range(5):
        ops.gemm_set_option(what, -1)


def _all_variants(run, want, name):
    first = None
    for vname, opts, kernel in VARIANTS:
        for what in range(5):
            ops.gemm_set_option(what, -1)
        for what, v in opts.items():
            ops.gemm_set_option(what, v)
        C = run()
        assert _lib.lib().ss_gemm_last_kernel() == kernel, (name, vname, _lib.lib().ss_gemm_last_kernel())
        assert_close_robust(C, want, 1.5e-2, name='%s %s' % (name, vname), max_outlier_frac=0)
        if first is None:
            first = C.clone()
        else:
            assert torch.equal(C, first), '%s: %s differs bitwise from %s (same f32 accumulation order expected)' % (name, vname, VARIANTS[0][0])
    for what in range(5):
        ops.gemm_set_option(what, -1)
    run()
    return _lib.lib().ss_gemm_last_kernel()


@pytest.mark.parametrize('shape', [(22000, 768, 768), (22000, 2304, 768), (22000, 3072, 768), (22000, 768, 3072), (22000, 768, 2304)])
def test_gemm_step_shapes_every_variant(cuda, knobs, shape):
    M, N, K = shape
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).to(cuda); b = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(cuda)
    bias = torch.randn(N, generator=g).to(cuda)
    want = torch.relu(a.float() @ b.float().t() + bias)

    def run():
        C = torch.zeros(M, N, dtype=torch.bfloat16, device=cuda)
        ops.gemm(a, b, C, M, N, K, ops.rowmap(K), ops.rowmap(K), ops.rowmap(N), bias=bias, relu=True)
        return C
    picked = _all_variants(run, want, 'gemm %s' % (shape,))
    assert picked in (3, 4), 'the cost model should pick the 8-wave kernel for %s, picked %d' % (shape, picked)


@pytest.mark.parametrize('rows_t', [(800, 1), (400, 2)])
def test_conv_rowmaps_at_step_size_every_variant(cuda, knobs, rows_t):
    """ResBlock convolutions as implicit GEMM at the real sizes: 110 sequences, C = 768, K = 2304; stride 1 over the 800-frame
    buffer (88 000 rows) and stride 2 (800 -> 400 frames, 44 000 rows)."""
    Tin, stride = (800, 1) if rows_t == (800, 1) else (800, 2)
    Bn, C = 110, 768
    Tout = Tin // stride
    g = torch.Generator().manual_seed(Tout)
    x = torch.zeros(Bn, Tin + 2, C, dtype=torch.bfloat16)
    x[:, 1:-1] = (torch.randn(Bn, Tin, C, generator=g) * 0.5).to(torch.bfloat16)
    w = (torch.randn(C, C, 3, generator=g) * 0.03).to(torch.bfloat16)
    xd, wd = x.to(cuda), w.permute(0, 2, 1).reshape(C, 3 * C).contiguous().to(cuda)
    want = torch.nn.functional.conv1d(xd[:, 1:-1].float().transpose(1, 2), w.to(cuda).float(), None, stride=stride, padding=1).transpose(1, 2).reshape(Bn * Tout, C)

    def run():
        y = torch.zeros(Bn * Tout, C, dtype=torch.bfloat16, device=cuda)
        ops.gemm(xd, wd, y, Bn * Tout, C, 3 * C, ops.rowmap(stride * C, Tout, (Tin + 2) * C), ops.rowmap(3 * C), ops.rowmap(C))
        return y
    _all_variants(run, want, 'conv stride %d' % stride)


def test_weight_gradient_kernels_at_step_size(cuda):
    """dW = dY^T X over the 22 000 frames: the 128-wide transposing-read kernel with the engine's split-K, and the grouped
    8-wave kernel on the four weight gradients of an encoder layer in one launch."""
    from silent_speech_amd import engine
    R = 22000
    g = torch.Generator().manual_seed(5)
    shapes = [(768, 3072), (3072, 768), (768, 768), (2304, 768)]
    dys = [(torch.randn(R, n, generator=g) * 0.05).to(torch.bfloat16).to(cuda) for n, _ in shapes]
    xs = [torch.randn(R, k, generator=g).to(torch.bfloat16).to(cuda) for _, k in shapes]
    wants = [dy.float().t() @ x.float() for dy, x in zip(dys, xs)]
    outs = [torch.zeros(n, k, device=cuda) for n, k in shapes]
    for dy, x, o, (n, k) in zip(dys, xs, outs, shapes):
        ops.gemm(dy, x, o, n, k, R, ops.rowmap(n), ops.rowmap(k), ops.rowmap(k), a_mode=OP_OC, b_mode=OP_OC, mode=2, split_k=engine._split_k(n, k, R))
        assert _lib.lib().ss_gemm_last_kernel() == 0
    for o, w, sh in zip(outs, wants, shapes):
        assert_close_robust(o, w, 2e-3, name='dW 128-wide %s' % (sh,), max_outlier_frac=0)
    outs2 = [torch.zeros(n, k, device=cuda) for n, k in shapes]
    ops.gemm_dw_grouped([(dy, x, o, n, k, R, ops.rowmap(n), ops.rowmap(k), k) for dy, x, o, (n, k) in zip(dys, xs, outs2, shapes)])
    for o, w, sh in zip(outs2, wants, shapes):
        assert_close_robust(o, w, 2e-3, name='dW grouped %s' % (sh,), max_outlier_frac=0)


def test_attention_at_step_size(cuda):
    """B = 110 rows x 8 heads = 880 (sequence, head) pairs on the persistent grid of the forward and the query-major backward (256 workgroups on
    256 CUs, each walking the pairs blockIdx.x, + 256, ...): three full rounds plus a fourth in which 112 workgroups take one more pair and the
    other 144 have left the loop.  The key-major backward launches one workgroup per pair."""
    from tests.test_attention import _run
    _run(cuda, torch.bfloat16, B=110, H=8, T=200, dh=96, D=100, seed=110, tol_f=2e-2, tol_b=3e-2)
