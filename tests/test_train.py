"""End-to-end runs of the two trainer entry points on a tiny synthetic dataset (MI355X only): a few optimiser steps,
one validation pass, checkpoint written with the reference's state_dict keys."""
import os

import numpy as np
import pytest
import torch

from silent_speech_amd import _lib
from silent_speech_amd.flags import FLAGS
from silent_speech_amd.synthetic import SyntheticEMGDataset


@pytest.fixture
def tiny_flags(tmp_path):
    keep = dict(FLAGS._over)
    FLAGS.model_size, FLAGS.num_layers, FLAGS.epochs = 64, 1, 1
    FLAGS.output_directory = str(tmp_path)
    yield tmp_path
    FLAGS._over.clear()
    FLAGS._over.update(keep)


@pytest.mark.gpu
def test_transduction_train_model_runs(tiny_flags):
    from silent_speech_amd import transduction_model as tm
    _lib.load()
    train = SyntheticEMGDataset(24, seed=1, min_frames=40, max_frames=120)
    devset = SyntheticEMGDataset(6, seed=2, min_frames=40, max_frames=120)
    model = tm.train_model(train, devset, 'cuda', save_sound_outputs=False, max_steps=3)
    sd = torch.load(os.path.join(str(tiny_flags), 'model.pt'))
    assert set(sd.keys()) == set(model.state_dict().keys())
    assert all(torch.isfinite(v.float()).all() for v in sd.values())
    loss, acc, conf = tm.test(model, devset, 'cuda')
    assert np.isfinite(loss) and 0.0 <= acc <= 1.0 and conf.sum() == sum(int(it['audio_features'].shape[0]) for it in devset.items)


@pytest.mark.gpu
def test_recognition_train_model_runs_and_learns(tiny_flags):
    from silent_speech_amd import recognition_model as rm
    _lib.load()
    FLAGS.learning_rate, FLAGS.learning_rate_warmup = 2e-3, 4
    train = SyntheticEMGDataset(8, seed=3, min_frames=40, max_frames=80)
    model = rm.train_model(train, train, 'cuda', n_epochs=1, max_steps=2)
    sd = torch.load(os.path.join(str(tiny_flags), 'model.pt'))
    assert 'w_out.weight' in sd and sd['w_out.weight'].shape[0] == 38 and 'w_aux.weight' not in sd
    assert all(torch.isfinite(v.float()).all() for v in sd.values())
    # the CTC loss of a fixed batch must go down under the trainer's own update rule
    batch = train.collate_raw(train.items[:4])
    from silent_speech_amd.optim import FusedAdamW
    from silent_speech_amd.transduction_model import _pack_batch
    opt = FusedAdamW(model, lr=2e-3, weight_decay=0.0)
    losses = []
    for it in range(12):
        opt.zero_grad()
        X, X_raw, sess = _pack_batch(batch, 'cuda')
        loss = rm.ctc_loss(model(X, X_raw, sess), batch, blank=37)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert np.isfinite(losses).all() and losses[-1] < 0.8 * losses[0], losses
    wer = rm.test(model, train, 'cuda')                       # one whole utterance per forward, like the reference
    wer_packed = rm.test(model, train, 'cuda', batch_size=8)  # packed 200-frame rows (context cut at row boundaries)
    assert 0.0 <= wer and 0.0 <= wer_packed


def test_fused_adamw_state_dict_round_trip():
    """state_dict() / load_state_dict() carry the fused moments and the step count (they live outside Optimizer.state)."""
    from tests import backend
    backend._ensure_emu()
    _lib.use_library_for_testing(backend.EMU)
    from silent_speech_amd.architecture import Model
    from silent_speech_amd.optim import FusedAdamW
    torch.manual_seed(0)
    m = Model(112, 80, 48, model_size=8, num_layers=1, dropout=0.0, compute_dtype=torch.float32)
    opt = FusedAdamW(m, lr=1e-2, weight_decay=0.0)
    _, gflat, n = m.flat_arenas()
    for _ in range(2):
        gflat.copy_(torch.randn(n))
        opt.step()
    sd = opt.state_dict()
    assert sd['fused']['step'] == 2 and sd['fused']['exp_avg'].numel() == n and float(sd['fused']['exp_avg'].abs().max()) > 0
    m2 = Model(112, 80, 48, model_size=8, num_layers=1, dropout=0.0, compute_dtype=torch.float32)
    m2.load_state_dict(m.state_dict())
    opt2 = FusedAdamW(m2, lr=1e-2, weight_decay=0.0)
    opt2.load_state_dict(sd)
    g = torch.randn(n)
    for mm, oo in ((m, opt), (m2, opt2)):
        mm.flat_arenas()[1].copy_(g)
        oo.step()
    assert torch.equal(m.flat_arenas()[0], m2.flat_arenas()[0])
    with pytest.raises(ValueError, match='one param group'):
        opt.add_param_group({'params': [torch.nn.Parameter(torch.zeros(1))]})
        opt.step()


@pytest.mark.gpu
def test_bench_multi_rank_path_on_one_gpu(tmp_path):
    """`bench.py --gpus 2` end to end (rendezvous, DataParallel.attach, begin_step, bucketed all-reduce from the plan's events, barriers,
    MAX / SUM reductions of the timing line, JSON) with two gloo ranks sharing the one GPU of the test box -- the driver's RCCL run is the
    first time the nccl backend itself executes, everything around it has run here.  Weak and strong scaling."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
    for scaling in ('weak', 'strong'):
        s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
        env = dict(os.environ, SS_BENCH_BACKEND='gloo', MASTER_ADDR='127.0.0.1')
        out = subprocess.check_output([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                                       '--master-port', str(port), os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '1',
                                       '--scaling', scaling, '--no-profile', '--no-legs'], env=env, timeout=600, stderr=subprocess.STDOUT).decode()
        line = [l for l in out.splitlines() if l.startswith('{')][-1]
        d = json.loads(line)
        assert d['n_gpus'] == 2 and d['scaling'] == scaling and d['steps'] == 3 and d['value'] > 0
        assert d['config']['parallelism'] == 'dp2' and d['config']['final_loss'] == d['config']['final_loss']


@pytest.mark.gpu
def test_bench_self_launches_its_ranks(tmp_path):
    """`python bench.py --gpus 2` WITHOUT torchrun: bench.py starts its own ranks (free port, MASTER_ADDR 127.0.0.1, LOCAL_RANK -> device; gloo ranks
    sharing the GPU when the box has fewer GPUs than ranks) and the rank-0 line carries what an N > 1 line is judged on: the backend and devices as the
    process group reports them, the communicators, the all-reduce bytes / bucket count / exposed time, and (--full) an N = 1 figure from the same
    call.  `--gpus 1` goes through the same entry."""
    import json
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    if torch.cuda.device_count() < 2:
        env['SS_BENCH_BACKEND'] = 'gloo'
    out = subprocess.check_output([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '1', '--no-profile', '--no-legs',
                                   '--full'], env=env, timeout=900).decode()
    d = json.loads([l for l in out.splitlines() if l.startswith('{')][-1])
    assert d['n_gpus'] == 2 and d['steps'] == 3 and d['value'] > 0 and d['config']['parallelism'] == 'dp2'
    assert d['rccl']['world_size'] == 2 and len(d['rccl']['ranks']) == 2 and d['rccl']['launcher'] == 'self'
    assert d['rccl']['schedule'] in ('two_communicators', 'single_communicator') and d['rccl']['communicators']['count'] in (1, 2)
    assert d['allreduce']['buckets'] >= 10 and 2.0e8 < d['allreduce']['bytes_per_step'] < 2.3e8          # the 53 M-float gradient arena in f32
    assert d['allreduce']['exposed_ms'] is not None and d['allreduce']['exposed_ms'] >= 0.0
    assert d['n1_comparison']['value'] and d['n1_comparison']['n_gpus'] == 1 and d['n1_comparison']['speedup_of_this_line'] > 0
    assert d['config']['unprofiled'] is not None
    out = subprocess.check_output([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--no-legs', '--cpu-rows', '0'],
                                  env=env, timeout=600).decode()
    d1 = json.loads([l for l in out.splitlines() if l.startswith('{')][-1])
    assert d1['n_gpus'] == 1 and 'rccl' not in d1 and d1['roofline']['frac'] > 0
    assert d1['config']['unprofiled'] is None          # without --full no comparison loops run after the timed one


@pytest.mark.gpu
def test_bench_four_ranks_share_one_gpu(tmp_path):
    """BASELINE configs[3] as far as one shared GPU can take it: plain `python bench.py --gpus 4` -- the self-launcher, four sampler shards, the count
    exchange, 12 BatchNorm exchanges and 10 gradient buckets per step across more than two ranks (gloo, all on the one GPU of the test box: a
    functional run of the N > 2 path and its memory, not a scaling figure).  Four ranks, because the test process and the launcher hold the GPU
    as well and no more than six processes may have it open at once; no N = 1 comparison run for the same reason.  What the driver's 8-GPU run
    adds is RCCL itself and the larger rank count."""
    import json
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    env['SS_BENCH_N1'] = '0'
    if torch.cuda.device_count() < 4:
        env['SS_BENCH_BACKEND'] = 'gloo'
    out = subprocess.check_output([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '4', '--steps', '2', '--warmup', '1', '--no-profile', '--no-legs', '--no-same'],
                                  env=env, timeout=1500).decode()
    d = json.loads([l for l in out.splitlines() if l.startswith('{')][-1])
    assert d['n_gpus'] == 4 and d['steps'] == 2 and d['value'] > 0 and d['config']['parallelism'] == 'dp4' and d['scaling'] == 'weak'
    assert d['rccl']['world_size'] == 4 and len(d['rccl']['ranks']) == 4 and sorted(r['rank'] for r in d['rccl']['ranks']) == list(range(4))
    assert d['allreduce']['buckets'] >= 10 and 2.0e8 < d['allreduce']['bytes_per_step'] < 2.3e8 and d['allreduce']['batchnorm_collectives_per_step'] == 12
    assert len(d['allreduce']['exposed_ms_per_rank']) == 4
    assert d['config']['final_loss'] == d['config']['final_loss']                     # finite on rank 0 after two 4-way steps
