"""Developer tool: whole-utterance inference as ragged batches (transduction_model.predict_utterances: plan_ragged_groups +
Model.forward_utterances, one native plan call per group) against the loop it replaces (predict_utterance: one plan call per utterance,
batch of 1), on the data of bench.py's eval.whole_utterance leg -- SyntheticEMGDataset(16, seed=6, min_frames=600, max_frames=1000,
silent_fraction=0.0), 768-d / 6 layers -- in bf16 and in f32 storage with bf16x3 matmuls.  Both are timed in the same process, alternating,
3 warm rounds, then the median of --rounds rounds each (host clock around a round that ends in a device synchronise); the spread reported is
(max - min) of the timed rounds.  Also: the padding share and the number of groups, the per-kernel rows of one profiled round of either
(ss_plan_profile), and the max |difference| between the two outputs on the timed inputs (asserted: 8e-2 of scale for bf16, 2e-4 for
bf16x3).  GPU only.

    python tools/ragged_inference_probe.py [--out profiles/ragged_inference_probe.txt] [--rounds 10] [--modes bf16,bf16x3]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from silent_speech_amd import _lib, engine  # noqa: E402
from silent_speech_amd.architecture import Model  # noqa: E402
from silent_speech_amd.synthetic import SyntheticEMGDataset  # noqa: E402
from silent_speech_amd.transduction_model import MAX_PADDING, MAX_SLOT_FRAMES, plan_ragged_groups, predict_utterance, predict_utterances  # noqa: E402

MODES = {'bf16': (dict(compute_dtype=torch.bfloat16), 8e-2), 'bf16x3': (dict(compute_dtype=torch.float32, f32_matmul='bf16x3'), 2e-4)}


def timed_round(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def profile_rows(model, fn):
    """Per-kernel rows of ONE call of fn (HIP events around every launch of the native plan)."""
    pb = engine.plan_binding(model)
    L = pb.lib
    L.ss_plan_profile(pb.handle, 1)
    fn()
    torch.cuda.synchronize()
    rows = (_lib.ProfileRow * 64)()
    n = L.ss_plan_profile_read(pb.handle, rows, 64)
    L.ss_plan_profile(pb.handle, 0)
    return sorted(((rows[i].name.decode(), int(rows[i].calls), rows[i].seconds * 1e3, rows[i].flops) for i in range(n)), key=lambda r: -r[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'ragged_inference_probe.txt'))
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--modes', default='bf16,bf16x3')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    _lib.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ds = SyntheticEMGDataset(16, seed=6, min_frames=600, max_frames=1000, silent_fraction=0.0)
    points = [ds[i] for i in range(len(ds))]
    lengths = [int(p['emg'].shape[0]) for p in points]
    groups = plan_ragged_groups(lengths, MAX_SLOT_FRAMES, MAX_PADDING)
    slots = sum(len(g) * max(lengths[i] for i in g) for g in groups)
    say('whole-utterance inference on %s: %d utterances of %d..%d frames (%d in all), 768-d / 6 layers' %
        (torch.cuda.get_device_name(0), len(points), min(lengths), max(lengths), sum(lengths)))
    say('ragged groups (<= %d slot frames, <= %.0f %% filler): %d groups of %s utterances, %d slot frames, %.1f %% filler' %
        (MAX_SLOT_FRAMES, 100 * MAX_PADDING, len(groups), [len(g) for g in groups], slots, 100.0 * (slots - sum(lengths)) / slots))
    failures = []
    for mode in a.modes.split(','):
        kw, bar = MODES[mode]
        torch.manual_seed(0)
        model = Model(112, 80, 48, model_size=768, num_layers=6, dropout=0.2, **kw).to(dev)

        def loop():
            return [predict_utterance(model, p, dev) for p in points]

        def ragged():
            return predict_utterances(model, points, dev)
        for _ in range(3):
            loop()
            ragged()
        t_loop, t_rag = [], []
        for _ in range(max(a.rounds, 10)):
            ms, want = timed_round(loop)
            t_loop.append(ms)
            ms, got = timed_round(ragged)
            t_rag.append(ms)
        scale = max(float(w.abs().max()) for w in want)
        diff = max(float((g.float() - w.float()).abs().max()) for g, w in zip(got, want))
        m_loop, m_rag = float(np.median(t_loop)), float(np.median(t_rag))
        s_loop, s_rag = max(t_loop) - min(t_loop), max(t_rag) - min(t_rag)
        say('%s:' % mode)
        say('  loop of predict_utterance   median %8.3f ms of %d rounds (min %.3f, max %.3f, spread %.3f)  %.2f M frames/s' %
            (m_loop, len(t_loop), min(t_loop), max(t_loop), s_loop, sum(lengths) / m_loop / 1e3))
        say('  predict_utterances (ragged) median %8.3f ms of %d rounds (min %.3f, max %.3f, spread %.3f)  %.2f M frames/s' %
            (m_rag, len(t_rag), min(t_rag), max(t_rag), s_rag, sum(lengths) / m_rag / 1e3))
        say('  ratio loop / ragged %.2f x; difference of the medians %.3f ms against the larger spread %.3f ms: %s' %
            (m_loop / m_rag, m_loop - m_rag, max(s_loop, s_rag), 'faster' if m_loop - m_rag > max(s_loop, s_rag) else 'NOT faster by more than the spread'))
        say('  max |ragged - loop| = %.3e = %.3e of scale %.3f (bar %.0e)' % (diff, diff / scale, scale, bar))
        for name, fn in (('loop', loop), ('ragged', ragged)):
            rows = profile_rows(model, fn)
            say('  per-kernel rows of one profiled round, %s (%.3f ms of kernels):' % (name, sum(r[2] for r in rows)))
            for n, calls, ms, flops in rows:
                say('    %-52s %5d launches %8.3f ms %8.1f TFLOP/s' % (n, calls, ms, flops / max(ms, 1e-9) / 1e9))
        if diff > bar * scale:
            failures.append('%s: ragged and per-utterance outputs differ by %.3e of scale (bar %.0e)' % (mode, diff / scale, bar))
        del model
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    assert not failures, failures


if __name__ == '__main__':
    main()
