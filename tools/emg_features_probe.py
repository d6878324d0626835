"""Developer tool: the hand-crafted EMG feature leg (csrc/emg_features.hip, ss_emg_features_batch) at the loader's shapes -- 40 recordings of
3-6 s, 8 channels, at 516.79 Hz.  Reports HIP-event time per batch call (table upload + the one launch), the time of the launch alone, the
bytes it must move (reads 8 C sum n, writes 4 112 sum F) against the 8 TB/s HBM roofline, and the median of DeviceBatchBuilder.build with
emg_features on and off (alternating builds, so clocks and the pinned staging ring affect both alike).  GPU only."""
import os
import sys
import time

import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from silent_speech_amd import _lib, read_emg  # noqa: E402
from silent_speech_amd.pipeline import DeviceBatchBuilder  # noqa: E402

dev = torch.device('cuda:0')
_lib.load()
rng = np.random.default_rng(7)
R, C = 40, 8
lens_1k = [int(v) for v in rng.integers(3000, 6001, R)]
lens = [read_emg.resampled_length(n, 516.79, 1000) for n in lens_1k]
frames = [read_emg.feature_frames(n) for n in lens]
packed = torch.from_numpy(rng.standard_normal((sum(lens), C)) * 30.0).to(dev)
offs = np.concatenate([[0], np.cumsum(lens)])
views = [packed[offs[u]:offs[u + 1]] for u in range(R)]


def timed(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


t_call = timed(lambda: read_emg.emg_features_batch(views))
oo = np.concatenate([[0], np.cumsum(frames)])
table = torch.from_numpy(np.stack([offs[:-1], lens, oo[:-1], frames], 1).astype(np.int64)).to(dev)
out = torch.empty(int(oo[-1]), 14 * C, dtype=torch.float32, device=dev)
L = _lib.lib()
t_launch = timed(lambda: _lib.check(L.ss_emg_features_batch(_lib.ptr(packed), _lib.ptr(out), _lib.ptr(table), R, C, int(oo[-1]), _lib.stream_of(packed))))
rd, wr = 8 * C * sum(lens), 4 * 14 * C * sum(frames)
print('batch: %d recordings, sum n = %d samples at 516.79 Hz, sum F = %d frames, %d channels' % (R, sum(lens), sum(frames), C))
print('emg_features_batch (table upload + 1 launch): %7.1f us per batch' % t_call)
print('ss_emg_features_batch launch alone:           %7.1f us per batch' % t_launch)
print('bytes: %.2f MB read + %.2f MB written = %.2f MB -> %.2f us at 8 TB/s (%.1f %% of the roofline at the launch time)' %
      (rd / 1e6, wr / 1e6, (rd + wr) / 1e6, (rd + wr) / 8e12 * 1e6, (rd + wr) / 8e12 * 1e6 / t_launch * 100))

# the loader leg: DeviceBatchBuilder.build with the features off / on, alternating
recs = []
for i in range(R):
    n = lens_1k[i]
    x = np.cumsum(rng.standard_normal((n + 400, 8)), 0) + 40.0 * np.sin(2 * np.pi * 60.0 * np.arange(n + 400) / 1000.0)[:, None] + rng.standard_normal((n + 400, 8)) * 30.0
    T = n * 22050 // 1000 // 256
    recs.append({'raw_emg': x[200:200 + n], 'raw_emg_before': x[:200], 'raw_emg_after': x[200 + n:], 'silent': i % 5 == 1,
                 'audio': np.clip(0.1 * rng.standard_normal(256 * (T + 2)), -1, 1).astype(np.float32), 'text_int': np.zeros(3, dtype=np.int64)})
    if recs[-1]['silent']:
        m = int(rng.integers(3000, 6001))
        y = np.cumsum(rng.standard_normal((m, 8)), 0) + rng.standard_normal((m, 8)) * 30.0
        recs[-1]['parallel'] = {'raw_emg': y, 'silent': False, 'audio': np.clip(0.1 * rng.standard_normal(256 * (m * 22050 // 1000 // 256 + 2)), -1, 1).astype(np.float32)}
builders = {False: DeviceBatchBuilder(dev), True: DeviceBatchBuilder(dev, emg_features=True)}
for _ in range(10):
    for on in (False, True):
        builders[on].build(recs)
torch.cuda.synchronize()
ts = {False: [], True: []}
for _ in range(15):
    for on in (False, True):
        t0 = time.perf_counter()
        builders[on].build(recs)
        torch.cuda.synchronize()
        ts[on].append(time.perf_counter() - t0)
off, on = float(np.median(ts[False])) * 1e3, float(np.median(ts[True])) * 1e3
print('DeviceBatchBuilder.build, %d recordings (%d silent with twins): emg_features off %.3f ms, on %.3f ms (median of 15, alternating): +%.3f ms' %
      (R, sum(r['silent'] for r in recs), off, on, on - off))
