"""Developer tool: the stored-audio kernels (csrc/audio.hip) alone at the loader leg's shape -- 32 utterances x 6 s at 16 kHz -> 22 050 Hz, the
shape bench.py's pipeline leg feeds at 22 050 Hz.  Reports HIP-event time per call of ss_audio_resample_batch with the phase table staged in LDS
and read through the caches (flags bit 1), its share of the 8 B-per-output-sample roofline (4 B written, ~2.9 B read per output at 441/320, counted
as the issue does: 8 B) at 8 TB/s, ss_audio_level_batch against its 4 B-per-sample roofline, the public calls (table upload + launch), and what a
user does today on the same box: scipy.signal.resample_poly per utterance on the host plus the upload.  GPU only."""
import os
import sys
import time

import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from silent_speech_amd import _lib, data_utils as D  # noqa: E402

dev = torch.device('cuda:0')
_lib.load()
L = _lib.lib()
rng = np.random.default_rng(7)
R, n = 32, 96000
up, down = D._rate_ratio(16000, 22050)
host = [np.clip(0.1 * rng.standard_normal(n), -1, 1).astype(np.float32) for _ in range(R)]
flat = torch.from_numpy(np.concatenate(host)).to(dev)
lens = [n] * R
out_lens = [D.resampled_length(n, up, down) for _ in range(R)]
io, oo = np.concatenate([[0], np.cumsum(lens)]), np.concatenate([[0], np.cumsum(out_lens)])
table = torch.from_numpy(np.stack([io[:-1], lens, oo[:-1], out_lens], 1).astype(np.int64)).to(dev)
out = torch.empty(int(oo[-1]), dtype=torch.float32, device=dev)
coef, half, tpp = D._resample_table(up, down, dev)
gains = torch.ones(R, dtype=torch.float32, device=dev)
st = _lib.stream_of(flat)


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def launch(flags, g=None):
    _lib.check(L.ss_audio_resample_batch(_lib.ptr(flat), _lib.ptr(out), _lib.ptr(table), R, up, down, half, tpp, _lib.ptr(coef), _lib.ptr(g), flags,
                                         int(oo[-1]), st), 'ss_audio_resample_batch')


total_out = int(oo[-1])
roof = 8.0 * total_out / 8e12 * 1e6
print('batch: %d utterances x %d samples at 16 kHz -> %d outputs at 22 050 Hz (%d/%d, %d taps per phase, %.1f KB table)' %
      (R, n, total_out, up, down, tpp, coef.numel() * 4 / 1024))
for name, flags in (('table in LDS', 0), ('table through the caches', 2)):
    t = timed(lambda: launch(flags))
    print('ss_audio_resample_batch, %-25s %8.1f us per call; 8 B/output = %.1f MB -> %.2f us at 8 TB/s: %.1f %% of the roofline' %
          (name + ':', t, 8.0 * total_out / 1e6, roof, roof / t * 100))
t = timed(lambda: launch(1, gains))
print('ss_audio_resample_batch, gain + clip epilogue:     %8.1f us per call' % t)
blocks = [(v + 511) // 512 for v in lens]
bo = np.concatenate([[0], np.cumsum(blocks)])
tab3 = torch.from_numpy(np.stack([io[:-1], lens, bo[:-1]], 1).astype(np.int64)).to(dev)
ws = torch.empty(2 * int(bo[-1]), dtype=torch.float32, device=dev)
level = torch.empty(R, 2, dtype=torch.float32, device=dev)
t = timed(lambda: _lib.check(L.ss_audio_level_batch(_lib.ptr(flat), _lib.ptr(tab3), R, int(bo[-1]), _lib.ptr(ws), ws.numel(), _lib.ptr(level), _lib.ptr(gains), st)))
roof_l = 4.0 * R * n / 8e12 * 1e6
print('ss_audio_level_batch (2 launches):                 %8.1f us per call; 4 B/sample = %.1f MB -> %.2f us at 8 TB/s: %.1f %% of the roofline' %
      (t, 4.0 * R * n / 1e6, roof_l, roof_l / t * 100))
t = timed(lambda: D.resample_audio_batch((flat, lens), 16000, 22050), reps=20)
print('resample_audio_batch (table upload + launch):      %8.1f us per call' % t)
t = timed(lambda: D.volume_gains((flat, lens)), reps=20)
print('volume_gains (table upload + 2 launches):          %8.1f us per call' % t)

# today: the band-limited resample per utterance on the host, then the upload of the 22 050 Hz audio
import scipy.signal  # noqa: E402
host64 = [h.astype(np.float64) for h in host]                   # what sf.read returns
ts = []
for _ in range(3):
    t0 = time.perf_counter()
    ys = [scipy.signal.resample_poly(h, up, down) for h in host64]
    t1 = time.perf_counter()
    d = torch.from_numpy(np.concatenate(ys).astype(np.float32)).to(dev)
    torch.cuda.synchronize()
    ts.append((t1 - t0, time.perf_counter() - t1))
rs, upl = float(np.median([a for a, _ in ts])), float(np.median([b for _, b in ts]))
print('host today: scipy.signal.resample_poly x %d: %.1f ms + concatenate / upload of %.1f MB: %.2f ms (median of 3)' % (R, rs * 1e3, d.numel() * 4 / 1e6, upl * 1e3))
err = float((D.resample_audio_batch((flat[:n], [n]), 16000, 22050)[0].cpu().double() - torch.from_numpy(ys[0])).abs().max())
print('max |device - scipy| on utterance 0: %.3g' % err)
