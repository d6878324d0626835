"""Developer tool: the spectral-gating kernels (csrc/spectral_gate.hip) alone at the loader leg's shape -- 32 utterances x 6 s at 16 kHz, the shape
tools/audio_resample_probe.py feeds the resampler.  Reports the HIP-event time of ss_spectral_gate_batch per call (analysis + synthesis + overlap-add)
with and without mask smoothing, the analysis kernel alone through ss_spectral_gate_profile over the whole batch taken as one clip (the per-kernel
split of the three launches comes from `rocprofv3 --kernel-trace --stats -- python tools/spectral_gate_probe.py`), the achieved share
of the algorithmic traffic (4 B in + 4 B out per sample at 8 TB/s; the bit rows add 2 x 68 B and the windowed-frame workspace 2 x 4096 B per frame of 256
new samples, written and read back: 0.5 B and 32 B per sample), the public calls, and the float64 oracle (tests/spectral_gate_oracle.py) on the same batch on the host.
--nonstationary adds the non-stationary gate (csrc/spectral_gate_ns.hip, ss_spectral_gate_ns_batch: magnitudes + level + synthesis + overlap-add) of the
same batch in the same run, alternating with the stationary gate, its traffic (4 B in + 4 B out per sample; per frame of 256 new samples three rows of
513 floats written -- A, s, m0 --, three read by the level pass and 2 n_t + 1 read by the synthesis, of which all but one hit the caches: 104 B per
sample at n_t = 3 counting every read; the frame workspace as above: 32 B) and its float64 oracle on utterance 0;
the split over its four launches comes from the same rocprofv3 command with --nonstationary.
GPU only."""
import argparse
import os
import sys
import time

import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from silent_speech_amd import _lib, data_utils as D  # noqa: E402
from tests import spectral_gate_oracle as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--nonstationary', action='store_true', help='also time the non-stationary gate on the same batch')
args = ap.parse_args()
dev = torch.device('cuda:0')
_lib.load()
L = _lib.lib()
rng = np.random.default_rng(7)
R, n, sr = 32, 96000, 16000
t = np.arange(n) / sr
host = [(0.2 * np.sin(2 * np.pi * (200 + 40 * u) * t) * (rng.uniform(size=n) > 0.3) + 0.01 * rng.standard_normal(n)).astype(np.float32) for u in range(R)]
noise = (0.01 * rng.standard_normal(sr)).astype(np.float32)
flat = torch.from_numpy(np.concatenate(host)).to(dev)
lens = [n] * R
table, total_frames = D._gate_table(lens, dev)
win = D._gate_windows(dev)
prof = D.NoiseProfile.from_noise(noise, sr)
n_f, n_t = D.gate_smoothing(sr)
out = torch.empty_like(flat)
bits_ws = torch.empty((total_frames, 17), dtype=torch.int32, device=dev)
rowmax = torch.empty((R, 513), dtype=torch.int32, device=dev)
frames = torch.empty((total_frames, 1024), dtype=torch.float32, device=dev)
st = _lib.stream_of(flat)


def timed(fn, reps=30, rounds=5):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / reps * 1e3)
    return float(np.median(ts))


def gate(nf=n_f, nt=n_t):
    _lib.check(L.ss_spectral_gate_batch(_lib.ptr(flat), _lib.ptr(out), _lib.ptr(table), R, total_frames, _lib.ptr(win), _lib.ptr(prof.thresh), nf, nt, 1.0,
                                        _lib.ptr(bits_ws), _lib.ptr(rowmax), _lib.ptr(frames), None, st), 'ss_spectral_gate_batch')


# the analysis kernel alone: the profile entry point runs it (with the f64 dB rows instead of the bits) over the whole batch taken as ONE clip
one_table, one_frames = D._gate_table([n * R], dev)
db_ws = torch.empty((one_frames, 513), dtype=torch.float64, device=dev)
thr = torch.empty(513, dtype=torch.float32, device=dev)


def profile_all():
    _lib.check(L.ss_spectral_gate_profile(_lib.ptr(flat), _lib.ptr(one_table), one_frames, _lib.ptr(win), 1.5, _lib.ptr(db_ws), _lib.ptr(rowmax), _lib.ptr(thr), st),
               'ss_spectral_gate_profile')


samples = R * n
roof = 8.0 * samples / 8e12 * 1e6
print('batch: %d utterances x %d samples at %d Hz = %d frames; mask smoothing %d rows x %d frames' % (R, n, sr, total_frames, n_f, n_t))
t_def = timed(gate)
t_none = timed(lambda: gate(0, 0))
print('ss_spectral_gate_batch, default smoothing: %8.1f us per call; 8 B/sample = %.1f MB -> %.2f us at 8 TB/s: %.1f %% of the algorithmic roofline' %
      (t_def, 8.0 * samples / 1e6, roof, roof / t_def * 100))
print('   with the bit rows (%.2f MB written + read) and the frame workspace (%.1f MB written + read): %.1f MB -> %.1f %% of 8 TB/s' %
      (2 * 68 * total_frames / 1e6, 2 * 4096 * total_frames / 1e6, (8.0 * samples + 2 * 4164 * total_frames) / 1e6,
       (8.0 * samples + 2 * 4164 * total_frames) / 8e12 * 1e6 / t_def * 100))
print('ss_spectral_gate_batch, no smoothing:      %8.1f us per call' % t_none)
print('ss_spectral_gate_profile over %d frames (analysis kernel writing f64 dB + reduction): %8.1f us per call' % (one_frames, timed(profile_all)))
print('reduce_noise_batch (table upload + 3 launches): %8.1f us per call' % timed(lambda: D.reduce_noise_batch((flat, lens), prof), reps=10))
print('NoiseProfile.from_noise, 1 s clip:              %8.1f us per call' % timed(lambda: D.NoiseProfile.from_noise(noise, sr), reps=10))

if args.nonstationary:
    from tests import spectral_gate_ns_oracle as NO  # noqa: E402
    b = D.nonstationary_coefficient(sr)
    mag = torch.empty((total_frames, 513), dtype=torch.float32, device=dev)
    level = torch.empty((total_frames, 513), dtype=torch.float32, device=dev)
    out_ns = torch.empty_like(flat)

    def gate_ns(nf=n_f, nt=n_t):
        _lib.check(L.ss_spectral_gate_ns_batch(_lib.ptr(flat), _lib.ptr(out_ns), _lib.ptr(table), R, total_frames, _lib.ptr(win), b, 2.0, 10.0, nf, nt, 1.0,
                                               _lib.ptr(mag), _lib.ptr(level), _lib.ptr(frames), None, st), 'ss_spectral_gate_ns_batch')

    pairs = [(timed(gate, rounds=3), timed(gate_ns, rounds=3)) for _ in range(3)]          # the two gates alternating in one run
    t_st, t_ns = float(np.median([p[0] for p in pairs])), float(np.median([p[1] for p in pairs]))
    # per frame of 256 new samples: A written; A read, s written, A and s read, m0 written by the level pass; 2 n_t + 1 rows of m0 read by the synthesis
    ns_bytes = 8.0 * samples + total_frames * (513 * 4.0 * (7 + 2 * n_t) + 2 * 4096.0)
    print('ss_spectral_gate_ns_batch, default smoothing: %8.1f us per call (stationary gate, alternating in the same run: %.1f us); pairs %s' %
          (t_ns, t_st, ', '.join('%.1f / %.1f' % p for p in pairs)))
    print('   traffic counting every read %.1f MB = %.0f B per sample -> %.1f us at 8 TB/s: %.1f %% of it' %
          (ns_bytes / 1e6, ns_bytes / samples, ns_bytes / 8e12 * 1e6, ns_bytes / 8e12 * 1e6 / t_ns * 100))
    print('ss_spectral_gate_ns_batch, no smoothing:      %8.1f us per call' % timed(lambda: gate_ns(0, 0)))
    print('reduce_noise_nonstationary_batch (table upload + 4 launches): %8.1f us per call' %
          timed(lambda: D.reduce_noise_nonstationary_batch((flat, lens), sr), reps=10))
    t0 = time.perf_counter()
    y0 = NO.reduce_noise(host[0], NO.coefficient(sr), n_f=n_f, n_t=n_t)
    print('host: the float64 non-stationary oracle on utterance 0: %.1f ms (x %d for the batch)' % ((time.perf_counter() - t0) * 1e3, R))
    got = D.reduce_noise_nonstationary_batch((flat[:n], [n]), sr)[0].cpu().numpy()
    print('max |device - oracle| on utterance 0: %.3g' % float(np.abs(got - y0).max()))

# the same batch through the float64 oracle on this host
th = prof.thresh.cpu().numpy()
ts = []
for _ in range(3):
    t0 = time.perf_counter()
    ys = [O.reduce_noise(h, th, n_f, n_t) for h in host[:4]]
    ts.append((time.perf_counter() - t0) * R / 4)
print('host: the float64 oracle on the same batch: %.1f ms (median of 3, 4 utterances timed, scaled to %d)' % (float(np.median(ts)) * 1e3, R))
got = D.reduce_noise_batch((flat[:n], [n]), prof)[0].cpu().numpy()
print('max |device - oracle| on utterance 0: %.3g (gate bits may differ at bins within rounding of the threshold)' % float(np.abs(got - ys[0]).max()))
