"""Developer tool: the HiFi-GAN generator (silent_speech_amd/vocoder.py, csrc/vocoder.hip) in the V1 configuration at T = 200 and 861 mel
frames (2.3 s and 10 s of audio), both arithmetic modes, against the same generator composed from torch.nn.functional convolutions (MIOpen)
on the same device in f32 and bf16.  Timing: HIP events around one whole call, 4 rotating inputs, 3 warm-ups, median of 12.  Also prints where
the time of a call goes by layer group (per-launch events, ops.LaunchProfiler) and the max |difference| of the three fast paths against the
f32 MIOpen composition.  Random weights (no checkpoint is needed for timing).  GPU only.

    python tools/vocoder_probe.py [--out profiles/vocoder_probe.txt]
    python tools/vocoder_probe.py --once 861        # one bf16x3 call and nothing else: the program to put under rocprofv3 --kernel-trace --stats
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from silent_speech_amd import _lib, ops  # noqa: E402
from silent_speech_amd.vocoder import Vocoder  # noqa: E402

V1 = dict(upsample_initial_channel=512, upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], resblock_kernel_sizes=[3, 7, 11],
          resblock_dilation_sizes=[[1, 3, 5]] * 3, resblock='1', num_mels=80)


def random_v1(seed=0):
    g = torch.Generator().manual_seed(seed)
    sd, C = {}, 512

    def conv(stem, shape, fan, scale=1.0):
        sd[stem + '.weight'] = torch.randn(*shape, generator=g) * scale / fan ** 0.5
        sd[stem + '.bias'] = torch.randn(shape[0] if 'ups' not in stem else shape[1], generator=g) * 0.05
    conv('conv_pre', (C, 80, 7), 80 * 7)
    for i, (u, k) in enumerate(zip(V1['upsample_rates'], V1['upsample_kernel_sizes'])):
        ci, co = C >> i, C >> (i + 1)
        conv('ups.%d' % i, (ci, co, k), ci * k / u)
        for j, kk in enumerate(V1['resblock_kernel_sizes']):
            for m in range(3):
                conv('resblocks.%d.convs1.%d' % (i * 3 + j, m), (co, co, kk), co * kk)
                conv('resblocks.%d.convs2.%d' % (i * 3 + j, m), (co, co, kk), co * kk, 0.3)
    conv('conv_post', (1, 32, 7), 32 * 7, 0.3)
    return sd


def torch_generator(sd, dtype, dev):
    """The same forward on torch's own convolutions (the yardstick)."""
    w = {k: v.to(device=dev, dtype=dtype) for k, v in sd.items()}

    def fwd(mel):
        x = F.conv1d(mel.to(dtype).T[None], w['conv_pre.weight'], w['conv_pre.bias'], padding=3)
        for i, (u, k) in enumerate(zip(V1['upsample_rates'], V1['upsample_kernel_sizes'])):
            x = F.conv_transpose1d(F.leaky_relu(x, 0.1), w['ups.%d.weight' % i], w['ups.%d.bias' % i], stride=u, padding=(k - u) // 2)
            xs = None
            for j, kk in enumerate(V1['resblock_kernel_sizes']):
                y, n = x, i * 3 + j
                for m, d in enumerate(V1['resblock_dilation_sizes'][j]):
                    t = F.conv1d(F.leaky_relu(y, 0.1), w['resblocks.%d.convs1.%d.weight' % (n, m)], w['resblocks.%d.convs1.%d.bias' % (n, m)], dilation=d, padding=(kk - 1) * d // 2)
                    t = F.conv1d(F.leaky_relu(t, 0.1), w['resblocks.%d.convs2.%d.weight' % (n, m)], w['resblocks.%d.convs2.%d.bias' % (n, m)], padding=(kk - 1) // 2)
                    y = t + y
                xs = y if xs is None else xs + y
            x = xs / 3
        return torch.tanh(F.conv1d(F.leaky_relu(x), w['conv_post.weight'], w['conv_post.bias'], padding=3)).reshape(-1).float()
    return fwd


def median_ms(fn, inputs, warm=3, n=12):
    for i in range(warm):
        fn(inputs[i % len(inputs)])
    torch.cuda.synchronize()
    ts = []
    for i in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(inputs[i % len(inputs)])
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'vocoder_probe.txt'))
    ap.add_argument('--once', type=int, default=0)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    _lib.load()
    sd = random_v1()
    g = torch.Generator().manual_seed(1)
    if a.once:
        voc = Vocoder(dev, config=V1, state_dict=sd)
        y = voc(torch.randn(a.once, 80, generator=g).to(dev))
        torch.cuda.synchronize()
        print('one bf16x3 V1 call, T = %d: %d samples, rms %.3f' % (a.once, y.numel(), float(y.pow(2).mean().sqrt())))
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    flop_per_frame = 613.6e6
    say('HiFi-GAN V1 generator on %s; algorithmic work 613.6 MFLOP per mel frame' % torch.cuda.get_device_name(0))
    with torch.no_grad():
        vocs = {m: Vocoder(dev, config=V1, state_dict=sd, matmul=m) for m in ('bf16x3', 'bf16')}
        refs = {'torch f32': torch_generator(sd, torch.float32, dev), 'torch bf16': torch_generator(sd, torch.bfloat16, dev)}
        for T in (200, 861):
            mels = [torch.randn(T, 80, generator=g).to(dev) for _ in range(4)]
            say('T = %d frames (%.2f s of audio, %.1f GFLOP):' % (T, T * 256 / 22050.0, T * flop_per_frame / 1e9))
            want = refs['torch f32'](mels[0])
            for name, fn in list(vocs.items()) + list(refs.items()):
                ms = median_ms(fn, mels)
                err = float((fn(mels[0]) - want).abs().max())
                say('  %-11s %8.3f ms per call  %7.1f TFLOP/s algorithmic   max |y - torch f32| %.2e' % (name, ms, T * flop_per_frame / ms / 1e9, err))
            for m, voc in vocs.items():
                ops.PROFILER = ops.LaunchProfiler()
                voc(mels[1])
                rows = ops.PROFILER.summary()
                ops.PROFILER = None
                for k, r in sorted(rows.items()):
                    say('    %-7s %-28s %3d launches %8.3f ms  %7.1f TFLOP/s  %6.2f TB/s (activation bytes)' %
                        (m, k, r['calls'], r['seconds'] * 1e3, r['flops'] / max(r['seconds'], 1e-9) / 1e12, r['bytes'] / max(r['seconds'], 1e-9) / 1e12))
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
