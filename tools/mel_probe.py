"""Developer tool: the log-mel kernel (csrc/mel.hip, ss_stft_logmel_fft) alone on a large ragged-free batch: HIP-event time per launch, frames / s and the
fraction of the 1344 B / frame HBM roofline.  GPU only.

--backward: the gradient with respect to the audio (csrc/mel_bwd.hip) at the loader's shape (32 signals x 6 s at 22 050 Hz) and at HiFi-GAN's segment
batch (16 x 8192 samples): per call, with one event pair per call after warm-up, (a) the forward alone, (b) forward + backward through
torch.ops.silent_speech.stft_logmel, (c) the same gradient through torch.stft + a dense mel matmul in float32 -- an outside yardstick on the same box; the
package never uses it.  Algorithmic bytes per frame of (b) at hop 256: forward 1 KB of new samples + 320 B out; backward 1 KB of samples again + 320 B
upstream + 4 KB frame gradient written + 4 KB read back + 1 KB of g_y = 10.3 KB, 11.6 KB with the forward's."""
import argparse
import sys, os
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from silent_speech_amd import data_utils

dev = torch.device('cuda:0')


def forward_probe():
    for n_utt, seconds in ((32, 6.0), (256, 8.0), (1024, 8.0)):
        L = int(22050 * seconds) // 256 * 256
        y = (0.1 * torch.randn(n_utt, L, device=dev)).clamp_(-1, 1)
        F = 1 + (L + 768 - 1024) // 256
        out = torch.empty(n_utt, 80, F, device=dev)
        run = lambda: data_utils._logmel_fft(y, None, None, L, n_utt, F, 384, False, 1024, 80, 22050, 256, 1024, 0, 8000, out, False)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 20
        a.record()
        for _ in range(n):
            run()
        b.record(); torch.cuda.synchronize()
        t = a.elapsed_time(b) / n * 1e-3
        fr = n_utt * F
        print('%5d x %.0f s: %7d frames  %8.1f us  %7.1f M frames/s  %5.1f %% of the 1344 B/frame HBM roofline' % (n_utt, seconds, fr, t * 1e6, fr / t / 1e6, fr * 1344 / t / 8e12 * 100))


def _per_call_us(run, warm=5, n=50):
    for _ in range(warm):
        run()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record(); run(); b.record()
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return float(np.median(t)), float(t.min()), float(t.max())


def backward_probe():
    hann = torch.hann_window(1024, device=dev)
    basis = torch.from_numpy(data_utils.slaney_mel_filterbank(22050, 1024, 80, 0, 8000)).to(dev)

    def torch_mel(y):
        yp = torch.nn.functional.pad(y.unsqueeze(1), (384, 384), mode='reflect').squeeze(1)
        spec = torch.stft(yp, 1024, hop_length=256, win_length=1024, window=hann, center=False, onesided=True, return_complex=True)
        mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
        return torch.log(torch.clamp(torch.matmul(basis, mag), min=1e-5))

    for B, L, what in ((32, int(22050 * 6.0) // 256 * 256, 'the loader\'s shape'), (16, 8192, 'HiFi-GAN\'s segment batch')):
        torch.manual_seed(0)
        y = (0.1 * torch.randn(B, L, device=dev)).clamp_(-1, 1)
        F = 1 + (L + 768 - 1024) // 256
        g = torch.randn(B, 80, F, device=dev)
        yg = y.clone().requires_grad_()
        mel = lambda t: data_utils.mel_spectrogram(t, 1024, 80, 22050, 256, 1024, 0, 8000)

        def fwd():
            with torch.no_grad():
                mel(y)

        def fwd_bwd():
            yg.grad = None
            mel(yg).backward(g)

        def torch_fwd_bwd():
            yg.grad = None
            torch_mel(yg).backward(g)

        fwd_bwd(); ours = yg.grad.clone()
        torch_fwd_bwd(); theirs = yg.grad.clone()
        rel = float((ours - theirs).abs().max() / theirs.abs().max())
        print('%d x %d samples (%s): %d frames; kernel vs torch gradient: max difference %.2g of the largest entry' % (B, L, what, B * F, rel))
        def bwd_kernels():                                          # the two backward launches without the dispatcher and autograd around them
            data_utils._mel_spectrogram_backward_impl(g, y, 1024, 80, 22050, 256, 1024, 0, 8000, False)

        for _ in range(3):
            bwd_kernels()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            bwd_kernels()
        b.record(); torch.cuda.synchronize()
        t = a.elapsed_time(b) / 20 * 1e3
        print('    %-44s %8.1f us per call, 20 calls back to back  %6.2f M frames/s  %5.1f %% of the 10.3 KB/frame HBM roofline'
              % ('backward kernels alone (frames + gather)', t, B * F / t, B * F * 10560 / (t * 1e-6) / 8e12 * 100))
        for name, run in (('forward alone', fwd), ('forward + backward (op)', fwd_bwd), ('torch.stft + dense mel, forward + backward', torch_fwd_bwd)):
            med, lo, hi = _per_call_us(run)
            print('    %-44s median %8.1f us  (min %8.1f, max %8.1f over 50 calls)  %6.2f M frames/s' % (name, med, lo, hi, B * F / med))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--backward', action='store_true', help='time the gradient (csrc/mel_bwd.hip) instead of the forward kernel alone')
    if ap.parse_args().backward:
        backward_probe()
    else:
        forward_probe()
