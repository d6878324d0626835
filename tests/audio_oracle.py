"""float64 numpy / scipy restatement of the stored-audio half of the reference's load_audio (data_utils.py:19-27, 64-83):
scipy.signal.resample_poly with its defaults (the pinned definition of the resample; librosa / soxr parity is unpinned), its closed form,
normalize_volume with librosa.feature.rms's defaults of librosa >= 0.10 (frames of 2048 every 512 samples, centred with ZERO padding,
1 + n // 512 frames), and load_audio on top of the mel oracle."""
import math

import numpy as np
import scipy.signal

from oracle import mel_ref


def ratio(orig_sr, target_sr):
    g = math.gcd(int(orig_sr), int(target_sr))
    return int(target_sr) // g, int(orig_sr) // g


def taps(up, down):
    """(h, half): the FIR resample_poly designs for (up, down), already scaled by up."""
    half = 10 * max(up, down)
    return scipy.signal.firwin(2 * half + 1, 1.0 / max(up, down), window=('kaiser', 5.0)) * up, half


def out_length(n, up, down):
    return -((-n * up) // down)


def resample(x, up, down):
    x = np.asarray(x, dtype=np.float64)
    return x.copy() if up == down else scipy.signal.resample_poly(x, up, down)


def resample_closed_form(x, up, down):
    """y[m] = sum_j x[j] h[m down + half - j up] over the j inside the signal and the taps inside h."""
    x = np.asarray(x, dtype=np.float64)
    h, half = taps(up, down)
    y = np.zeros(out_length(len(x), up, down))
    for m in range(len(y)):
        p = m * down + half
        j = np.arange(max(0, -((2 * half - p) // up)), min(len(x) - 1, p // up) + 1)
        y[m] = np.sum(x[j] * h[p - j * up])
    return y


def bound(up, down, max_abs):
    """(taps + 2) 2^-24 max_phase sum |h| max |x|: one rounding per product of the longest phase, plus the rounding of the table and of the input."""
    h, half = taps(up, down)
    n_taps = (2 * half) // up + 1
    phase_sum = max(float(np.abs(h[ph::up]).sum()) for ph in range(up))
    return (n_taps + 2) * 2.0 ** -24 * phase_sum * float(max_abs)


def levels(x):
    """(max over frames of the frame RMS, max |x|)"""
    x = np.asarray(x, dtype=np.float64)
    xp = np.pad(x, (1024, 1024))
    rms = [math.sqrt(float(np.mean(xp[512 * f:512 * f + 2048] ** 2))) for f in range(1 + len(x) // 512)]
    return max(rms), (float(np.abs(x).max()) if len(x) else 0.0)


def volume_gain(x):
    max_rms, peak = levels(x)
    g = 0.2 / (max_rms + 0.01)
    return 1.0 / peak if g * peak > 1.0 else g


def normalize_volume(x):
    return np.asarray(x, dtype=np.float64) * volume_gain(x)


def load_audio(audio, sample_rate, start=None, end=None, max_frames=None, renormalize_volume=False):
    audio = np.asarray(audio, dtype=np.float64)
    if audio.ndim > 1:
        audio = audio[:, 0]
    if start is not None or end is not None:
        audio = audio[start:end]
    if renormalize_volume:
        audio = normalize_volume(audio)
    if sample_rate != 22050:
        audio = resample(audio, *ratio(sample_rate, 22050))
    audio = np.clip(audio, -1, 1)
    mspec = mel_ref.mel_spectrogram_ref(audio[None].astype(np.float32))[0].T
    return mspec[:max_frames] if max_frames is not None and mspec.shape[0] > max_frames else mspec
