#!/usr/bin/env python3
"""Generate tests/golden/emg_features.npz by running the reference's own data_utils.get_emg_features (data_utils.py:85-136) in the
build container.  Run from the repo root:   python tests/golden/make_golden_emg_features.py

Like make_golden.py, modules the reference imports that are not installed here come from the stand-ins in tests/golden/_stubs.  The stub
`librosa` only serves the mel basis; get_emg_features also calls librosa.util.frame, librosa.feature.rms,
librosa.feature.zero_crossing_rate and librosa.stft, so this script attaches OUR restatement of those four librosa 0.10 functions (their
published definitions, center=False paths only) to the stub module in-process before it imports the reference.  librosa itself is absent,
so these four are 'parity unpinned' in the same sense as the mel basis: the fixture pins everything get_emg_features does around them
(mean removal, the double box filter and its edges, the column layout, the f32 cast).  Only the resulting DATA (.npz) is committed.

Inputs: the 516.79 Hz signals `short`, `mid`, `context` (*/emg) of filters.npz -- what load_utterance hands get_emg_features -- and seeded
8-channel signals of n = 16, 21, 22 and 4000 samples (a large DC offset, a 100 Hz tone); in one of them a column is zeroed in place the way
FLAGS.remove_channels does it (read_emg.py:74-76).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('SS_REFERENCE', '/root/reference')
sys.path.insert(0, os.path.join(HERE, '_stubs'))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))

import librosa  # noqa: E402  (the stub)


# ------------------------------------------------------------------ librosa 0.10 restated (util.frame, feature.rms, feature.zero_crossing_rate, stft)
def frame(x, *, frame_length, hop_length, axis=-1, writeable=False, subok=False):
    """librosa.util.frame for 1-d x (and the last axis of framed input): (..., frame_length, n_frames) strided view."""
    x = np.asarray(x)
    if x.shape[-1] < frame_length:
        raise ValueError('Input is too short (n=%d) for frame_length=%d' % (x.shape[-1], frame_length))
    n_frames = 1 + (x.shape[-1] - frame_length) // hop_length
    shape = x.shape[:-1] + (frame_length, n_frames)
    strides = x.strides[:-1] + (x.strides[-1], hop_length * x.strides[-1])
    return np.lib.stride_tricks.as_strided(x, shape=shape, strides=strides, writeable=False)


def rms(*, y=None, S=None, frame_length=2048, hop_length=512, center=True, pad_mode='constant', dtype=np.float32):
    """librosa.feature.rms on a time series, center=False: sqrt(mean(|frame|^2)) with the power in `dtype` (float32 by default)."""
    assert y is not None and not center
    x = frame(y, frame_length=frame_length, hop_length=hop_length)
    power = np.mean(np.square(x, dtype=dtype), axis=-2, keepdims=True)
    return np.sqrt(power)


def zero_crossings(y, *, threshold=1e-10, ref_magnitude=None, pad=True, zero_pos=True, axis=-1):
    assert ref_magnitude is None and zero_pos
    if threshold is None:
        threshold = 0.0
    if threshold > 0:
        y = y.copy()
        y[np.abs(y) <= threshold] = 0
    y_sign = np.signbit(y)
    pre = [slice(None)] * y.ndim; pre[axis] = slice(1, None)
    post = [slice(None)] * y.ndim; post[axis] = slice(-1)
    padding = [(0, 0)] * y.ndim; padding[axis] = (1, 0)
    return np.pad((y_sign[tuple(post)] != y_sign[tuple(pre)]), padding, mode='constant', constant_values=pad)


def zero_crossing_rate(y, *, frame_length=2048, hop_length=512, center=True, **kwargs):
    """librosa.feature.zero_crossing_rate, center=False: crossings of the framed signal (no front pad) averaged over the frame."""
    assert not center
    y_framed = frame(y, frame_length=frame_length, hop_length=hop_length)
    kwargs['axis'] = -2
    kwargs.setdefault('pad', False)
    return np.mean(zero_crossings(y_framed, **kwargs), axis=-2, keepdims=True)


def stft(y, *, n_fft=2048, hop_length=None, win_length=None, window='hann', center=True, dtype=None, pad_mode='constant', out=None):
    """librosa.stft, center=False, win_length = n_fft: rfft of the periodic-Hann-windowed frames, complex128 for f64 input."""
    import scipy.signal
    assert not center and window == 'hann' and (win_length is None or win_length == n_fft)
    hop_length = n_fft // 4 if hop_length is None else hop_length
    fft_window = scipy.signal.get_window('hann', n_fft, fftbins=True).reshape(-1, 1)
    y_frames = frame(y, frame_length=n_fft, hop_length=hop_length)
    return np.fft.rfft(fft_window * y_frames, axis=-2).astype(np.complex128 if dtype is None else dtype)


librosa.util = types.SimpleNamespace(frame=frame)
librosa.feature = types.SimpleNamespace(rms=rms, zero_crossing_rate=zero_crossing_rate)
librosa.stft = stft

import data_utils as ref_data  # noqa: E402


def main():
    filt = np.load(os.path.join(HERE, 'filters.npz'))
    rng = np.random.default_rng(23)
    arrs = {}
    for tag in ('short', 'mid', 'context'):
        x = filt[tag + '/emg']
        arrs[tag + '/x'] = x
        arrs[tag + '/features'] = ref_data.get_emg_features(x)
    for n in (16, 21, 22, 4000):
        t = np.arange(n) / 516.79
        x = rng.standard_normal((n, 8)) * 25.0 + rng.uniform(-1e4, 1e4, (1, 8)) + 40.0 * np.sin(2 * np.pi * 100.0 * t + 0.7)[:, None] \
            + 0.2 * np.cumsum(rng.standard_normal((n, 8)), 0)
        x = np.round(x * 64.0) / 64.0                        # a 1/64 grid: the fixture compresses, nothing else changes
        if n == 4000:
            x[:, 5] = 0                                      # read_emg.py:74-76: the column is zeroed in place before get_emg_features
        arrs['n%d/x' % n] = x
        arrs['n%d/features' % n] = ref_data.get_emg_features(x)
    path = os.path.join(HERE, 'emg_features.npz')
    np.savez_compressed(path, **arrs)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
