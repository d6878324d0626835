"""Drop-in for the hot-path parts of the reference's data_utils.py:

    mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False)   (:39-62)
    normalize_volume(audio) / load_audio(decoded array, sample_rate, ...)                              (:19-27, :64-83; file decoding stays out)
    resample_audio / resample_audio_batch / volume_gains: the band-limited resample (:75) and the levelling of a ragged batch (csrc/audio.hip)
    NoiseProfile / reduce_noise / reduce_noise_batch / clean_session: the stationary spectral gate and the levelling of data_collection/clean_audio.py
                                                                     (noisereduce's reduce_noise, csrc/spectral_gate.hip; file decoding stays out)
    reduce_noise_nonstationary / reduce_noise_nonstationary_batch:    noisereduce's default, non-stationary gate for recordings without a silence clip
                                                                     (csrc/spectral_gate_ns.hip; clean_session(gate='nonstationary'))
    get_emg_features(emg_data, debug=False)                                                            (:85-136)
    combine_fixed_length(tensor_list, length) / decollate_tensor(tensor, lengths)                      (:158-178)
    FeatureNormalizer                                                                                   (:138-156)
    phoneme_inventory                                                                                   (:17)

mel_spectrogram runs on the MI355X as two exact-f32 MFMA GEMMs: frames x windowed-DFT matrix (the
hop-strided, overlapping frames of the reflect-padded signal are just a RowMap -- nothing is copied),
then |.| (HIP kernel) and the mel filterbank GEMM with the log-clamp fused in its epilogue.
A 1024-point DFT as a dense contraction costs 2.1 MFLOP/frame -- ~13 ns at the f32 MFMA rate -- and
has no butterfly data movement, which is why it beats an FFT on this machine for n_fft = 1024.
"""
import math

import numpy as np
import torch

from . import _lib, ops

phoneme_inventory = ['aa', 'ae', 'ah', 'ao', 'aw', 'ax', 'axr', 'ay', 'b', 'ch', 'd', 'dh', 'dx', 'eh', 'el', 'em', 'en', 'er', 'ey', 'f', 'g',
                     'hh', 'hv', 'ih', 'iy', 'jh', 'k', 'l', 'm', 'n', 'nx', 'ng', 'ow', 'oy', 'p', 'r', 's', 'sh', 't', 'th', 'uh', 'uw',
                     'v', 'w', 'y', 'z', 'zh', 'sil']


def slaney_mel_filterbank(sr, n_fft, n_mels, fmin, fmax):
    """What librosa.filters.mel(sr=, n_fft=, n_mels=, fmin=, fmax=) returns with its defaults (Slaney mel
    scale, 'slaney' area normalisation, float32) -- the call at data_utils.py:47.  librosa is a
    third-party dependency absent from the reference tree: basis values are 'parity unpinned'."""
    if fmax is None:
        fmax = sr / 2.0
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0

    def to_mel(f):
        f = np.asarray(f, dtype=np.float64)
        return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-30) / min_log_hz) / logstep, f / f_sp)

    def to_hz(m):
        m = np.asarray(m, dtype=np.float64)
        return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), m * f_sp)

    n_bins = 1 + n_fft // 2
    freqs = np.linspace(0.0, sr / 2.0, n_bins)
    edges = to_hz(np.linspace(to_mel(fmin), to_mel(fmax), n_mels + 2))
    fdiff = np.diff(edges)
    ramps = edges[:, None] - freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    w *= (2.0 / (edges[2:n_mels + 2] - edges[:n_mels]))[:, None]
    return w.astype(np.float32)


_dft_cache = {}
_mel_cache = {}


def _settle_cache(device):
    """A cached constant (DFT matrix, mel basis, FFT tables) is uploaded on whichever stream misses the cache first and read from every stream after that
    (pipeline.DeviceBatchBuilder runs the audio half of a batch on a side stream): the upload is followed by ONE device-wide synchronisation, so that no
    later reader on another stream can start before the bytes are there (round-5 advisor finding; a cache miss happens once per configuration)."""
    if getattr(device, 'type', str(device)) == 'cuda' and torch.cuda.is_available():
        torch.cuda.synchronize(device)


def _windowed_dft(n_fft, win_size, device):
    """[2*nb][n_fft] f32: rows 0..nb-1 = hann(n) cos(2 pi k n / N), rows nb..2nb-1 = hann(n) sin(.)   (nb = N/2+1)"""
    key = (n_fft, win_size, str(device))
    if key not in _dft_cache:
        nb = n_fft // 2 + 1
        n = np.arange(n_fft, dtype=np.float64)
        win = np.zeros(n_fft, dtype=np.float64)
        off = (n_fft - win_size) // 2
        win[off:off + win_size] = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_size) / win_size)).astype(np.float32)   # torch.hann_window (periodic), f32
        ang = 2.0 * np.pi * np.outer(np.arange(nb), n) / n_fft
        mat = np.concatenate([np.cos(ang) * win[None, :], np.sin(ang) * win[None, :]], 0).astype(np.float32)
        _dft_cache[key] = torch.from_numpy(mat).to(device)
        _settle_cache(device)
    return _dft_cache[key]


def _mel_basis(sampling_rate, n_fft, num_mels, fmin, fmax, device, ld):
    key = (sampling_rate, n_fft, num_mels, fmin, fmax, str(device), ld)
    if key not in _mel_cache:
        b = slaney_mel_filterbank(sampling_rate, n_fft, num_mels, fmin, fmax)
        pad = np.zeros((num_mels, ld), dtype=np.float32)
        pad[:, :b.shape[1]] = b
        _mel_cache[key] = torch.from_numpy(pad).to(device)
        _settle_cache(device)
    return _mel_cache[key]


def mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False):
    """y: (B, L) float32 in [-1, 1] on the GPU -> (B, num_mels, F) float32 log-mel, F = 1 + (L + n_fft - hop - n_fft)//hop.
    (The reference's min/max range warnings (:40-43) would force a device sync and are omitted.)  Dispatches through
    torch.ops.silent_speech.stft_logmel (torch_ops.py).  With y.requires_grad the result is differentiable with respect to y (csrc/mel_bwd.hip) whenever the
    direct FFT kernel takes the call: n_fft = 1024, center=False, win_size <= 1024, a filterbank that fits the kernel's tables and L > (n_fft - hop) / 2; its
    value is the no-grad result bit for bit.  Every other configuration raises a ValueError at the call (no gradient exists for the DFT-GEMM formulation)."""
    if y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError('y must be a float32 (B, L) tensor')
    if hop_size % 4 or n_fft % 4:
        raise ValueError('hop_size and n_fft must be multiples of 4 (16-byte f32 rows)')
    from . import torch_ops  # noqa: F401
    if torch.is_grad_enabled() and y.requires_grad:
        why = _not_differentiable(y.shape[1], n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center, y.device)
        if why:
            raise ValueError('mel_spectrogram: y requires grad, but %s; only the n_fft = 1024, center=False path (the direct FFT kernel) is differentiable' % why)
    return torch.ops.silent_speech.stft_logmel(y, int(n_fft), int(num_mels), int(sampling_rate), int(hop_size), int(win_size), int(fmin), int(fmax), bool(center))


def _mel_spectrogram_impl(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center):
    y = y.contiguous()
    B, L = y.shape
    pad = int((n_fft - hop_size) / 2)
    Lp = L + 2 * pad
    dev = y.device
    if not center and y.dtype == torch.float32 and L > pad and Lp >= n_fft:
        # n_fft = 1024: one kernel straight from y (reflection is index arithmetic in the frames that touch the ends): no padded copy
        F = 1 + (Lp - n_fft) // hop_size
        out = torch.empty(B, num_mels, F, dtype=torch.float32, device=dev)
        if _logmel_fft(y, None, None, L, B, F, pad, False, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, out, frame_major=False):
            return out

    def reflect_pad(src, row_stride, n, p, ld_out):
        # B rows of one length n are a ragged batch whose offsets and lengths are made on the device; the kernel writes the zeros behind each row too
        offs, lens = torch.arange(B, dtype=torch.int64, device=dev) * row_stride, torch.full((B,), n, dtype=torch.int32, device=dev)
        out = torch.empty(B, ld_out, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().ss_reflect_pad_ragged(_lib.ptr(src), _lib.ptr(offs), _lib.ptr(lens), _lib.ptr(out), B, n, p, ld_out, 0, _lib.stream_of(y)), 'ss_reflect_pad_ragged')
        return out

    ldp = (Lp + 3) // 4 * 4
    ypad = reflect_pad(y, L, L, pad, ldp)
    if center:          # torch.stft(center=True, pad_mode='reflect') (data_utils.py:54): n_fft//2 more samples, reflected off the PADDED signal
        pad2 = n_fft // 2
        if pad2 >= Lp:
            raise ValueError('signal too short for centred frames')
        Lp2 = Lp + 2 * pad2
        ldp2 = (Lp2 + 3) // 4 * 4
        ypad, Lp, ldp = reflect_pad(ypad, ldp, Lp, pad2, ldp2), Lp2, ldp2
    if Lp < n_fft:
        raise ValueError('signal too short for one frame')
    F = 1 + (Lp - n_fft) // hop_size
    out = torch.empty(B, num_mels, F, dtype=torch.float32, device=dev)
    if not _logmel_fft(ypad, None, None, ldp, B, F, 0, False, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, out, frame_major=False):    # (center=True: rows already padded twice)
        _stft_logmel(ypad, B, F, ldp, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, out, frame_major=False)
    return out


_fft_cache = {}


def _fft_tables(n_fft, win_size, num_mels, sampling_rate, fmin, fmax, device):
    """What ss_stft_logmel_fft reads besides the signal: the f32 hann window (torch.hann_window, periodic, centred in n_fft like torch.stft does) and
    the mel filterbank in sparse form -- per band the first non-zero bin, the length of the run up to the last non-zero bin (padded to a multiple of 4
    with zero weights) and the packed weights --, and the deal of the bands to the 64 lanes of a wave (longest band first onto the least loaded lane,
    two bands per lane at most).  None when the filterbank does not fit the kernel's tables."""
    key = (n_fft, win_size, num_mels, sampling_rate, fmin, fmax, str(device))
    if key not in _fft_cache:
        win = np.zeros(n_fft, dtype=np.float32)
        off = (n_fft - win_size) // 2
        win[off:off + win_size] = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_size) / win_size)).astype(np.float32)
        basis = slaney_mel_filterbank(sampling_rate, n_fft, num_mels, fmin, fmax)
        nb = n_fft // 2 + 1
        lo, cnt, offs, ws = [], [], [], []
        for m in range(num_mels):
            nz = np.nonzero(basis[m])[0]
            a, n = (int(nz[0]), int(nz[-1]) - int(nz[0]) + 1) if len(nz) else (0, 0)
            n4 = (n + 3) // 4 * 4
            run = np.zeros(n4, dtype=np.float32)
            run[:n] = basis[m, a:a + n]
            lo.append(a); cnt.append(n4); offs.append(sum(len(w) for w in ws)); ws.append(run)
        n_w = int(sum(cnt))
        load, lanes = [0] * 64, [[] for _ in range(64)]
        for m in sorted(range(num_mels), key=lambda m: -cnt[m]):
            l = min((l for l in range(64) if len(lanes[l]) < 2), key=lambda l: load[l], default=None)
            if l is None:
                break
            lanes[l].append(m); load[l] += cnt[m]
        ok = num_mels <= 128 and n_w <= 4096 and sum(len(x) for x in lanes) == num_mels and all(lo[m] + cnt[m] <= nb + 7 for m in range(num_mels))
        if not ok:
            _fft_cache[key] = None
        else:
            lb = np.full((2, 64), -1, dtype=np.int32)
            for l in range(64):
                for it, m in enumerate(lanes[l]):
                    lb[it, l] = m
            w = np.concatenate(ws) if n_w else np.zeros(1, dtype=np.float32)
            t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(device)
            _fft_cache[key] = (t(win, np.float32), t(lo, np.int32), t(cnt, np.int32), t(offs, np.int32), t(w, np.float32), t(lb, np.int32), n_w)
            _settle_cache(device)
    return _fft_cache[key]


def _logmel_fft(y, offs, lens, uniform_len, B, F, pad, clip, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, out, frame_major):
    """One ss_stft_logmel_fft launch (csrc/mel.hip) on the caller's signals; False when this configuration needs the GEMM formulation."""
    if n_fft != 1024 or win_size > n_fft:
        return False
    tabs = _fft_tables(n_fft, win_size, num_mels, sampling_rate, fmin, fmax, y.device)
    if tabs is None:
        return False
    win, lo, cnt, boff, w, lb, n_w = tabs
    sb, sf, sm = (F * num_mels, num_mels, 1) if frame_major else (num_mels * F, 1, F)
    _lib.check(_lib.lib().ss_stft_logmel_fft(_lib.ptr(y), _lib.ptr(offs) if offs is not None else None, _lib.ptr(lens) if lens is not None else None, int(uniform_len), B, F,
                                             pad, int(bool(clip)), n_fft, hop_size, _lib.ptr(win), _lib.ptr(lo), _lib.ptr(cnt), _lib.ptr(boff), _lib.ptr(w), _lib.ptr(lb),
                                             num_mels, n_w, 1e-5, _lib.ptr(out), sb, sf, sm, _lib.stream_of(y)), 'ss_stft_logmel_fft')
    return True


_fft_bwd_cache = {}
BWD_MAX_TAPS = 2          # csrc/mel_bwd.hip: bands with a non-zero weight over one bin


def _fft_bwd_tables(n_fft, win_size, num_mels, sampling_rate, fmin, fmax, device):
    """What ss_stft_logmel_fft_backward reads on top of _fft_tables: the TRANSPOSED filterbank per bin -- bin_band[513] = m0 | m1 << 8, the bands with a non-zero
    weight over the bin (255 = none; a bin lies under at most two neighbouring Slaney triangles), bin_w[513][2] their weights -- and the largest number of
    bands over one bin, which the launcher checks.  None when a bin lies under more than BWD_MAX_TAPS bands or the forward's tables do not fit."""
    key = (n_fft, win_size, num_mels, sampling_rate, fmin, fmax, str(device))
    if key not in _fft_bwd_cache:
        tabs = None
        if n_fft == 1024 and win_size <= n_fft and _fft_tables(n_fft, win_size, num_mels, sampling_rate, fmin, fmax, device) is not None:
            basis = slaney_mel_filterbank(sampling_rate, n_fft, num_mels, fmin, fmax)
            nb = n_fft // 2 + 1
            band = np.full(nb, 255 | 255 << 8, dtype=np.int32)
            w = np.zeros((nb, 2), dtype=np.float32)
            taps = 0
            for k in range(nb):
                ms = np.nonzero(basis[:, k])[0]
                taps = max(taps, len(ms))
                if len(ms) <= BWD_MAX_TAPS:
                    m = [int(x) for x in ms] + [255] * (2 - len(ms))
                    band[k] = m[0] | m[1] << 8
                    w[k, :len(ms)] = basis[ms, k]
            if taps <= BWD_MAX_TAPS and num_mels < 255:
                tabs = (torch.from_numpy(band).to(device), torch.from_numpy(w).to(device), taps)
                _settle_cache(device)
        _fft_bwd_cache[key] = tabs
    return _fft_bwd_cache[key]


def _not_differentiable(L, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center, device):
    """Why this configuration has no gradient (a phrase for the error message), or None when the direct FFT kernel and its backward take it."""
    if center:
        return 'center=True runs on the twice padded rows'
    if n_fft != 1024 or win_size > n_fft:
        return 'n_fft = %d / win_size = %d runs on the DFT-GEMM formulation' % (n_fft, win_size)
    pad = int((n_fft - hop_size) / 2)
    if L <= pad or L + 2 * pad < n_fft:
        return 'a signal of %d samples is too short for the direct kernel (hop %d reflects %d samples)' % (L, hop_size, pad)
    if _fft_bwd_tables(n_fft, win_size, num_mels, sampling_rate, fmin, fmax, device) is None:
        return 'the filterbank (%d bands, %d Hz, %s .. %s Hz) does not fit the kernel\'s tables and runs on the DFT-GEMM formulation' % (num_mels, sampling_rate, fmin, fmax)
    return None


def _logmel_fft_backward(g, y, offs, lens, uniform_len, max_len, B, F, pad, clip, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, strides, g_y):
    """One ss_stft_logmel_fft_backward call (csrc/mel_bwd.hip): g is the upstream gradient, read in place through strides = (signal, frame, band) in
    elements; g_y has y's layout.  A configuration without a gradient is an error, never a fallback."""
    tabs = _fft_tables(n_fft, win_size, num_mels, sampling_rate, fmin, fmax, y.device) if n_fft == 1024 and win_size <= n_fft else None
    btabs = _fft_bwd_tables(n_fft, win_size, num_mels, sampling_rate, fmin, fmax, y.device)
    if tabs is None or btabs is None:
        raise ValueError('stft_logmel backward: n_fft = %d, win_size = %d, %d bands have no gradient; only the n_fft = 1024, center=False path is differentiable'
                         % (n_fft, win_size, num_mels))
    win, lo, cnt, boff, w, lb, n_w = tabs
    bin_band, bin_w, taps = btabs
    ws_bytes = _lib.lib().ss_stft_logmel_fft_backward_workspace_bytes(B, F)
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=y.device)
    sb, sf, sm = strides
    _lib.check(_lib.lib().ss_stft_logmel_fft_backward(_lib.ptr(y), _lib.ptr(offs) if offs is not None else None, _lib.ptr(lens) if lens is not None else None,
                                                      int(uniform_len), int(max_len), B, F, pad, int(bool(clip)), n_fft, hop_size, _lib.ptr(win), _lib.ptr(lo),
                                                      _lib.ptr(cnt), _lib.ptr(boff), _lib.ptr(w), _lib.ptr(lb), num_mels, n_w, _lib.ptr(bin_band), _lib.ptr(bin_w), taps,
                                                      1e-5, _lib.ptr(g), sb, sf, sm, _lib.ptr(ws), ws_bytes, _lib.ptr(g_y), _lib.stream_of(y)),
               'ss_stft_logmel_fft_backward')
    return g_y


def _mel_spectrogram_backward_impl(g, y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center):
    """d loss / d y of mel_spectrogram's direct path from g = d loss / d mel (B, num_mels, F), any strides."""
    B, L = y.shape
    why = _not_differentiable(L, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center, y.device)
    if why:
        raise ValueError('stft_logmel backward: %s; only the n_fft = 1024, center=False path is differentiable' % why)
    y = y.contiguous()
    pad = int((n_fft - hop_size) / 2)
    F = 1 + (L + 2 * pad - n_fft) // hop_size
    if tuple(g.shape) != (B, num_mels, F) or g.dtype != torch.float32 or g.device != y.device:
        raise ValueError('stft_logmel backward: the upstream gradient must be a (%d, %d, %d) float32 tensor on the device of y' % (B, num_mels, F))
    g_y = torch.empty_like(y)
    return _logmel_fft_backward(g, y, None, None, L, L, B, F, pad, False, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax,
                                (g.stride(0), g.stride(2), g.stride(1)), g_y)


def _ragged_layout(flat, offsets, lengths, n_fft, hop_size):
    """Host-side check of a ragged batch description before a kernel follows it: every signal lies inside the flat buffer and is longer than the reflected
    stretch (one small device -> host copy).  Returns (lengths as a list, pad)."""
    pad = int((n_fft - hop_size) / 2)
    if flat.dim() != 1 or flat.dtype != torch.float32 or not flat.is_contiguous():
        raise ValueError('stft_logmel_ragged: a flat contiguous float32 buffer is expected')
    if offsets.dim() != 1 or lengths.shape != offsets.shape or offsets.dtype != torch.int64 or lengths.dtype != torch.int32 or offsets.shape[0] < 1 \
            or offsets.device != flat.device or lengths.device != flat.device or not offsets.is_contiguous() or not lengths.is_contiguous():
        raise ValueError('stft_logmel_ragged: offsets (B >= 1) int64 and lengths (B) int32, contiguous, on the device of the buffer')
    if hop_size % 4 or hop_size <= 0:
        raise ValueError('hop_size must be a positive multiple of 4')
    o, n = offsets.cpu().tolist(), lengths.cpu().tolist()
    for a, L in zip(o, n):
        if a < 0 or a + L > flat.shape[0]:
            raise ValueError('stft_logmel_ragged: signal [%d, %d) lies outside the buffer of %d samples' % (a, a + L, flat.shape[0]))
        if L <= pad or L + 2 * pad < n_fft:
            raise ValueError('signal too short for one frame')
    return n, pad


def _mel_ragged_impl(flat, offsets, lengths, F, clip, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax):
    lens, pad = _ragged_layout(flat, offsets, lengths, n_fft, hop_size)
    B = len(lens)
    if F < max(1 + (L + 2 * pad - n_fft) // hop_size for L in lens):
        raise ValueError('stft_logmel_ragged: F = %d is less than the longest signal\'s frame count' % F)
    out = torch.empty(B, F, num_mels, dtype=torch.float32, device=flat.device)
    if not _logmel_fft(flat, offsets, lengths, 0, B, F, pad, clip, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, out, frame_major=True):
        raise ValueError('stft_logmel_ragged: n_fft = %d, win_size = %d, %d bands run on the DFT-GEMM formulation; only the n_fft = 1024 path is differentiable'
                         % (n_fft, win_size, num_mels))
    return out


def _mel_ragged_backward_impl(g, flat, offsets, lengths, clip, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax):
    """d loss / d flat from g = d loss / d buf (B, F, num_mels), any strides; samples of the buffer outside every signal get 0."""
    lens, pad = _ragged_layout(flat, offsets, lengths, n_fft, hop_size)
    B = len(lens)
    if g.dim() != 3 or g.shape[0] != B or g.shape[2] != num_mels or g.dtype != torch.float32 or g.device != flat.device:
        raise ValueError('stft_logmel_ragged backward: the upstream gradient must be a (%d, F, %d) float32 tensor on the device of the buffer' % (B, num_mels))
    g_y = torch.zeros_like(flat)
    return _logmel_fft_backward(g, flat, offsets, lengths, 0, max(lens), B, int(g.shape[1]), pad, clip, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax,
                                (g.stride(0), g.stride(1), g.stride(2)), g_y)


def _stft_logmel(ypad, B, F, ldp, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, out, frame_major):
    """padded signals [B][ldp] -> log-mel of frames 0..F-1 of every row: the GEMM formulation (any n_fft): two f32 GEMMs (windowed DFT matrix, mel basis)
    around the magnitude kernel.  frame_major: out is [B*F][num_mels] (frames of a signal are contiguous rows) instead of the reference's (B, num_mels, F)."""
    dev = ypad.device
    nb = n_fft // 2 + 1
    W = _windowed_dft(n_fft, win_size, dev)
    ld_spec = (2 * nb + 7) // 8 * 8
    spec = torch.empty(B * F, ld_spec, dtype=torch.float32, device=dev)
    ops.gemm(ypad, W, spec, B * F, 2 * nb, n_fft, ops.rowmap(hop_size, F, ldp), ops.rowmap(n_fft), ops.rowmap(ld_spec))
    ld_mag = (nb + 7) // 8 * 8
    mag = torch.empty(B * F, ld_mag, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().ss_stft_magnitude(_lib.ptr(spec), ld_spec, nb, _lib.ptr(mag), ld_mag, B * F, _lib.stream_of(ypad)), 'ss_stft_magnitude')
    basis = _mel_basis(sampling_rate, n_fft, num_mels, fmin, fmax, dev, ld_mag)
    if frame_major:
        ops.gemm_ex(mag, basis, out, B * F, num_mels, ld_mag, ops.rowmap(ld_mag), ops.rowmap(ld_mag), ops.rowmap(num_mels), log_clamp=1e-5)
    else:
        ops.gemm_ex(mag, basis, out, B * F, num_mels, ld_mag, ops.rowmap(ld_mag), ops.rowmap(ld_mag), ops.rowmap(1, F, num_mels * F),
                    col_perm=(num_mels, F, 0), log_clamp=1e-5)
    return out


def mel_spectrogram_batch(signals, n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0, fmax=8000, clip=True):
    """load_audio's `np.clip` + `mel_spectrogram(..., center=False)` (data_utils.py:76-78) for EVERY utterance of a batch in one
    launch sequence: one ragged clip + reflect-pad kernel, ONE hop-strided DFT GEMM over all frames of all utterances (rows of the
    padded buffer = utterances, RowMap batch stride), magnitude, one mel GEMM with the log-clamp epilogue.
    signals: list of 1-D f32 device tensors at `sampling_rate`, or the pair (flat f32 device tensor holding them back to back, lengths) -- what
    a loader that uploaded the whole batch in one copy has.  Returns (buf [B][F_max][num_mels] f32, frames per utterance):
    utterance b's `pytorch_mspec.squeeze(0).T` is buf[b, :frames[b]] -- a contiguous view, no per-utterance copy.
    When grad is enabled and the flat buffer or any listed signal requires grad, the call goes through torch.ops.silent_speech.stft_logmel_ragged and buf
    carries a grad_fn (csrc/mel_bwd.hip; n_fft = 1024 only, anything else raises a ValueError); otherwise the code path below runs as before.  The rows
    buf[b, frames[b]:] are filler: they contribute no gradient, whatever the upstream gradient holds there."""
    if hop_size % 4 or n_fft % 4:
        raise ValueError('hop_size and n_fft must be multiples of 4 (16-byte f32 rows)')
    packed = isinstance(signals, tuple)
    lens = [int(n) for n in signals[1]] if packed else [int(t.shape[0]) for t in signals]
    B = len(lens)
    pad = int((n_fft - hop_size) / 2)
    if min(lens) + 2 * pad < n_fft or min(lens) <= pad:
        raise ValueError('signal too short for one frame')
    dev = signals[0].device
    if packed:
        flat = signals[0].reshape(-1)
        if flat.dtype != torch.float32 or int(flat.shape[0]) != sum(lens):
            raise ValueError('packed signals: a flat float32 tensor of sum(lengths) samples')
    else:
        flat = torch.cat([t.reshape(-1).to(torch.float32) for t in signals]) if B > 1 else signals[0].reshape(-1).to(torch.float32).contiguous()
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    frames = [1 + (L + 2 * pad - n_fft) // hop_size for L in lens]
    F = max(frames)
    ldp = (max(lens) + 2 * pad + 3) // 4 * 4
    offs_d = torch.from_numpy(offs).to(dev, non_blocking=True)
    lens_d = torch.from_numpy(np.asarray(lens, dtype=np.int32)).to(dev, non_blocking=True)
    if torch.is_grad_enabled() and flat.requires_grad:                 # (a listed signal that requires grad makes the concatenation require it)
        why = _not_differentiable(min(lens), n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, False, dev)
        if why:
            raise ValueError('mel_spectrogram_batch: the signals require grad, but %s; only the n_fft = 1024 path (the direct FFT kernel) is differentiable' % why)
        from . import torch_ops  # noqa: F401
        buf = torch.ops.silent_speech.stft_logmel_ragged(flat, offs_d, lens_d, F, bool(clip), int(n_fft), int(num_mels), int(sampling_rate), int(hop_size),
                                                         int(win_size), int(fmin), int(fmax))
        return buf, frames
    out = torch.empty(B, F, num_mels, dtype=torch.float32, device=dev)
    if _logmel_fft(flat, offs_d, lens_d, 0, B, F, pad, clip, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, out, frame_major=True):
        return out, frames
    ypad = torch.empty(B, ldp, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().ss_reflect_pad_ragged(_lib.ptr(flat), _lib.ptr(offs_d), _lib.ptr(lens_d), _lib.ptr(ypad), B, min(lens), pad, ldp, int(bool(clip)),
                                                _lib.stream_of(flat)), 'ss_reflect_pad_ragged')
    _stft_logmel(ypad, B, F, ldp, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, out, frame_major=True)
    return out, frames


# ------------------------------------------------------------------ stored audio: band-limited resampling and volume levelling (csrc/audio.hip)
RESAMPLE_TILE, RESAMPLE_SPAN, RESAMPLE_TABLE_FLOATS = 2048, 8192, 12288      # csrc/audio.hip: outputs per tile, bounds of a tile's staged input samples and of the table
_resample_cache = {}


def _rate_ratio(orig_sr, target_sr):
    for r in (orig_sr, target_sr):
        if isinstance(r, bool) or int(r) != r or int(r) <= 0:
            raise ValueError('sample rates must be positive integers (got %r -> %r)' % (orig_sr, target_sr))
    g = math.gcd(int(orig_sr), int(target_sr))
    return int(target_sr) // g, int(orig_sr) // g


def resample_filter(up, down):
    """The FIR of scipy.signal.resample_poly(x, up, down) with its defaults, in closed form (f64):
    firwin(2 half + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up with half = 10 max(up, down).  Returns (h, half); up == down is the copy ([1.], 0)."""
    if up == down:
        return np.ones(1), 0
    mx = max(up, down)
    half = 10 * mx
    m = np.arange(2 * half + 1) - float(half)
    cutoff = 1.0 / mx
    h = cutoff * np.sinc(cutoff * m)
    h *= np.i0(5.0 * np.sqrt(1.0 - (m / half) ** 2)) / np.i0(5.0)          # kaiser(beta = 5), symmetric
    h /= np.sum(h)                                                          # firwin(scale=True): unit gain at 0 Hz
    return h * up, half


def _resample_table(up, down, device):
    """(coef [up][tpp] f32 on the device, half, tpp): h phase-major -- coef[ph][i] = h[ph + i up], zero past the end, tpp = the taps of the longest
    phase rounded up to a multiple of 4 --, designed in f64, rounded once, cached per (up, down, device) like the mel basis."""
    key = (up, down, str(device))
    if key not in _resample_cache:
        half = 0 if up == down else 10 * max(up, down)
        tpp = ((2 * half) // up + 1 + 3) // 4 * 4
        if not _lib.lib().ss_audio_resample_supported(up, down, half, tpp):
            raise ValueError('resampling by %d/%d is not supported: its phase table (%d floats) or the input span of a %d-sample output tile exceeds the '
                             "kernel's bounds (%d floats, %d samples, 64 KB together)" % (up, down, up * tpp, RESAMPLE_TILE, RESAMPLE_TABLE_FLOATS, RESAMPLE_SPAN))
        h, _ = resample_filter(up, down)
        pad = np.zeros(up * tpp, dtype=np.float64)
        pad[:h.shape[0]] = h
        coef = np.ascontiguousarray(pad.reshape(tpp, up).T).astype(np.float32)
        _resample_cache[key] = (torch.from_numpy(coef).to(device), half, tpp)
        _settle_cache(device)
    return _resample_cache[key]


def resampled_length(n, up, down):
    return (int(n) * up + down - 1) // down


def _flat_signals(signals):
    """list of 1-D tensors / arrays, or (flat, lengths) -> (flat f32 tensor where the kernels read, lengths)."""
    if isinstance(signals, tuple):
        flat, lens = signals[0].reshape(-1), [int(n) for n in signals[1]]
        if flat.dtype != torch.float32 or int(flat.shape[0]) != sum(lens):
            raise ValueError('packed signals: a flat float32 tensor of sum(lengths) samples')
    else:
        ts = [t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(np.asarray(t))) for t in signals]
        if any(t.dim() != 1 for t in ts):
            raise ValueError('every signal must be 1-D')
        lens = [int(t.shape[0]) for t in ts]
        flat = torch.cat([t.to(torch.float32) for t in ts]) if len(ts) > 1 else ts[0].to(torch.float32).contiguous()
    if not lens:
        raise ValueError('at least one signal is expected')
    return flat.to(_lib.kernel_device_for(flat)), lens


def _resample_rows(flat, out, rows, up, down, gains=None, clip=False):
    """One ss_audio_resample_batch launch: rows = [(first input sample, n, first output sample, n_out)] into the flat buffers `flat` -> `out`."""
    from . import staging, torch_ops  # noqa: F401
    coef, half, tpp = _resample_table(up, down, flat.device)
    table, = staging.upload([np.asarray(rows, dtype=np.int64).reshape(-1, 4)], flat.device)
    torch.ops.silent_speech.audio_resample(flat, out, table, coef, gains, up, down, half, tpp, bool(clip), int(sum(r[3] for r in rows)))
    return out


def resample_audio_batch(signals, orig_sr, target_sr, *, gains=None, clip=False):
    """scipy.signal.resample_poly(x, target_sr / g, orig_sr / g) (the band-limited resample of load_audio, data_utils.py:75; g = gcd) of every signal of
    a batch in ONE launch.  signals: a list of 1-D signals, or (flat f32 tensor holding them back to back, lengths).  gains: optional per-signal
    scale (tensor or sequence, e.g. volume_gains) applied to the output; clip: np.clip(., -1, 1) afterwards (:78).  Returns (flat f32 device tensor,
    lengths) with lengths[u] = ceil(n_u up / down) -- what mel_spectrogram_batch takes."""
    up, down = _rate_ratio(orig_sr, target_sr)
    flat, lens = _flat_signals(signals)
    out_lens = [resampled_length(n, up, down) for n in lens]
    out = torch.empty(sum(out_lens), dtype=torch.float32, device=flat.device)
    if gains is not None:
        gains = torch.as_tensor(gains, dtype=torch.float32).to(flat.device).contiguous()
        if tuple(gains.shape) != (len(lens),):
            raise ValueError('one gain per signal')
    _resample_table(up, down, flat.device)                      # an unsupported ratio is refused even for an empty batch
    if out.numel():
        io, oo = np.concatenate([[0], np.cumsum(lens)]), np.concatenate([[0], np.cumsum(out_lens)])
        _resample_rows(flat, out, [(int(io[u]), lens[u], int(oo[u]), out_lens[u]) for u in range(len(lens))], up, down, gains, clip)
    return out, out_lens


def resample_audio(audio, orig_sr, target_sr, *, clip=False):
    """One 1-D signal (tensor or array) -> its resample_poly at target_sr, a float32 tensor on the device."""
    if np.ndim(audio) != 1:
        raise ValueError('audio must be 1-D')
    return resample_audio_batch([audio], orig_sr, target_sr, clip=clip)[0]


def volume_levels(signals):
    """(levels [R][2] = {max frame RMS, max |x|}, gains [R]) of normalize_volume for every signal, on the device (librosa.feature.rms defaults of
    librosa >= 0.10: frames of 2048 every 512 samples, centred with zero padding)."""
    from . import staging, torch_ops  # noqa: F401
    flat, lens = _flat_signals(signals)
    blocks = [(n + 511) // 512 for n in lens]
    io, bo = np.concatenate([[0], np.cumsum(lens)]), np.concatenate([[0], np.cumsum(blocks)])
    table, = staging.upload([np.asarray([(int(io[u]), lens[u], int(bo[u])) for u in range(len(lens))], dtype=np.int64)], flat.device)
    if not flat.numel():
        flat = flat.new_zeros(1)
    return torch.ops.silent_speech.audio_level(flat, table, int(bo[-1]))


def volume_gains(signals):
    """normalize_volume's scale per signal (data_utils.py:19-27): 0.2 / (max frame RMS + 0.01), or 1 / max |x| where that would leave the peak above 1.
    A device f32 tensor [R]; nothing returns to the host."""
    return volume_levels(signals)[1]


def normalize_volume(audio):
    """data_utils.py:19-27 on the device: a 1-D signal -> the levelled float32 signal."""
    if np.ndim(audio) != 1:
        raise ValueError('audio must be 1-D')
    flat, lens = _flat_signals([audio])
    return resample_audio_batch((flat, lens), 1, 1, gains=volume_gains((flat, lens)))[0]


def load_audio(audio, sample_rate, start=None, end=None, max_frames=None, renormalize_volume=False):
    """data_utils.py:64-83 from an array already in memory: first channel of a 2-D array, audio[start:end], optional normalize_volume, the band-limited
    resample to 22 050 Hz when sample_rate differs, clip to [-1, 1], mel_spectrogram(1024, 80, 22050, 256, 1024, 0, 8000) -> (frames, 80) float32 on the
    device, truncated to max_frames.  Decoding a file is out of scope."""
    if isinstance(audio, (str, bytes)) or hasattr(audio, '__fspath__'):
        raise TypeError('load_audio: decoding an audio file is out of scope -- pass the decoded samples and their sample rate')
    x = audio if torch.is_tensor(audio) else torch.from_numpy(np.ascontiguousarray(np.asarray(audio)))
    if x.dim() > 1:
        x = x[:, 0]
    if start is not None or end is not None:
        x = x[start:end]
    flat, lens = _flat_signals([x])
    gains = volume_gains((flat, lens)) if renormalize_volume else None
    if int(sample_rate) != 22050 or gains is not None:
        flat, lens = resample_audio_batch((flat, lens), sample_rate, 22050, gains=gains, clip=True)
    mel, frames = mel_spectrogram_batch((flat, lens), clip=True)
    n = frames[0] if max_frames is None else min(frames[0], int(max_frames))
    return mel[0, :n]


# ------------------------------------------------------------------ noise reduction: stationary spectral gating (csrc/spectral_gate.hip)
GATE_N_FFT, GATE_HOP, GATE_BINS, GATE_MAX_NF, GATE_MAX_NT = 1024, 256, 513, 32, 8       # the sizes noisereduce uses; bounds of the mask smoothing
_gate_cache = {}


def _gate_windows(device):
    """(3, 1024) f32 on the device: [w / W | w W / 512 | w^2] of the periodic Hann window w, W = sum w; designed in f64, rounded once, cached."""
    key = str(device)
    if key not in _gate_cache:
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(GATE_N_FFT) / GATE_N_FFT)
        W = float(w.sum())
        _gate_cache[key] = torch.from_numpy(np.stack([w / W, w * (W / 512.0), w * w]).astype(np.float32)).to(device)
        _settle_cache(device)
    return _gate_cache[key]


def gate_frames(n):
    """frames of a signal of n >= 1 samples: ceil(n / 256) + 1 (centred frames of 1024 every 256 samples, the last one at or behind the end)."""
    return (int(n) + GATE_HOP - 1) // GATE_HOP + 1


def gate_smoothing(sample_rate, freq_mask_smooth_hz=500, time_mask_smooth_ms=50):
    """(n_f, n_t): half widths of the mask's triangular smoothing as noisereduce derives them (513 rows over sr / 2, frames of 256 samples); both
    arguments None: no smoothing.  Refused beyond the kernel's 32 rows x 8 frames."""
    if not (float(sample_rate) > 0):
        raise ValueError('the sample rate must be positive (got %r)' % (sample_rate,))
    if freq_mask_smooth_hz is None and time_mask_smooth_ms is None:
        return 0, 0
    n_f = 0 if freq_mask_smooth_hz is None else int(freq_mask_smooth_hz / (sample_rate / 512))
    n_t = 0 if time_mask_smooth_ms is None else int(time_mask_smooth_ms / (256000 / sample_rate))
    if not (0 <= n_f <= GATE_MAX_NF and 0 <= n_t <= GATE_MAX_NT):
        raise ValueError('mask smoothing over %d frequency rows x %d frames (%r Hz, %r ms at %r Hz) is not supported: at most %d x %d'
                         % (n_f, n_t, freq_mask_smooth_hz, time_mask_smooth_ms, sample_rate, GATE_MAX_NF, GATE_MAX_NT))
    return n_f, n_t


def _gate_table(lens, device, rows=None):
    """(table (R, 4) int64 on the device = (first sample, L, first frame, F) of the signals `rows` (default: all) of a flat buffer that holds signals of
    `lens` samples back to back, total frames)"""
    from . import staging
    rows = list(range(len(lens))) if rows is None else list(rows)
    if any(lens[u] < 1 for u in rows):
        raise ValueError('an empty signal cannot be gated')
    if any(lens[u] >= 2 ** 31 - 2048 for u in rows):
        raise ValueError('signals of 2^31 samples and more are not supported')
    io = np.concatenate([[0], np.cumsum(lens)])
    frames = [gate_frames(lens[u]) for u in rows]
    fo = np.concatenate([[0], np.cumsum(frames)])
    table, = staging.upload([np.stack([[int(io[u]) for u in rows], [lens[u] for u in rows], fo[:-1], frames], 1).astype(np.int64)], device)
    return table, int(fo[-1])


def _gate_rows(flat, out, lens, rows, profile, n_f, n_t, prop_decrease=1.0, return_bits=False):
    """One ss_spectral_gate_batch launch sequence: the signals `rows` of the flat buffer `flat` -> their places in `out`."""
    from . import torch_ops  # noqa: F401
    table, total_frames = _gate_table(lens, flat.device, rows)
    return torch.ops.silent_speech.spectral_gate(flat, out, table, _gate_windows(flat.device), profile.thresh.to(flat.device), total_frames, n_f, n_t,
                                                 float(prop_decrease), bool(return_bits))


class NoiseProfile(object):
    """The stationary gate's threshold per frequency row: thresh (513,) f32 in dB on the device, with the sample rate and n_std it was made for."""

    def __init__(self, thresh, sample_rate, n_std_thresh_stationary=1.5):
        if tuple(thresh.shape) != (GATE_BINS,) or thresh.dtype != torch.float32:
            raise ValueError('thresh: a (513,) float32 tensor')
        self.thresh, self.sr, self.n_std = thresh.contiguous(), sample_rate, float(n_std_thresh_stationary)

    @classmethod
    def from_noise(cls, noise, sample_rate, n_std_thresh_stationary=1.5):
        """mean + n_std * std (population) over the noise clip's frames of 20 log10(|STFT| + eps), clamped per row at its maximum - 80."""
        from . import torch_ops  # noqa: F401
        if not (float(sample_rate) > 0):
            raise ValueError('the sample rate must be positive (got %r)' % (sample_rate,))
        if np.ndim(noise) != 1 or len(noise) == 0:
            raise ValueError('the noise clip must be 1-D and non-empty')
        flat, lens = _flat_signals([noise])
        table, frames = _gate_table(lens, flat.device)
        thresh = torch.ops.silent_speech.spectral_gate_profile(flat, table, _gate_windows(flat.device), frames, float(n_std_thresh_stationary))
        return cls(thresh, sample_rate, n_std_thresh_stationary)


def reduce_noise_batch(signals, profile, *, prop_decrease=1.0, freq_mask_smooth_hz=500, time_mask_smooth_ms=50, return_bits=False):
    """noisereduce.reduce_noise(y, sr, y_noise, stationary=True) of every signal of a batch against ONE NoiseProfile, one launch per kernel for the whole
    batch.  signals: a list of 1-D signals, or (flat f32 tensor, lengths) as for resample_audio_batch.  Returns (flat f32 device tensor, lengths) --
    and the final binary gate (total frames, 17) int32 as a third item with return_bits."""
    if not isinstance(profile, NoiseProfile):
        raise TypeError('profile: a NoiseProfile (NoiseProfile.from_noise(noise, sample_rate))')
    if not (0.0 <= float(prop_decrease) <= 1.0):
        raise ValueError('prop_decrease must lie in [0, 1]')
    n_f, n_t = gate_smoothing(profile.sr, freq_mask_smooth_hz, time_mask_smooth_ms)
    flat, lens = _flat_signals(signals)
    out = torch.empty_like(flat)
    bits = _gate_rows(flat, out, lens, None, profile, n_f, n_t, prop_decrease, return_bits)
    return (out, lens, bits) if return_bits else (out, lens)


def reduce_noise(y, sr, y_noise=None, *, profile=None, stationary=True, prop_decrease=1.0, n_std_thresh_stationary=1.5, freq_mask_smooth_hz=500,
                 time_mask_smooth_ms=50):
    """noisereduce.reduce_noise(y=y, sr=sr, y_noise=y_noise, stationary=True, ...) (data_collection/clean_audio.py:53) on the device: a float32 tensor of
    len(y) samples.  The threshold comes from `profile`, else from y_noise, else from y itself."""
    if not stationary:
        raise NotImplementedError('reduce_noise: the non-stationary gate is out of scope; only stationary=True is built here -- '
                                  'the non-stationary gate is reduce_noise_nonstationary')
    if not (float(sr) > 0):
        raise ValueError('the sample rate must be positive (got %r)' % (sr,))
    if np.ndim(y) != 1 or len(y) == 0:
        raise ValueError('y must be 1-D and non-empty')
    if profile is None:
        if y_noise is not None and (np.ndim(y_noise) != 1 or len(y_noise) == 0):
            raise ValueError('the noise clip must be 1-D and non-empty')
        profile = NoiseProfile.from_noise(y if y_noise is None else y_noise, sr, n_std_thresh_stationary)
    return reduce_noise_batch([y], profile, prop_decrease=prop_decrease, freq_mask_smooth_hz=freq_mask_smooth_hz, time_mask_smooth_ms=time_mask_smooth_ms)[0]


def nonstationary_coefficient(sample_rate, time_constant_s=2.0):
    """b of the non-stationary gate's one-pole level smoother, as noisereduce derives it: t = time_constant_s * sample_rate / 256 frames,
    b = (sqrt(1 + 4 t^2) - 1) / (2 t^2)."""
    if not (float(sample_rate) > 0):
        raise ValueError('the sample rate must be positive (got %r)' % (sample_rate,))
    if not (float(time_constant_s) > 0):
        raise ValueError('time_constant_s must be positive (got %r)' % (time_constant_s,))
    t = float(time_constant_s) * float(sample_rate) / GATE_HOP
    return (np.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t)


def _gate_ns_rows(flat, out, lens, rows, b, n_f, n_t, n_mult=2.0, slope=10.0, prop_decrease=1.0, return_mask=False):
    """One ss_spectral_gate_ns_batch launch sequence: the signals `rows` of the flat buffer `flat` -> their places in `out`."""
    from . import torch_ops  # noqa: F401
    table, total_frames = _gate_table(lens, flat.device, rows)
    return torch.ops.silent_speech.spectral_gate_nonstationary(flat, out, table, _gate_windows(flat.device), total_frames, float(b), float(n_mult), float(slope),
                                                               n_f, n_t, float(prop_decrease), bool(return_mask))


def reduce_noise_nonstationary_batch(signals, sample_rate, *, time_constant_s=2.0, thresh_n_mult_nonstationary=2.0, sigmoid_slope_nonstationary=10.0,
                                     prop_decrease=1.0, freq_mask_smooth_hz=500, time_mask_smooth_ms=50, return_mask=False):
    """noisereduce.reduce_noise(y, sr) -- its default, NON-STATIONARY gate -- of every signal of a batch, one launch per kernel for the whole batch
    (csrc/spectral_gate_ns.hip).  No noise clip: per frequency row the level is the signal's own |STFT| smoothed forward and backward over time with the
    time constant time_constant_s, and the mask a sigmoid on the relative excess over it.  Every signal is ONE chunk with scipy's steady-state initial
    conditions (noisereduce cuts at 600 000 samples and surrounds each chunk with zeros: DESIGN section 8).  signals: a list of 1-D signals, or
    (flat f32 tensor, lengths).  Returns (flat f32 device tensor, lengths) -- and the unsmoothed mask (total frames, 513) f32 as a third item with
    return_mask."""
    b = nonstationary_coefficient(sample_rate, time_constant_s)
    if not (float(sigmoid_slope_nonstationary) > 0):
        raise ValueError('sigmoid_slope_nonstationary must be positive (got %r)' % (sigmoid_slope_nonstationary,))
    if not np.isfinite(float(thresh_n_mult_nonstationary)):
        raise ValueError('thresh_n_mult_nonstationary must be finite')
    if not (0.0 <= float(prop_decrease) <= 1.0):
        raise ValueError('prop_decrease must lie in [0, 1]')
    n_f, n_t = gate_smoothing(sample_rate, freq_mask_smooth_hz, time_mask_smooth_ms)
    flat, lens = _flat_signals(signals)
    out = torch.empty_like(flat)
    mask = _gate_ns_rows(flat, out, lens, None, b, n_f, n_t, thresh_n_mult_nonstationary, sigmoid_slope_nonstationary, prop_decrease, return_mask)
    return (out, lens, mask) if return_mask else (out, lens)


def reduce_noise_nonstationary(y, sr, *, time_constant_s=2.0, thresh_n_mult_nonstationary=2.0, sigmoid_slope_nonstationary=10.0, prop_decrease=1.0,
                               freq_mask_smooth_hz=500, time_mask_smooth_ms=50):
    """noisereduce.reduce_noise(y=y, sr=sr) with its default stationary=False on the device: a float32 tensor of len(y) samples."""
    if np.ndim(y) != 1 or len(y) == 0:
        raise ValueError('y must be 1-D and non-empty')
    return reduce_noise_nonstationary_batch([y], sr, time_constant_s=time_constant_s, thresh_n_mult_nonstationary=thresh_n_mult_nonstationary,
                                            sigmoid_slope_nonstationary=sigmoid_slope_nonstationary, prop_decrease=prop_decrease,
                                            freq_mask_smooth_hz=freq_mask_smooth_hz, time_mask_smooth_ms=time_mask_smooth_ms)[0]


def session_gains(max_rmses, silent_cutoff=0.02, smoothing_width=20, target_rms=0.2):
    """clean_audio.py:33-47 on the host (a few dozen scalars): file i's gain is target_rms / the mean of the max frame RMS values above the cutoff among
    the files i - 20 .. i + 20; None when some file has no such neighbour ("long run of quiet audio": no levelling at all)."""
    m = [float(v) for v in max_rmses]
    gains = []
    for i in range(len(m)):
        vs = [m[j] for j in range(max(0, i - smoothing_width), min(i + 1 + smoothing_width, len(m))) if m[j] > silent_cutoff]
        if not vs:
            return None
        gains.append(target_rms / float(np.mean(vs)))
    return gains


def clean_session(signals, sample_rate, noise=None, *, gate='stationary'):
    """data_collection/clean_audio.py clean_directory from decoded arrays: the session's recordings in file order (signals[0] is the silence clip
    0_audio unless `noise` is given) -> (flat f32 device tensor at 22 050 Hz, lengths).  Max frame RMS per file (volume_levels on the raw signals) ->
    the +-20-file smoothing on the host -> the stationary gate against the noise clip's profile -> the band-limited resample to 22 050 Hz with the
    gain 0.2 / smoothed max -> x / max |x| * 0.99 where the peak exceeds 0.99.  A long run of quiet audio skips the levelling, as the reference does.
    gate='nonstationary': for sessions without a silence clip -- no profile is made, every signal (signals[0] included) goes through
    reduce_noise_nonstationary_batch with its defaults, gated against itself; `noise` must then be None."""
    if gate not in ('stationary', 'nonstationary'):
        raise ValueError("gate: 'stationary' or 'nonstationary' (got %r)" % (gate,))
    if gate == 'nonstationary' and noise is not None:
        raise ValueError("gate='nonstationary' takes no noise clip")
    flat, lens = _flat_signals(signals)
    levels = volume_levels((flat, lens))[0][:, 0].cpu().tolist()
    gains = session_gains(levels)
    if gate == 'nonstationary':
        clean, lens = reduce_noise_nonstationary_batch((flat, lens), sample_rate)
    else:
        if noise is None:
            noise = flat[:lens[0]]
        profile = NoiseProfile.from_noise(noise, sample_rate)
        clean, lens = reduce_noise_batch((flat, lens), profile)
    out, out_lens = resample_audio_batch((clean, lens), sample_rate, 22050, gains=gains)
    if gains is not None:
        peak = volume_levels((out, out_lens))[0][:, 1]
        scale = torch.where(peak > 0.99, 0.99 / peak, torch.ones_like(peak))
        out, out_lens = resample_audio_batch((out, out_lens), 1, 1, gains=scale)
    return out, out_lens


def get_emg_features(emg_data, debug=False):
    """data_utils.py:85-136: (n, C) EMG at 516.79 Hz -> (1 + (n - 16) // 6, 14 C) float32 hand-crafted features (per channel: frame mean
    and RMS of the twice box-filtered signal w, RMS / mean / zero-crossing rate of the residual p = x - mean - w, 9 |rfft| bins of the
    Hann-windowed frame).  A numpy array in gives a numpy array out; a tensor gives a tensor on its device.  Computed in f64 on the device by
    csrc/emg_features.hip through torch.ops.silent_speech.emg_features (torch_ops.py).  debug=True (the reference's matplotlib plots) is
    not supported."""
    if debug:
        raise NotImplementedError('get_emg_features(debug=True): the diagnostic plots are not part of this package')
    from .read_emg import _to_device_2d
    if np.ndim(emg_data) != 2:
        raise ValueError('emg_data must be (samples, channels)')
    if emg_data.shape[0] < 16:
        raise ValueError('Input is too short (n=%d) for frame_length=16' % emg_data.shape[0])      # librosa.util.frame raises
    x, restore = _to_device_2d(emg_data)
    from . import torch_ops  # noqa: F401
    y = torch.ops.silent_speech.emg_features(x)
    return y.cpu().numpy() if not torch.is_tensor(emg_data) else y


class FeatureNormalizer(object):
    """data_utils.py:138-156 (normalize mutates its argument in place, like the reference)."""

    def __init__(self, feature_samples, share_scale=False):
        feature_samples = np.concatenate(feature_samples, axis=0)
        self.feature_means = feature_samples.mean(axis=0, keepdims=True)
        self.feature_stddevs = feature_samples.std() if share_scale else feature_samples.std(axis=0, keepdims=True)

    def normalize(self, sample):
        sample -= self.feature_means
        sample /= self.feature_stddevs
        return sample

    def inverse(self, sample):
        return sample * self.feature_stddevs + self.feature_means


class PackJob(object):
    """One combine_fixed_length (or plain concatenation, length=None) of device tensors as data: the [pointers | cumulative byte
    offsets] table the gather kernel (csrc/optim.hip `ss_concat_pad`) reads, and the launch over it.  Building the table is host
    arithmetic on ~40 (pointer, size) pairs; it travels to the device through staging.upload -- alone (combine_fixed_length) or
    together with every other table of the batch (transduction_model.prepare_batch: ONE copy per batch)."""

    def __init__(self, tensor_list, length=None):
        first = tensor_list[0]
        trailing = tuple(first.shape[1:])
        ts = [t if t.is_contiguous() else t.contiguous() for t in tensor_list]
        assert all(t.dtype == first.dtype and tuple(t.shape[1:]) == trailing for t in ts), 'utterances of one batch share dtype and feature shape'
        frames = sum(int(t.shape[0]) for t in ts)
        row_bytes = first.element_size()
        for d in trailing:
            row_bytes *= int(d)
        if length is None:
            self.out_shape = (frames,) + trailing
            total = frames * row_bytes
        else:
            rows = (frames + length - 1) // length
            self.out_shape = (rows, length) + trailing
            total = rows * length * row_bytes
        n = len(ts)
        table = np.empty(2 * n + 1, dtype=np.int64)
        table[:n] = np.fromiter((t.data_ptr() for t in ts), dtype=np.uint64, count=n).view(np.int64)
        sizes = np.fromiter((int(t.shape[0]) for t in ts), dtype=np.int64, count=n) * row_bytes
        table[n] = 0
        np.cumsum(sizes, out=table[n + 1:])
        gran = 16
        probe = int(np.bitwise_or.reduce(table[:n])) | int(np.bitwise_or.reduce(sizes)) | total
        while gran > 1 and probe % gran:
            gran //= 2
        self.gran = 1 if gran == 2 else gran
        self.table, self.n, self.total, self.keep = table, n, total, ts
        self.dtype, self.device = first.dtype, first.device

    def launch(self, table_dev):
        out = torch.empty(self.out_shape, dtype=self.dtype, device=self.device)
        _lib.check(_lib.lib().ss_concat_pad(_lib.ptr(table_dev), self.n, _lib.ptr(out), self.total, self.gran, _lib.stream_of(out)), 'ss_concat_pad')
        return out


def _host_pack(tensor_list, length, pin=False):
    first = tensor_list[0]
    trailing = tuple(first.shape[1:])
    frames = sum(int(t.shape[0]) for t in tensor_list)
    rows = frames if length is None else (frames + length - 1) // length * length
    out = torch.empty((rows,) + trailing, dtype=first.dtype, pin_memory=pin)
    if frames:
        torch.cat(list(tensor_list), 0, out=out[:frames])
    out[frames:].zero_()
    return out if length is None else out.view((rows // length, length) + trailing)


def combine_fixed_length(tensor_list, length):
    """data_utils.py:158-167: the utterances back to back along time, zero-padded to a whole number of rows of `length` frames,
    viewed as (rows, length, ...).  Device tensors are packed by ONE gather launch over an offset table (csrc/optim.hip
    `ss_concat_pad`; the table is rebuilt for every call -- a training loop hands over new tensors every step -- and uploaded
    from pinned memory).  Host tensors (staging code, tests) are packed with a host concatenation."""
    first = tensor_list[0]
    on_device = _lib.kernels_can_read(first)
    if not on_device:
        return _host_pack(tensor_list, length)
    from . import staging
    job = PackJob(tensor_list, length)
    table, = staging.upload([job.table], first.device)
    return job.launch(table)


def decollate_tensor(tensor, lengths):
    """data_utils.py:169-178."""
    b, s, d = tensor.size()
    tensor = tensor.reshape(b * s, d)
    results, idx = [], 0
    for length in lengths:
        assert idx + length <= b * s
        results.append(tensor[idx:idx + length])
        idx += length
    return results
