"""float64 numpy restatement of noisereduce 3's STATIONARY spectral gate with its defaults (the reference's data_collection/clean_audio.py:53,
nr.reduce_noise(y=data, sr=rate, y_noise=silence, stationary=True)) -- the pinned definition of csrc/spectral_gate.hip.  noisereduce itself is
third-party and not vendored: parity with its own numbers is unpinned.

N = 1024, hop H = 256, w = periodic Hann(1024), W = sum w.  A signal of L >= 1 samples has F = ceil(L / H) + 1 frames; frame f covers the samples
[f H - 512, f H + 512), zeros outside [0, L).  For L >= 1024 this is scipy.signal.stft(x, nfft=1024, nperseg=1024, noverlap=768, padded=False) and
scipy.signal.istft (tests/test_spectral_gate.py asserts it); for shorter signals scipy shrinks nperseg, hence the explicit framing.

Error bounds (all derived, none fitted).  u = 2^-24, the unit roundoff of f32.
  G = 32: the roundings on the longest path of the kernel's forward FFT, counted from csrc/fft1024.h and csrc/spectral_gate.hip: window product 1; three
      radix-8 butterflies of 5 each (the +- of the radix-2 split, the sum and the 1 / sqrt 2 product of the odd twiddles, two +- levels of the 4-point
      transform) = 15; two twiddle products of 3 each (the rounded twiddle, the product, the fma) = 6; the recombination of the real signal's bins 5
      (sum, twiddle product 3, sum); |X| 3 (square, fma, square root): 30, taken as 32 for the component-wise sqrt 2 of the three complex products.
      The inverse path has the same count (5 for building Z, 21 for the passes, 2 for the rounded synthesis window and its product).
  per bin:   | |X| kernel - |X| oracle | <= G u S_f,  S_f = sum_n |w[n] frame_f[n]| / W  (every intermediate is a partial sum of those terms).
  per frame: the passes are unitary up to scale, so in the 2-norm  |dX_f| <= G u |X_f|  and for the resynthesised frame y_f = W irfft(X m)
             |dy_f|_2 <= u (G max_k m[k, f] |w frame_f|_2 + (G + 2) |y_f|_2)   (forward error through the mask; the rounded mask and the product: 2; the inverse: G),
             which also bounds every sample of dy_f.
  output:    out = sum_f w y_f / sum_f w^2:  |d out[n]| <= (sum_f w e_f + 8 u sum_f |w y_f|) / sum_f w^2  (3 + 3 additions, the rounded w^2, the division).
"""
import numpy as np

N, H, BINS, ROW = 1024, 256, 513, 17
EPS = float(np.finfo(np.float64).eps)
U = 2.0 ** -24
G = 32
w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)          # periodic Hann
W = float(w.sum())


def n_frames(L):
    return -(-int(L) // H) + 1


def frames(x):
    """(F, 1024): frame f = x[f H - 512 : f H + 512], zeros outside the signal."""
    x = np.asarray(x, dtype=np.float64)
    F = n_frames(len(x))
    xp = np.concatenate([np.zeros(N // 2), x, np.zeros((F - 1) * H + N // 2 - len(x))])
    return np.stack([xp[f * H:f * H + N] for f in range(F)])


def stft(x):
    """X (513, F) = rfft(w frame) / W"""
    return np.fft.rfft(frames(x) * w, axis=1).T / W


def frame_sums(x):
    """S_f = sum_n |w[n] frame_f[n]| / W"""
    return np.abs(frames(x) * w).sum(1) / W


def synthesis_frames(Y):
    """y_f (F, 1024) = irfft(Y[:, f]) W"""
    return np.fft.irfft(Y.T, n=N, axis=1) * W


def overlap_add(yf, L, skip_frame=None):
    """out[n] = sum_f w y_f / sum_f w^2 over the frames that cover n (skip_frame: one frame left out, for the test that the bound discriminates)"""
    F = yf.shape[0]
    num, den = np.zeros((F - 1) * H + N), np.zeros((F - 1) * H + N)
    for f in range(F):
        if f != skip_frame:
            num[f * H:f * H + N] += w * yf[f]
            den[f * H:f * H + N] += w * w
    return (num / np.where(den > 1e-10, den, 1.0))[N // 2:N // 2 + L]


def istft(Y, L):
    return overlap_add(synthesis_frames(Y), L)


def db(X):
    """20 log10(|X| + eps), clamped per frequency row at the row's maximum - 80 (top_db)"""
    d = 20.0 * np.log10(np.abs(X) + EPS)
    return np.maximum(d, d.max(axis=1, keepdims=True) - 80.0)


def profile(noise, n_std=1.5):
    """thresh (513,) f64 = mean + n_std std (population) of the noise clip's clamped dB"""
    d = db(stft(noise))
    return d.mean(1) + n_std * d.std(1)


def smoothing(sr, freq_mask_smooth_hz=500, time_mask_smooth_ms=50):
    if freq_mask_smooth_hz is None and time_mask_smooth_ms is None:
        return 0, 0
    return (0 if freq_mask_smooth_hz is None else int(freq_mask_smooth_hz / (sr / 512)),
            0 if time_mask_smooth_ms is None else int(time_mask_smooth_ms / (256000 / sr)))


def tri(n):
    return np.concatenate([np.linspace(0, 1, n + 1, endpoint=False), np.linspace(1, 0, n + 2)])[1:-1]


def smooth(m, n_f, n_t):
    """fftconvolve(m, outer(tri(n_f), tri(n_t)) / sum, mode='same'): zeros outside the mask (direct sums: the filter is tiny)"""
    filt = np.outer(tri(n_f), tri(n_t))
    filt /= filt.sum()
    Fk, Ft = m.shape
    mp = np.zeros((Fk + 2 * n_f, Ft + 2 * n_t))
    mp[n_f:n_f + Fk, n_t:n_t + Ft] = m
    out = np.zeros_like(m, dtype=np.float64)
    for a in range(2 * n_f + 1):
        for b in range(2 * n_t + 1):
            out += filt[2 * n_f - a, 2 * n_t - b] * mp[a:a + Fk, b:b + Ft]
    return out


def gate(X, thresh):
    """(bits (513, F) bool = clamped dB > thresh, open rows (513,) bool).  thresh in dB, f64 or the f32 table the kernel gets."""
    d = 20.0 * np.log10(np.abs(X) + EPS)
    top = d.max(axis=1) - 80.0
    th = np.asarray(thresh, dtype=np.float64)
    return np.maximum(d, top[:, None]) > th[:, None], top > th


def margins(X, thresh, S):
    """How far every bin, and every row's top_db decision, is from flipping, against the kernel's error bound:
    (| |X| - 10^(thresh / 20) | - G u S_f  per bin,  | max_f |X| 1e-4 - 10^(thresh / 20) | - G u 1e-4 max_f S_f  per row); positive = decided."""
    a = 10.0 ** (np.asarray(thresh, dtype=np.float64) / 20.0)
    mag = np.abs(X)
    return np.abs(mag - a[:, None]) - G * U * S[None, :], np.abs(mag.max(1) * 1e-4 - a) - G * U * 1e-4 * S.max()


def reduce_noise(x, thresh, n_f=0, n_t=0, p=1.0, mask=None, skip_frame=None, shift_mask=0, details=False):
    """The stationary gate of signal x against thresh (513,) in dB.  mask (513, F) replaces the binary gate; skip_frame / shift_mask distort the
    result on purpose (a frame left out of the overlap-add, the mask moved by a bin).  details: also returns a dict with the derived bound."""
    x = np.asarray(x, dtype=np.float64)
    X = stft(x)
    bits = gate(X, thresh)[0] if mask is None else np.asarray(mask, dtype=np.float64)
    m = smooth(bits * p + (1.0 - p), n_f, n_t)
    if shift_mask:
        m = np.roll(m, shift_mask, axis=0)
    yf = synthesis_frames(X * m)
    out = overlap_add(yf, len(x), skip_frame)
    if not details:
        return out
    fr = frames(x) * w
    e = U * (G * np.abs(m).max(0) * np.sqrt((fr ** 2).sum(1)) + (G + 2) * np.sqrt((yf ** 2).sum(1)))          # per frame, bounds every sample of dy_f
    F = yf.shape[0]
    num, den = np.zeros((F - 1) * H + N), np.zeros((F - 1) * H + N)
    for f in range(F):
        num[f * H:f * H + N] += w * e[f] + 8 * U * np.abs(w * yf[f])
        den[f * H:f * H + N] += w * w
    bound = (num / np.where(den > 1e-10, den, 1.0))[N // 2:N // 2 + len(x)]
    return out, {'X': X, 'mask': m, 'S': frame_sums(x), 'bound': bound}


def profile_bound(noise, n_std=1.5):
    """(thresh f64, bound per row) for a kernel whose |X| is within G u S_f per bin and which does the rest in f64 and rounds thresh to f32 once:
    the interval [|X| - e, |X| + e] through 20 log10(. + eps) and the clamp (both monotone), then |d mean| <= mean |d|, |d std| <= sqrt(mean d^2)."""
    X = stft(noise)
    mag, e = np.abs(X), G * U * frame_sums(noise)[None, :]
    lo, hi = 20.0 * np.log10(np.maximum(mag - e, 0.0) + EPS), 20.0 * np.log10(mag + e + EPS)
    lo, hi = np.maximum(lo, lo.max(1, keepdims=True) - 80.0), np.maximum(hi, hi.max(1, keepdims=True) - 80.0)
    d = db(X)
    dev = np.maximum(hi - d, d - lo)
    th = d.mean(1) + n_std * d.std(1)
    return th, dev.mean(1) + n_std * np.sqrt((dev ** 2).mean(1)) + 2 * U * np.abs(th) + 1e-9


def unpack_bits(rows, F0=0, F=None):
    """(frames, 17) int32 gate rows of the kernel -> (513, F) bool"""
    r = np.asarray(rows).astype(np.int64) & 0xffffffff
    r = r[F0:] if F is None else r[F0:F0 + F]
    k = np.arange(BINS)
    return ((r[:, k >> 5] >> (k & 31)) & 1).astype(bool).T
