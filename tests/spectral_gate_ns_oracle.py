"""float64 numpy restatement of noisereduce 3's NON-STATIONARY spectral gate (its default mode, nr.reduce_noise(y, sr)) -- the pinned definition of
csrc/spectral_gate_ns.hip.  The framing, the STFT and the overlap-add are those of tests/spectral_gate_oracle.py.  noisereduce itself is third-party
and not vendored: parity with its own numbers is unpinned, and the stated differences (one chunk per signal, no 30 000 zero samples around it, the
recurrence started from scipy's steady-state initial conditions, a finite mask for digital silence) are listed in DESIGN section 8.

For one signal x of L >= 1 samples at rate sr (N = 1024, hop 256, F = ceil(L / 256) + 1 frames):
  X = stft(x) (513 x F), A = |X|
  t = time_constant_s sr / 256,  b = (sqrt(1 + 4 t^2) - 1) / (2 t^2)
  S = scipy.signal.filtfilt([b], [1, b - 1], A, axis=-1, padtype=None), i.e. per row
      forward   s[f] = b A[f] + (1 - b) s[f - 1],  s[-1] := A[0]
      backward  S[f] = b s[f] + (1 - b) S[f + 1],  S[F]  := s[F - 1]
  r = (A - S) / S, r := 0 where S == 0;  m0 = 1 / (1 + exp(-(r - n_mult) slope))
  m1 = smooth(m0) with outer(tri(n_f), tri(n_t)) / sum, zeros outside the 513 x F mask;  m = m1 p + (1 - p)   (p AFTER the smoothing)
  out = istft(X m, L)

Error bounds (all derived, none fitted).  u = 2^-24, G = 32 as in the stationary oracle: | A kernel - A | <= e_f = G u S_f per bin of frame f,
S_f = sum_n |w[n] frame_f[n]| / W.
  level:  both passes are weighted averages with non-negative weights that sum to 1 (the initial conditions included), so an error of the input passes
          through the SAME filter: |ds| <= forward(e).  The kernel holds the recurrences in f64 (2 roundings of 2^-53 per step, under 1e-12 S over any
          F) and keeps s between the passes as f32: one more u (s + ds).  |dS| <= backward(forward(e) + u (s + forward(e))) + 1e-12 S =: dS.
  m0:     r is increasing in A and decreasing in S, the sigmoid is increasing: the kernel's m0 lies in
          [sig(max(A - e, 0) / (S + dS) - 1), sig((A + e) / (S - dS) - 1)]   (the upper end is 1 where S - dS <= 0),
          dm0 = the larger distance of the two ends from m0, + u for the one rounding to f32 + 1e-12 for the f64 exp, capped at 1.  No Lipschitz constant.
  mask:   the smoothing is an average (weights >= 0, sum <= 1): |dm1| <= smooth(dm0).  The kernel sums in f32 in a fixed order: at most 17 time taps and
          65 frequency taps of non-negative terms, a product and a sum each (2 x 82 roundings), the division by the weights' sum, the rounded p and
          1 - p, their fma: SUMS = 168, relative to the result since every term is >= 0:  dm = p smooth(dm0) + SUMS u m.
  output: the stationary oracle's per-frame and overlap-add bounds, with the mask's error as one more per-frame term: dy_f = W irfft(X dm), and by
          Parseval for the real transform |dy_f|_2 <= W sqrt(2 / N) |X_f dm_f|_2, which bounds every sample of dy_f.
On the chirp signals of the tests (sr 22 050 and 16 000 at 2 s, 22 050 at 0.05 s) S >= 9e-6 everywhere, dm0 peaks at 1.9e-2 and exceeds 1e-4 in at
most 8.3 % of the entries: loose, not vacuous -- test_the_bounds_discriminate shows which restatement errors it still catches.
"""
import numpy as np

from tests.spectral_gate_oracle import (BINS, G, H, N, U, W, frame_sums, frames, n_frames, overlap_add, smooth, smoothing, stft,  # noqa: F401
                                         synthesis_frames, tri, w)

SUMS = 168


def coefficient(sr, time_constant_s=2.0):
    """b of the one-pole smoother whose forward-backward cascade has the time constant time_constant_s, in frames of 256 samples"""
    t = float(time_constant_s) * float(sr) / H
    return (np.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t)


def forward(A, b):
    """s[f] = b A[f] + (1 - b) s[f - 1] along the last axis, s[-1] := A[0]"""
    A = np.asarray(A, dtype=np.float64)
    s = np.empty_like(A)
    prev = A[..., 0]
    for f in range(A.shape[-1]):
        prev = b * A[..., f] + (1.0 - b) * prev
        s[..., f] = prev
    return s


def backward(s, b):
    """S[f] = b s[f] + (1 - b) S[f + 1] along the last axis, S[F] := s[F - 1]"""
    s = np.asarray(s, dtype=np.float64)
    S = np.empty_like(s)
    nxt = s[..., -1]
    for f in range(s.shape[-1] - 1, -1, -1):
        nxt = b * s[..., f] + (1.0 - b) * nxt
        S[..., f] = nxt
    return S


def level(A, b):
    """filtfilt([b], [1, b - 1], A, axis=-1, padtype=None)"""
    return backward(forward(A, b), b)


def sigmoid_mask(A, S, n_mult=2.0, slope=10.0):
    """m0 = sigmoid(((A - S) / S - n_mult) slope), r := 0 where S == 0 (np.inf in A or a non-positive S stand for the open ends of an interval)"""
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        r = np.where(S > 0, (A - S) / np.where(S > 0, S, 1.0), np.where(A > 0, np.inf, 0.0))
        return 1.0 / (1.0 + np.exp(-(r - n_mult) * slope))


def mask0_bound(x, b, n_mult=2.0, slope=10.0):
    """(X, m0, dm0) of signal x: the unsmoothed mask and its derived bound per entry"""
    x = np.asarray(x, dtype=np.float64)
    X = stft(x)
    A = np.abs(X)
    e = np.broadcast_to(G * U * frame_sums(x)[None, :], A.shape)
    s = forward(A, b)
    S = backward(s, b)
    ds = forward(e, b)
    dS = backward(ds + U * (s + ds), b) + 1e-12 * S
    m0 = sigmoid_mask(A, S, n_mult, slope)
    lo = sigmoid_mask(np.maximum(A - e, 0.0), S + dS, n_mult, slope)
    hi = np.where(S - dS > 0, sigmoid_mask(A + e, np.where(S - dS > 0, S - dS, 1.0), n_mult, slope), np.where((A + e > 0) | (S > 0), 1.0, m0))
    dm0 = np.minimum(np.maximum(hi - m0, m0 - lo) + U + 1e-12, 1.0)
    return X, m0, dm0


def final_mask(m0, n_f=0, n_t=0, p=1.0, p_first=False):
    """m = smooth(m0) p + (1 - p); p_first: the stationary gate's order, smooth(m0 p + (1 - p)) -- a distortion here"""
    if p_first:
        return smooth(m0 * p + (1.0 - p), n_f, n_t)
    return smooth(m0, n_f, n_t) * p + (1.0 - p)


def reduce_noise(x, b, n_mult=2.0, slope=10.0, n_f=0, n_t=0, p=1.0, mask0=None, details=False):
    """The non-stationary gate of signal x.  mask0 (513, F) replaces the oracle's own m0 (then the bound covers the smoothing and the synthesis only).
    details: also returns a dict with m0, dm0, the final mask, its bound and the output bound per sample."""
    x = np.asarray(x, dtype=np.float64)
    X, m0, dm0 = mask0_bound(x, b, n_mult, slope)
    if mask0 is not None:
        m0, dm0 = np.asarray(mask0, dtype=np.float64), np.zeros_like(dm0)
    m = final_mask(m0, n_f, n_t, p)
    yf = synthesis_frames(X * m)
    out = overlap_add(yf, len(x))
    if not details:
        return out
    dm = p * smooth(dm0, n_f, n_t) + SUMS * U * m
    fr = frames(x) * w
    e = U * (G * np.abs(m).max(0) * np.sqrt((fr ** 2).sum(1)) + (G + 2) * np.sqrt((yf ** 2).sum(1)))          # per frame, as in the stationary oracle
    e = e + W * np.sqrt(2.0 / N) * np.sqrt(((np.abs(X) * dm) ** 2).sum(0))                                       # the mask's error through the inverse
    F = yf.shape[0]
    num, den = np.zeros((F - 1) * H + N), np.zeros((F - 1) * H + N)
    for f in range(F):
        num[f * H:f * H + N] += w * e[f] + 8 * U * np.abs(w * yf[f])
        den[f * H:f * H + N] += w * w
    bound = (num / np.where(den > 1e-10, den, 1.0))[N // 2:N // 2 + len(x)]
    return out, {'X': X, 'm0': m0, 'dm0': dm0, 'mask': m, 'dmask': dm, 'bound': bound}
