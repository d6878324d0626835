"""Inputs with EXACTLY representable costs for the fused DTW loss path (csrc/loss.hip silent_cost_skewed_kernel -> csrc/dtw.hip dtw_kernel<false> ->
silent_loss_kernel), and the numpy / C-oracle reference of what that path must give.  Shares no code with the kernels.

The construction (the alignment can then be demanded bit for bit, lambda != 0 included):
  * mel predictions and targets are small integers stored as f32, so ss = sum (p - y)^2 is an exact integer (< 2^24) in ANY summation order and the
    only rounding of the mel term is the one sqrtf, which must equal np.sqrt(np.float32(ss));
  * frame q's phoneme logits hold one class at an integer g_q in {0, 1, 2, 3} and every other class at g_q - 64 k, k in {1, 2, 3}: expf(<= -64) is far
    below 2^-25, the f32 sum of the exponentials is exactly 1.0f in any order, lse[q] = g_q exactly and lse[q] - logit[q][ph] is 0 or 64 k.  g_q varies
    from frame to frame (log-softmax is shift-invariant: only a varying g_q exposes a mis-indexed lse);
  * lambda in {0, 0.25, 0.5}: lambda * (0 | 64 k) is exact, and so is its sum with the root only up to ONE f32 rounding, the same on both sides.
The cost matrix is built here from ss in int64 (|p|^2 + |y|^2 - 2 p y^T, never a (T1, T2, n_mel) broadcast) and goes through the C oracle
oracle/dtw_ref.c (`align_from_distances_c(costs.T)`: f32, one add per cell, first minimum of up / left / diagonal).  Loss, gradient, accuracy count and
confusion matrix are recomputed in float64 from that alignment.  The helper asserts its own preconditions (ss against a float64 sum, lse == g_q in f32
numpy arithmetic, ss < 2^24)."""
import numpy as np

from oracle import dtw_ref

N_PH = 6                 # phoneme classes (not a multiple of 4: n_mel + N_PH is rounded up for the row stride)
PAD_COLS = 8             # spare head columns behind the rounded-up width (poisoned)
SPARE_ROWS = 5           # packed rows behind the last utterance (poisoned)
EPS = 1e-6               # F.pairwise_distance eps of the voiced term


class Utt(object):
    """One utterance: T1 predicted frames, T2 target frames (voiced: T2 == T1).  kind selects the mel features:
       'ties'   integers 0..3 in ONE non-zero column (every ss a perfect square 0, 1, 4, 9: many exact cost ties, no dependence on sqrtf's rounding);
       'ints'   general integer vectors in [-2, 2] (ss any integer: sqrtf must be correctly rounded);
       'const'  constant features (an all-ties matrix);
       'ramp'   a_q = q, b_k = k in one column (unique zero-cost diagonal);
       'plateau_pred' a_q = min(q, T2 - 1), b_k = k  (the path runs left along the last row);
       'plateau_tgt'  a_q = q, b_k = min(k, T1 - 1)  (hundreds of k align to the last q)."""

    def __init__(self, T1, T2=None, silent=True, kind='ints'):
        self.T1, self.T2, self.silent, self.kind = int(T1), int(T1 if T2 is None else T2), bool(silent), kind
        assert self.silent or self.T2 == self.T1


def head_ld(n_mel):
    return (n_mel + N_PH + 3) // 4 * 4 + PAD_COLS


def _features(rng, u, n_mel):
    col = int(rng.integers(0, n_mel))
    p = np.zeros((u.T1, n_mel), dtype=np.int64)
    y = np.zeros((u.T2, n_mel), dtype=np.int64)
    q, k = np.arange(u.T1), np.arange(u.T2)
    if u.kind == 'ties':
        p[:, col] = rng.integers(0, 4, u.T1)
        y[:, col] = rng.integers(0, 4, u.T2)
    elif u.kind == 'ints':
        p[:] = rng.integers(-2, 3, (u.T1, n_mel))
        y[:] = rng.integers(-2, 3, (u.T2, n_mel))
    elif u.kind == 'const':
        p[:, col] = 2
        y[:, col] = 1
    elif u.kind == 'ramp':
        p[:, col], y[:, col] = q, k
    elif u.kind == 'plateau_pred':
        p[:, col], y[:, col] = np.minimum(q, u.T2 - 1), k
    elif u.kind == 'plateau_tgt':
        p[:, col], y[:, col] = q, np.minimum(k, u.T1 - 1)
    else:
        raise ValueError(u.kind)
    return p, y


def _logits(rng, T):
    """(T, N_PH) integer logits, g (T,), hot class (T,)."""
    g = rng.integers(0, 4, T)
    if T > 1 and (g == g[0]).all():
        g[-1] = (g[0] + 1) % 4
    hot = rng.integers(0, N_PH, T)
    a = g[:, None] - 64 * rng.integers(1, 4, (T, N_PH))
    a[np.arange(T), hot] = g
    return a.astype(np.int64), g, hot


def lse_f32(a):
    """Per-row log-sum-exp in f32 numpy arithmetic (max, exp of the differences, f32 sum, log), as the kernel forms it."""
    a = np.asarray(a, dtype=np.float32)
    m = a.max(axis=1)
    s = np.exp(a - m[:, None], dtype=np.float32).sum(axis=1, dtype=np.float32)
    return (m + np.log(s, dtype=np.float32)).astype(np.float32)


def sq_dists(p, y):
    """(T1, T2) int64 squared distances of integer feature rows, by |p|^2 + |y|^2 - 2 p y^T; checked against a direct float64 sum on sampled rows."""
    ss = (p * p).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2 * (p @ y.T)
    assert ss.min() >= 0 and ss.max() < 2 ** 24
    rows = np.unique(np.linspace(0, p.shape[0] - 1, 7).astype(np.int64))
    direct = ((p[rows, None, :].astype(np.float64) - y[None, :, :].astype(np.float64)) ** 2).sum(-1)
    assert np.array_equal(direct, ss[rows].astype(np.float64))
    return ss


def cost_matrix(ss, logits, g, phones, lam):
    """(T1, T2) f32: costs[q][k] = sqrtf(ss) + lam * (lse[q] - logit[q][phone_k]), every step rounded as f32 arithmetic rounds it."""
    root = np.sqrt(ss.astype(np.float32))
    assert root.dtype == np.float32
    ph = (g[:, None] - logits[:, phones]).astype(np.float32)            # 0 or 64 k, exact
    return (root + np.float32(lam) * ph).astype(np.float32)


class Batch(object):
    pass


def build(utts, n_mel, lam, seed, need_phoneme_effect=None, need_lse_effect=False):
    """The inputs of one _dtw_loss_plan call and everything the checks compare with.  For lam != 0 the seed is advanced until the phoneme term changes
    the oracle alignment of at least one silent utterance (need_phoneme_effect, default: lam != 0); need_lse_effect: and until taking lse from the
    frame before (lse[q - 1] for lse[q]) changes it too -- for the tiny cases, where such an error could otherwise hide behind the phoneme term's size."""
    need = (lam != 0) if need_phoneme_effect is None else need_phoneme_effect
    for attempt in range(64):
        b = _build(utts, n_mel, lam, seed + 1000 * attempt, need_lse_effect)
        if (not need or b.phoneme_term_matters) and (not need_lse_effect or b.lse_index_matters):
            return b
    raise AssertionError('no seed found at which the phoneme term (or the lse index) changes the alignment: the case proves nothing about it')


def _build(utts, n_mel, lam, seed, probe_lse=False):
    rng = np.random.default_rng(seed)
    b = Batch()
    b.utts, b.n_mel, b.n_ph, b.lam = utts, n_mel, N_PH, lam
    b.ld = head_ld(n_mel)
    b.used = sum(u.T1 for u in utts)
    b.rows = b.used + SPARE_ROWS
    b.total = sum(u.T2 for u in utts)
    head = np.full((b.rows, b.ld), np.nan, dtype=np.float32)
    dhead = np.zeros((b.rows, b.ld), dtype=np.float64)
    b.audio, b.phones, b.align = [], [], []
    b.g = np.zeros(b.used, dtype=np.float32)
    b.hot = np.zeros(b.used, dtype=np.int64)
    b.confusion = np.zeros((N_PH, N_PH), dtype=np.int64)
    b.correct = 0
    b.phoneme_term_matters = b.lse_index_matters = False
    loss = 0.0
    p0 = 0
    for u in utts:
        p, y = _features(rng, u, n_mel)
        a, g, hot = _logits(rng, u.T1)
        phones = rng.integers(0, N_PH, u.T2)
        assert np.array_equal(lse_f32(a), g.astype(np.float32))
        head[p0:p0 + u.T1, :n_mel] = p
        head[p0:p0 + u.T1, n_mel:n_mel + N_PH] = a
        b.g[p0:p0 + u.T1], b.hot[p0:p0 + u.T1] = g, hot
        b.audio.append(y.astype(np.float32))
        b.phones.append(phones.astype(np.int64))
        sm = np.exp(a.astype(np.float64) - g[:, None])                   # softmax: lse == g
        sm /= sm.sum(1, keepdims=True)
        if u.silent:
            ss = sq_dists(p, y)
            costs = cost_matrix(ss, a, g, phones, lam)
            al = np.asarray(dtw_ref.align_from_distances_c(costs.T), dtype=np.int64)
            assert al.shape == (u.T2,)
            if lam != 0 and not b.phoneme_term_matters:
                plain = dtw_ref.align_from_distances_c(cost_matrix(ss, a, g, phones, 0.0).T)
                b.phoneme_term_matters = plain != al.tolist()
            if lam != 0 and probe_lse and not b.lse_index_matters:
                shifted = dtw_ref.align_from_distances_c(cost_matrix(ss, a, np.roll(g, 1), phones, lam).T)
                b.lse_index_matters = shifted != al.tolist()
            b.align.append(al)
            k = np.arange(u.T2)
            dist = np.sqrt(ss[al, k].astype(np.float64))
            loss += float((dist + lam * (g[al] - a[al, phones])).sum())
            gs = np.where(dist > 0, 1.0 / np.where(dist > 0, dist, 1.0), 0.0)
            np.add.at(dhead[p0:p0 + u.T1, :n_mel], al, (p[al] - y).astype(np.float64) * gs[:, None])
            onehot = np.zeros((u.T2, N_PH))
            onehot[k, phones] = 1.0
            np.add.at(dhead[p0:p0 + u.T1, n_mel:n_mel + N_PH], al, lam * (sm[al] - onehot))
            pred_ph = hot[al]
        else:
            b.align.append(None)
            d = y.astype(np.float64) - p.astype(np.float64) + EPS
            dist = np.sqrt((d * d).sum(1))
            loss += float((dist + lam * (g - a[np.arange(u.T1), phones])).sum())
            dhead[p0:p0 + u.T1, :n_mel] = -d / dist[:, None]
            onehot = np.zeros((u.T1, N_PH))
            onehot[np.arange(u.T1), phones] = 1.0
            dhead[p0:p0 + u.T1, n_mel:n_mel + N_PH] = lam * (sm - onehot)
            pred_ph = hot
        np.add.at(b.confusion, (pred_ph, phones), 1)
        b.correct += int((pred_ph == phones).sum())
        p0 += u.T1
    b.head = head
    b.loss = loss / b.total
    b.dhead = dhead / b.total
    return b
