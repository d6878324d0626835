"""TEST INFRASTRUCTURE ONLY -- float64 restatement of the definitions include/silent_speech_hip.h gives for ss_ctc_nbest_logp /
ss_ctc_nbest_backward / ss_nbest_expected_risk and of recognition_model.mwer_loss, composed from the read-only oracle.ctc_ref.ctc_loss_packed
(called per hypothesis on its utterance's frames alone, n = 1: logp = -nll, d logp / d logits = -max(S, 1) d).  Shares no code with the package."""
import numpy as np

from oracle.ctc_ref import ctc_loss_packed


def softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def hyp_logp(frames, h, blank):
    """frames (T, V) f64 logits of ONE utterance, h a label string -> (logp, d logp / d logits (T, V), occ (T, V)); an infeasible string gives
    (-inf, 0, 0)."""
    frames = np.asarray(frames, dtype=np.float64)
    T, V = frames.shape
    h = [int(c) for c in h]
    zero = np.zeros((T, V))
    if T == 0:
        return (0.0 if not h else -np.inf), zero, zero
    with np.errstate(all='ignore'):
        _, d, nll = ctc_loss_packed(frames[None], [T], [h], blank, vec=True)
    if not np.isfinite(nll[0]):
        return -np.inf, zero, zero
    dlogp = -max(len(h), 1) * d[0]
    return -float(nll[0]), dlogp, dlogp + softmax(frames)


def nbest_logp(flat, first, frames, hyps, blank):
    """flat (M, V) f64; per utterance first frame, frame count and list of strings -> per utterance a list of (logp, dlogp, occ)."""
    return [[hyp_logp(flat[f0:f0 + T], h, blank) for h in lst] for f0, T, lst in zip(first, frames, hyps)]


def nbest_backward(flat, first, frames, scored, g):
    """d sum_h g_h logp_h / d flat and the per-element bar of tests/test_ctc_nbest.py: sum_h |g_h| 2e-3 (|dlogp_h| + occ_h) + 1e-6 sum_h |g_h|.
    scored: what nbest_logp returned; g: flat cotangents in utterance-then-list order."""
    want, bar = np.zeros_like(flat), np.zeros_like(flat)
    at = 0
    for f0, T, lst in zip(first, frames, scored):
        for logp, dlogp, occ in lst:
            if np.isfinite(logp):
                want[f0:f0 + T] += g[at] * dlogp
                bar[f0:f0 + T] += abs(g[at]) * (2e-3 * (np.abs(dlogp) + occ) + 1e-6)
            at += 1
    return want, bar


def expected_risk(logp_lists, cost_lists, scale):
    """Lists of f64 log-likelihoods and costs -> (loss, risk per list (NaN without a finite entry), post and dlogp per list)."""
    risks, posts, dl = [], [], []
    for lp, c in zip(logp_lists, cost_lists):
        lp, c = np.asarray(lp, dtype=np.float64), np.asarray(c, dtype=np.float64)
        fin = np.isfinite(lp)
        post, d = np.zeros(len(lp)), np.zeros(len(lp))
        if not fin.any():
            risks.append(np.nan)
        else:
            z = scale * lp[fin]
            e = np.exp(z - z.max())
            p = e / e.sum()
            cc = c[fin] - c[fin].mean()
            r = float((p * cc).sum())
            post[fin], d[fin] = p, scale * p * (cc - r)
            risks.append(r)
        posts.append(post)
        dl.append(d)
    used = [r for r in risks if r == r]
    n = len(used)
    return (float(np.sum(used)) / n if n else 0.0), np.asarray(risks), posts, [d / max(n, 1) for d in dl]


def words(ints, space, unit='word'):
    ints = [int(c) for c in ints]
    if unit == 'char':
        return ints
    out, run = [], []
    for c in ints + [space]:
        if c == space:
            if run:
                out.append(tuple(run))
            run = []
        else:
            run.append(c)
    return out


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (x != y), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[-1]


def mwer(flat, first, frames, refs, hyps, blank, space, scale=1.0, unit='word', ctc_weight=0.0):
    """Value and gradient (M, V) of mwer_loss on given lists, with the pieces the bars are built from:
    returns dict(loss, grad, bar (the kernel bar of the gradient at the oracle's cotangents), logp, post, cost, dlogp (flat), risk, slack)."""
    scored = nbest_logp(flat, first, frames, hyps, blank)
    costs = [[float(levenshtein(words(ref, space, unit), words(h, space, unit))) for h in lst] for ref, lst in zip(refs, hyps)]
    loss, risk, posts, dl = expected_risk([[s[0] for s in lst] for lst in scored], costs, scale)
    g = np.concatenate([np.zeros(0)] + dl)
    grad, bar = nbest_backward(flat, first, frames, scored, g)
    out = dict(loss=loss, risk=risk, logp=np.asarray([s[0] for lst in scored for s in lst]), post=np.concatenate([np.zeros(0)] + posts),
               cost=np.asarray([c for lst in costs for c in lst]), dlogp=g, scored=scored)
    if ctc_weight:
        M, V = flat.shape
        used = int(sum(frames))
        assert list(first) == list(np.concatenate([[0], np.cumsum(frames)])[:-1])
        closs, d, _ = ctc_loss_packed(flat[:used][None], list(frames), [list(r) for r in refs], blank, vec=True)
        loss += ctc_weight * closs
        grad[:used] += ctc_weight * d[0]
        sm = softmax(flat[:used])
        off = 0
        for T, r in zip(frames, refs):
            sc = 1.0 / (max(len(r), 1) * len(frames))
            bar[off:off + T] += ctc_weight * (2e-3 * (np.abs(d[0][off:off + T]) + sm[off:off + T] * sc - d[0][off:off + T]) + 1e-6)
            off += T
    out.update(loss=loss, grad=grad, bar=bar)
    return out
