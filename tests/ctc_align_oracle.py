"""Oracle of the forced alignment (the contract include/silent_speech_hip.h states for ss_ctc_align), in plain Python / numpy, written from that
definition: the Viterbi recursion over the extended CTC states (or over the tokens, linear topology) with back-pointers, ties to the smallest jump
and to the token state at the end.  dtype = np.float64 is the reference; dtype = np.float32 restates the kernel's arithmetic (f32 log-sum-exp,
logp = logit - lse, ONE addition per step) and measures what single precision costs.  rescore() validates a frame path and sums its log-probabilities
in float64; brute_force() enumerates every valid path of a tiny case.  Shares no code with csrc/ctc_align.hip."""
import numpy as np


def log_probs(x, dtype=np.float64):
    """(T, V) logits -> logit - lse in `dtype` (the log-sum-exp itself computed in that precision too)."""
    x = np.asarray(x).astype(dtype)
    if x.shape[0] == 0:
        return x
    m = x.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True, dtype=dtype))).astype(dtype)
    return (x - lse).astype(dtype)


def _topology(y, blank):
    """labels of the states and whether the jump s-2 -> s is allowed; blank < 0: linear."""
    S = len(y)
    if blank < 0:
        return np.asarray(y, dtype=np.int64), np.zeros(S, dtype=bool)
    lab = np.full(2 * S + 1, blank, dtype=np.int64)
    lab[1::2] = y
    skip = np.zeros(2 * S + 1, dtype=bool)
    for k in range(1, S):
        skip[2 * k + 1] = y[k] != y[k - 1]
    return lab, skip


def _bad(y, V, blank):
    return any(c < 0 or c >= V or c == blank for c in y)


def _frames_of(states, blank):
    return [int(s) if blank < 0 else ((int(s) - 1) // 2 if s % 2 else -1) for s in states]


def align(x, y, blank, dtype=np.float64):
    """x (T, V) logits, y label list, blank (-1: linear topology).  Returns (score, frames): frames = list of token indices (-1 blank), or None
    when score is -inf."""
    x = np.asarray(x)
    T, V = x.shape
    y = [int(c) for c in y]
    S = len(y)
    if _bad(y, V, blank):
        return -np.inf, None
    if T == 0:
        return (0.0, []) if S == 0 else (-np.inf, None)
    if blank < 0 and S == 0:
        return -np.inf, None
    lp = log_probs(x, dtype)
    lab, skip = _topology(y, blank)
    n = len(lab)
    ninf = dtype(-np.inf)
    d = np.full(n, ninf, dtype=dtype)
    d[0] = lp[0, lab[0]]
    if blank >= 0 and n > 1:
        d[1] = lp[0, lab[1]]
    back = np.zeros((T, n), dtype=np.int8)
    for t in range(1, T):
        p1 = np.concatenate([[ninf], d[:-1]]).astype(dtype)
        p2 = np.concatenate([[ninf, ninf], d[:-2]]).astype(dtype)[:n]
        best, bp = d.copy(), np.zeros(n, dtype=np.int8)
        m = p1 > best
        best, bp = np.where(m, p1, best), np.where(m, 1, bp)
        m = skip & (p2 > best)
        best, bp = np.where(m, p2, best), np.where(m, 2, bp)
        step = lp[t, lab]
        with np.errstate(invalid='ignore'):
            d = np.where(best > ninf, (best + step).astype(dtype), ninf).astype(dtype)
        back[t] = bp
    if blank >= 0:
        s = 2 * S - 1 if S > 0 and d[2 * S - 1] >= d[2 * S] else 2 * S
    else:
        s = S - 1
    score = float(d[s])
    if not score > -np.inf:
        return -np.inf, None
    states = [s]
    for t in range(T - 1, 0, -1):
        s -= int(back[t, s])
        states.append(s)
    return score, _frames_of(states[::-1], blank)


def spans(x, y, blank, frames, dtype=np.float32):
    """token_first, token_frames, token_logp of a frame path: the logp summed over the token's frames in ascending order in `dtype`."""
    lp = log_probs(x, dtype)
    S = len(y)
    first, count, logp = [-1] * S, [0] * S, [dtype(0)] * S
    for t, k in enumerate(frames):
        if k >= 0:
            if first[k] < 0:
                first[k] = t
            count[k] += 1
            logp[k] = dtype(logp[k] + lp[t, y[k]])
    return first, count, [float(v) for v in logp]


def path_states(y, blank, frames):
    """The state sequence of a frame path if it is a valid alignment of y, else None."""
    S, T = len(y), len(frames)
    if T == 0:
        return [] if S == 0 else None
    states, k = [], -1                                                   # k = the last token seen
    for f in frames:
        f = int(f)
        if blank < 0:
            if f < 0 or f >= S:
                return None
            s = f
        elif f == -1:
            s = 2 * (k + 1)
        elif 0 <= f < S:
            s, k = 2 * f + 1, f
        else:
            return None
        states.append(s)
    _, skip = _topology(y, blank)
    if states[0] not in ((0,) if blank < 0 else (0, 1)):
        return None
    if states[-1] not in ((S - 1,) if blank < 0 else (2 * S - 1, 2 * S)):
        return None
    for a, b in zip(states, states[1:]):
        if b - a not in (0, 1) and not (b - a == 2 and blank >= 0 and skip[b]):
            return None
    return states


def rescore(x, y, blank, frames):
    """float64 log-probability of a frame path; None if it is no valid alignment of y."""
    states = path_states(y, blank, frames)
    if states is None:
        return None
    lp = log_probs(x, np.float64)
    lab, _ = _topology(y, blank)
    return float(sum(lp[t, lab[s]] for t, s in enumerate(states)))


def brute_force(x, y, blank):
    """Every valid state path of a tiny case: [(float64 score, frames)], best first."""
    x = np.asarray(x)
    T, V = x.shape
    y = [int(c) for c in y]
    S = len(y)
    if _bad(y, V, blank) or T == 0 or (blank < 0 and S == 0):
        return [(0.0, [])] if T == 0 and S == 0 and not _bad(y, V, blank) else []
    lp = log_probs(x, np.float64)
    lab, skip = _topology(y, blank)
    n = len(lab)
    ends = (S - 1,) if blank < 0 else (2 * S - 1, 2 * S)
    out = []

    def walk(path, total):
        if len(path) == T:
            if path[-1] in ends:
                out.append((total, _frames_of(path, blank)))
            return
        s = path[-1]
        for j in (0, 1, 2):
            q = s + j
            if q < n and (j < 2 or (blank >= 0 and skip[q])):
                walk(path + [q], total + lp[len(path), lab[q]])
    for s0 in ((0,) if blank < 0 else (0, 1)):
        if s0 < n:
            walk([s0], lp[0, lab[s0]])
    return sorted(out, key=lambda r: -r[0])
