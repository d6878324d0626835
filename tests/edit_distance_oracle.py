"""Plain Python / numpy restatement of the definitions include/silent_speech_hip.h gives for ss_edit_distance and ss_nbest_risk.  Shares no
code with csrc/edit_distance.hip or with recognition_model._edit_distance.

    D[0][j] = j, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (a[i-1] != b[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)
    the predecessor of a cell is the first of {diagonal, up, left} that attains the minimum; row 0: left, column 0: up
    ops: the path from (0, 0) to (n_a, n_b), 0 hit, 1 substitution, 2 deletion (up), 3 insertion (left); the counts are those of the path
"""
import functools

import numpy as np

HIT, SUB, DEL, INS = 0, 1, 2, 3


def matrix(a, b):
    """The whole (n_a + 1, n_b + 1) table, a row at a time: D[i][j] = min_k<=j (t[k] + j - k), t[0] = i, t[k] = min(diagonal, up) of column k."""
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    D = np.zeros((a.size + 1, b.size + 1), dtype=np.int64)
    cols = np.arange(b.size + 1, dtype=np.int64)
    D[0] = cols
    t = np.zeros(b.size + 1, dtype=np.int64)
    for i in range(1, a.size + 1):
        t[0] = i
        t[1:] = np.minimum(D[i - 1, :-1] + (b != a[i - 1]), D[i - 1, 1:] + 1)
        D[i] = np.minimum.accumulate(t - cols) + cols
    return D


def align(a, b):
    """(distance, (hits, substitutions, deletions, insertions), ops int8 from the beginning)"""
    a, b = [int(x) for x in a], [int(x) for x in b]
    D = matrix(a, b)
    i, j, back = len(a), len(b), []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i, j] == D[i - 1, j - 1] + (a[i - 1] != b[j - 1]):
            back.append(HIT if a[i - 1] == b[j - 1] else SUB)
            i, j = i - 1, j - 1
        elif i > 0 and (j == 0 or D[i, j] == D[i - 1, j] + 1):
            back.append(DEL)
            i -= 1
        else:
            assert j > 0 and D[i, j] == D[i, j - 1] + 1
            back.append(INS)
            j -= 1
    ops = np.asarray(back[::-1], dtype=np.int8)
    counts = tuple(int((ops == k).sum()) for k in (HIT, SUB, DEL, INS))
    return int(D[len(a), len(b)]), counts, ops


def distance(a, b):
    return int(matrix(a, b)[-1, -1])


def distance_recursive(a, b):
    """An independent statement of the distance: memoised recursion over prefixes."""
    a, b = tuple(a), tuple(b)

    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        return min(d(i - 1, j - 1) + (a[i - 1] != b[j - 1]), d(i - 1, j) + 1, d(i, j - 1) + 1)
    return d(len(a), len(b))


def replay(a, ops):
    """The hypothesis the steps turn the reference into: a hit copies, a substitution and an insertion ask for 'some token' (None)."""
    out, i = [], 0
    for op in ops:
        if op == HIT:
            out.append(a[i]); i += 1
        elif op == SUB:
            out.append(None); i += 1
        elif op == DEL:
            i += 1
        else:
            assert op == INS
            out.append(None)
    assert i == len(a)
    return out


def nbest(hyps, weights):
    """(dmat (K, K) int64, risk (K) f64 = sum_k f32 weight[k] * dmat[i][k] in f64, ascending k, pick = the smallest index of least risk)"""
    K = len(hyps)
    d = np.zeros((K, K), dtype=np.int64)
    for i in range(K):
        for k in range(i + 1, K):
            d[i, k] = d[k, i] = distance(hyps[i], hyps[k])
    w = np.asarray(weights, dtype=np.float32)
    risk = np.zeros(K, dtype=np.float64)
    for i in range(K):
        acc = np.float64(0.0)
        for k in range(K):
            acc = acc + np.float64(w[k]) * np.float64(d[i, k])
        risk[i] = acc
    pick = 0
    for i in range(1, K):
        if risk[i] < risk[pick]:
            pick = i
    return d, risk, pick
