"""Oracle of the CTC prefix beam search (the contract include/silent_speech_hip.h states for ss_ctc_beam_search), in plain Python: a dict from
prefix (the label string as `bytes`, V <= 128: hashed once, not per lookup like a tuple) to [lb, lnb, lm score], float64 by default;
`dtype=np.float32` runs the same steps in single precision (that run against the float64 one is where the score bars of
tests/test_ctc_beam.py come from).  It shares no code with csrc/ctc_decode.hip.

`brute_force` ranks EVERY label string by its exact log-likelihood through oracle/ctc_ref.ctc_utterance: with a beam at least as wide as the
number of prefixes nothing is pruned and the search must reproduce it."""
import itertools
import math

import numpy as np

from oracle import ctc_ref


def _lae64(a, b):
    if a < b:
        a, b = b, a
    if b == -math.inf:
        return a
    return a + math.log1p(math.exp(b - a))


def log_softmax(logits, dtype=np.float64):
    x = np.asarray(logits).astype(dtype)
    m = x.max(1, keepdims=True)
    return (x - (m + np.log(np.exp(x - m).sum(1, keepdims=True, dtype=dtype)))).astype(dtype)


def beam_search(logits, blank, beam_width, n_best=1, lm=None, alpha=0.0, beta=0.0, dtype=np.float64, trace=None):
    """logits (T, V) of ONE utterance -> list of at most n_best (labels tuple, score, ctc score), best first.  lm: (C+1, C+1, C) natural-log
    table over the labels numbered with the blank skipped, context index C = before the start.  trace: a list that receives the set of
    prefixes (tuples) in the beam after every frame."""
    logits = np.asarray(logits)
    T, V = logits.shape
    C = V - 1
    f64 = np.dtype(dtype) == np.float64
    if f64:
        lae, cast, NEG = _lae64, float, -math.inf
    else:
        lae, cast, NEG = np.logaddexp, dtype, dtype(-np.inf)
    logp = log_softmax(logits, dtype)
    lab = [c - (1 if c > blank else 0) for c in range(V)]
    if lm is not None:
        lm = np.asarray(lm).astype(dtype)
        a, b = cast(alpha), cast(beta)
    one = [bytes([c]) for c in range(V)]
    beam = {b'': [cast(0.0), NEG, cast(0.0)]}
    with np.errstate(all='ignore'):
        for t in range(T):
            row = [cast(v) for v in logp[t]]
            new = {}
            for p, (lb, lnb, lms) in beam.items():
                tot = lae(lb, lnb)
                last = p[-1] if p else -1
                stay_b, stay_nb = tot + row[blank], (lnb + row[last] if p else NEG)
                e = new.get(p)
                if e is None:
                    new[p] = [stay_b, stay_nb, lms]
                else:
                    e[0], e[1] = lae(e[0], stay_b), lae(e[1], stay_nb)
                for c in range(V):
                    if c == blank:
                        continue
                    q = p + one[c]
                    v = (lb if c == last else tot) + row[c]
                    e = new.get(q)
                    if e is None:
                        s = lms
                        if lm is not None:
                            i2 = lab[p[-2]] if len(p) >= 2 else C
                            i1 = lab[last] if p else C
                            s = lms + (a * cast(lm[i2, i1, lab[c]]) + b)
                        new[q] = [NEG, v, s]
                    else:
                        e[1] = lae(e[1], v)
            cands = [(lae(e[0], e[1]) + e[2], q) for q, e in new.items()]
            cands = [x for x in cands if x[0] > NEG]                     # a candidate of score -inf does not exist
            cands.sort(key=lambda x: -x[0])                              # stable: ties keep the order of appearance
            beam = {q: new[q] for _, q in cands[:beam_width]}
            if trace is not None:
                trace.append({tuple(q) for q in beam})
        final = [(q, lae(e[0], e[1]) + e[2], lae(e[0], e[1])) for q, e in beam.items()]
    final = [x for x in final if x[1] > NEG]
    final.sort(key=lambda x: -x[1])
    return [(tuple(q), float(s), float(cs)) for q, s, cs in final[:n_best]]


def brute_force(logits, blank):
    """Every label string of at most T labels with its exact float64 log-likelihood, best first: [(labels tuple, log-likelihood)], the
    impossible strings (log-likelihood -inf) left out."""
    logits = np.asarray(logits, dtype=np.float64)
    T, V = logits.shape
    if T == 0:
        return [((), 0.0)]
    logp = log_softmax(logits)
    labels = [c for c in range(V) if c != blank]
    out = []
    with np.errstate(all='ignore'):
        for n in range(T + 1):
            for q in itertools.product(labels, repeat=n):
                ll = -ctc_ref.ctc_utterance(logp, np.asarray(q, dtype=np.int64), blank)[0]
                if ll > -np.inf:
                    out.append((q, float(ll)))
    out.sort(key=lambda x: -x[1])
    return out
