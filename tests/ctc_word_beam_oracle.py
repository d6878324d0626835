"""Oracle of the lexicon-constrained CTC prefix beam search with a word n-gram (the contract include/silent_speech_hip.h states for
ss_ctc_word_beam_search), in plain Python: a dict from prefix (the label string as `bytes`) to [lb, lnb, lm score], float64 by default;
`dtype=np.float32` runs the same steps in single precision (that run against the float64 one is where the score bars of
tests/test_ctc_word_beam.py come from).  The lexicon node, the word context and the word term of a prefix are functions of the label string
and are carried beside the masses as (the unfinished word's labels, w2, w1).  It shares no code with csrc/ctc_word_decode.hip, nor with
recognition_model.WordNgramLM: the model comes in as plain containers (`Tables`) and the backoff rule is restated in `lnp`.

`brute_force` ranks EVERY label string the rules allow by its exact log-likelihood through oracle/ctc_ref.ctc_utterance plus the word terms:
with a beam at least as wide as the number of prefixes nothing is pruned and the search must reproduce it."""
import itertools
import math

import numpy as np

from oracle import ctc_ref
from tests.ctc_beam_oracle import _lae64, log_softmax


class Tables(object):
    """spellings: one tuple of CLASS numbers per word (word id = index); uni: (n + 1, 2) [ln P, backoff], row n = the start context;
    bi: {(w1, w): (ln P, backoff)}; tri: {(w2, w1, w): ln P}.  Values are used as they are stored (f32 numbers), cast to the run's dtype."""

    def __init__(self, spellings, uni, bi, tri):
        self.spellings, self.uni, self.bi, self.tri = [tuple(int(c) for c in s) for s in spellings], np.asarray(uni), dict(bi), dict(tri)
        self.start = len(self.spellings)
        self.word_of = {bytes(s): w for w, s in enumerate(self.spellings)}
        self.prefixes = {bytes(s[:k]) for s in self.spellings for k in range(len(s) + 1)} | {b''}

    @classmethod
    def of(cls, lm, blank):
        """From a recognition_model.WordNgramLM (its HOST tables only); label number -> class number puts the blank back."""
        to_class = [i + (1 if i >= blank else 0) for i in range(len(lm.chars))]
        return cls([[to_class[lm.chars.index(ch)] for ch in w] for w in lm.words], lm.unigrams, lm.bigrams, lm.trigrams)

    def lnp(self, w2, w1, w, cast=float):
        """ln P(w | w2, w1); w2 = -1: none."""
        if w2 >= 0 and (w2, w1, w) in self.tri:
            return cast(self.tri[(w2, w1, w)])
        p2 = cast(self.bi[(w1, w)][0]) if (w1, w) in self.bi else cast(self.uni[w1][1]) + cast(self.uni[w][0])
        if w2 < 0:
            return p2
        return (cast(self.bi[(w2, w1)][1]) if (w2, w1) in self.bi else cast(0.0)) + p2


def _split(q, space):
    """label string -> (finished words as bytes, the unfinished rest as bytes)"""
    parts = bytes(q).split(bytes([space]))
    return parts[:-1], parts[-1]


def allowed(q, tables, space):
    """Is q a string the rules can build: every finished word a word of the lexicon, the rest a prefix of one."""
    done, rest = _split(q, space)
    return all(w in tables.word_of for w in done) and rest in tables.prefixes


def lm_terms(q, tables, space, alpha, beta, cast=float):
    """(sum of the finished words' alpha lnP + beta accumulated one word at a time, the unfinished rest's term or None if it is no word,
    number of finished words, complete?)"""
    done, rest = _split(q, space)
    w2, w1, s = -1, tables.start, cast(0.0)
    for part in done:
        w = tables.word_of[part]
        s = s + (cast(alpha) * tables.lnp(w2, w1, w, cast) + cast(beta))
        w2, w1 = w1, w
    last = None
    if rest in tables.word_of:
        last = cast(alpha) * tables.lnp(w2, w1, tables.word_of[rest], cast) + cast(beta)
    return s, last, len(done), (rest == b'' or last is not None)


def beam_search(logits, blank, space, beam_width, tables, alpha, beta, n_best=1, dtype=np.float64, trace=None):
    """logits (T, V) of ONE utterance -> list of at most n_best (labels tuple, score, ctc score, complete), complete entries first, best first.
    trace: a list that receives the number of candidates of every frame (at most beam_width of them: nothing was pruned)."""
    logits = np.asarray(logits)
    T, V = logits.shape
    f64 = np.dtype(dtype) == np.float64
    if f64:
        lae, cast, NEG = _lae64, float, -math.inf
    else:
        lae, cast, NEG = np.logaddexp, dtype, dtype(-np.inf)
    logp = log_softmax(logits, dtype)
    a, b = cast(alpha), cast(beta)
    one = [bytes([c]) for c in range(V)]
    # state of a prefix: (rest = the unfinished word's labels, w2, w1): a function of the string, kept beside the masses
    beam = {b'': [cast(0.0), NEG, cast(0.0), (b'', -1, tables.start)]}
    with np.errstate(all='ignore'):
        for t in range(T):
            row = [cast(v) for v in logp[t]]
            new = {}
            for p, (lb, lnb, lms, state) in beam.items():
                tot = lae(lb, lnb)
                last = p[-1] if p else -1
                stay_b, stay_nb = tot + row[blank], (lnb + row[last] if p else NEG)
                e = new.get(p)
                if e is None:
                    new[p] = [stay_b, stay_nb, lms, state]
                else:
                    e[0], e[1] = lae(e[0], stay_b), lae(e[1], stay_nb)
                rest, w2, w1 = state
                for c in range(V):
                    if c == blank:
                        continue
                    if c == space:
                        if rest not in tables.word_of:
                            continue
                        w = tables.word_of[rest]
                        s, nstate = lms + (a * tables.lnp(w2, w1, w, cast) + b), (b'', w1, w)
                    else:
                        if rest + one[c] not in tables.prefixes:
                            continue
                        s, nstate = lms, (rest + one[c], w2, w1)
                    q = p + one[c]
                    v = (lb if c == last else tot) + row[c]
                    e = new.get(q)
                    if e is None:
                        new[q] = [NEG, v, s, nstate]
                    else:
                        e[1] = lae(e[1], v)
            cands = [(lae(e[0], e[1]) + e[2], q) for q, e in new.items()]
            cands = [x for x in cands if x[0] > NEG]                     # a candidate of score -inf does not exist
            cands.sort(key=lambda x: -x[0])                              # stable: ties keep the order of appearance
            beam = {q: new[q] for _, q in cands[:beam_width]}
            if trace is not None:
                trace.append(len(cands))
        final = []
        for q, (lb, lnb, lms, (rest, w2, w1)) in beam.items():
            ctc = lae(lb, lnb)
            word = rest != b'' and rest in tables.word_of
            s = lms + ((a * tables.lnp(w2, w1, tables.word_of[rest], cast) + b) if word else cast(0.0))
            final.append((q, ctc + s, ctc, bool(rest == b'' or word)))
    final = [x for x in final if x[1] > NEG]
    final.sort(key=lambda x: (not x[3], -x[1]))                          # stable: ties keep the beam order
    return [(tuple(q), float(s), float(cs), done) for q, s, cs, done in final[:n_best]]


def brute_force(logits, blank, space, tables, alpha, beta):
    """Every label string of at most T labels that the rules allow, ranked as the search ranks its final beam: [(labels tuple, score,
    log-likelihood, complete)], complete strings first, then by exact float64 log-likelihood + alpha ln P + beta of every word (an unfinished
    last word that is a word counted), the impossible strings (log-likelihood -inf) left out."""
    logits = np.asarray(logits, dtype=np.float64)
    T, V = logits.shape
    if T == 0:
        return [((), 0.0, 0.0, True)]
    logp = log_softmax(logits)
    labels = [c for c in range(V) if c != blank]
    out = []
    with np.errstate(all='ignore'):
        for n in range(T + 1):
            for q in itertools.product(labels, repeat=n):
                if not allowed(q, tables, space):
                    continue
                ll = -ctc_ref.ctc_utterance(logp, np.asarray(q, dtype=np.int64), blank)[0]
                if ll > -np.inf:
                    s, last, _, done = lm_terms(q, tables, space, alpha, beta)
                    out.append((q, float(ll) + s + (last if last is not None else 0.0), float(ll), done))
    out.sort(key=lambda x: (not x[3], -x[1]))
    return out
