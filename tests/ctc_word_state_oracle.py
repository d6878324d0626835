"""Oracle of the lexicon-constrained CTC prefix beam search with a word n-gram of any order (the contract include/silent_speech_hip.h states for
ss_ctc_word_state_beam_search), in plain Python.  The search is the one of tests/ctc_word_beam_oracle.py -- a dict from prefix (the label string as
`bytes`) to [lb, lnb, lm score], float64 by default, `dtype=np.float32` for the same steps in single precision -- but the word model is scored with
the FULL-HISTORY backoff rule of the ARPA format, not with context states: every prefix carries its whole word history, and

    ln P(w | h) = the n-gram (h, w) if the model holds it, else (the backoff of the n-gram h, 0 if the model does not hold it) + ln P(w | h without
                  its oldest word),      h = the last order - 1 words of the history,

summed from the lowest order outward.  There are no states, no suffix links and no hash table here: it shares no code with
csrc/ctc_word_state_decode.hip nor with the state tables of recognition_model.WordStateLM (the model comes in as the plain n-gram dictionary).
`Tables.levels` counts how often each n-gram level answered a lookup.

`brute_force` ranks EVERY label string the rules allow by its exact log-likelihood through oracle/ctc_ref.ctc_utterance plus the word terms."""
import collections
import itertools
import math

import numpy as np

from oracle import ctc_ref
from tests.ctc_beam_oracle import _lae64, log_softmax
from tests.ctc_word_beam_oracle import _split, allowed


class Tables(object):
    """spellings: one tuple of CLASS numbers per word (word id = index, the start context = len(spellings));
    ngrams: {(w_1, .., w_n): (ln P, backoff)}, used as they are stored (f32 numbers), cast to the run's dtype; order: contexts hold order - 1 words."""

    def __init__(self, spellings, ngrams, order):
        self.spellings, self.ngrams, self.order = [tuple(int(c) for c in s) for s in spellings], dict(ngrams), int(order)
        self.start = len(self.spellings)
        self.word_of = {bytes(s): w for w, s in enumerate(self.spellings)}
        self.prefixes = {bytes(s[:k]) for s in self.spellings for k in range(len(s) + 1)} | {b''}
        self.levels = collections.Counter()

    @classmethod
    def of(cls, lm, blank):
        """From a recognition_model.WordStateLM (its n-gram dictionary only); label number -> class number puts the blank back."""
        to_class = [i + (1 if i >= blank else 0) for i in range(len(lm.chars))]
        return cls([[to_class[lm.chars.index(ch)] for ch in w] for w in lm.words], lm.ngrams, lm.order)

    def lnp(self, history, w, cast=float):
        """ln P(w | history) by the full-history rule; history: every word so far, oldest first (the start context leads a sentence)."""
        h = tuple(history)
        h = h[len(h) - min(len(h), self.order - 1):]
        return self._p(h, w, cast)

    def _p(self, h, w, cast):
        g = h + (w,)
        if g in self.ngrams:
            self.levels[len(g)] += 1
            return cast(self.ngrams[g][0])
        bo = cast(self.ngrams[h][1]) if h in self.ngrams else cast(0.0)
        return bo + self._p(h[1:], w, cast)                              # (every unigram is in the model: the recursion ends)

    def known_context(self, history):
        """The longest suffix of the history, at most order - 1 words, that is an n-gram of the model: what a context state MEANS."""
        h = tuple(history)
        h = h[len(h) - min(len(h), self.order - 1):]
        while h and h not in self.ngrams:
            h = h[1:]
        return h


def lm_terms(q, tables, space, alpha, beta, cast=float):
    """(sum of the finished words' alpha lnP + beta accumulated one word at a time, the unfinished rest's term or None if it is no word,
    number of finished words, complete?)"""
    done, rest = _split(q, space)
    hist, s = (tables.start,), cast(0.0)
    for part in done:
        w = tables.word_of[part]
        s = s + (cast(alpha) * tables.lnp(hist, w, cast) + cast(beta))
        hist = hist + (w,)
    last = None
    if rest in tables.word_of:
        last = cast(alpha) * tables.lnp(hist, tables.word_of[rest], cast) + cast(beta)
    return s, last, len(done), (rest == b'' or last is not None)


def beam_search(logits, blank, space, beam_width, tables, alpha, beta, n_best=1, dtype=np.float64, trace=None):
    """logits (T, V) of ONE utterance -> list of at most n_best (labels tuple, score, ctc score, complete), complete entries first, best first.
    trace: a list that receives the number of candidates of every frame (at most beam_width of them: nothing was pruned)."""
    logits = np.asarray(logits)
    T, V = logits.shape
    if np.dtype(dtype) == np.float64:
        lae, cast, NEG = _lae64, float, -math.inf
    else:
        lae, cast, NEG = np.logaddexp, dtype, dtype(-np.inf)
    logp = log_softmax(logits, dtype)
    a, b = cast(alpha), cast(beta)
    one = [bytes([c]) for c in range(V)]
    # state of a prefix: (rest = the unfinished word's labels, the whole word history): a function of the string, kept beside the masses
    beam = {b'': [cast(0.0), NEG, cast(0.0), (b'', (tables.start,))]}
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
                rest, hist = state
                for c in range(V):
                    if c == blank:
                        continue
                    q = p + one[c]
                    v = (lb if c == last else tot) + row[c]
                    e = new.get(q)
                    if e is not None:                                    # reached before: its LM score and state are functions of the string
                        e[1] = lae(e[1], v)
                        continue
                    if c == space:
                        if rest not in tables.word_of:
                            continue
                        w = tables.word_of[rest]
                        s, nstate = lms + (a * tables.lnp(hist, w, cast) + b), (b'', hist + (w,))
                    else:
                        if rest + one[c] not in tables.prefixes:
                            continue
                        s, nstate = lms, (rest + one[c], hist)
                    new[q] = [NEG, v, s, nstate]
            cands = [(lae(e[0], e[1]) + e[2], q) for q, e in new.items()]
            cands = [x for x in cands if x[0] > NEG]                     # a candidate of score -inf does not exist
            cands.sort(key=lambda x: -x[0])                              # stable: ties keep the order of appearance
            beam = {q: new[q] for _, q in cands[:beam_width]}
            if trace is not None:
                trace.append(len(cands))
        final = []
        for q, (lb, lnb, lms, (rest, hist)) in beam.items():
            ctc = lae(lb, lnb)
            word = rest != b'' and rest in tables.word_of
            s = lms + ((a * tables.lnp(hist, tables.word_of[rest], cast) + b) if word else cast(0.0))
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
