"""Drop-in for the training path of the reference's recognition_model.py ("next" row N1, BASELINE cfg5):

    ctc_loss(logits, example, blank)         the three loss lines :96-101 fused on the packed layout
    greedy_decode(logits, lengths, blank)    best-path CTC decode (argmax, collapse repeats, drop blanks)
    beam_decode(logits, lengths, blank)      CTC prefix beam search on the device (csrc/ctc_decode.hip), optionally fused with a LabelNgramLM
    beam_decode_utterances(logits)           the same for the list Model.forward_utterances returns
    LabelNgramLM                             label trigram table counted from text, the language model of the beam search
    WordNgramLM                              word n-gram with backoff (orders 1 .. 3, from ARPA text or counted from transcripts) + the lexicon of
                                             its vocabulary: beam_decode* with it run the lexicon-constrained search of csrc/ctc_word_decode.hip
    WordStateLM                              the same of any order up to 6 (a pruned 5-gram ARPA file), held as context states: beam_decode* with it
                                             run the search of csrc/ctc_word_state_decode.hip
    forced_align(logits, lengths, targets)   best alignment of KNOWN label strings to the frames on the device (csrc/ctc_align.hip): Alignment per
                                             utterance; forced_align_utterances for the list Model.forward_utterances returns
    word_segments(alignment, text_int, tt)   (word, start_s, end_s, confidence) of a character alignment; align(model, testset, device) for a data set
    edit_distance(references, hypotheses)    Levenshtein distance with hits / substitutions / deletions / insertions and the alignment, a batch of
                                             pairs in one launch (csrc/edit_distance.hip); word_errors / cer: the jiwer measures of transcripts
    mbr_rerank(nbest, space=..)              minimum-Bayes-risk choice from n-best lists (all K^2 word distances per list on the device);
                                             oracle_errors: the best hypothesis of every list against its reference
    nbest_logp(pred, lengths, hyps)          full-sum CTC log-likelihood of arbitrary label strings, several per utterance, with a gradient
                                             (csrc/ctc.hip); nbest_logp_utterances; rescore_nbest: exact scores for the lists of beam_decode
    mwer_loss(pred, example, space=..)       minimum expected word error over the model's own n-best lists (+ ctc_weight * ctc_loss);
                                             train_model(.., mwer=dict(..)) trains on it
    test(model, testset, device)             :30-58 -> WER; decoder='greedy' (default) or 'beam'; mbr=K, details=True
    train_model(trainset, devset, device)    :61-117 (AdamW, warm-up, x2 gradient accumulation, MultiStepLR)

The encoder is the same MI355X engine as the transduction trainer (Model without the aux head).  The CTC
alpha/beta recursion and its gradient run in csrc/ctc.hip straight on the packed (rows*200, V) logits, so the
decollate + pad_sequence copies and the (T_max, N, V) log-prob tensor of the reference never exist.
The search of the reference's decoder (ctcdecode, :33-35,48-49) is here as a kernel of its own: a prefix beam search over whole batches
in one launch, with shallow fusion of a label n-gram table that lives on the device (LabelNgramLM), or -- as ctcdecode does it with a
KenLM model -- confined to the spellings of a vocabulary with a WORD n-gram with backoff scored at every word end (WordNgramLM: orders 1 to 3 as
hashed n-gram keys; WordStateLM: orders 1 to 6 as KenLM-style context states; both read from ARPA text or counted from transcripts; the search is lexicon-constrained, there is no out-of-vocabulary escape).  Out of scope: the
KenLM BINARY format (third-party C++; convert lm.binary to ARPA text) and parity with ctcdecode's own numbers, which stays unpinned because
ctcdecode is not available to compare against.  The same holds for the scoring (edit_distance, word_errors, mbr_rerank on csrc/edit_distance.hip):
WER and CER do not depend on it, but which of several alignments of equal cost jiwer / rapidfuzz report -- and with it their split into
substitutions, deletions and insertions in a tie -- is unpinned; the header states the tie rule used here.  test() reports greedy WER by default and beam-search WER with decoder='beam'.
"""
import collections
import logging
import os
import string

import numpy as np
import torch

from . import _lib, staging
from .pipeline import SizeAwareSampler
from .architecture import Model
from .flags import FLAGS
from .optim import FusedAdamW
from .transduction_model import prepare_batch

_L = _lib.lib
_p = _lib.ptr


class TextTransform(object):
    """data_utils.py:243-258 without the unidecode/jiwer dependencies (ASCII punctuation stripping + lower-casing)."""

    def __init__(self):
        self.chars = string.ascii_lowercase + string.digits + ' '

    def clean_text(self, text):
        return ''.join(c for c in text.lower() if c not in string.punctuation)

    def text_to_int(self, text):
        return [self.chars.index(c) for c in self.clean_text(text)]

    def int_to_text(self, ints):
        return ''.join(self.chars[i] for i in ints)


class _CtcPlan(object):
    """Utterance descriptors for ss_ctc_loss (include/silent_speech_hip.h)."""

    def __init__(self, lengths, targets, rows_total, device):
        lengths = [int(n) for n in lengths]
        tl = [int(t.shape[0]) for t in targets]
        assert sum(lengths) <= rows_total
        assert len(tl) == len(lengths)
        f0 = np.concatenate([[0], np.cumsum(lengths)])
        g0 = np.concatenate([[0], np.cumsum(tl)])
        ws = np.concatenate([[0], np.cumsum([n * (2 * s + 1) for n, s in zip(lengths, tl)])])
        desc = np.stack([f0[:-1], lengths, g0[:-1], tl, ws[:-1]], 1).astype(np.int64) if lengths else np.zeros((0, 5), np.int64)
        self.n, self.max_s, self.ws_floats = len(lengths), max(tl) if tl else 0, int(ws[-1])
        # both tables cross PCIe in ONE pinned copy on the current stream (staging.upload): two pageable .to(device) calls cost a blocking
        # copy each -- more than the CTC kernels of the batch (bench.py ctc.ctc_loss.hip_ms 0.34 ms with them against 0.18 ms of kernels)
        if all(torch.is_tensor(t) and t.device.type == 'cpu' for t in targets) or not targets:
            flat = np.concatenate([t.reshape(-1).numpy().astype(np.int32) for t in targets]) if sum(tl) else np.zeros(1, dtype=np.int32)
            self.desc, self.targets = staging.upload([desc if desc.size else np.zeros((1, 5), np.int64), flat], device)
            self.desc = self.desc[:len(lengths)]
        else:                                                            # labels that already live on the device
            self.desc, = staging.upload([desc if desc.size else np.zeros((1, 5), np.int64)], device)
            self.desc = self.desc[:len(lengths)]
            self.targets = torch.cat([t.reshape(-1).to(device=device, dtype=torch.int32) for t in targets]).contiguous() if sum(tl) else torch.zeros(1, dtype=torch.int32, device=device)
        self.lengths, self.tlens = lengths, tl


def ctc_loss(pred, example, blank=None, *, return_plan=False):
    """recognition_model.py:96-101 in one call.  pred: (rows, 200, V) raw model outputs (NOT log-softmaxed);
    example: the collate_raw batch dict ('lengths', 'text_int').  Returns the 0-dim mean loss
    (per-utterance nll / max(target length, 1), averaged), attached to autograd."""
    B, T, V = pred.shape
    blank = V - 1 if blank is None else int(blank)
    logits = pred.reshape(B * T, V).float().contiguous()
    plan = _CtcPlan(example['lengths'], example['text_int'], B * T, pred.device)
    loss, _, nll, amax = torch.ops.silent_speech.ctc_loss(logits, plan.desc, plan.targets, plan.n, plan.max_s, plan.ws_floats, V, blank)
    plan.nll, plan.argmax = nll.detach()[:plan.n], amax
    loss = loss[0]
    return (loss, plan) if return_plan else loss


def _collapse(path, blank):
    out, prev = [], -1
    for c in path:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return out


def greedy_decode(pred, lengths, blank=None):
    """Best-path decode of packed logits (rows, T, V): per-frame argmax on the device (ss_frame_lse), then
    collapse-repeats / drop-blanks per utterance on the host.  Returns a list of int lists."""
    B, T, V = pred.shape
    blank = V - 1 if blank is None else int(blank)
    logits = pred.reshape(B * T, V).float().contiguous()
    M = B * T
    lse = torch.empty(M, dtype=torch.float32, device=pred.device)
    amax = torch.empty(M, dtype=torch.int32, device=pred.device)
    _lib.check(_L().ss_frame_lse(_p(logits), V, 0, V, M, _p(lse), _p(amax), _lib.stream_of(logits)), 'ss_frame_lse')
    path = amax.cpu().numpy()
    out, off = [], 0
    for n in lengths:
        out.append(_collapse(path[off:off + int(n)], blank))
        off += int(n)
    return out


def _edit_distance(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def wer(references, predictions):
    """jiwer.wer (:58): total word edit distance / total reference words."""
    errs = sum(_edit_distance(r.split(), p.split()) for r, p in zip(references, predictions))
    words = sum(len(r.split()) for r in references)
    return errs / max(words, 1)


EditResult = collections.namedtuple('EditResult', ['distance', 'hits', 'substitutions', 'deletions', 'insertions', 'ops'])
EditResult.__doc__ = """Levenshtein distance of one (reference, hypothesis) pair with its breakdown (ss_edit_distance in include/silent_speech_hip.h states the
definition and the tie rule): hits + substitutions + deletions = reference length, hits + substitutions + insertions = hypothesis length,
substitutions + deletions + insertions = distance.  ops: the alignment as an int8 array, one entry per step from the beginning (0 hit, 1 substitution,
2 deletion, 3 insertion), or None when it was not asked for."""
ErrorCounts = collections.namedtuple('ErrorCounts', ['hits', 'substitutions', 'deletions', 'insertions', 'reference_tokens', 'rate', 'per_utterance'])
ErrorCounts.__doc__ = """The measures jiwer reports for a test set: the four counts summed over the utterances, the number of reference tokens N,
rate = (S + D + I) / max(N, 1) -- the WER for words, the CER for characters -- and the EditResult of every utterance."""
MAX_EDIT_TOKENS = 1023
MAX_NBEST = 128


def _scoring_device(device):
    if device is not None:
        return torch.device(device)
    return torch.device('cpu') if _lib.is_emulator() else torch.device('cuda')


class _TokenTable(object):
    """Sequences of hashable tokens as the flat int32 tokens and the (first token, length) table of ss_edit_distance; ids are interned per table."""

    def __init__(self, who):
        self.who, self.ids, self.flat, self.rows = who, {}, [], []

    def add(self, seq):
        seq = list(seq)
        if len(seq) > MAX_EDIT_TOKENS:
            raise ValueError('%s: a sequence of %d tokens (at most %d)' % (self.who, len(seq), MAX_EDIT_TOKENS))
        ids = self.ids
        self.rows.append((len(self.flat), len(seq)))
        self.flat.extend(ids.setdefault(t, len(ids)) for t in seq)
        return len(self.rows) - 1

    def arrays(self):
        """(tokens with one spare entry: never an empty upload, seqs)"""
        return np.asarray(self.flat + [0], dtype=np.int32), np.asarray(self.rows, dtype=np.int64).reshape(len(self.rows), 2)


def _edit_results(table, pairs, ops, device):
    """One upload, one launch, one read-back: the EditResult of every (reference row, hypothesis row) of `pairs` over the sequences of `table`."""
    if not pairs:
        return []
    flat, seqs = table.arrays()
    tokens, seqs_d, pairs_d = staging.upload([flat, seqs, np.asarray(pairs, dtype=np.int32).reshape(len(pairs), 2)], device)
    dist, counts, ops_d, _ = torch.ops.silent_speech.edit_distance(tokens, seqs_d, pairs_d, bool(ops))
    back = torch.cat([dist, counts.reshape(-1), ops_d.to(torch.int32)]).cpu().numpy()                  # ONE read-back
    n = len(pairs)
    dist, counts, steps = back[:n], back[n:5 * n].reshape(n, 4), back[5 * n:].astype(np.int8)
    out, at = [], 0
    for p, (a, b) in enumerate(pairs):
        if dist[p] < 0:
            raise RuntimeError('edit_distance: pair %d was refused by the kernel' % p)
        path = None
        if ops:
            room, n_path = table.rows[a][1] + table.rows[b][1], int(counts[p].sum())
            path, at = steps[at:at + n_path].copy(), at + room
        out.append(EditResult(int(dist[p]), int(counts[p, 0]), int(counts[p, 1]), int(counts[p, 2]), int(counts[p, 3]), path))
    return out


def edit_distance(references, hypotheses, *, ops=False, device=None):
    """Levenshtein distance with the jiwer breakdown of every (reference, hypothesis) pair, the whole batch in one launch on the device
    (csrc/edit_distance.hip).  references / hypotheses: equally many token lists (ints or any hashables, compared by ==, at most 1023 each).
    ops=True adds the alignment.  Returns a list of EditResult.  The tie rule among alignments of equal cost is the one the header states; parity
    with jiwer's own choice is unpinned (jiwer is not available to compare against) -- the distance and the rates do not depend on it."""
    references, hypotheses = list(references), list(hypotheses)
    if len(references) != len(hypotheses):
        raise ValueError('edit_distance: %d references for %d hypotheses' % (len(references), len(hypotheses)))
    table = _TokenTable('edit_distance')
    pairs = [(table.add(r), table.add(h)) for r, h in zip(references, hypotheses)]
    return _edit_results(table, pairs, ops, _scoring_device(device))


def _error_counts(results, n_ref):
    h, s, d, i = (sum(r[k] for r in results) for k in (1, 2, 3, 4))
    return ErrorCounts(h, s, d, i, n_ref, (s + d + i) / max(n_ref, 1), results)


def _units(text, unit, who):
    if unit == 'word':
        return text.split()
    if unit == 'char':
        return list(text)
    raise ValueError("%s: unit is 'word' or 'char'" % who)


def word_errors(references, predictions, *, unit='word', device=None):
    """What jiwer.compute_measures reports for transcripts: hits, substitutions, deletions and insertions over the words (unit='char': the
    characters) of the reference strings against the predicted strings, one launch for the test set.  Returns ErrorCounts; its rate is the
    value wer() returns for unit='word'."""
    refs = [_units(r, unit, 'word_errors') for r in references]
    hyps = [_units(p, unit, 'word_errors') for p in predictions]
    return _error_counts(edit_distance(refs, hyps, device=device), sum(len(r) for r in refs))


def cer(references, predictions, *, device=None):
    """Character error rate: total character edit distance / total reference characters."""
    return word_errors(references, predictions, unit='char', device=device).rate


def _label_units(ints, space, unit, who):
    """The scoring tokens of a label string: unit='word' the runs of labels between `space` labels (as tuples), unit='char' the labels."""
    ints = [int(c) for c in ints]
    if unit == 'char':
        return ints
    if unit != 'word':
        raise ValueError("%s: unit is 'word' or 'char'" % who)
    words, run = [], []
    for c in ints + [space]:
        if c != space:
            run.append(c)
        elif run:
            words.append(tuple(run))
            run = []
    return words


def mbr_rerank(nbest, *, space, scale=1.0, unit='word', device=None):
    """Minimum-Bayes-risk selection from the n-best lists beam_decode*(.., n_best=K) return: per utterance the hypothesis of the least expected
    word (unit='char': label) edit distance to the others under the list's own posterior, softmax(scale * score) over the list (f64 on the
    host, rounded to f32).  Words are the runs of labels between `space` labels, interned across the batch.  All K^2 distances of every
    list, the risks and the choice are computed on the device (ss_nbest_risk, two launches).  Returns per utterance (pick, risks): the index of the
    chosen hypothesis (the better rank among equal risks; -1 for an empty list) and the f64 risk of every hypothesis.  At most 128 hypotheses
    per utterance; an utterance with fewer than K is a smaller group."""
    space = int(space)
    table, groups, weights = _TokenTable('mbr_rerank'), [], []
    for hyps in nbest:
        hyps = list(hyps)
        if len(hyps) > MAX_NBEST:
            raise ValueError('mbr_rerank: %d hypotheses for one utterance (at most %d)' % (len(hyps), MAX_NBEST))
        if hyps:
            groups.append((len(table.rows), len(hyps)))
            z = np.asarray([float(score) for _, score in hyps], dtype=np.float64) * float(scale)
            z = np.exp(z - z.max())
            weights.extend((z / z.sum()).astype(np.float32))
        for ints, _ in hyps:
            table.add(_label_units(ints, space, unit, 'mbr_rerank'))
    out = [(-1, np.zeros(0, dtype=np.float64)) for _ in nbest]
    if not groups:
        return out
    flat, seqs = table.arrays()
    tokens, seqs_d, groups_d, weights_d = staging.upload([flat, seqs, np.asarray(groups, dtype=np.int64), np.asarray(weights, dtype=np.float32)],
                                                         _scoring_device(device))
    _, risk, pick = torch.ops.silent_speech.nbest_risk(tokens, seqs_d, groups_d, weights_d)
    back = torch.cat([risk, pick.to(torch.float64)]).cpu().numpy()                                      # ONE read-back
    risk, pick = back[:len(table.rows)], back[len(table.rows):].astype(np.int64)
    g = 0
    for u, hyps in enumerate(nbest):
        if len(hyps):
            first, K = groups[g]
            if pick[g] < 0:
                raise RuntimeError('mbr_rerank: utterance %d was refused by the kernel' % u)
            out[u] = (int(pick[g]), risk[first:first + K].copy())
            g += 1
    return out


def oracle_errors(references, nbest, *, space, unit='word', device=None):
    """Oracle error rate of n-best lists: per utterance the hypothesis of the least word (unit='char': label) edit distance to the reference
    (the better rank among equals), from ONE edit-distance launch over all (utterance, hypothesis) pairs.  references: one label string (ints,
    the labels of the hypotheses) per utterance; nbest: what beam_decode*(.., n_best=K) returns.  An empty list counts as the empty hypothesis
    (choice -1).  Returns (choices, ErrorCounts of the chosen hypotheses)."""
    references, nbest = list(references), list(nbest)
    if len(references) != len(nbest):
        raise ValueError('oracle_errors: %d references for %d n-best lists' % (len(references), len(nbest)))
    space = int(space)
    table, pairs, spans, n_ref = _TokenTable('oracle_errors'), [], [], 0
    for ref, hyps in zip(references, nbest):
        r = table.add(_label_units(ref, space, unit, 'oracle_errors'))
        n_ref += table.rows[r][1]
        cand = [table.add(_label_units(ints, space, unit, 'oracle_errors')) for ints, _ in hyps] or [table.add([])]
        spans.append((len(pairs), len(cand), len(hyps)))
        pairs.extend((r, h) for h in cand)
    results = _edit_results(table, pairs, False, _scoring_device(device))
    choices, chosen = [], []
    for first, n, n_hyps in spans:
        best = min(range(n), key=lambda k: (results[first + k].distance, k))
        choices.append(best if n_hyps else -1)
        chosen.append(results[first + best])
    return choices, _error_counts(chosen, n_ref)


def greedy_decode_utterances(logits):
    """Best-path decode of the per-utterance logits Model.forward_utterances returns -- (T_b, V) views of ONE (B T_max, >= V) head buffer --: one
    per-frame arg-max launch over all slots (ss_frame_lse) and ONE read-back for the group, then collapse-repeats / drop-blanks per utterance on
    the host over its own T_b frames (the filler rows of a slot are never looked at).  blank = V - 1.  Returns a list of int lists."""
    if not logits:
        return []
    head, V = logits[0]._base, logits[0].shape[1]
    B, T = len(logits), max(int(y.shape[0]) for y in logits)                 # the slots are as long as the longest utterance
    if head is None or head.dim() != 2 or head.dtype != torch.float32 or not head.is_contiguous() or head.shape[0] != B * T or \
            any(y._base is not head or y.shape[1] != V or y.storage_offset() != b * T * head.shape[1] for b, y in enumerate(logits)):
        raise ValueError('greedy_decode_utterances takes the list Model.forward_utterances returned')
    ld = head.shape[1]
    lse = torch.empty(B * T, dtype=torch.float32, device=head.device)
    amax = torch.empty(B * T, dtype=torch.int32, device=head.device)
    _lib.check(_L().ss_frame_lse(_p(head), ld, 0, V, B * T, _p(lse), _p(amax), _lib.stream_of(head)), 'ss_frame_lse')
    path = amax.cpu().numpy().reshape(B, T)
    return [_collapse(path[b, :y.shape[0]], V - 1) for b, y in enumerate(logits)]


class LabelNgramLM(object):
    """Label trigram table for the beam search: table[i2, i1, c] = ln P(label c | the two labels before it), f32 (C + 1, C + 1, C) over the
    C labels of the text transform (the CTC classes with the blank skipped); context index C = "before the start of the text"."""

    def __init__(self, table):
        table = torch.as_tensor(table, dtype=torch.float32)
        if table.dim() != 3 or table.shape[0] != table.shape[2] + 1 or table.shape[1] != table.shape[2] + 1:
            raise ValueError('LabelNgramLM: a (C + 1, C + 1, C) table is expected')
        self.table = table.contiguous()

    @property
    def n_labels(self):
        return self.table.shape[2]

    @classmethod
    def from_texts(cls, texts, text_transform, add_k=0.1, order=3):
        """Counts label n-grams over `texts` (each starting in the "before the start" context) and smooths every context with add_k:
        P(c | context) = (count + add_k) / (context count + add_k C).  order 3 = trigram; 2 / 1 = bigram / unigram, stored in the same
        table (constant along the leading axes they do not look at)."""
        if order not in (1, 2, 3) or not add_k > 0:
            raise ValueError('LabelNgramLM.from_texts: order 1, 2 or 3 and add_k > 0')
        C = len(text_transform.chars)
        counts = np.zeros((C + 1, C + 1, C), dtype=np.float64)
        for text in texts:
            i2 = i1 = C
            for c in text_transform.text_to_int(text):
                counts[i2 if order >= 3 else 0, i1 if order >= 2 else 0, c] += 1
                i2, i1 = i1, c
        if order < 3:
            counts[:] = counts[:1]
        if order < 2:
            counts[:] = counts[:, :1]
        prob = (counts + add_k) / (counts.sum(2, keepdims=True) + add_k * C)
        return cls(torch.from_numpy(np.log(prob).astype(np.float32)))

    def save(self, path):
        with open(path, 'wb') as f:
            np.savez(f, table=self.table.cpu().numpy())

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(torch.from_numpy(z['table']))

    def to(self, device):
        return LabelNgramLM(self.table.to(device))


_NGRAM_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
_LN10 = float(np.log(10.0))


def _ngram_home(keys):
    """Home slot (before masking with slots - 1) of packed n-gram keys: the low 32 bits of the splitmix64 finaliser of key + 0x9E3779B97F4A7C15,
    as include/silent_speech_hip.h states it for ss_word_lm."""
    x = np.asarray(keys, dtype=np.uint64).copy()
    with np.errstate(over='ignore'):
        x += np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x & np.uint64(0xFFFFFFFF)


def _ngram_table(keys, values, columns, min_slots):
    """Open addressing, linear probing, load factor <= 0.5: (keys (slots) uint64 with all ones = empty, values (columns, slots) f32, longest
    probe); no keys: no table (0 slots)."""
    keys, values = np.asarray(keys, dtype=np.uint64), np.asarray(values, dtype=np.float32).reshape(len(keys), columns)
    if len(keys) == 0:
        return np.zeros(0, dtype=np.uint64), np.zeros((columns, 0), dtype=np.float32), 0
    slots = 1
    while slots < max(2 * len(keys), int(min_slots)):
        slots *= 2
    tab, val, probe = np.full(slots, _NGRAM_EMPTY, dtype=np.uint64), np.zeros((values.shape[1], slots), dtype=np.float32), 0
    home = (_ngram_home(keys) & np.uint64(slots - 1)).astype(np.int64)
    for i in np.argsort(keys, kind='stable'):
        s, n = int(home[i]), 1
        while tab[s] != _NGRAM_EMPTY:
            s, n = (s + 1) & (slots - 1), n + 1
        tab[s], val[:, s], probe = keys[i], values[i], max(probe, n)
    return tab, val, probe


def _read_arpa(path_or_file, max_order, who):
    """The sections of ARPA text (\\data\\, \\1-grams: .. , \\end\\): {n: [(words tuple, ln P, ln backoff)]}, log10 -> ln, a missing backoff = 0.
    A section or a non-zero count above max_order: ValueError in the name of `who`."""
    f = open(path_or_file) if isinstance(path_or_file, (str, os.PathLike)) else path_or_file
    try:
        lines = [line.strip() for line in f]
    finally:
        if f is not path_or_file:
            f.close()
    grams, order = {k: [] for k in range(1, max_order + 1)}, 0
    for line in lines:
        if not line or line == '\\data\\':
            continue
        if line == '\\end\\':
            break
        if line.startswith('ngram '):
            n, count = line[6:].split('=')
            if int(n) > max_order and int(count) > 0:
                raise ValueError('%s.from_arpa: order %d (orders 1 to %d are supported)' % (who, int(n), max_order))
            continue
        if line.startswith('\\') and line.endswith('-grams:'):
            order = int(line[1:-7])
            if order > max_order:
                raise ValueError('%s.from_arpa: order %d (orders 1 to %d are supported)' % (who, order, max_order))
            continue
        if order == 0:
            continue
        f_ = line.split()
        if len(f_) not in (order + 1, order + 2):
            raise ValueError('%s.from_arpa: cannot read %r as a %d-gram' % (who, line, order))
        grams[order].append((tuple(f_[1:order + 1]), float(f_[0]) * _LN10, float(f_[order + 1]) * _LN10 if len(f_) == order + 2 else 0.0))
    return grams


def _arpa_vocabulary(unigrams, text_transform):
    """(words = the sorted cleaned spellings, {ARPA word: id} with '<s>' = len(words)) of the unigram section: </s> and <unk> are never predicted, a
    word whose clean_text spelling is empty, holds a space or a character outside text_transform.chars is dropped, and of two words with one
    cleaned spelling the one with the larger unigram probability keeps it."""
    chars = text_transform.chars
    best = {}                                                            # cleaned spelling -> (unigram ln P, ARPA word)
    for (w,), lp, _ in unigrams:
        if w in ('<s>', '</s>', '<unk>'):
            continue
        sp = text_transform.clean_text(w)
        if sp and all(c != ' ' and c in chars for c in sp) and (sp not in best or lp > best[sp][0]):
            best[sp] = (lp, w)
    words = sorted(best)
    ids = {best[sp][1]: i for i, sp in enumerate(words)}
    ids['<s>'] = len(words)
    return words, ids


def _discounted(counts, lower, n, discount):
    """Absolute discounting of one n-gram level: {context: {w: P}} and {context: ln backoff} from {(context..., w): count}; lower(context, w) =
    the lower level's P, n = the vocabulary size."""
    by = {}
    for k, c in counts.items():
        by.setdefault(k[:-1], {})[k[-1]] = c
    P, BO = {}, {}
    for h, cs in by.items():
        total = float(sum(cs.values()))
        rest = 1.0 - sum(lower(h, w) for w in cs)
        if len(cs) == n or rest <= 1e-12:
            P[h], BO[h] = {w: c / total for w, c in cs.items()}, 0.0
        else:
            P[h] = {w: (c - discount) / total for w, c in cs.items()}
            BO[h] = float(np.log((1.0 - sum(P[h].values())) / rest))
    return P, BO


def _lexicon_trie(words, chars):
    """The trie of the spellings: (lex_child (n_nodes, C) int32 = child node or -1, lex_word (n_nodes) int32 = the word a node spells or -1); node 0
    is the root, label number = index into chars."""
    C = len(chars)
    child, word = [[-1] * C], [-1]
    for w, spelling in enumerate(words):
        node = 0
        for ch in spelling:
            c = chars.index(ch)
            if child[node][c] < 0:
                child[node][c] = len(child)
                child.append([-1] * C)
                word.append(-1)
            node = child[node][c]
        word[node] = w
    return torch.from_numpy(np.asarray(child, dtype=np.int32).reshape(len(child), C)), torch.from_numpy(np.asarray(word, dtype=np.int32))


class WordNgramLM(object):
    """Word n-gram with backoff of order 1 to 3 and the lexicon trie of its vocabulary: the language model of the lexicon-constrained beam search
    (include/silent_speech_hip.h: ss_word_lm, ss_ctc_word_beam_search).  Natural log, f32.

    words        the vocabulary, cleaned spellings over `chars`; word id = index, the start context <s> has id n_words
    unigrams     (n_words + 1, 2) [ln P(w), backoff of the context (w)]
    bigrams      {(w1, w): (ln P(w | w1), backoff of the context (w1, w))},  trigrams {(w2, w1, w): ln P(w | w2, w1)}
    chars        the labels of the text transform; label number = index (the CTC classes with the blank skipped)
    min_slots    least slot count of each hash table (tests force wrap-around and long probes with it)

    Device form (torch tensors, `to(device)`): lex_child (n_nodes, C) / lex_word (n_nodes) int32, uni (2, n_words + 1) f32, bi_keys (slots) int64 +
    bi_val (2, slots) f32, tri_keys (slots) int64 + tri_val (slots) f32, bi_probe / tri_probe = the longest probe sequence of each table."""
    MAX_WORDS = 1 << 21

    def __init__(self, words, unigrams, bigrams, trigrams, chars, min_slots=0):
        words = [str(w) for w in words]
        n = len(words)
        uni = np.asarray(unigrams, dtype=np.float32).reshape(-1, 2)
        if n + 1 > self.MAX_WORDS or uni.shape[0] != n + 1:
            raise ValueError('WordNgramLM: %d words (< 2^21) need %d unigram rows, the last one the start context' % (n, n + 1))
        if len(set(words)) != n or any(not w or any(c == ' ' or c not in chars for c in w) for w in words):
            raise ValueError('WordNgramLM: the words must be distinct, non-empty and spelled with the labels %r without the space' % (chars,))
        self.words, self.chars, self.min_slots = words, str(chars), int(min_slots)
        self.unigrams = uni
        self.bigrams = {(int(a), int(b)): (np.float32(v[0]), np.float32(v[1])) for (a, b), v in (bigrams or {}).items()}
        self.trigrams = {(int(a), int(b), int(c)): np.float32(v) for (a, b, c), v in (trigrams or {}).items()}
        if any(not (0 <= a <= n and 0 <= b < n) for a, b in self.bigrams) or any(not (0 <= a <= n and 0 <= b < n and 0 <= c < n) for a, b, c in self.trigrams):
            raise ValueError('WordNgramLM: n-gram word ids must be below %d (the start context %d only leads)' % (n, n))
        self.lex_child, self.lex_word = _lexicon_trie(words, self.chars)
        # the hash tables
        bk = sorted(self.bigrams)
        tk = sorted(self.trigrams)
        bkeys = np.asarray([(a << 21) | b for a, b in bk], dtype=np.uint64)
        tkeys = np.asarray([(a << 42) | (b << 21) | c for a, b, c in tk], dtype=np.uint64)
        btab, bval, self.bi_probe = _ngram_table(bkeys, [self.bigrams[k] for k in bk], 2, min_slots)
        ttab, tval, self.tri_probe = _ngram_table(tkeys, [self.trigrams[k] for k in tk], 1, min_slots)
        self.uni = torch.from_numpy(np.ascontiguousarray(uni.T))
        self.bi_keys, self.bi_val = torch.from_numpy(btab.view(np.int64)), torch.from_numpy(bval)
        self.tri_keys, self.tri_val = torch.from_numpy(ttab.view(np.int64)), torch.from_numpy(tval.reshape(-1))

    _DEVICE_FORM = ('lex_child', 'lex_word', 'uni', 'bi_keys', 'bi_val', 'tri_keys', 'tri_val')

    @property
    def n_words(self):
        return len(self.words)

    @property
    def start(self):
        return len(self.words)

    @property
    def order(self):
        return 3 if self.trigrams else 2 if self.bigrams else 1

    def to(self, device):
        """The same model with its tables on `device` (the host form is shared, not copied)."""
        other = object.__new__(WordNgramLM)
        other.__dict__.update(self.__dict__)
        for name in self._DEVICE_FORM:
            setattr(other, name, getattr(self, name).to(device))
        return other

    def word_ids(self, text, text_transform):
        """Ids of the words of `text` after clean_text; raises KeyError on a word outside the vocabulary."""
        index = getattr(self, '_index', None)
        if index is None:
            index = self._index = {w: i for i, w in enumerate(self.words)}
        return [index[w] for w in text_transform.clean_text(text).split()]

    def score_words(self, word_ids, dtype=np.float64, context=None):
        """ln P of every word of a sentence given the words before it -- the backoff rule of ss_word_lm restated on the host tables, in `dtype`
        arithmetic: tri(w2, w1, w) if present; else (backoff of bi(w2, w1), 0 if absent) + P2, P2 = bi(w1, w) if present, else backoff(w1) +
        uni(w); with w2 = none (-1), P2.  context = (w2, w1) the sentence starts in; default (none, <s>)."""
        w2, w1 = (-1, self.start) if context is None else (int(context[0]), int(context[1]))
        out = np.zeros(len(word_ids), dtype=dtype)
        for i, w in enumerate(word_ids):
            w = int(w)
            if not (0 <= w <= self.n_words) or not (-1 <= w1 <= self.n_words) or not (-1 <= w2 <= self.n_words):
                raise ValueError('score_words: word id outside the model')
            if w1 < 0:
                p = dtype(self.unigrams[w, 0])
            elif w2 >= 0 and (w2, w1, w) in self.trigrams:
                p = dtype(self.trigrams[(w2, w1, w)])
            else:
                p = dtype(self.bigrams[(w1, w)][0]) if (w1, w) in self.bigrams else dtype(self.unigrams[w1, 1]) + dtype(self.unigrams[w, 0])
                if w2 >= 0 and (w2, w1) in self.bigrams:
                    p = dtype(self.bigrams[(w2, w1)][1]) + p
            out[i] = p
            w2, w1 = w1, w
        return out

    def score_triples(self, triples):
        """torch.ops.silent_speech.word_ngram_score on this model's tables: ln P(w | w2, w1) of (n, 3) int32 rows (w2, w1, w) on the tables' device."""
        return torch.ops.silent_speech.word_ngram_score(triples, self.uni, self.bi_keys, self.bi_val, self.tri_keys, self.tri_val, self.bi_probe, self.tri_probe)

    # ---- builders
    @classmethod
    def from_arpa(cls, path_or_file, text_transform, min_slots=0):
        """Reads ARPA text (\\data\\, \\1-grams: .. \\3-grams:, \\end\\; log10 values, a missing backoff = 0).  <s> is the start context; </s> and
        <unk> are read and never predicted (the search is lexicon-constrained, so n-grams holding them can never be asked for and are left out).
        A word whose clean_text spelling is empty, holds a space or a character outside text_transform.chars is dropped with every n-gram
        holding it; of two words with one cleaned spelling the one with the larger unigram probability keeps it.  Order > 3: ValueError."""
        grams = _read_arpa(path_or_file, 3, 'WordNgramLM')
        words, ids = _arpa_vocabulary(grams[1], text_transform)
        uni = np.zeros((len(words) + 1, 2), dtype=np.float64)
        uni[len(words), 0] = -99.0 * _LN10
        for (w,), lp, bo in grams[1]:
            if w in ids:
                uni[ids[w]] = (lp, bo)
        bi = {(ids[a], ids[b]): (lp, bo) for (a, b), lp, bo in grams[2] if a in ids and b in ids and b != '<s>'}
        tri = {(ids[a], ids[b], ids[c]): lp for (a, b, c), lp, _ in grams[3] if a in ids and b in ids and c in ids and b != '<s>' and c != '<s>'}
        return cls(words, uni, bi, tri, text_transform.chars, min_slots)

    @classmethod
    def from_texts(cls, texts, text_transform, order=3, discount=0.75, add_k=0.1, min_slots=0):
        """Counts word n-grams over the cleaned texts, each starting in the <s> context.  Unigrams: add-k over the vocabulary,
        P(w) = (c(w) + add_k) / (N + add_k n_words).  Seen bigrams and trigrams: absolute discounting, P(w | h) = (c(h w) - discount) / c(h .),
        and the backoff weight of every seen context gives the rest to the lower order so that the probabilities over the vocabulary sum to 1:
        bo(h) = (1 - sum_seen P(w | h)) / (1 - sum_seen P_lower(w | h')).  (A context after which EVERY word of the vocabulary was seen keeps
        its undiscounted relative frequencies.)  Words that clean_text cannot spell with text_transform.chars are skipped with the n-grams
        holding them."""
        if order not in (1, 2, 3) or not (0 < discount < 1) or not add_k > 0:
            raise ValueError('WordNgramLM.from_texts: order 1, 2 or 3, 0 < discount < 1 and add_k > 0')
        chars = text_transform.chars
        sents = [[w if all(c in chars for c in w) else None for w in text_transform.clean_text(t).split()] for t in texts]
        words = sorted({w for s in sents for w in s if w is not None})
        n, ids = len(words), {}
        ids.update({w: i for i, w in enumerate(words)})
        c1, c2, c3 = np.zeros(n, dtype=np.float64), {}, {}
        for s in sents:
            seq = [n] + [ids[w] if w is not None else None for w in s]
            for i in range(1, len(seq)):
                if seq[i] is None:
                    continue
                c1[seq[i]] += 1
                if order >= 2 and seq[i - 1] is not None:
                    c2[(seq[i - 1], seq[i])] = c2.get((seq[i - 1], seq[i]), 0) + 1
                    if order >= 3 and i >= 2 and seq[i - 2] is not None:
                        k = (seq[i - 2], seq[i - 1], seq[i])
                        c3[k] = c3.get(k, 0) + 1
        p1 = (c1 + add_k) / (c1.sum() + add_k * max(n, 1))
        uni = np.zeros((n + 1, 2), dtype=np.float64)
        uni[:n, 0] = np.log(p1)
        uni[n, 0] = -99.0 * _LN10
        P2, BO1 = _discounted(c2, lambda h, w: p1[w], n, discount)
        for (w1,), bo in BO1.items():
            uni[w1, 1] = bo

        def p_bi(w1, w):
            return P2[(w1,)][w] if (w1,) in P2 and w in P2[(w1,)] else float(np.exp(uni[w1, 1])) * p1[w]
        P3, BO2 = _discounted(c3, lambda h, w: p_bi(h[1], w), n, discount)
        bi = {(w1, w): (float(np.log(p)), BO2.get((w1, w), 0.0)) for (w1,), ps in P2.items() for w, p in ps.items()}
        tri = {(w2, w1, w): float(np.log(p)) for (w2, w1), ps in P3.items() for w, p in ps.items()}
        return cls(words, uni, bi, tri, chars, min_slots)

    def write_arpa(self, path):
        """ARPA text of the model (log10 values; the words as their cleaned spellings), readable by from_arpa and by other n-gram tools."""
        n = self.n_words
        name = self.words + ['<s>']
        with open(path, 'w') as f:
            f.write('\\data\\\nngram 1=%d\n' % (n + 1))
            if self.bigrams:
                f.write('ngram 2=%d\n' % len(self.bigrams))
            if self.trigrams:
                f.write('ngram 3=%d\n' % len(self.trigrams))
            f.write('\n\\1-grams:\n')
            for w in range(n + 1):
                f.write('%.9g\t%s\t%.9g\n' % (float(self.unigrams[w, 0]) / _LN10, name[w], float(self.unigrams[w, 1]) / _LN10))
            if self.bigrams:
                f.write('\n\\2-grams:\n')
                for (a, b) in sorted(self.bigrams):
                    lp, bo = self.bigrams[(a, b)]
                    f.write('%.9g\t%s %s\t%.9g\n' % (float(lp) / _LN10, name[a], name[b], float(bo) / _LN10))
            if self.trigrams:
                f.write('\n\\3-grams:\n')
                for (a, b, c) in sorted(self.trigrams):
                    f.write('%.9g\t%s %s %s\n' % (float(self.trigrams[(a, b, c)]) / _LN10, name[a], name[b], name[c]))
            f.write('\n\\end\\\n')

    def save(self, path):
        bk, tk = sorted(self.bigrams), sorted(self.trigrams)
        with open(path, 'wb') as f:
            np.savez(f, words=np.asarray(self.words, dtype=np.str_), chars=np.asarray(self.chars), unigrams=self.unigrams, min_slots=np.asarray(self.min_slots),
                     bi_ids=np.asarray(bk, dtype=np.int32).reshape(len(bk), 2), bi_val=np.asarray([self.bigrams[k] for k in bk], dtype=np.float32).reshape(len(bk), 2),
                     tri_ids=np.asarray(tk, dtype=np.int32).reshape(len(tk), 3), tri_val=np.asarray([self.trigrams[k] for k in tk], dtype=np.float32))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            bi = {tuple(k): tuple(v) for k, v in zip(z['bi_ids'].tolist(), z['bi_val'])}
            tri = {tuple(k): v for k, v in zip(z['tri_ids'].tolist(), z['tri_val'])}
            return cls([str(w) for w in z['words']], z['unigrams'], bi, tri, str(z['chars']), int(z['min_slots']))


class WordStateLM(object):
    """Word n-gram with backoff of ANY order 1 to 6 held as context states, and the lexicon trie of its vocabulary: the language model of
    csrc/ctc_word_state_decode.hip (include/silent_speech_hip.h: ss_word_state_lm, ss_ctc_word_state_beam_search).  Natural log, f32.

    words        the vocabulary, cleaned spellings over `chars`; word id = index, the start context <s> has id n_words and may only lead an n-gram
    ngrams       {(w_1, .., w_n): (ln P(w_n | w_1 .. w_{n-1}), backoff of the context (w_1 .. w_n))}, 1 <= n <= order; every unigram, <s> included,
                 must be there, and the model must be PREFIX-CLOSED: the context (w_1 .. w_{n-1}) of every n-gram is itself an n-gram (KenLM and
                 SRILM files are; dropping words with every n-gram that holds them keeps them so)
    order        default max(2, the longest n-gram); contexts of up to order - 1 words become states
    min_slots    least slot count of the hash table (tests force wrap-around and long probes with it)

    A STATE is a context the model knows: 0 = the empty context, 1 + w = (w), then every n-gram of 2 .. order - 1 words by increasing length, so
    shorter[s] (the state of the longest proper suffix of s that is a state) < s.  An ARC is an n-gram of >= 2 words: key (state of its context
    << 21 | word) -> (ln P, next = the state of the longest suffix of the whole n-gram that is a state).  ln P(w | s): the first state of the chain
    s, shorter[s], .. (0 left out) with an arc for w gives p and next, none gives the unigram and next = 1 + w; the value adds the backoffs of the
    states passed, summed from the lowest order outward -- for order <= 3 the f32 numbers of WordNgramLM.

    Device form (torch tensors, `to(device)`): lex_child (n_nodes, C) / lex_word (n_nodes) int32, uni_logp (n_words + 1) f32, st_bo (n_states) f32,
    st_shorter (n_states) int32, arc_keys (slots) int64 + arc_logp (slots) f32 + arc_next (slots) int32; arc_probe = the longest probe sequence."""
    MAX_WORDS = 1 << 21
    MAX_ORDER = 6

    def __init__(self, words, ngrams, chars, order=None, min_slots=0):
        words = [str(w) for w in words]
        n = len(words)
        if n + 1 > self.MAX_WORDS:
            raise ValueError('WordStateLM: %d words (< 2^21)' % n)
        if len(set(words)) != n or any(not w or any(c == ' ' or c not in chars for c in w) for w in words):
            raise ValueError('WordStateLM: the words must be distinct, non-empty and spelled with the labels %r without the space' % (chars,))
        self.words, self.chars, self.min_slots = words, str(chars), int(min_slots)
        self.ngrams = {tuple(int(w) for w in g): (np.float32(v[0]), np.float32(v[1])) for g, v in ngrams.items()}
        longest = max((len(g) for g in self.ngrams), default=0)
        self._order = max(2, longest) if order is None else int(order)
        if not (1 <= longest <= self._order <= self.MAX_ORDER):
            raise ValueError('WordStateLM: n-grams of 1 .. %d words and order %d (at most %d)' % (longest, self._order, self.MAX_ORDER))
        if any(not g or not (0 <= g[0] <= n) or any(not (0 <= w < n) for w in g[1:]) for g in self.ngrams):
            raise ValueError('WordStateLM: n-gram word ids must be below %d (the start context %d only leads)' % (n, n))
        if any((w,) not in self.ngrams for w in range(n + 1)):
            raise ValueError('WordStateLM: every unigram, the start context %d included, must be present' % n)
        for g in self.ngrams:
            if len(g) > 1 and g[:-1] not in self.ngrams:
                raise ValueError('WordStateLM: the model is not prefix-closed: the context of the n-gram %r is no n-gram' % (g,))
        self.lex_child, self.lex_word = _lexicon_trie(words, self.chars)
        # states: the empty context, the unigrams, then the n-grams of 2 .. order - 1 words by increasing length
        contexts = [()] + [(w,) for w in range(n + 1)] + sorted((g for g in self.ngrams if 2 <= len(g) < self._order), key=lambda g: (len(g), g))
        self._state = {c: s for s, c in enumerate(contexts)}
        self._contexts = contexts
        bo = np.asarray([0.0] + [self.ngrams[c][1] for c in contexts[1:]], dtype=np.float32)
        shorter = np.asarray([0] + [self.state_of(c[1:]) for c in contexts[1:]], dtype=np.int32)
        # arcs: one hash table for the n-grams of >= 2 words
        arcs = sorted(g for g in self.ngrams if len(g) >= 2)
        keys = np.asarray([(self._state[g[:-1]] << 21) | g[-1] for g in arcs], dtype=np.uint64)
        tab, val, self.arc_probe = _ngram_table(keys, [self.ngrams[g][0] for g in arcs], 1, min_slots)
        nxt = np.zeros(tab.shape[0], dtype=np.int32)
        slot = {int(k): i for i, k in enumerate(tab.tolist()) if k != int(_NGRAM_EMPTY)}
        for g, k in zip(arcs, keys.tolist()):
            nxt[slot[k]] = self.state_of(g)
        self._arcs = {(self._state[g[:-1]], g[-1]): (self.ngrams[g][0], self.state_of(g)) for g in arcs}
        self._bo, self._shorter = bo, shorter
        self.uni_logp = torch.from_numpy(np.asarray([self.ngrams[(w,)][0] for w in range(n + 1)], dtype=np.float32))
        self.st_bo, self.st_shorter = torch.from_numpy(bo), torch.from_numpy(shorter)
        self.arc_keys, self.arc_logp, self.arc_next = torch.from_numpy(tab.view(np.int64)), torch.from_numpy(val.reshape(-1)), torch.from_numpy(nxt)

    _DEVICE_FORM = ('lex_child', 'lex_word', 'uni_logp', 'st_bo', 'st_shorter', 'arc_keys', 'arc_logp', 'arc_next')

    @property
    def n_words(self):
        return len(self.words)

    @property
    def start(self):
        return len(self.words)

    @property
    def start_state(self):
        return 1 + len(self.words)

    @property
    def order(self):
        return self._order

    @property
    def n_states(self):
        return len(self._contexts)

    def to(self, device):
        """The same model with its tables on `device` (the host form is shared, not copied)."""
        other = object.__new__(WordStateLM)
        other.__dict__.update(self.__dict__)
        for name in self._DEVICE_FORM:
            setattr(other, name, getattr(self, name).to(device))
        return other

    def state_of(self, context_words):
        """The state of the longest suffix of the word ids `context_words` (oldest first, at most order - 1 of them count) that is a state."""
        c = tuple(int(w) for w in context_words)
        c = c[max(0, len(c) - (self._order - 1)):]
        while c not in self._state:
            c = c[1:]
        return self._state[c]

    def context_of(self, state):
        """The word ids of a state's context, oldest first."""
        return self._contexts[int(state)]

    def word_ids(self, text, text_transform):
        """Ids of the words of `text` after clean_text; raises KeyError on a word outside the vocabulary."""
        index = getattr(self, '_index', None)
        if index is None:
            index = self._index = {w: i for i, w in enumerate(self.words)}
        return [index[w] for w in text_transform.clean_text(text).split()]

    def score_words(self, word_ids, dtype=np.float64, context=()):
        """ln P of every word of a sentence given the words before it -- the state rule of ss_word_state_lm restated on the host dictionaries, in
        `dtype` arithmetic.  context: the word ids the sentence starts behind, oldest first; the default () is the sentence start (<s>), ids
        below 0 are "no word", so (-1,) is the empty context."""
        ctx = tuple(int(w) for w in context) if len(context) else (self.start,)
        ctx = tuple(w for w in ctx if w >= 0)
        if any(w > self.n_words for w in ctx):
            raise ValueError('score_words: word id outside the model')
        s = self.state_of(ctx)
        out = np.zeros(len(word_ids), dtype=dtype)
        for i, w in enumerate(word_ids):
            w = int(w)
            if not (0 <= w <= self.n_words):
                raise ValueError('score_words: word id outside the model')
            passed, at = [], s
            while at != 0 and (at, w) not in self._arcs:
                passed.append(at)
                at = int(self._shorter[at])
            p, s = (dtype(self.ngrams[(w,)][0]), 1 + w) if at == 0 else (dtype(self._arcs[(at, w)][0]), self._arcs[(at, w)][1])
            for q in reversed(passed):
                p = dtype(self._bo[q]) + p
            out[i] = p
        return out

    def score_states(self, pairs):
        """torch.ops.silent_speech.word_state_score on this model's tables: (ln P(word | state), the state after the word) of (n, 2) int32 rows
        (state, word) on the tables' device."""
        return torch.ops.silent_speech.word_state_score(pairs, self.uni_logp, self.st_bo, self.st_shorter, self.arc_keys, self.arc_logp, self.arc_next,
                                                        self.arc_probe, self._order)

    # ---- builders
    @classmethod
    def from_ngram_lm(cls, lm):
        """The same model as a WordNgramLM, order 3 whatever it holds: every bigram is a state with its stored backoff, as the table search assumes."""
        grams = {(w,): tuple(lm.unigrams[w]) for w in range(lm.n_words + 1)}
        grams.update(lm.bigrams)
        grams.update({g: (p, 0.0) for g, p in lm.trigrams.items()})
        return cls(lm.words, grams, lm.chars, 3, lm.min_slots)

    @classmethod
    def from_arpa(cls, path_or_file, text_transform, min_slots=0):
        """Reads ARPA text (\\data\\, \\1-grams: .. \\6-grams:, \\end\\; log10 values, a missing backoff = 0) with the rules of
        WordNgramLM.from_arpa: <s> is the start context; </s> and <unk> are read and never predicted; a word whose clean_text spelling is empty,
        holds a space or a character outside text_transform.chars is dropped with every n-gram holding it; of two words with one cleaned
        spelling the one with the larger unigram probability keeps it.  Order > 6: ValueError."""
        grams = _read_arpa(path_or_file, cls.MAX_ORDER, 'WordStateLM')
        words, ids = _arpa_vocabulary(grams[1], text_transform)
        out = {(w,): (0.0, 0.0) for w in range(len(words) + 1)}
        out[(len(words),)] = (-99.0 * _LN10, 0.0)
        for k in range(1, cls.MAX_ORDER + 1):
            for g, lp, bo in grams[k]:
                if all(w in ids for w in g) and '<s>' not in g[1:]:
                    out[tuple(ids[w] for w in g)] = (lp, bo)
        return cls(words, out, text_transform.chars, None, min_slots)

    @classmethod
    def from_texts(cls, texts, text_transform, order=3, discount=0.75, add_k=0.1, min_slots=0):
        """WordNgramLM.from_texts for any order up to 6 (for order <= 3 the same f32 numbers): unigrams add-k over the vocabulary, every higher
        level absolute discounting, P(w | h) = (c(h w) - discount) / c(h .), the backoff weight of every seen context giving the rest to the
        next lower level so that the probabilities over the vocabulary sum to 1."""
        if order not in range(1, cls.MAX_ORDER + 1) or not (0 < discount < 1) or not add_k > 0:
            raise ValueError('WordStateLM.from_texts: order 1 .. %d, 0 < discount < 1 and add_k > 0' % cls.MAX_ORDER)
        chars = text_transform.chars
        sents = [[w if all(c in chars for c in w) else None for w in text_transform.clean_text(t).split()] for t in texts]
        words = sorted({w for s in sents for w in s if w is not None})
        n = len(words)
        ids = {w: i for i, w in enumerate(words)}
        c1, counts = np.zeros(n, dtype=np.float64), {k: {} for k in range(2, order + 1)}
        for s in sents:
            seq = [n] + [ids[w] if w is not None else None for w in s]
            for i in range(1, len(seq)):
                if seq[i] is None:
                    continue
                c1[seq[i]] += 1
                for k in range(2, order + 1):                                 # the k-gram that ends here, while it stays inside the line and its words are spelled
                    if i - k + 1 < 0 or seq[i - k + 1] is None:
                        break
                    g = tuple(seq[i - k + 1:i + 1])
                    counts[k][g] = counts[k].get(g, 0) + 1
        p1 = (c1 + add_k) / (c1.sum() + add_k * max(n, 1))
        P, BO = {}, {}                                                       # P[k]: the seen k-grams, BO[k]: ln backoff of the seen contexts of k words

        def prob(k, h, w):
            """P(w | the k - 1 words h) through level k and below"""
            if k == 1:
                return p1[w]
            if h in P[k] and w in P[k][h]:
                return P[k][h][w]
            return float(np.exp(BO[k - 1].get(h, 0.0))) * prob(k - 1, h[1:], w)
        for k in range(2, order + 1):
            P[k], BO[k - 1] = _discounted(counts[k], lambda h, w, k=k: prob(k - 1, h[1:], w), n, discount)
        BO[order] = {}
        grams = {(w,): (float(np.log(p1[w])), BO[1].get((w,), 0.0)) for w in range(n)}
        grams[(n,)] = (-99.0 * _LN10, BO[1].get((n,), 0.0))
        for k in range(2, order + 1):
            grams.update({h + (w,): (float(np.log(p)), BO[k].get(h + (w,), 0.0)) for h, ps in P[k].items() for w, p in ps.items()})
        return cls(words, grams, chars, order, min_slots)

    def write_arpa(self, path):
        """ARPA text of the model (log10 values; the words as their cleaned spellings), readable by from_arpa and by other n-gram tools."""
        name = self.words + ['<s>']
        by = {}
        for g in sorted(self.ngrams):
            by.setdefault(len(g), []).append(g)
        with open(path, 'w') as f:
            f.write('\\data\\\n' + ''.join('ngram %d=%d\n' % (k, len(by[k])) for k in sorted(by)))
            for k in sorted(by):
                f.write('\n\\%d-grams:\n' % k)
                for g in by[k]:
                    lp, bo = self.ngrams[g]
                    f.write('%.9g\t%s' % (float(lp) / _LN10, ' '.join(name[w] for w in g)) + ('\t%.9g\n' % (float(bo) / _LN10) if k < self._order else '\n'))
            f.write('\n\\end\\\n')

    def save(self, path):
        by = {}
        for g in sorted(self.ngrams):
            by.setdefault(len(g), []).append(g)
        arrays = {}
        for k, gs in by.items():
            arrays['ids_%d' % k] = np.asarray(gs, dtype=np.int32).reshape(len(gs), k)
            arrays['val_%d' % k] = np.asarray([self.ngrams[g] for g in gs], dtype=np.float32).reshape(len(gs), 2)
        with open(path, 'wb') as f:
            np.savez(f, words=np.asarray(self.words, dtype=np.str_), chars=np.asarray(self.chars), order=np.asarray(self._order),
                     min_slots=np.asarray(self.min_slots), **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            grams = {}
            for k in range(1, cls.MAX_ORDER + 1):
                if 'ids_%d' % k in z:
                    grams.update({tuple(g): tuple(v) for g, v in zip(z['ids_%d' % k].tolist(), z['val_%d' % k])})
            return cls([str(w) for w in z['words']], grams, str(z['chars']), int(z['order']), int(z['min_slots']))


def _beam_search(head, V, blank, first, frames, beam_width, n_best, lm, alpha, beta, space=None):
    """One table upload, lse + search launches, one read-back.  head: (M, ld) f32 on the device; first / frames: per utterance, host ints.
    A WordNgramLM or a WordStateLM selects the lexicon-constrained search of its kernel (space: the class that ends a word, default V - 2)."""
    n = len(frames)
    if n == 0:
        return []
    utt, = staging.upload([np.stack([np.asarray(first, dtype=np.int64), np.asarray(frames, dtype=np.int64)], 1)], head.device)
    max_len = max(max(frames), 1)
    if isinstance(lm, WordNgramLM):
        if len(lm.chars) != V - 1:
            raise ValueError('beam search: the WordNgramLM spells with %d labels, the logits have %d classes' % (len(lm.chars), V))
        space = V - 2 if space is None else int(space)
        lm = lm.to(head.device)
        labels, lengths, scores, _, _ = torch.ops.silent_speech.ctc_word_beam_search(
            head, utt, V, blank, space, int(sum(frames)), max_len, int(beam_width), int(n_best), lm.lex_child, lm.lex_word, lm.uni, lm.bi_keys, lm.bi_val,
            lm.tri_keys, lm.tri_val, lm.n_words, lm.start, lm.bi_probe, lm.tri_probe, float(alpha), float(beta))
    elif isinstance(lm, WordStateLM):
        if len(lm.chars) != V - 1:
            raise ValueError('beam search: the WordStateLM spells with %d labels, the logits have %d classes' % (len(lm.chars), V))
        space = V - 2 if space is None else int(space)
        lm = lm.to(head.device)
        labels, lengths, scores, _, _ = torch.ops.silent_speech.ctc_word_state_beam_search(
            head, utt, V, blank, space, int(sum(frames)), max_len, int(beam_width), int(n_best), lm.lex_child, lm.lex_word, lm.uni_logp, lm.st_bo, lm.st_shorter,
            lm.arc_keys, lm.arc_logp, lm.arc_next, lm.n_words, lm.start_state, lm.arc_probe, lm.order, float(alpha), float(beta))
    else:
        if lm is not None:
            lm = (lm.table if isinstance(lm, LabelNgramLM) else torch.as_tensor(lm, dtype=torch.float32)).to(head.device).contiguous()
        labels, lengths, scores, _ = torch.ops.silent_speech.ctc_beam_search(head, utt, V, blank, int(sum(frames)), max_len, int(beam_width), int(n_best),
                                                                             lm, float(alpha), float(beta))
    back = torch.cat([labels.reshape(n, n_best * max_len), lengths, scores.view(torch.int32)], 1).cpu().numpy()       # ONE read-back
    labels, lengths = back[:, :n_best * max_len].reshape(n, n_best, max_len), back[:, n_best * max_len:n_best * max_len + n_best]
    scores = np.ascontiguousarray(back[:, n_best * max_len + n_best:]).view(np.float32)
    if n_best == 1:
        return [labels[b, 0, :max(lengths[b, 0], 0)].tolist() for b in range(n)]
    return [[(labels[b, r, :lengths[b, r]].tolist(), float(scores[b, r])) for r in range(n_best) if lengths[b, r] >= 0] for b in range(n)]


def beam_decode(pred, lengths, blank=None, *, beam_width=100, n_best=1, lm=None, alpha=0.0, beta=0.0, space=None):
    """CTC prefix beam search of packed logits (rows, T, V) (NOT log-softmaxed), utterances back to back with `lengths` frames each, in one
    launch on the device; lm: a LabelNgramLM (or its table) fused as alpha * ln P(label | two labels before) + beta per label, or a WordNgramLM / WordStateLM:
    the search is then confined to the spellings of its vocabulary and adds alpha * ln P(word | two words before) + beta per word; space = the
    class that ends a word (default V - 2, where TextTransform puts it; pass text_transform.chars.index(' ')).
    Returns a list of int lists, or for n_best > 1 a list of [(ints, score), ...] lists, best first (fewer than n_best if fewer prefixes exist;
    with a WordNgramLM the strings that end at a word boundary or on a word come first)."""
    B, T, V = pred.shape
    blank = V - 1 if blank is None else int(blank)
    logits = pred.reshape(B * T, V).float().contiguous()
    frames = [int(n) for n in lengths]
    if sum(frames) > B * T or any(n < 0 for n in frames):
        raise ValueError('beam_decode: the lengths do not fit the %d packed frames' % (B * T))
    first = np.concatenate([[0], np.cumsum(frames)])[:-1] if frames else []
    return _beam_search(logits, V, blank, first, frames, beam_width, n_best, lm, alpha, beta, space)


def beam_decode_utterances(logits, *, beam_width=100, n_best=1, lm=None, alpha=0.0, beta=0.0, space=None):
    """beam_decode for the per-utterance logits Model.forward_utterances returns -- (T_b, V) views of ONE (B T_max, >= V) head buffer --: the
    search reads the slots in place (first frame b T_max, T_b frames; filler rows and columns are never looked at).  blank = V - 1."""
    if not logits:
        return []
    head, V = logits[0]._base, logits[0].shape[1]
    B, T = len(logits), max(int(y.shape[0]) for y in logits)
    if head is None or head.dim() != 2 or head.dtype != torch.float32 or not head.is_contiguous() or head.shape[0] != B * T or \
            any(y._base is not head or y.shape[1] != V or y.storage_offset() != b * T * head.shape[1] for b, y in enumerate(logits)):
        raise ValueError('beam_decode_utterances takes the list Model.forward_utterances returned')
    return _beam_search(head, V, V - 1, [b * T for b in range(B)], [int(y.shape[0]) for y in logits], beam_width, n_best, lm, alpha, beta, space)


Alignment = collections.namedtuple('Alignment', ['score', 'frames', 'token_first', 'token_frames', 'token_logp'])
Alignment.__doc__ = """Best alignment of one utterance's label string to its frames (ss_ctc_align in include/silent_speech_hip.h): score (float, natural log;
-inf = no alignment exists), frames (T,) int32 = index of the token a frame belongs to, -1 for blank (all -2 without an alignment), and per token its
first frame, its frame count and the sum of the log-probabilities of its frames ((S,) int32, int32, float32; -1 / 0 / 0 without an alignment)."""
MAX_ALIGN_TARGET = 511
FRAME_SECONDS = 256 / 22050          # one output frame of the model = 8 raw samples at 689.06 Hz = the mel hop


def _forced_align(name, head, V, blank, topology, first, frames, targets):
    """One table upload, lse + alignment launches, one read-back.  head: (M, ld) f32 on the device; first / frames: per utterance, host ints."""
    if topology not in ('ctc', 'linear'):
        raise ValueError("%s: topology is 'ctc' or 'linear'" % name)
    n = len(frames)
    if len(targets) != n:
        raise ValueError('%s: %d target strings for %d utterances' % (name, len(targets), n))
    ys = [np.asarray(y.detach().cpu() if isinstance(y, torch.Tensor) else y, dtype=np.int64).reshape(-1) for y in targets]
    blank = -1 if topology == 'linear' else int(blank)
    if topology == 'ctc' and not (0 <= blank < V):
        raise ValueError('%s: blank %d is not one of the %d classes' % (name, blank, V))
    for b, y in enumerate(ys):
        if y.size > MAX_ALIGN_TARGET:
            raise ValueError('%s: target %d has %d labels (at most %d)' % (name, b, y.size, MAX_ALIGN_TARGET))
        if y.size and (y.min() < 0 or y.max() >= V or (y == blank).any()):
            raise ValueError('%s: target %d has a label outside [0, %d) or equal to the blank %d' % (name, b, V, blank))
    if n == 0:
        return []
    S = [int(y.size) for y in ys]
    tfirst = np.concatenate([[0], np.cumsum(S)])[:-1]
    table = np.stack([np.asarray(first, dtype=np.int64), np.asarray(frames, dtype=np.int64), tfirst.astype(np.int64), np.asarray(S, dtype=np.int64)], 1)
    flat = np.concatenate(ys + [np.zeros(1, dtype=np.int64)]).astype(np.int32)          # one spare entry: never an empty upload
    utt, tg = staging.upload([table, flat], head.device)
    score, frame_token, token_first, token_frames, token_logp = torch.ops.silent_speech.ctc_forced_align(
        head, utt, tg, V, blank, int(sum(frames)), max(S))
    back = torch.cat([score.view(torch.int32), frame_token, token_first, token_frames, token_logp.view(torch.int32)]).cpu().numpy()       # ONE read-back
    M, nt = frame_token.shape[0], flat.shape[0]
    score, frame_token = back[:n].view(np.float32), back[n:n + M]
    token_first, token_frames, token_logp = back[n + M:n + M + nt], back[n + M + nt:n + M + 2 * nt], back[n + M + 2 * nt:].view(np.float32)
    return [Alignment(float(score[b]), frame_token[first[b]:first[b] + frames[b]].copy(), token_first[tfirst[b]:tfirst[b] + S[b]].copy(),
                      token_frames[tfirst[b]:tfirst[b] + S[b]].copy(), token_logp[tfirst[b]:tfirst[b] + S[b]].copy()) for b in range(n)]


def forced_align(pred, lengths, targets, blank=None, *, topology='ctc'):
    """Best (Viterbi) alignment of known label strings to packed logits (rows, T, V) (NOT log-softmaxed), utterances back to back with `lengths`
    frames each, in one launch on the device.  targets: a list of int lists or tensors, one per utterance; blank defaults to V - 1.
    topology='linear' aligns without a blank (heads that have none, such as the transduction model's phoneme head): every frame belongs to a token.
    Returns a list of Alignment; an utterance no alignment exists for (too few frames, repeated labels without room for the blank between them)
    has score -inf.  Raises ValueError for lengths that do not fit, a target longer than 511 or a label outside [0, V) or equal to the blank."""
    B, T, V = pred.shape
    blank = V - 1 if blank is None else int(blank)
    frames = [int(n) for n in lengths]
    if sum(frames) > B * T or any(n < 0 for n in frames):
        raise ValueError('forced_align: the lengths do not fit the %d packed frames' % (B * T))
    first = [int(f) for f in np.concatenate([[0], np.cumsum(frames)])[:-1]] if frames else []
    if topology not in ('ctc', 'linear'):
        raise ValueError("forced_align: topology is 'ctc' or 'linear'")
    return _forced_align('forced_align', pred.reshape(B * T, V).float().contiguous(), V, blank, topology, first, frames, targets)


def forced_align_utterances(logits, targets, *, topology='ctc'):
    """forced_align for the per-utterance logits Model.forward_utterances returns -- (T_b, V) views of ONE (B T_max, >= V) head buffer --: the
    slots are read in place (first frame b T_max, T_b frames; filler rows and columns are never looked at).  blank = V - 1."""
    if not logits:
        return []
    head, V = logits[0]._base, logits[0].shape[1]
    B, T = len(logits), max(int(y.shape[0]) for y in logits)
    if head is None or head.dim() != 2 or head.dtype != torch.float32 or not head.is_contiguous() or head.shape[0] != B * T or \
            any(y._base is not head or y.shape[1] != V or y.storage_offset() != b * T * head.shape[1] for b, y in enumerate(logits)):
        raise ValueError('forced_align_utterances takes the list Model.forward_utterances returned')
    return _forced_align('forced_align_utterances', head, V, V - 1, topology, [b * T for b in range(B)], [int(y.shape[0]) for y in logits], targets)


def word_segments(alignment, text_int, text_transform, frame_seconds=FRAME_SECONDS):
    """Word time stamps of an Alignment of the character string text_int: a list of (word, start_s, end_s, confidence).  A word is a maximal run
    of non-space characters; it starts at the first frame of its first character and ends behind the last frame of its last character (blanks
    between its characters are inside it; spaces and the blanks around them belong to no word); confidence = exp(sum of its characters'
    token_logp / sum of their frames), the geometric mean of the frame posteriors along the path.  No alignment (score -inf): []."""
    ints = [int(c) for c in (text_int.tolist() if hasattr(text_int, 'tolist') else text_int)]
    if not alignment.score > -np.inf:
        return []
    if len(ints) != len(alignment.token_first):
        raise ValueError('word_segments: %d characters, but the alignment has %d tokens' % (len(ints), len(alignment.token_first)))
    space = text_transform.chars.index(' ')
    words, run = [], []
    for k, c in enumerate(ints + [space]):
        if c != space:
            run.append(k)
        elif run:
            a, z = run[0], run[-1]
            logp = float(np.sum(alignment.token_logp[a:z + 1], dtype=np.float64))
            nfr = int(np.sum(alignment.token_frames[a:z + 1]))
            words.append((text_transform.int_to_text(ints[a:z + 1]), int(alignment.token_first[a]) * frame_seconds,
                          int(alignment.token_first[z] + alignment.token_frames[z]) * frame_seconds, float(np.exp(logp / max(nfr, 1)))))
            run = []
    return words


def align(model, testset, device, *, batch_size=8):
    """Word time stamps of every example of testset against its own transcript: eval-mode Model.forward_utterances in groups of batch_size whole
    utterances, forced_align_utterances against each example's text_int, word_segments per utterance.  Returns one list of
    (word, start_s, end_s, confidence) per example ([] where the transcript does not fit the utterance's frames)."""
    model.eval()
    tt = testset.text_transform
    out = []
    with torch.no_grad():
        for first in range(0, len(testset), batch_size):
            group = [testset[i] for i in range(first, min(first + batch_size, len(testset)))]
            logits = model.forward_utterances([ex['raw_emg'].to(dtype=torch.float32) for ex in group])
            texts = [torch.as_tensor(ex['text_int']).tolist() for ex in group]
            for al, text in zip(forced_align_utterances(logits, texts), texts):
                out.append(word_segments(al, text, tt))
    model.train()
    return out


MAX_NBEST_LABELS = 511


class _NbestPlan(object):
    """The tables of ss_ctc_nbest_logp (include/silent_speech_hip.h) for one list of label strings per utterance, as host arrays: utt (n, 4) =
    first frame, frames, first hypothesis, K; hyp (H, 3) = first label, S, workspace offset; the flat labels (one spare entry: never an empty
    upload).  Hypotheses are numbered utterance by utterance, in list order."""

    def __init__(self, who, first, frames, hyps, V, blank):
        if len(hyps) != len(frames):
            raise ValueError('%s: %d lists for %d utterances' % (who, len(hyps), len(frames)))
        if not (0 <= blank < V):
            raise ValueError('%s: blank %d is not one of the %d classes' % (who, blank, V))
        utt, hyp, flat, ws, at = [], [], [], 0, 0
        for u, (f0, T, lst) in enumerate(zip(first, frames, hyps)):
            lst = [np.asarray(y.detach().cpu() if isinstance(y, torch.Tensor) else y, dtype=np.int64).reshape(-1) for y in lst]
            utt.append((int(f0), int(T), len(hyp), len(lst)))
            for y in lst:
                if y.size > MAX_NBEST_LABELS:
                    raise ValueError('%s: a hypothesis of utterance %d has %d labels (at most %d)' % (who, u, y.size, MAX_NBEST_LABELS))
                if y.size and (y.min() < 0 or y.max() >= V or (y == blank).any()):
                    raise ValueError('%s: a hypothesis of utterance %d has a label outside [0, %d) or equal to the blank %d' % (who, u, V, blank))
                hyp.append((at, y.size, ws))
                flat.append(y)
                at += y.size
                ws += int(T) * (2 * y.size + 1)
        self.n, self.n_hyp, self.ws_floats = len(utt), len(hyp), ws
        self.max_s = max([h[1] for h in hyp] or [0])
        self.sizes = [k for _, _, _, k in utt]
        self.utt = np.asarray(utt, dtype=np.int64).reshape(len(utt), 4)
        self.hyp = np.asarray(hyp, dtype=np.int64).reshape(len(hyp), 3)
        self.flat = np.concatenate(flat + [np.zeros(1, dtype=np.int64)]).astype(np.int32)

    def arrays(self):
        """What goes up (never an empty array: one spare row each)"""
        return [self.utt if self.n else np.zeros((1, 4), np.int64), self.hyp if self.n_hyp else np.zeros((1, 3), np.int64), self.flat]

    def bind(self, utt, hyp, targets):
        self.utt_dev, self.hyp_dev, self.targets = utt[:self.n], hyp[:self.n_hyp], targets
        return self


def _nbest_logp(who, head, V, blank, first, frames, hyps, return_plan):
    plan = _NbestPlan(who, first, frames, hyps, V, blank)
    plan.bind(*staging.upload(plan.arrays(), head.device))                # ONE pinned copy, as _CtcPlan
    logp, _, _ = torch.ops.silent_speech.ctc_nbest_logp(head, plan.utt_dev, plan.hyp_dev, plan.targets, plan.max_s, plan.ws_floats, V, blank)
    return (logp, plan) if return_plan else logp


def _packed_frames(who, pred, lengths):
    B, T, V = pred.shape
    frames = [int(n) for n in lengths]
    if sum(frames) > B * T or any(n < 0 for n in frames):
        raise ValueError('%s: the lengths do not fit the %d packed frames' % (who, B * T))
    first = [int(f) for f in np.concatenate([[0], np.cumsum(frames)])[:-1]] if frames else []
    return first, frames


def nbest_logp(pred, lengths, hyps, blank=None, *, return_plan=False):
    """Full-sum CTC log-likelihood ln P(h | utterance) of ARBITRARY label strings, several per utterance on the same frames (csrc/ctc.hip,
    ss_ctc_nbest_logp: the alpha / beta kernel of ctc_loss, one workgroup pair per hypothesis).  pred: (rows, T, V) raw model outputs (NOT
    log-softmaxed), utterances back to back with `lengths` frames each; hyps: one list of int sequences (lists or tensors, at most 511 labels,
    never the blank) per utterance, possibly empty.  Returns a 1-D f32 tensor of sum K_u values in utterance-then-list order, attached to
    autograd (-inf where no alignment exists; such entries get no gradient).  blank defaults to V - 1."""
    B, T, V = pred.shape
    blank = V - 1 if blank is None else int(blank)
    first, frames = _packed_frames('nbest_logp', pred, lengths)
    return _nbest_logp('nbest_logp', pred.reshape(B * T, V).float().contiguous(), V, blank, first, frames, list(hyps), return_plan)


def nbest_logp_utterances(logits, hyps, *, return_plan=False):
    """nbest_logp for the per-utterance logits Model.forward_utterances returns -- (T_b, V) views of ONE (B T_max, >= V) head buffer --: the slots
    are read in place (first frame b T_max, T_b frames; filler rows and columns are never looked at, and get a zero gradient).  blank = V - 1."""
    if not logits:
        return torch.zeros(0, dtype=torch.float32)
    head, V = logits[0]._base, logits[0].shape[1]
    B, T = len(logits), max(int(y.shape[0]) for y in logits)
    if head is None or head.dim() != 2 or head.dtype != torch.float32 or not head.is_contiguous() or head.shape[0] != B * T or \
            any(y._base is not head or y.shape[1] != V or y.storage_offset() != b * T * head.shape[1] for b, y in enumerate(logits)):
        raise ValueError('nbest_logp_utterances takes the list Model.forward_utterances returned')
    return _nbest_logp('nbest_logp_utterances', head, V, V - 1, [b * T for b in range(B)], [int(y.shape[0]) for y in logits], list(hyps), return_plan)


def rescore_nbest(pred, lengths, nbest, blank=None):
    """The n-best lists of beam_decode(.., n_best=K) with every score replaced by the full-sum CTC log-likelihood of its string (the beam's own
    score is the mass of the paths that survived pruning): the exact weights for mbr_rerank.  No gradient.  Returns lists of (ints, logp)."""
    nbest = [list(h) for h in nbest]
    with torch.no_grad():
        logp = nbest_logp(pred.detach(), lengths, [[ints for ints, _ in h] for h in nbest], blank).cpu().numpy()
    out, at = [], 0
    for h in nbest:
        out.append([(list(ints), float(logp[at + k])) for k, (ints, _) in enumerate(h)])
        at += len(h)
    return out


def mwer_loss(pred, example, *, space, blank=None, n_best=4, beam_width=16, lm=None, alpha=0.0, beta=0.0, unit='word', scale=1.0, ctc_weight=0.01,
              add_reference=False, nbest=None, return_details=False):
    """Minimum expected word error over the model's own n-best lists (ss_nbest_expected_risk in include/silent_speech_hip.h states the risk):
        sum_k post_k (cost_k - mean cost) per utterance, post = softmax(scale * full-sum log-likelihood) over the list, cost = the word
        (unit='char': label) errors S + D + I of the hypothesis against example['text_int'], averaged over the utterances with a feasible
        hypothesis, + ctc_weight * ctc_loss(pred, example).
    The lists are decoded with beam_decode(n_best=, beam_width=, lm=, alpha=, beta=) from the DETACHED logits (one read-back of labels and lengths)
    unless nbest= supplies them ([(ints, score), ...] per utterance); they are not differentiated through (a decoded string of more than 511 labels is left out of its list).  add_reference=True appends the reference
    string to a list that does not hold it.  Words are the runs of labels between `space` labels, interned on the host; then one edit-distance launch
    over all (reference, hypothesis) pairs, one ctc_nbest_logp, one nbest_expected_risk (and ctc_loss when ctc_weight != 0), costs and
    likelihoods staying on the device.  Returns the 0-dim loss, attached to autograd; with return_details=True also a dict: 'nbest' (the lists
    used), 'logp', 'post', 'cost' (flat, utterance-then-list order), 'sizes' (K per utterance) and 'risk' (f64 per utterance, NaN where no
    hypothesis is feasible)."""
    B, T, V = pred.shape
    blank = V - 1 if blank is None else int(blank)
    space = int(space)
    first, frames = _packed_frames('mwer_loss', pred, example['lengths'])
    refs = [[int(c) for c in torch.as_tensor(y).reshape(-1).tolist()] for y in example['text_int']]
    if len(refs) != len(frames):
        raise ValueError('mwer_loss: %d transcripts for %d utterances' % (len(refs), len(frames)))
    if nbest is None:
        with torch.no_grad():
            nbest = beam_decode(pred.detach(), frames, blank, beam_width=beam_width, n_best=n_best, lm=lm, alpha=alpha, beta=beta,
                                space=space if isinstance(lm, (WordNgramLM, WordStateLM)) else None)
        if n_best == 1:
            nbest = [[(ints, float('nan'))] for ints in nbest]
        nbest = [[(ints, score) for ints, score in h if len(ints) <= MAX_NBEST_LABELS] for h in nbest]      # longer than the kernel scores: left out of the list
    nbest = [[(list(ints), float(score)) for ints, score in h] for h in nbest]
    if len(nbest) != len(frames):
        raise ValueError('mwer_loss: %d n-best lists for %d utterances' % (len(nbest), len(frames)))
    if add_reference:
        for ref, h in zip(refs, nbest):
            if all(ints != ref for ints, _ in h):
                h.append((list(ref), float('nan')))
    if any(len(h) > MAX_NBEST for h in nbest):
        raise ValueError('mwer_loss: more than %d hypotheses for one utterance' % MAX_NBEST)
    logits = pred.reshape(B * T, V).float().contiguous()
    plan = _NbestPlan('mwer_loss', first, frames, [[ints for ints, _ in h] for h in nbest], V, blank)
    table, pairs = _TokenTable('mwer_loss'), []
    for ref, h in zip(refs, nbest):
        r = table.add(_label_units(ref, space, unit, 'mwer_loss'))
        pairs.extend((r, table.add(_label_units(ints, space, unit, 'mwer_loss'))) for ints, _ in h)
    flat, seqs = table.arrays()
    groups = plan.utt[:, 2:].copy() if plan.n else np.zeros((0, 2), np.int64)
    up = staging.upload(plan.arrays() + [flat, seqs if len(seqs) else np.zeros((1, 2), np.int64),
                                         np.asarray(pairs if pairs else [(0, 0)], dtype=np.int32).reshape(-1, 2),
                                         groups if len(groups) else np.zeros((1, 2), np.int64)], logits.device)            # ONE pinned copy
    plan.bind(*up[:3])
    tokens, seqs_d, pairs_d, groups_d = up[3], up[4][:len(seqs)], up[5][:len(pairs)], up[6][:len(groups)]
    dist, _, _, _ = torch.ops.silent_speech.edit_distance(tokens, seqs_d, pairs_d, False)
    cost = dist.to(torch.float32)
    logp, _, _ = torch.ops.silent_speech.ctc_nbest_logp(logits, plan.utt_dev, plan.hyp_dev, plan.targets, plan.max_s, plan.ws_floats, V, blank)
    risk_loss, risk, post, _ = torch.ops.silent_speech.nbest_expected_risk(logp, cost, groups_d, float(scale))
    loss = risk_loss[0]
    if ctc_weight != 0:
        loss = loss + float(ctc_weight) * ctc_loss(pred, example, blank)
    if not return_details:
        return loss
    return loss, {'nbest': nbest, 'logp': logp.detach(), 'post': post.detach(), 'cost': cost, 'sizes': plan.sizes, 'risk': risk.detach()}


def test(model, testset, device, *, batch_size=1, whole_utterances=False, decoder='greedy', beam_width=100, lm=None, alpha=0.0, beta=0.0,
         mbr=None, mbr_scale=1.0, details=False):
    """:30-58.  Default (batch_size=1) = the reference: eval-mode forward of ONE WHOLE utterance at a time (:37-43), so the convolutions
    and the +-99-frame attention band span the utterance (the banded attention kernels take any T).  batch_size > 1 packs the utterances
    into 200-frame rows like training does -- faster, but context is cut at the row boundaries, so its WER is not the reference's number.
    whole_utterances=True with batch_size > 1: groups of up to batch_size WHOLE utterances go through Model.forward_utterances (one ragged-batch
    plan call per group, every utterance computed as it is alone) and one arg-max launch + one read-back per group: the function of the
    default, at batched speed.
    decoder='greedy' (default): best-path decoding.  decoder='beam': the prefix beam search of beam_decode / beam_decode_utterances with
    beam_width, and lm / alpha / beta if a LabelNgramLM, a WordNgramLM or a WordStateLM is given, in all three branches.  With a word model (the reference's
    setting is alpha=1.5, beta=1.85) every predicted word is a word of its lexicon; ONE language model at a time: a LabelNgramLM and a
    WordNgramLM together (lm given as a list or tuple) raise ValueError.
    mbr=K (with decoder='beam', 2 <= K <= 128): the search returns its K best and the scored prediction is their minimum-Bayes-risk choice under
    softmax(mbr_scale * score) (mbr_rerank).  details=True: the ErrorCounts of word_errors (hits, substitutions, deletions, insertions, the
    rate and every utterance's own counts) instead of the bare rate."""
    if decoder not in ('greedy', 'beam'):
        raise ValueError("test: decoder is 'greedy' or 'beam'")
    if mbr is not None and (decoder != 'beam' or not (2 <= int(mbr) <= MAX_NBEST)):
        raise ValueError("test: mbr=K needs decoder='beam' and 2 <= K <= %d" % MAX_NBEST)
    if isinstance(lm, (list, tuple)):
        raise ValueError('test: one language model at a time -- a LabelNgramLM and a WordNgramLM cannot be combined')
    model.eval()
    tt = testset.text_transform
    blank = len(tt.chars)
    if decoder == 'beam':
        lm = lm.to(device) if isinstance(lm, (LabelNgramLM, WordNgramLM, WordStateLM)) else lm   # the tables cross to the device once, not per utterance
        search = dict(beam_width=beam_width, lm=lm, alpha=alpha, beta=beta)
        if isinstance(lm, (WordNgramLM, WordStateLM)):
            search['space'] = tt.chars.index(' ')
        if mbr is not None:
            search['n_best'] = int(mbr)
            space = tt.chars.index(' ')

            def choose(lists):
                picks = mbr_rerank(lists, space=space, scale=mbr_scale, device=device)
                return [hyps[pick][0] if pick >= 0 else [] for hyps, (pick, _) in zip(lists, picks)]
        else:
            choose = lambda ints: ints
        decode = lambda pred, lengths: choose(beam_decode(pred, lengths, blank, **search))
        decode_utterances = lambda logits: choose(beam_decode_utterances(logits, **search))
    else:
        decode = lambda pred, lengths: greedy_decode(pred, lengths, blank)
        decode_utterances = greedy_decode_utterances
    references, predictions = [], []
    with torch.no_grad():
        if batch_size == 1:
            for i in range(len(testset)):
                ex = testset[i]
                X = ex['emg'].to(device=device, dtype=torch.float32).unsqueeze(0)
                X_raw = ex['raw_emg'].to(device=device, dtype=torch.float32).unsqueeze(0)
                sess = ex['session_ids'].to(device=device).unsqueeze(0)
                pred = model(X, X_raw, sess)                                   # (1, T, V) logits
                predictions.append(tt.int_to_text(decode(pred, [pred.shape[1]])[0]))
                references.append(tt.int_to_text(torch.as_tensor(ex['text_int']).tolist()))
        elif whole_utterances:
            for first in range(0, len(testset), batch_size):
                group = [testset[i] for i in range(first, min(first + batch_size, len(testset)))]
                logits = model.forward_utterances([ex['raw_emg'].to(dtype=torch.float32) for ex in group])
                for ints, ex in zip(decode_utterances(logits), group):
                    predictions.append(tt.int_to_text(ints))
                    references.append(tt.int_to_text(torch.as_tensor(ex['text_int']).tolist()))
        else:
            dataloader = torch.utils.data.DataLoader(testset, batch_size=batch_size, collate_fn=testset.collate_raw)
            for batch in dataloader:
                X, X_raw, sess = prepare_batch(batch, device, loss_plan=False)
                pred = model(X, X_raw, sess)
                for ints, tgt in zip(decode(pred, batch['lengths']), batch['text_int']):
                    predictions.append(tt.int_to_text(ints))
                    references.append(tt.int_to_text(tgt.tolist()))
    model.train()
    if details:
        return word_errors(references, predictions, device=device)
    return wer(references, predictions)


def train_model(trainset, devset, device, n_epochs=200, *, compute_dtype=torch.bfloat16, f32_matmul='exact', max_steps=None, mwer=None):
    """:61-117 on the MI355X: batches under a 128 000-sample budget, AdamW (lr 3e-4 in the reference's flags), linear
    warm-up, an optimiser step every SECOND batch (gradients accumulate in the flat .grad arena), MultiStepLR.
    mwer=dict(space=.., n_best=.., ...): the criterion is mwer_loss with these keywords (sequence-discriminative second stage, usually started
    from a CTC-trained model through the start_training_from flag) in place of ctc_loss; None (default): the step is the reference's."""
    dataloader = torch.utils.data.DataLoader(trainset, collate_fn=devset.collate_raw, num_workers=0, batch_sampler=SizeAwareSampler(trainset, 128000))
    n_chars = len(devset.text_transform.chars)
    model = Model(devset.num_features, n_chars + 1, compute_dtype=compute_dtype, f32_matmul=f32_matmul).to(device)
    # flag defaults of recognition_model.py:20-28 (they differ from the transduction trainer's)
    lr0, warmup, l2 = FLAGS.lookup('learning_rate', 3e-4), FLAGS.lookup('learning_rate_warmup', 1000), FLAGS.lookup('l2', 0.0)
    out_dir, start = FLAGS.lookup('output_directory', 'output'), FLAGS.lookup('start_training_from', None)
    if start is not None:
        model.load_state_dict(torch.load(start, map_location=torch.device(device)), strict=False)
    optim = FusedAdamW(model, lr=lr0, weight_decay=l2)
    lr_sched = torch.optim.lr_scheduler.MultiStepLR(optim, milestones=[125, 150, 175], gamma=.5)

    def set_lr(new_lr):
        for param_group in optim.param_groups:
            param_group['lr'] = new_lr

    target_lr = lr0

    def schedule_lr(iteration):
        iteration = iteration + 1
        if iteration <= warmup:
            set_lr(iteration * target_lr / warmup)

    batch_idx = 0
    optim.zero_grad()
    for epoch_idx in range(n_epochs):
        losses = []
        for batch in dataloader:
            schedule_lr(batch_idx)
            X, X_raw, sess = prepare_batch(batch, device, loss_plan=False)
            pred = model(X, X_raw, sess)
            loss = ctc_loss(pred, batch, blank=n_chars) if mwer is None else mwer_loss(pred, batch, **dict({'blank': n_chars}, **mwer))
            losses.append(loss.detach())
            loss.backward()
            if (batch_idx + 1) % 2 == 0:
                optim.step()
                optim.zero_grad()
            batch_idx += 1
            if max_steps is not None and batch_idx >= max_steps:
                break
        train_loss = float(torch.stack(losses).mean()) if losses else float('nan')
        val = test(model, devset, device)
        lr_sched.step()
        logging.info(f'finished epoch {epoch_idx+1} - training loss: {train_loss:.4f} validation WER: {val*100:.2f}')
        os.makedirs(out_dir, exist_ok=True)
        torch.save(model.state_dict(), os.path.join(out_dir, 'model.pt'))
        if max_steps is not None and batch_idx >= max_steps:
            break
    return model
