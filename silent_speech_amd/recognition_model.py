"""Drop-in for the training path of the reference's recognition_model.py ("next" row N1, BASELINE cfg5):

    ctc_loss(logits, example, blank)         the three loss lines :96-101 fused on the packed layout
    greedy_decode(logits, lengths, blank)    best-path CTC decode (argmax, collapse repeats, drop blanks)
    beam_decode(logits, lengths, blank)      CTC prefix beam search on the device (csrc/ctc_decode.hip), optionally fused with a LabelNgramLM
    beam_decode_utterances(logits)           the same for the list Model.forward_utterances returns
    LabelNgramLM                             label trigram table counted from text, the language model of the beam search
    test(model, testset, device)             :30-58 -> WER; decoder='greedy' (default) or 'beam'
    train_model(trainset, devset, device)    :61-117 (AdamW, warm-up, x2 gradient accumulation, MultiStepLR)

The encoder is the same MI355X engine as the transduction trainer (Model without the aux head).  The CTC
alpha/beta recursion and its gradient run in csrc/ctc.hip straight on the packed (rows*200, V) logits, so the
decollate + pad_sequence copies and the (T_max, N, V) log-prob tensor of the reference never exist.
The search of the reference's decoder (ctcdecode, :33-35,48-49) is here as a kernel of its own: a prefix beam search over whole batches
in one launch, with shallow fusion of a label n-gram table that lives on the device (LabelNgramLM).  Its KenLM WORD language model
(third-party C++ plus an lm.binary file) stays out of scope, so parity with the reference's WER stays unpinned; test() reports greedy
WER by default and beam-search WER with decoder='beam'.
"""
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


def _beam_search(head, V, blank, first, frames, beam_width, n_best, lm, alpha, beta):
    """One table upload, lse + search launches, one read-back.  head: (M, ld) f32 on the device; first / frames: per utterance, host ints."""
    n = len(frames)
    if n == 0:
        return []
    if lm is not None:
        lm = (lm.table if isinstance(lm, LabelNgramLM) else torch.as_tensor(lm, dtype=torch.float32)).to(head.device).contiguous()
    utt, = staging.upload([np.stack([np.asarray(first, dtype=np.int64), np.asarray(frames, dtype=np.int64)], 1)], head.device)
    max_len = max(max(frames), 1)
    labels, lengths, scores, _ = torch.ops.silent_speech.ctc_beam_search(head, utt, V, blank, int(sum(frames)), max_len, int(beam_width), int(n_best),
                                                                         lm, float(alpha), float(beta))
    back = torch.cat([labels.reshape(n, n_best * max_len), lengths, scores.view(torch.int32)], 1).cpu().numpy()       # ONE read-back
    labels, lengths = back[:, :n_best * max_len].reshape(n, n_best, max_len), back[:, n_best * max_len:n_best * max_len + n_best]
    scores = np.ascontiguousarray(back[:, n_best * max_len + n_best:]).view(np.float32)
    if n_best == 1:
        return [labels[b, 0, :max(lengths[b, 0], 0)].tolist() for b in range(n)]
    return [[(labels[b, r, :lengths[b, r]].tolist(), float(scores[b, r])) for r in range(n_best) if lengths[b, r] >= 0] for b in range(n)]


def beam_decode(pred, lengths, blank=None, *, beam_width=100, n_best=1, lm=None, alpha=0.0, beta=0.0):
    """CTC prefix beam search of packed logits (rows, T, V) (NOT log-softmaxed), utterances back to back with `lengths` frames each, in one
    launch on the device; lm: a LabelNgramLM (or its table) fused as alpha * ln P(label | two labels before) + beta per label.
    Returns a list of int lists, or for n_best > 1 a list of [(ints, score), ...] lists, best first (fewer than n_best if fewer prefixes exist)."""
    B, T, V = pred.shape
    blank = V - 1 if blank is None else int(blank)
    logits = pred.reshape(B * T, V).float().contiguous()
    frames = [int(n) for n in lengths]
    if sum(frames) > B * T or any(n < 0 for n in frames):
        raise ValueError('beam_decode: the lengths do not fit the %d packed frames' % (B * T))
    first = np.concatenate([[0], np.cumsum(frames)])[:-1] if frames else []
    return _beam_search(logits, V, blank, first, frames, beam_width, n_best, lm, alpha, beta)


def beam_decode_utterances(logits, *, beam_width=100, n_best=1, lm=None, alpha=0.0, beta=0.0):
    """beam_decode for the per-utterance logits Model.forward_utterances returns -- (T_b, V) views of ONE (B T_max, >= V) head buffer --: the
    search reads the slots in place (first frame b T_max, T_b frames; filler rows and columns are never looked at).  blank = V - 1."""
    if not logits:
        return []
    head, V = logits[0]._base, logits[0].shape[1]
    B, T = len(logits), max(int(y.shape[0]) for y in logits)
    if head is None or head.dim() != 2 or head.dtype != torch.float32 or not head.is_contiguous() or head.shape[0] != B * T or \
            any(y._base is not head or y.shape[1] != V or y.storage_offset() != b * T * head.shape[1] for b, y in enumerate(logits)):
        raise ValueError('beam_decode_utterances takes the list Model.forward_utterances returned')
    return _beam_search(head, V, V - 1, [b * T for b in range(B)], [int(y.shape[0]) for y in logits], beam_width, n_best, lm, alpha, beta)


def test(model, testset, device, *, batch_size=1, whole_utterances=False, decoder='greedy', beam_width=100, lm=None, alpha=0.0, beta=0.0):
    """:30-58.  Default (batch_size=1) = the reference: eval-mode forward of ONE WHOLE utterance at a time (:37-43), so the convolutions
    and the +-99-frame attention band span the utterance (the banded attention kernels take any T).  batch_size > 1 packs the utterances
    into 200-frame rows like training does -- faster, but context is cut at the row boundaries, so its WER is not the reference's number.
    whole_utterances=True with batch_size > 1: groups of up to batch_size WHOLE utterances go through Model.forward_utterances (one ragged-batch
    plan call per group, every utterance computed as it is alone) and one arg-max launch + one read-back per group: the function of the
    default, at batched speed.
    decoder='greedy' (default): best-path decoding.  decoder='beam': the prefix beam search of beam_decode / beam_decode_utterances with
    beam_width, and lm / alpha / beta if a LabelNgramLM is given, in all three branches (the reference's KenLM word model is out of scope)."""
    if decoder not in ('greedy', 'beam'):
        raise ValueError("test: decoder is 'greedy' or 'beam'")
    model.eval()
    tt = testset.text_transform
    blank = len(tt.chars)
    if decoder == 'beam':
        lm = lm.to(device) if isinstance(lm, LabelNgramLM) else lm                  # the table crosses to the device once, not per utterance
        search = dict(beam_width=beam_width, lm=lm, alpha=alpha, beta=beta)
        decode = lambda pred, lengths: beam_decode(pred, lengths, blank, **search)
        decode_utterances = lambda logits: beam_decode_utterances(logits, **search)
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
    return wer(references, predictions)


def train_model(trainset, devset, device, n_epochs=200, *, compute_dtype=torch.bfloat16, f32_matmul='exact', max_steps=None):
    """:61-117 on the MI355X: batches under a 128 000-sample budget, AdamW (lr 3e-4 in the reference's flags), linear
    warm-up, an optimiser step every SECOND batch (gradients accumulate in the flat .grad arena), MultiStepLR."""
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
            loss = ctc_loss(pred, batch, blank=n_chars)
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
