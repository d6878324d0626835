"""Scoring on the device against the host loop it replaces (recognition_model._edit_distance), three workloads, seeded:
  (a) 32 character-level pairs of up to 850 tokens (the character strings of the longest utterances), with and without the alignment;
  (b) the minimum-Bayes-risk pass for 19 utterances x 100 hypotheses of 5 .. 40 words (all K^2 word distances per list, risks, choice);
  (c) the same at K = 128;
and, for (b), the word-state beam search (leg 2 of tools/ctc_decode_probe.py --states: the reference-size batch, beam width 100, a random order-3
model of 20 000 words) asked for its 100 best in the same run, with the MBR pass over the lists it returned.
Device time from events -- 3 warm rounds, median and spread of 12; the host loop is timed once (for (b) and (c) on 300 random pairs of every list and
scaled to all of them, as said in the line).  --out PATH also writes the lines to a file (profiles/edit_distance_probe.txt holds a run).
Tuning aid (GPU only; run from the repository root)."""
import argparse
import statistics
import time

import numpy as np
import torch

from silent_speech_amd import recognition_model as rm

parser = argparse.ArgumentParser()
parser.add_argument('--out', help='also write the report to this file')
ARGS = parser.parse_args()
WARM, ROUNDS = 3, 12
dev = torch.device('cuda')
REPORT = []


def say(text):
    REPORT.append(text)
    print(text, flush=True)


def device_ms(fn):
    out = []
    for i in range(WARM + ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= WARM:
            out.append(e0.elapsed_time(e1))
    return out


def wall_ms(fn):
    out = []
    for i in range(WARM + ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= WARM:
            out.append(1e3 * (time.perf_counter() - t0))
    return out


def line(name, ms, extra=''):
    say('%-66s median %8.3f ms  (min %8.3f, max %8.3f, %d rounds)%s' % (name, statistics.median(ms), min(ms), max(ms), len(ms), extra))


def tables(seqs):
    rows, at = [], 0
    for s in seqs:
        rows.append((at, len(s)))
        at += len(s)
    flat = np.asarray([t for s in seqs for t in s] + [0], dtype=np.int32)
    return torch.from_numpy(flat).to(dev), torch.tensor(rows, dtype=torch.int64, device=dev)


def host_seconds(pairs):
    t0 = time.perf_counter()
    out = [rm._edit_distance(a, b) for a, b in pairs]
    return time.perf_counter() - t0, out


def characters(rng):
    """(a): references of 200 .. 850 characters over 27 symbols, the first one 850; hypotheses = the reference after ~15 % random edits"""
    refs, hyps = [], []
    for k in range(32):
        n = 850 if k == 0 else int(rng.integers(200, 851))
        r = rng.integers(0, 27, n).tolist()
        h = []
        for c in r:
            u = rng.random()
            if u < 0.05:
                continue
            h.append(int(rng.integers(0, 27)) if u < 0.10 else c)
            if u > 0.95:
                h.append(int(rng.integers(0, 27)))
        refs.append(r)
        hyps.append(h[:850])
    return refs, hyps


def word_lists(rng, n_utt, K):
    """(b), (c): per utterance a truth of 5 .. 40 words out of 2000 and K hypotheses, each the truth after 0 .. 6 random word edits"""
    lists = []
    for _ in range(n_utt):
        truth = rng.integers(0, 2000, int(rng.integers(5, 41))).tolist()
        hyps = []
        for _ in range(K):
            h = list(truth)
            for _ in range(int(rng.integers(0, 7))):
                kind, at = int(rng.integers(0, 3)), int(rng.integers(0, len(h)))
                if kind == 0:
                    h[at] = int(rng.integers(0, 2000))
                elif kind == 1 and len(h) > 5:
                    del h[at]
                elif len(h) < 40:
                    h.insert(at, int(rng.integers(0, 2000)))
            hyps.append(h)
        lists.append(hyps)
    return lists


def mbr_leg(name, lists, rng):
    seqs = [h for hyps in lists for h in hyps]
    tokens, rows = tables(seqs)
    groups, at = [], 0
    for hyps in lists:
        groups.append((at, len(hyps)))
        at += len(hyps)
    groups = torch.tensor(groups, dtype=torch.int64, device=dev)
    w = np.concatenate([np.exp(z - z.max()) / np.exp(z - z.max()).sum() for z in (np.sort(rng.standard_normal(len(h)))[::-1] for h in lists)]).astype(np.float32)
    w = torch.from_numpy(w).to(dev)
    unordered = sum(len(h) * (len(h) - 1) // 2 for h in lists)
    ms = device_ms(lambda: torch.ops.silent_speech.nbest_risk(tokens, rows, groups, w))
    line('%s nbest_risk op (2 launches + the sizes read back), device' % name, ms, '  = %.1f ns per distance' % (1e6 * statistics.median(ms) / max(unordered, 1)))
    dmat, _, pick = torch.ops.silent_speech.nbest_risk(tokens, rows, groups, w)
    sample, offs, off = [], [], 0                                         # 300 unordered pairs of every list, drawn at random
    for hyps in lists:
        K = len(hyps)
        for _ in range(300 if K > 1 else 0):
            i, k = sorted(rng.choice(K, 2, replace=False).tolist())
            sample.append((hyps[i], hyps[k]))
            offs.append(off + i * K + k)
        off += K * K
    sec, d = host_seconds(sample)
    same = dmat[torch.tensor(offs, device=dev)].cpu().tolist() == d
    say('%s host _edit_distance loop: %.3f s for %d of the distances (300 pairs of every list) = about %.1f s for all %d; same distances: %s; '
        'choice other than rank 0 in %d of %d lists' % (name, sec, len(d), sec * unordered / max(len(d), 1), unordered, same, int((pick != 0).sum()), len(lists)))
    return statistics.median(ms)


def random_word_lm(n_words=20000, seed=5):
    """The lexicon and tables of tools/ctc_decode_probe.py: random lower-case words of 1 .. 8 letters, ~4 bigrams and ~4 trigrams per word."""
    rng = np.random.default_rng(seed)
    chars = rm.TextTransform().chars
    words = set()
    while len(words) < n_words:
        words.add(''.join(chars[i] for i in rng.integers(0, 26, rng.integers(1, 9))))
    words = sorted(words)
    uni = np.zeros((n_words + 1, 2))
    x = rng.standard_normal(n_words) * 1.5
    uni[:n_words, 0] = x - np.log(np.exp(x).sum())
    uni[:, 1] = -rng.random(n_words + 1)
    ctx, nxt = rng.integers(0, n_words + 1, 4 * n_words), rng.integers(0, n_words, 4 * n_words)
    bi = {(int(a), int(b)): (-4 * rng.random(), -rng.random()) for a, b in zip(ctx, nxt)}
    pairs = sorted(bi)
    tri = {pairs[j] + (int(w),): -4 * rng.random() for j, w in zip(rng.integers(0, len(pairs), 4 * n_words), rng.integers(0, n_words, 4 * n_words))}
    return rm.WordNgramLM(words, uni, bi, tri, chars)


def search_leg(mbr_b):
    from silent_speech_amd.architecture import Model
    from silent_speech_amd.synthetic import reference_size_batch
    b = reference_size_batch(seed=11, budget=128000, device=dev)
    torch.manual_seed(0)
    model = Model(112, 38).to(dev).eval()
    logits = model.forward_utterances([r.to(dtype=torch.float32) for r in b['raw_emg']])
    frames = [int(y.shape[0]) for y in logits]
    T, V, head = max(frames), logits[0].shape[1], logits[0]._base
    utt = torch.tensor([[i * T, n] for i, n in enumerate(frames)], dtype=torch.int64, device=dev)
    lm = rm.WordStateLM.from_ngram_lm(random_word_lm()).to(dev)

    def search(n_best):
        return torch.ops.silent_speech.ctc_word_state_beam_search(head, utt, V, V - 1, V - 2, sum(frames), T, 100, n_best, lm.lex_child, lm.lex_word, lm.uni_logp, lm.st_bo,
                                                                   lm.st_shorter, lm.arc_keys, lm.arc_logp, lm.arc_next, lm.n_words, lm.start_state, lm.arc_probe, lm.order, 0.5, 0.5)
    say('word-state beam search: utterances %d, frames %d, longest %d frames, V = %d, beam width 100, order-3 model of %d words' % (len(frames), sum(frames), T, V, lm.n_words))
    one = device_ms(lambda: search(1))
    line('ctc_word_state_beam_search, 1 best, device', one)
    best = device_ms(lambda: search(100))
    line('ctc_word_state_beam_search, 100 best, device', best)
    lists = rm.beam_decode_utterances(logits, beam_width=100, n_best=100, lm=lm, alpha=0.5, beta=0.5)
    space = V - 2
    wall = wall_ms(lambda: rm.mbr_rerank(lists, space=space))
    line('mbr_rerank of the lists it returned (interning, upload, launches, read-back), wall', wall)
    picks = rm.mbr_rerank(lists, space=space)
    say('lists of %s hypotheses, mean %.1f words; MBR choice other than rank 0 in %d of %d utterances'
        % (sorted({len(h) for h in lists}), float(np.mean([1 + ints.count(space) for h in lists for ints, _ in h])), sum(p != 0 for p, _ in picks), len(lists)))
    say('(b) next to the search it follows: MBR pass %.3f ms, search for 100 best %.3f ms = %.1f %% of the search'
        % (mbr_b, statistics.median(best), 100 * mbr_b / statistics.median(best)))


with torch.no_grad():
    rng = np.random.default_rng(17)
    say('%s  edit distance / MBR probe' % time.strftime('%Y-%m-%d'))
    refs, hyps = characters(rng)
    tokens, rows = tables(refs + hyps)
    pairs = torch.tensor([(k, 32 + k) for k in range(32)], dtype=torch.int32, device=dev)
    say('(a) 32 character pairs, references %d .. %d tokens, hypotheses %d .. %d' % (min(map(len, refs)), max(map(len, refs)), min(map(len, hyps)), max(map(len, hyps))))
    for want in (False, True):
        ms = device_ms(lambda: torch.ops.silent_speech.edit_distance(tokens, rows, pairs, want))
        cells = sum(len(r) * len(h) for r, h in zip(refs, hyps))
        line('(a) edit_distance op, %s, device' % ('with the alignment' if want else 'distance and counts'), ms,
             '  = %.2f us per dependent row of the longest pair' % (1e3 * statistics.median(ms) / 850))
    line('(a) recognition_model.edit_distance with the alignment (upload, launch, read-back), wall', wall_ms(lambda: rm.edit_distance(refs, hyps, ops=True)))
    sec, d = host_seconds(list(zip(refs, hyps)))
    got = torch.ops.silent_speech.edit_distance(tokens, rows, pairs, False)[0].cpu().tolist()
    say('(a) host _edit_distance loop: %.3f s for the 32 pairs (%.1f M cells); same distances: %s' % (sec, cells / 1e6, got == d))
    mbr_b = mbr_leg('(b) 19 x 100', word_lists(rng, 19, 100), rng)
    mbr_leg('(c) 19 x 128', word_lists(rng, 19, 128), rng)
    search_leg(mbr_b)
    if ARGS.out:
        with open(ARGS.out, 'w') as f:
            f.write('\n'.join(REPORT) + '\n')
