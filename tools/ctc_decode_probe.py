"""CTC prefix beam search of a reference-size recognition batch (the batch of tools/ctc_probe.py: 128 000-sample budget, utterances of up to 860
frames, V = 38) at beam width 100: device time of torch.ops.silent_speech.ctc_beam_search (per-frame lse launch + the one search launch) from
events -- 3 warm rounds, median and spread of 12 -- and the time per DEPENDENT frame (the frames of the longest utterance run in sequence inside one
workgroup; the utterances run side by side) -- plain, with a label trigram table fused, and the lexicon-constrained search with a word n-gram
(ctc_word_beam_search; a seeded random lexicon of 20 000 words with ~4 bigrams and ~4 trigrams per word).  Beside it, on the same batch: beam_decode_utterances with its upload and read-back, greedy_decode_utterances,
and the ragged forward that produces the logits.  Tuning aid (GPU only).

--states: the same batch through three legs instead -- (1) ctc_word_beam_search on that random order-3 model, the yardstick; (2)
ctc_word_state_beam_search on WordStateLM.from_ngram_lm of the same model, which must decode the identical strings; (3) ctc_word_state_beam_search
on a random order-5 model of the same vocabulary with ~4 n-grams per context at every level -- with the table sizes, the longest probe and the
time per dependent frame of each; --out PATH also writes the lines to a file (profiles/ctc_word_state_probe.txt holds a run)."""
import argparse
import statistics
import time

import numpy as np
import torch

from silent_speech_amd import recognition_model as rm
from silent_speech_amd.architecture import Model
from silent_speech_amd.synthetic import reference_size_batch

parser = argparse.ArgumentParser()
parser.add_argument('--states', action='store_true', help='the three legs of the word-state search instead of the default report')
parser.add_argument('--out', help='with --states: also write the report to this file')
ARGS = parser.parse_args()
W, WARM, ROUNDS = 100, 3, 12
dev = torch.device('cuda')
b = reference_size_batch(seed=11, budget=128000, device=dev)
torch.manual_seed(0)
model = Model(112, 38).to(dev).eval()
raws = [r.to(dtype=torch.float32) for r in b['raw_emg']]


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


def random_word_lm(n_words=20000, seed=5):
    """A lexicon of random lower-case words of 1 .. 8 letters over TextTransform's labels, random natural-log tables."""
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


def random_state_lm(words, chars, order=5, seed=6):
    """A random prefix-closed model of `order` over `words`: ~4 bigrams per context word, then on every level as many contexts as there are
    words, drawn from the n-grams of the level below, with ~4 n-grams each."""
    rng = np.random.default_rng(seed)
    n = len(words)
    x = rng.standard_normal(n) * 1.5
    lp = x - np.log(np.exp(x).sum())
    grams = {(w,): (float(lp[w]), -float(rng.random())) for w in range(n)}
    grams[(n,)] = (-99.0, -float(rng.random()))
    level = [(int(w),) for w in rng.integers(0, n + 1, 4 * n)]
    for k in range(2, order + 1):
        new = {h + (int(w),): (-4 * float(rng.random()), -float(rng.random()) if k < order else 0.0) for h, w in zip(level, rng.integers(0, n, len(level)))}
        grams.update(new)
        keys = sorted(new)
        level = [keys[j] for j in rng.integers(0, len(keys), 4 * n)]
    return rm.WordStateLM(words, grams, chars, order)


REPORT = []


def line(name, ms, extra=''):
    REPORT.append('%-58s median %8.3f ms  (min %8.3f, max %8.3f, %d rounds)%s' % (name, statistics.median(ms), min(ms), max(ms), len(ms), extra))
    print('%-58s median %8.3f ms  (min %8.3f, max %8.3f, %d rounds)%s' % (name, statistics.median(ms), min(ms), max(ms), len(ms), extra))


def states_legs(logits, head, utt, frames, T, V):
    def say(text):
        REPORT.append(text)
        print(text)

    def state_search(lm, n_best=1):
        return torch.ops.silent_speech.ctc_word_state_beam_search(head, utt, V, V - 1, V - 2, sum(frames), T, W, n_best, lm.lex_child, lm.lex_word, lm.uni_logp, lm.st_bo,
                                                                   lm.st_shorter, lm.arc_keys, lm.arc_logp, lm.arc_next, lm.n_words, lm.start_state, lm.arc_probe, lm.order, 0.5, 0.5)
    say('%s  utterances %d, frames %d, longest %d frames, V = %d, beam width %d' % (time.strftime('%Y-%m-%d'), len(frames), sum(frames), T, V, W))
    table = random_word_lm()
    same = rm.WordStateLM.from_ngram_lm(table)
    five = random_state_lm(table.words, table.chars)
    wlm, slm, flm = table.to(dev), same.to(dev), five.to(dev)
    say('leg 1, table model, order 3: %d words, %d bigrams in %d slots (longest probe %d), %d trigrams in %d slots (longest probe %d)'
        % (wlm.n_words, len(wlm.bigrams), wlm.bi_keys.numel(), wlm.bi_probe, len(wlm.trigrams), wlm.tri_keys.numel(), wlm.tri_probe))
    for name, lm in (('leg 2, state model of the same n-grams, order 3', slm), ('leg 3, random state model, order 5', flm)):
        by = [sum(len(g) == k for g in lm.ngrams) for k in range(1, lm.order + 1)]
        say('%s: %d states, n-grams per level %s, %d arcs in %d slots (longest probe %d)' % (name, lm.n_states, by, sum(by[1:]), lm.arc_keys.numel(), lm.arc_probe))
    per = '  = %.2f us per dependent frame'
    for rnd in range(2):                                                   # the legs in turn, twice: the second pass shows the run-to-run spread
        ms = device_ms(lambda: torch.ops.silent_speech.ctc_word_beam_search(head, utt, V, V - 1, V - 2, sum(frames), T, W, 1, wlm.lex_child, wlm.lex_word, wlm.uni, wlm.bi_keys,
                                                                           wlm.bi_val, wlm.tri_keys, wlm.tri_val, wlm.n_words, wlm.start, wlm.bi_probe, wlm.tri_probe, 0.5, 0.5))
        line('leg 1 ctc_word_beam_search, table order 3, pass %d' % (rnd + 1), ms, per % (1e3 * statistics.median(ms) / T))
        ms = device_ms(lambda: state_search(slm))
        line('leg 2 ctc_word_state_beam_search, same model, pass %d' % (rnd + 1), ms, per % (1e3 * statistics.median(ms) / T))
        ms = device_ms(lambda: state_search(flm))
        line('leg 3 ctc_word_state_beam_search, order 5, pass %d' % (rnd + 1), ms, per % (1e3 * statistics.median(ms) / T))
    a = rm.beam_decode_utterances(logits, beam_width=W, lm=wlm, alpha=0.5, beta=0.5)
    b2 = rm.beam_decode_utterances(logits, beam_width=W, lm=slm, alpha=0.5, beta=0.5)
    c = rm.beam_decode_utterances(logits, beam_width=W, lm=flm, alpha=0.5, beta=0.5)
    say('legs 1 and 2 decode identical strings in %d of %d utterances; mean decoded length %.1f labels, %.1f words (leg 3: %.1f labels, %.1f words)'
        % (sum(x == y for x, y in zip(a, b2)), len(a), float(np.mean([len(x) for x in a])), float(np.mean([1 + x.count(V - 2) for x in a])),
           float(np.mean([len(x) for x in c])), float(np.mean([1 + x.count(V - 2) for x in c]))))
    if ARGS.out:
        with open(ARGS.out, 'w') as f:
            f.write('\n'.join(REPORT) + '\n')
    if a != b2:
        raise SystemExit('legs 1 and 2 differ')


with torch.no_grad():
    logits = model.forward_utterances(raws)
    frames = [int(y.shape[0]) for y in logits]
    B, T, V = len(frames), max(frames), logits[0].shape[1]
    head = logits[0]._base
    print('utterances %d, frames %d, longest %d frames, V = %d, beam width %d' % (B, sum(frames), T, V, W))
    utt = torch.tensor([[i * T, n] for i, n in enumerate(frames)], dtype=torch.int64, device=dev)
    if ARGS.states:
        states_legs(logits, head, utt, frames, T, V)
        raise SystemExit(0)
    search = device_ms(lambda: torch.ops.silent_speech.ctc_beam_search(head, utt, V, V - 1, sum(frames), T, W, 1, None, 0.0, 0.0))
    line('ctc_beam_search op (lse + search launches), device', search, '  = %.2f us per dependent frame' % (1e3 * statistics.median(search) / T))
    table = torch.log_softmax(torch.randn(V, V, V - 1, device=dev), 2).contiguous()
    fused = device_ms(lambda: torch.ops.silent_speech.ctc_beam_search(head, utt, V, V - 1, sum(frames), T, W, 1, table, 0.5, 0.5))
    line('  with a label trigram table fused, device', fused, '  = %.2f us per dependent frame' % (1e3 * statistics.median(fused) / T))
    wlm = random_word_lm().to(dev)
    print('word model: %d words, %d lexicon nodes, %d bigrams in %d slots (longest probe %d), %d trigrams in %d slots (longest probe %d)'
          % (wlm.n_words, wlm.lex_word.numel(), len(wlm.bigrams), wlm.bi_keys.numel(), wlm.bi_probe, len(wlm.trigrams), wlm.tri_keys.numel(), wlm.tri_probe))
    word = device_ms(lambda: torch.ops.silent_speech.ctc_word_beam_search(head, utt, V, V - 1, V - 2, sum(frames), T, W, 1, wlm.lex_child, wlm.lex_word, wlm.uni, wlm.bi_keys,
                                                                         wlm.bi_val, wlm.tri_keys, wlm.tri_val, wlm.n_words, wlm.start, wlm.bi_probe, wlm.tri_probe, 0.5, 0.5))
    line('ctc_word_beam_search op (lexicon + word trigram), device', word, '  = %.2f us per dependent frame' % (1e3 * statistics.median(word) / T))
    wdec = rm.beam_decode_utterances(logits, beam_width=W, lm=wlm, alpha=0.5, beta=0.5)
    print('word search: mean decoded length %.1f labels, %.1f words' % (float(np.mean([len(x) for x in wdec])), float(np.mean([1 + x.count(V - 2) for x in wdec]))))
    line('beam_decode_utterances (upload, launches, read-back), wall', wall_ms(lambda: rm.beam_decode_utterances(logits, beam_width=W)))
    line('greedy_decode_utterances (launch, read-back, collapse), wall', wall_ms(lambda: rm.greedy_decode_utterances(logits)))
    line('Model.forward_utterances of the batch, device', device_ms(lambda: model.forward_utterances(raws)))
    dec, gre = rm.beam_decode_utterances(logits, beam_width=W), rm.greedy_decode_utterances(logits)
    print('beam result equals the greedy one in %d of %d utterances; mean decoded length %.1f labels' % (sum(x == y for x, y in zip(dec, gre)), B, float(np.mean([len(x) for x in dec]))))
