"""CTC prefix beam search of a reference-size recognition batch (the batch of tools/ctc_probe.py: 128 000-sample budget, utterances of up to 860
frames, V = 38) at beam width 100: device time of torch.ops.silent_speech.ctc_beam_search (per-frame lse launch + the one search launch) from
events -- 3 warm rounds, median and spread of 12 -- and the time per DEPENDENT frame (the frames of the longest utterance run in sequence inside one
workgroup; the utterances run side by side).  Beside it, on the same batch: beam_decode_utterances with its upload and read-back, greedy_decode_utterances,
and the ragged forward that produces the logits.  Tuning aid (GPU only)."""
import statistics
import time

import numpy as np
import torch

from silent_speech_amd import recognition_model as rm
from silent_speech_amd.architecture import Model
from silent_speech_amd.synthetic import reference_size_batch

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


def line(name, ms, extra=''):
    print('%-58s median %8.3f ms  (min %8.3f, max %8.3f, %d rounds)%s' % (name, statistics.median(ms), min(ms), max(ms), len(ms), extra))


with torch.no_grad():
    logits = model.forward_utterances(raws)
    frames = [int(y.shape[0]) for y in logits]
    B, T, V = len(frames), max(frames), logits[0].shape[1]
    head = logits[0]._base
    print('utterances %d, frames %d, longest %d frames, V = %d, beam width %d' % (B, sum(frames), T, V, W))
    utt = torch.tensor([[i * T, n] for i, n in enumerate(frames)], dtype=torch.int64, device=dev)
    search = device_ms(lambda: torch.ops.silent_speech.ctc_beam_search(head, utt, V, V - 1, sum(frames), T, W, 1, None, 0.0, 0.0))
    line('ctc_beam_search op (lse + search launches), device', search, '  = %.2f us per dependent frame' % (1e3 * statistics.median(search) / T))
    table = torch.log_softmax(torch.randn(V, V, V - 1, device=dev), 2).contiguous()
    fused = device_ms(lambda: torch.ops.silent_speech.ctc_beam_search(head, utt, V, V - 1, sum(frames), T, W, 1, table, 0.5, 0.5))
    line('  with a label trigram table fused, device', fused, '  = %.2f us per dependent frame' % (1e3 * statistics.median(fused) / T))
    line('beam_decode_utterances (upload, launches, read-back), wall', wall_ms(lambda: rm.beam_decode_utterances(logits, beam_width=W)))
    line('greedy_decode_utterances (launch, read-back, collapse), wall', wall_ms(lambda: rm.greedy_decode_utterances(logits)))
    line('Model.forward_utterances of the batch, device', device_ms(lambda: model.forward_utterances(raws)))
    dec, gre = rm.beam_decode_utterances(logits, beam_width=W), rm.greedy_decode_utterances(logits)
    print('beam result equals the greedy one in %d of %d utterances; mean decoded length %.1f labels' % (sum(x == y for x, y in zip(dec, gre)), B, float(np.mean([len(x) for x in dec]))))
