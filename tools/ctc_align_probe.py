"""Forced alignment of a reference-size recognition batch: 32 utterances of up to 850 frames / 141 labels (one label per 6 frames), V = 38, seeded
random logits in the packed layout.  Device time from events -- 3 warm rounds, median and spread of 12 -- of torch.ops.silent_speech.ctc_forced_align
(per-frame lse launch + the one alignment launch), of ss_ctc_align alone, and per DEPENDENT frame (the frames of the longest utterance run in
sequence inside one wave; the utterances run side by side); the whole recognition_model.forced_align call with its upload and read-back; the CTC
loss (forward + gradient) on the same batch; and the float64 host restatement (tests/ctc_align_oracle.py) on the longest utterance.  Tuning aid
(GPU only; run from the repository root)."""
import statistics
import time

import numpy as np
import torch

from silent_speech_amd import _lib
from silent_speech_amd import recognition_model as rm
from tests import ctc_align_oracle as oracle

B, T_MAX, V, WARM, ROUNDS = 32, 850, 38, 3, 12
dev = torch.device('cuda')
rng = np.random.default_rng(11)
frames = [T_MAX] + [int(n) for n in rng.integers(200, T_MAX + 1, B - 1)]
targets = [[int(c) for c in rng.integers(0, V - 1, n // 6)] for n in frames]
x = (rng.standard_normal((sum(frames), V)) * 3).astype(np.float32)
pred = torch.from_numpy(x).to(dev).reshape(1, -1, V)
head = pred.reshape(-1, V)


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
    print('%-62s median %8.3f ms  (min %8.3f, max %8.3f, %d rounds)%s' % (name, statistics.median(ms), min(ms), max(ms), len(ms), extra))


with torch.no_grad():
    S = [len(y) for y in targets]
    print('utterances %d, frames %d, longest %d frames / %d labels, V = %d' % (B, sum(frames), max(frames), max(S), V))
    f0, g0 = np.concatenate([[0], np.cumsum(frames)])[:-1], np.concatenate([[0], np.cumsum(S)])[:-1]
    utt = torch.tensor(np.stack([f0, frames, g0, S], 1), dtype=torch.int64, device=dev)
    tg = torch.tensor([c for y in targets for c in y], dtype=torch.int32, device=dev)
    args = (head, utt, tg, V, V - 1, sum(frames), max(S))
    op = device_ms(lambda: torch.ops.silent_speech.ctc_forced_align(*args))
    line('ctc_forced_align op (lse + alignment launches), device', op)
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_of(head)
    lse, amax = torch.empty(head.shape[0], device=dev), torch.empty(head.shape[0], dtype=torch.int32, device=dev)
    _lib.check(lib.ss_frame_lse(p(head), V, 0, V, head.shape[0], p(lse), p(amax), st))
    ws = torch.empty(lib.ss_ctc_align_workspace_bytes(B, sum(frames), max(S)) // 4, dtype=torch.int32, device=dev)
    score, ft = torch.empty(B, device=dev), torch.empty(head.shape[0], dtype=torch.int32, device=dev)
    tf, tn, tl = torch.empty_like(tg), torch.empty_like(tg), torch.empty(tg.shape[0], device=dev)
    for blank, name in ((V - 1, 'CTC topology'), (-1, 'linear topology')):
        alone = device_ms(lambda: _lib.check(lib.ss_ctc_align(p(head), V, V, blank, head.shape[0], p(lse), p(utt), B, sum(frames), max(S), p(tg), tg.shape[0],
                                                              p(ws), p(score), p(ft), p(tf), p(tn), p(tl), st)))
        line('  ss_ctc_align alone, %s, device' % name, alone, '  = %.3f us per dependent frame' % (1e3 * statistics.median(alone) / max(frames)))
    line('  ss_frame_lse alone, device', device_ms(lambda: _lib.check(lib.ss_frame_lse(p(head), V, 0, V, head.shape[0], p(lse), p(amax), st))))
    print('back-pointer workspace %.1f MB (256 bytes per frame), logits %.1f MB' % (ws.numel() * 4 / 1e6, head.numel() * 4 / 1e6))
    line('forced_align (upload, launches, read-back, slicing), wall', wall_ms(lambda: rm.forced_align(pred, frames, targets)))
    example = {'lengths': frames, 'text_int': [torch.tensor(y, dtype=torch.int64) for y in targets]}
    plan = rm._CtcPlan(example['lengths'], example['text_int'], head.shape[0], dev)
    loss = device_ms(lambda: torch.ops.silent_speech.ctc_loss(head, plan.desc, plan.targets, plan.n, plan.max_s, plan.ws_floats, V, V - 1))
    line('ctc_loss op (lse + alpha / beta + gradient) on the same batch, device', loss)
    t0 = time.perf_counter()
    ref, path = oracle.align(x[:frames[0]], targets[0], V - 1)
    host = time.perf_counter() - t0
    got = rm.forced_align(pred, frames, targets)
    print('float64 host restatement of the longest utterance: %.3f s; its score %.4f, the device %.4f, same path: %s'
          % (host, ref, got[0].score, got[0].frames.tolist() == path))
    nll = torch.ops.silent_speech.ctc_loss(head, plan.desc, plan.targets, plan.n, plan.max_s, plan.ws_floats, V, V - 1)[2][:B].cpu().numpy()
    print('score <= -nll on %d of %d utterances; mean frames per token along the paths %.2f'
          % (sum(a.score <= -float(v) + 1e-3 for a, v in zip(got, nll)), B, float(np.mean([a.token_frames.mean() for a in got]))))
