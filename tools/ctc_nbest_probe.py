"""n-best scoring of a reference-size recognition batch: 32 utterances of up to 850 frames / 141 labels (one label per 6 frames), V = 38, seeded
random logits in the packed layout; the hypotheses of an utterance are its reference with a few labels substituted, dropped or inserted, K = 4 and
K = 16 per utterance.  Device time from events -- three rotating copies of the logits, 3 warm rounds, median and spread of 12 -- of the forward
launches of ss_ctc_nbest_logp (descriptors + alpha / beta for the H hypotheses + sign), of ss_ctc_nbest_backward, of ss_nbest_expected_risk, and of
the ops with their lse launch and allocations; the workspace; and, as the yardstick, what can be written without them:
torch.nn.functional.ctc_loss(reduction='none') on the log-softmaxed logits with every utterance repeated K times, forward and backward, in the same
run.  Tuning aid (GPU only): PYTHONPATH=. python tools/ctc_nbest_probe.py > profiles/ctc_nbest_probe.txt from the repository root."""
import statistics

import numpy as np
import torch
import torch.nn.functional as F

from silent_speech_amd import _lib
from silent_speech_amd import recognition_model as rm

B, T_MAX, V, WARM, ROUNDS, COPIES = 32, 850, 38, 3, 12, 3
dev = torch.device('cuda')
rng = np.random.default_rng(11)
frames = [T_MAX] + [int(n) for n in rng.integers(200, T_MAX + 1, B - 1)]
refs = [[int(c) for c in rng.integers(0, V - 1, n // 6)] for n in frames]
first = [int(f) for f in np.concatenate([[0], np.cumsum(frames)])[:-1]]
M = sum(frames)
heads = [torch.from_numpy((rng.standard_normal((M, V)) * 3).astype(np.float32)).to(dev) for _ in range(COPIES)]


def perturb(ref):
    h = list(ref)
    for _ in range(int(rng.integers(1, 6))):
        i, kind = int(rng.integers(0, len(h))), int(rng.integers(0, 3))
        if kind == 0:
            h[i] = int(rng.integers(0, V - 1))
        elif kind == 1 and len(h) > 1:
            del h[i]
        else:
            h.insert(i, int(rng.integers(0, V - 1)))
    return h[:141]


def device_ms(fn):
    out = []
    for i in range(WARM + ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i % COPIES)
        e1.record()
        torch.cuda.synchronize()
        if i >= WARM:
            out.append(e0.elapsed_time(e1))
    return out


def line(name, ms):
    print('%-78s median %8.3f ms  (min %8.3f, max %8.3f, %d rounds)' % (name, statistics.median(ms), min(ms), max(ms), len(ms)))


lib, p = _lib.lib(), _lib.ptr
print('utterances %d, frames %d, longest %d frames / %d labels, V = %d' % (B, M, max(frames), max(len(r) for r in refs), V))
for K in (4, 16):
    hyps = [[list(r)] + [perturb(r) for _ in range(K - 1)] for r in refs]
    plan = rm._NbestPlan('probe', first, frames, hyps, V, V - 1)
    t = [torch.from_numpy(a).to(dev) for a in plan.arrays()]
    H = plan.n_hyp
    st = _lib.stream_of(heads[0])
    ws_bytes = lib.ss_ctc_nbest_workspace_bytes(H, plan.ws_floats)
    ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=dev)
    lse = [torch.empty(M, device=dev) for _ in range(COPIES)]
    amax = torch.empty(M, dtype=torch.int32, device=dev)
    for c in range(COPIES):
        _lib.check(lib.ss_frame_lse(p(heads[c]), V, 0, V, M, p(lse[c]), p(amax), st))
    logp, g, dlogits = torch.empty(H, device=dev), torch.randn(H, device=dev), torch.empty_like(heads[0])
    cost = torch.randint(0, 9, (H,), device=dev).float()
    groups = t[0][:, 2:].contiguous()
    loss, risk, post, dlogp = torch.empty(1, device=dev), torch.empty(B, dtype=torch.float64, device=dev), torch.empty(H, device=dev), torch.empty(H, device=dev)
    print('K = %d: %d hypotheses, workspace %.1f MB (descriptors, alpha, beta), logits %.1f MB' % (K, H, ws_bytes / 1e6, M * V * 4 / 1e6))
    line('  ss_ctc_nbest_logp (descriptors + alpha / beta + sign), device',
         device_ms(lambda c: _lib.check(lib.ss_ctc_nbest_logp(p(heads[c]), V, V, V - 1, M, p(lse[c]), p(t[0]), B, p(t[1]), H, plan.max_s, p(t[2]), t[2].shape[0],
                                                                p(ws), plan.ws_floats, p(logp), st))))
    line('  ss_ctc_nbest_backward, device',
         device_ms(lambda c: _lib.check(lib.ss_ctc_nbest_backward(p(heads[c]), V, V, V - 1, M, p(lse[c]), p(t[0]), B, H, p(t[2]), p(ws), plan.ws_floats, p(logp), p(g),
                                                                    p(dlogits), st))))
    line('  ss_nbest_expected_risk, device',
         device_ms(lambda c: _lib.check(lib.ss_nbest_expected_risk(p(logp), p(cost), H, p(groups), B, 1.0, p(loss), p(risk), p(post), p(dlogp), st))))

    def op_step(c):
        x = heads[c].detach().requires_grad_(True)
        lp, _, _ = torch.ops.silent_speech.ctc_nbest_logp(x, t[0], t[1], t[2], plan.max_s, plan.ws_floats, V, V - 1)
        torch.ops.silent_speech.nbest_expected_risk(lp, cost, groups, 1.0)[0][0].backward()
    line('  ctc_nbest_logp + nbest_expected_risk ops, forward + backward (lse, allocations), device', device_ms(op_step))
    # the yardstick: every utterance repeated K times through F.ctc_loss
    T_pad = max(frames)
    idx = torch.zeros((T_pad, B), dtype=torch.int64)
    for u in range(B):
        idx[:, u] = first[u] + torch.clamp(torch.arange(T_pad), max=frames[u] - 1)
    idx = idx.to(dev)
    flat_t = torch.tensor([c for lst in hyps for h in lst for c in h], dtype=torch.int64, device=dev)
    t_len = torch.tensor([len(h) for lst in hyps for h in lst], dtype=torch.int64, device=dev)
    in_len = torch.tensor([n for n in frames for _ in range(K)], dtype=torch.int64, device=dev)

    def torch_step(c):
        x = heads[c].detach().requires_grad_(True)
        lpm = F.log_softmax(x, 1)[idx]                                   # (T_pad, B, V)
        lpm = lpm.repeat_interleave(K, 1)                                # (T_pad, B K, V)
        nll = F.ctc_loss(lpm, flat_t, in_len, t_len, blank=V - 1, reduction='none', zero_infinity=True)
        (nll * g).sum().backward()
    line('  F.ctc_loss(reduction="none"), utterances repeated K times, forward + backward, device', device_ms(torch_step))
    lp, _, _ = torch.ops.silent_speech.ctc_nbest_logp(heads[0], t[0], t[1], t[2], plan.max_s, plan.ws_floats, V, V - 1)
    lpm = F.log_softmax(heads[0], 1)[idx].repeat_interleave(K, 1)
    ref_lp = -F.ctc_loss(lpm, flat_t, in_len, t_len, blank=V - 1, reduction='none')
    fin = torch.isfinite(ref_lp)
    print('  largest |logp - (-F.ctc_loss)| / |logp| over the %d feasible hypotheses: %.2e' % (int(fin.sum()), float(((lp - ref_lp)[fin].abs() / ref_lp[fin].abs()).max())))
print('not measured here: the recognition training step with and without mwer= and the share of the beam search in it')
