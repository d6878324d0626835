"""PyTorch dispatcher registration of the hot path: `torch.ops.silent_speech.*` (torch.library custom ops over the C ABI).

    model_forward / model_backward   Model.forward (architecture.py:61-84) and what loss.backward() triggers: one native plan each
    model_forward_ragged             the eval-mode forward of a batch of WHOLE utterances of different lengths in one native plan (inference only)
    dtw_loss                         transduction_model.py:98-157 (cost matrices in strip layout, DTW + backtrace, loss and d loss / d head)
    dtw_align                        align.py:16-34 on one device matrix
    ctc_loss                         recognition_model.py:96-101
    ctc_beam_search                  the search of recognition_model.py:33-35,48-49: CTC prefix beam search + label n-gram table, one launch per batch (inference only)
    ctc_word_beam_search             the same search confined to a lexicon, a word n-gram with backoff scored at every word end (WordNgramLM), inference only
    ctc_forced_align                 best alignment of known label strings to the frame posteriors (CTC or blank-free linear topology), frame labels and token spans, one launch per batch (inference only)
    edit_distance / nbest_risk       Levenshtein distance with its error breakdown and alignment for a batch of pairs in one launch; all K^2 distances, risks and the MBR choice of n-best lists
    word_ngram_score                 ln P(w | w2, w1) of word triples by the device function of that search (tests, n-best rescoring)
    ctc_word_state_beam_search       the lexicon-constrained search with a word n-gram of any order up to 6 held as context states (WordStateLM), inference only
    word_state_score                 ln P(word | state) and the state after it by the device function of that search (tests, n-best rescoring)
    stft_logmel / stft_logmel_backward                 data_utils.py:39-62 and its gradient with respect to the audio (csrc/mel_bwd.hip)
    stft_logmel_ragged / stft_logmel_ragged_backward   the same pair for a ragged batch in one flat buffer (load_audio's clip included)
    emg_features                     data_utils.py:85-136 (get_emg_features; no autograd: the reference's features are numpy)
    audio_resample / audio_level     the band-limited resample (:75) and normalize_volume's levels (:19-27) of load_audio for a ragged batch of stored audio
    spectral_gate_profile / spectral_gate      the stationary noise gate of data_collection/clean_audio.py:53 (noisereduce's reduce_noise) for a ragged batch
    spectral_gate_nonstationary      noisereduce's default, non-stationary gate (no noise clip: the level follows the recording itself) for a ragged batch
    fused_adamw                      torch.optim.AdamW over the flat parameter arena (transduction_model.py:178,210)
    vocoder_conv1d / vocoder_conv_transpose1d / vocoder_tail      the three kernel families of the HiFi-GAN generator (vocoder.py:16-36), inference only

The package's own entry points (Model.forward, dtw_loss, ctc_loss, FusedAdamW.step, mel_spectrogram, align_from_distances) call these
ops, so the drop-in surface reaches the kernels THROUGH the dispatcher; every op has a fake (meta) implementation for shape inference
and, where the reference differentiates through it, a registered autograd formula whose backward is itself one of the ops.  Ops take
tensors and plain scalars only; per-model state (bound plan, weight copies) is looked up through an integer handle.
Emulator builds (tests) run the same registrations on CPU tensors.
"""
import ctypes
import weakref
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib, ops

_L = _lib.lib
_p = _lib.ptr

# ------------------------------------------------------------------------------------------------ model handles
_models = {}
_next_id = [1]
_KEEP = 2          # saved forward contexts per model (a recognition step runs forward / backward twice before its optimiser step)


def model_handle(model):
    h = getattr(model, '_op_handle', None)
    if h is None:
        h = model._op_handle = _next_id[0]
        _next_id[0] += 1
        _models[h] = weakref.ref(model)
        model._saved_ctx = {}
    return h


def _model(handle):
    ref = _models.get(int(handle))
    m = ref() if ref is not None else None
    if m is None:
        raise RuntimeError('silent_speech::model_*: unknown or freed model handle %d' % handle)
    return m


@torch.library.custom_op('silent_speech::model_forward', mutates_args=())
def model_forward(x_raw: Tensor, anchor: Tensor, handle: int, training: bool, shift_r: int, seed: int) -> Tuple[Tensor, Tensor]:
    """x_raw (B, 8 T, 8) f32 -> head [B T][n_head_cols] f32 = [mel prediction | phoneme logits | pad] per frame.  `anchor` is a
    1-element tensor that requires grad: the parameters are updated in place by model_backward (their .grad live in the flat
    arena), so autograd needs one differentiable input to call the backward formula at all.  The op is FUNCTIONAL: x_raw is not touched; the
    time-shifted signal of a training-mode forward is the second output (empty without a shift) and Model.forward copies it back into its
    argument, mirroring the reference's in-place shift (architecture.py:67-68) outside the operator.  The forward context is kept for the
    backward only when the anchor asks for a gradient (Model.forward hands over a detached anchor under no_grad / in eval mode): a forward
    that will never be back-propagated does not pin its multi-GB workspace."""
    from . import engine
    m = _model(handle)
    head, saved, shifted = engine.forward(m, x_raw, training, shift_r, seed)
    if saved is not None and anchor.requires_grad:
        ctxs = m._saved_ctx
        while len(ctxs) >= _KEEP:                      # a training-mode forward that is never back-propagated must not pin its 5 GB workspace
            ctxs.pop(next(iter(ctxs)))
        ctxs[int(seed)] = saved
    return head, (shifted if shifted is not None else x_raw.new_empty(0))


@model_forward.register_fake
def _(x_raw, anchor, handle, training, shift_r, seed):
    from . import engine
    m = _model(handle)
    return (x_raw.new_empty((x_raw.shape[0] * (x_raw.shape[1] // 8), engine.prepared(m).n_head_cols), dtype=torch.float32),
            torch.empty_like(x_raw) if (training and shift_r > 0) else x_raw.new_empty(0))


@torch.library.custom_op('silent_speech::model_backward', mutates_args=())
def model_backward(dhead: Tensor, handle: int, seed: int) -> None:
    """Accumulates into the .grad of every parameter of the model (flat gradient arena) from d loss / d head."""
    from . import engine
    m = _model(handle)
    saved = m._saved_ctx.pop(int(seed), None)
    if saved is None:
        raise RuntimeError('backward through a forward pass that ran in eval mode, ran twice, or was displaced by %d later forward passes' % _KEEP)
    engine.backward(m, saved, dhead)


@model_backward.register_fake
def _(dhead, handle, seed):
    return None


def _model_setup(ctx, inputs, output):
    ctx.handle, ctx.seed, ctx.training = inputs[2], inputs[5], inputs[3]


def _model_bwd(ctx, dhead, g_shifted):
    if not ctx.training:
        raise RuntimeError('backward through a forward pass that ran in eval mode')
    torch.ops.silent_speech.model_backward(dhead.contiguous(), ctx.handle, ctx.seed)
    return None, None, None, None, None, None


model_forward.register_autograd(_model_bwd, setup_context=_model_setup)


@torch.library.custom_op('silent_speech::model_forward_ragged', mutates_args=())
def model_forward_ragged(x_raw: Tensor, lens: Tensor, handle: int) -> Tensor:
    """Eval-mode forward (running BatchNorm statistics, no dropout, no shift) of B whole utterances in equal slots: x_raw (B, 8 T_max, 8) f32 with utterance
    b in the first 8 lens[b] samples of slot b and zeros behind them, lens (B,) int32 on the same device -> head [B T_max][n_head_cols] f32.  Rows
    [b T_max, b T_max + lens[b]) are exactly what model_forward gives for utterance b alone (its convolutions see zero padding at the utterance's end,
    its attention sees its own keys only); the other rows are unspecified.  NOT differentiable: no autograd formula is registered and nothing is
    saved -- training on ragged slots would need masked BatchNorm statistics and a backward pass."""
    from . import engine
    m = _model(handle)
    host = getattr(m, '_ragged_lens_host', None)           # Model.forward_utterances leaves the lengths it uploaded: profile rows count real attention work
    return engine.forward_ragged(m, x_raw, lens, host if host is not None and len(host) == x_raw.shape[0] else None)


@model_forward_ragged.register_fake
def _(x_raw, lens, handle):
    m = _model(handle)
    n_head_cols = (m.num_outs + (m.num_aux_outs or 0) + 7) // 8 * 8          # the fused heads, as engine.Prepared lays them out
    return x_raw.new_empty((x_raw.shape[0] * (x_raw.shape[1] // 8), n_head_cols), dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ dtw_loss
@torch.library.custom_op('silent_speech::dtw_loss', mutates_args=())
def dtw_loss(head: Tensor, Y: Tensor, phones: Tensor, idx: Tensor, desc: Tensor, n_mel: int, n_ph: int, lam: float, inv_total: float,
             n_voiced: int, n_silent_frames: int, n_silent: int, ws_bytes: int, res_total: int, max_n: int, max_m: int,
             cells: float, perimeter: float) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """head [M][ld] f32; Y / phones: all utterances' targets back to back; idx: the five per-frame int32 tables of ss_loss_index_tables
    back to back (vo_pred, vo_tgt | si_tgt, si_base, si_res; sizes max(n_voiced, 1) resp. max(n_silent_frames, 1)); desc: the DTW
    descriptors of the silent utterances.  Returns (loss [1], correct [1] int32, d loss / d head, alignment results, per-frame arg-max)."""
    dev = head.device
    M, ld = head.shape
    st = _lib.stream_of(head)
    nv, ns = max(n_voiced, 1), max(n_silent_frames, 1)
    vo_pred, vo_tgt = idx[:nv], idx[nv:2 * nv]
    si_tgt, si_base, si_res = idx[2 * nv:2 * nv + ns], idx[2 * nv + ns:2 * nv + 2 * ns], idx[2 * nv + 2 * ns:]
    lse = torch.empty(M, dtype=torch.float32, device=dev)
    amax = torch.empty(M, dtype=torch.int32, device=dev)
    dhead = torch.zeros_like(head)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    correct = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(_L().ss_frame_lse(_p(head), ld, n_mel, n_ph, M, _p(lse), _p(amax), st), 'ss_frame_lse')
    if n_voiced:
        _lib.check(_L().ss_voiced_loss(_p(head), ld, n_mel, n_ph, _p(lse), _p(amax), _p(Y), _p(phones), _p(vo_pred), _p(vo_tgt),
                                       n_voiced, lam, inv_total, _p(dhead), _p(loss), _p(correct), st), 'ss_voiced_loss')
    results = torch.empty(max(res_total, 1), dtype=torch.int32, device=dev)
    if n_silent:
        ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
        ops.timed('silent_cost_skewed_kernel', 0, 4.0 * cells + 4.0 * (n_mel + n_ph) * perimeter,
                  lambda: _lib.check(_L().ss_silent_cost_skewed(_p(head), ld, n_mel, _p(lse), _p(Y), _p(phones), _p(desc), n_silent, max_n, max_m,
                                                                lam, _p(ws), _p(results), st), 'ss_silent_cost_skewed'))
        ops.timed('dtw_kernel', 0, 8.0 * cells,         # 8 N M bytes per matrix (f32 cost in + f32 cumulative out)
                  lambda: _lib.check(_L().ss_dtw_align_skewed(_p(desc), n_silent, _p(ws), _p(results), st), 'ss_dtw_align_skewed'))
        _lib.check(_L().ss_silent_loss(_p(head), ld, n_mel, n_ph, _p(lse), _p(amax), _p(Y), _p(phones), _p(results), _p(si_tgt),
                                       _p(si_base), _p(si_res), n_silent_frames, lam, inv_total, _p(dhead), _p(loss), _p(correct), st), 'ss_silent_loss')
    return loss, correct, dhead, results, amax


@dtw_loss.register_fake
def _(head, Y, phones, idx, desc, n_mel, n_ph, lam, inv_total, n_voiced, n_silent_frames, n_silent, ws_bytes, res_total, max_n, max_m, cells, perimeter):
    M = head.shape[0]
    return (head.new_empty(1), head.new_empty(1, dtype=torch.int32), torch.empty_like(head), head.new_empty(max(res_total, 1), dtype=torch.int32),
            head.new_empty(M, dtype=torch.int32))


def _dtw_setup(ctx, inputs, output):
    ctx.save_for_backward(output[2])           # (an op output kept as a plain attribute would form a tensor -> grad_fn -> ctx -> tensor cycle)


def _dtw_bwd(ctx, g_loss, g_correct, g_dhead, g_results, g_amax):
    return (ctx.saved_tensors[0] * g_loss,) + (None,) * 17


dtw_loss.register_autograd(_dtw_bwd, setup_context=_dtw_setup)


# ------------------------------------------------------------------------------------------------ dtw_align
@torch.library.custom_op('silent_speech::dtw_align', mutates_args=())
def dtw_align(costs: Tensor) -> Tensor:
    """align.py:16-34 on one (N, M) float32 device matrix (any strides: `costs.T` is read in place): int32 [N], results[i] = the column
    the optimal monotone path visits last in row i (first-minimum tie order up, left, diagonal, bit-exact with the reference)."""
    from .align import dtw_align_batch
    if costs.dim() != 2 or costs.dtype != torch.float32:
        raise ValueError('dtw_align: a 2-D float32 matrix is expected')
    N, M = costs.shape
    res, _ = dtw_align_batch(costs, [(N, M)], [0], [costs.stride()])
    return res[:N].clone()


@dtw_align.register_fake
def _(costs):
    return costs.new_empty(costs.shape[0], dtype=torch.int32)


# ------------------------------------------------------------------------------------------------ ctc_loss
@torch.library.custom_op('silent_speech::ctc_loss', mutates_args=())
def ctc_loss(logits: Tensor, desc: Tensor, targets: Tensor, n: int, max_s: int, ws_floats: int, V: int, blank: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """logits [M][V] f32 raw model outputs of the packed rows; desc [n][5] int64 = (first frame, frames, first label, labels, workspace
    offset) per utterance; targets int32.  Returns (mean loss [1], d loss / d logits, per-utterance nll, per-frame arg-max)."""
    dev = logits.device
    M, ld = logits.shape
    st = _lib.stream_of(logits)
    lse = torch.empty(M, dtype=torch.float32, device=dev)
    amax = torch.empty(M, dtype=torch.int32, device=dev)
    _lib.check(_L().ss_frame_lse(_p(logits), ld, 0, V, M, _p(lse), _p(amax), st), 'ss_frame_lse')
    ws = torch.empty(2 * max(ws_floats, 1), dtype=torch.float32, device=dev)
    nll = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    dlogits = torch.empty_like(logits)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    _lib.check(_L().ss_ctc_loss(_p(logits), ld, V, blank, _p(lse), _p(desc) if n else None, n, max_s, M, _p(targets),
                                _p(ws), _p(ws[max(ws_floats, 1):]), _p(nll), _p(dlogits), _p(loss), st), 'ss_ctc_loss')
    return loss, dlogits, nll, amax


@ctc_loss.register_fake
def _(logits, desc, targets, n, max_s, ws_floats, V, blank):
    return logits.new_empty(1), torch.empty_like(logits), logits.new_empty(max(n, 1)), logits.new_empty(logits.shape[0], dtype=torch.int32)


def _ctc_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])


def _ctc_bwd(ctx, g_loss, g_dl, g_nll, g_amax):
    return (ctx.saved_tensors[0] * g_loss,) + (None,) * 7


ctc_loss.register_autograd(_ctc_bwd, setup_context=_ctc_setup)


# ------------------------------------------------------------------------------------------------ ctc_nbest_logp / nbest_expected_risk
def _nbest_tables(name, logits, utt, hyp, targets):
    dev = logits.device
    if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise RuntimeError('%s: logits must be a contiguous (frames, ld) float32 matrix' % name)
    if utt.dim() != 2 or utt.shape[1] != 4 or utt.dtype != torch.int64 or not utt.is_contiguous() or utt.device != dev:
        raise RuntimeError('%s: utt must be a contiguous (n, 4) int64 table on the device of the logits' % name)
    if hyp.dim() != 2 or hyp.shape[1] != 3 or hyp.dtype != torch.int64 or not hyp.is_contiguous() or hyp.device != dev:
        raise RuntimeError('%s: hyp must be a contiguous (n, 3) int64 table on the device of the logits' % name)
    if targets.dim() != 1 or targets.dtype != torch.int32 or not targets.is_contiguous() or targets.device != dev:
        raise RuntimeError('%s: targets must be a contiguous flat int32 tensor on the device of the logits' % name)


@torch.library.custom_op('silent_speech::ctc_nbest_logp', mutates_args=())
def ctc_nbest_logp(logits: Tensor, utt: Tensor, hyp: Tensor, targets: Tensor, max_s: int, ws_floats: int, V: int, blank: int) -> Tuple[Tensor, Tensor, Tensor]:
    """Full-sum CTC log-likelihood of several label strings per utterance (ss_ctc_nbest_logp in include/silent_speech_hip.h states the
    definition).  logits [M][ld >= V] f32 raw model outputs; utt [n][4] int64 = (first frame, frames, first hypothesis, K); hyp [H][3] int64 =
    (first label in targets, S, workspace offset in floats); targets int32; max_s >= the longest hypothesis, ws_floats = the sum of the
    T (2 S + 1) blocks.  Returns (logp [H] f32, per-frame lse [M], the workspace the backward pass reads)."""
    _nbest_tables('ctc_nbest_logp', logits, utt, hyp, targets)
    dev = logits.device
    M, ld = logits.shape
    H = hyp.shape[0]
    st = _lib.stream_of(logits)
    ws_bytes = _L().ss_ctc_nbest_workspace_bytes(H, ws_floats)
    if ws_bytes < 0:
        raise RuntimeError('ctc_nbest_logp: %d hypotheses with %d workspace floats' % (H, ws_floats))
    lse = torch.empty(max(M, 1), dtype=torch.float32, device=dev)
    amax = torch.empty(max(M, 1), dtype=torch.int32, device=dev)
    if M:
        _lib.check(_L().ss_frame_lse(_p(logits), ld, 0, V, M, _p(lse), _p(amax), st), 'ss_frame_lse')
    ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=dev)
    logp = torch.empty(H, dtype=torch.float32, device=dev)
    _lib.check(_L().ss_ctc_nbest_logp(_p(logits) if M else None, ld, V, blank, M, _p(lse), _p(utt) if utt.shape[0] else None, utt.shape[0],
                                      _p(hyp) if H else None, H, max_s, _p(targets) if targets.shape[0] else None, targets.shape[0], _p(ws), ws_floats,
                                      _p(logp) if H else None, st), 'ss_ctc_nbest_logp')
    return logp, lse, ws


@ctc_nbest_logp.register_fake
def _(logits, utt, hyp, targets, max_s, ws_floats, V, blank):
    return (logits.new_empty(hyp.shape[0]), logits.new_empty(max(logits.shape[0], 1)),
            logits.new_empty(torch.library.get_ctx().new_dynamic_size(), dtype=torch.int64))


@torch.library.custom_op('silent_speech::ctc_nbest_backward', mutates_args=())
def ctc_nbest_backward(logits: Tensor, lse: Tensor, utt: Tensor, hyp: Tensor, targets: Tensor, ws: Tensor, logp: Tensor, g: Tensor,
                       ws_floats: int, V: int, blank: int) -> Tensor:
    """d (sum_h g_h logp_h) / d logits for the outputs of ctc_nbest_logp (ss_ctc_nbest_backward): every row of the result is written."""
    _nbest_tables('ctc_nbest_backward', logits, utt, hyp, targets)
    M, ld = logits.shape
    H = hyp.shape[0]
    g = g.to(torch.float32).contiguous()
    if g.shape != (H,) or logp.shape != (H,):
        raise RuntimeError('ctc_nbest_backward: %d cotangents for %d hypotheses' % (g.numel(), H))
    dlogits = torch.empty_like(logits)
    _lib.check(_L().ss_ctc_nbest_backward(_p(logits) if M else None, ld, V, blank, M, _p(lse), _p(utt) if utt.shape[0] else None, utt.shape[0], H,
                                          _p(targets) if targets.shape[0] else None, _p(ws), ws_floats, _p(logp) if H else None, _p(g) if H else None,
                                          _p(dlogits) if M else None, _lib.stream_of(logits)), 'ss_ctc_nbest_backward')
    return dlogits


@ctc_nbest_backward.register_fake
def _(logits, lse, utt, hyp, targets, ws, logp, g, ws_floats, V, blank):
    return torch.empty_like(logits)


def _ctc_nbest_setup(ctx, inputs, output):
    logits, utt, hyp, targets, max_s, ws_floats, V, blank = inputs
    ctx.save_for_backward(logits, utt, hyp, targets, output[0], output[1], output[2])
    ctx.nbest_args = (ws_floats, V, blank)


def _ctc_nbest_bwd(ctx, g_logp, g_lse, g_ws):
    logits, utt, hyp, targets, logp, lse, ws = ctx.saved_tensors
    ws_floats, V, blank = ctx.nbest_args
    if g_logp is None:
        g_logp = torch.zeros_like(logp)
    return (ctc_nbest_backward(logits, lse, utt, hyp, targets, ws, logp, g_logp, ws_floats, V, blank),) + (None,) * 7


ctc_nbest_logp.register_autograd(_ctc_nbest_bwd, setup_context=_ctc_nbest_setup)


@torch.library.custom_op('silent_speech::nbest_expected_risk', mutates_args=())
def nbest_expected_risk(logp: Tensor, cost: Tensor, groups: Tensor, scale: float) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Expected risk of n-best lists under their own posterior softmax(scale logp) (ss_nbest_expected_risk in include/silent_speech_hip.h):
    logp, cost [H] f32; groups [n][2] int64 = (first hypothesis, K <= 128).  Returns (loss [1] f32 = the mean risk over the lists that have a
    finite entry, risk [n] f64, post [H] f32, dlogp [H] f32 = d loss / d logp); autograd reaches logp through dlogp."""
    dev = logp.device
    H, ng = logp.shape[0], groups.shape[0]
    if logp.dim() != 1 or logp.dtype != torch.float32 or cost.shape != logp.shape or cost.dtype != torch.float32 or cost.device != dev:
        raise RuntimeError('nbest_expected_risk: logp and cost must be float32 vectors of one length on one device')
    if groups.dim() != 2 or groups.shape[1] != 2 or groups.dtype != torch.int64 or not groups.is_contiguous() or groups.device != dev:
        raise RuntimeError('nbest_expected_risk: groups must be a contiguous (n, 2) int64 table (first hypothesis, K) on the device of logp')
    if ng > 65535:
        raise RuntimeError('nbest_expected_risk: %d lists (at most 65535 in one call)' % ng)
    logp, cost = logp.contiguous(), cost.contiguous()
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    risk = torch.empty(ng, dtype=torch.float64, device=dev)
    post = torch.empty(H, dtype=torch.float32, device=dev)
    dlogp = torch.empty(H, dtype=torch.float32, device=dev)
    _lib.check(_L().ss_nbest_expected_risk(_p(logp) if H else None, _p(cost) if H else None, H, _p(groups) if ng else None, ng, scale, _p(loss),
                                           _p(risk) if ng else None, _p(post) if H else None, _p(dlogp) if H else None, _lib.stream_of(logp)),
               'ss_nbest_expected_risk')
    return loss, risk, post, dlogp


@nbest_expected_risk.register_fake
def _(logp, cost, groups, scale):
    return logp.new_empty(1), logp.new_empty(groups.shape[0], dtype=torch.float64), torch.empty_like(logp), torch.empty_like(logp)


def _nbest_risk_setup(ctx, inputs, output):
    ctx.save_for_backward(output[3])


def _nbest_risk_bwd(ctx, g_loss, g_risk, g_post, g_dlogp):
    return ctx.saved_tensors[0] * g_loss, None, None, None


nbest_expected_risk.register_autograd(_nbest_risk_bwd, setup_context=_nbest_risk_setup)


# ------------------------------------------------------------------------------------------------ ctc_beam_search (inference only: no autograd)
def _beam_search_checks(name, min_classes, logits, utt, V, blank, total_frames, max_len, beam_width, n_best):
    """The argument checks ctc_beam_search and ctc_word_beam_search share."""
    if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise RuntimeError('%s: logits must be a contiguous (frames, ld) float32 matrix' % name)
    if utt.dim() != 2 or utt.shape[1] != 2 or utt.dtype != torch.int64 or not utt.is_contiguous() or utt.device != logits.device:
        raise RuntimeError('%s: utt must be a contiguous (n, 2) int64 table on the device of the logits' % name)
    # everything the launches rely on is checked HERE: ss_frame_lse reads V columns at stride ld whatever it is told
    if not (min_classes <= V <= min(logits.shape[1], 128)) or not (0 <= blank < V):
        raise RuntimeError('%s: %d classes (%d .. min(row stride %d, 128)), blank %d' % (name, V, min_classes, logits.shape[1], blank))
    if not (1 <= beam_width <= 128) or not (1 <= n_best <= beam_width):
        raise RuntimeError('%s: beam width %d (1 .. 128), n_best %d (1 .. beam width)' % (name, beam_width, n_best))
    if max_len < 1 or total_frames < 0:
        raise RuntimeError('%s: max_len %d, total_frames %d' % (name, max_len, total_frames))


def _beam_search_buffers(name, logits, utt, V, total_frames, max_len, beam_width, n_best, workspace_bytes):
    """Behind the checks: the per-frame lse launch, the trie workspace and the outputs every search has.
    Returns (lse, workspace, stream, (labels, lengths, scores, ctc_scores))."""
    dev = logits.device
    M, ld = logits.shape
    n = utt.shape[0]
    st = _lib.stream_of(logits)
    ws_bytes = workspace_bytes(n, total_frames, beam_width)
    if ws_bytes < 0:
        raise RuntimeError('%s: beam width %d (1 .. 128)' % (name, beam_width))
    lse = torch.empty(max(M, 1), dtype=torch.float32, device=dev)
    amax = torch.empty(max(M, 1), dtype=torch.int32, device=dev)
    if M:
        _lib.check(_L().ss_frame_lse(_p(logits), ld, 0, V, M, _p(lse), _p(amax), st), 'ss_frame_lse')
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    labels = torch.empty((n, n_best, max_len), dtype=torch.int32, device=dev)
    lengths = torch.empty((n, n_best), dtype=torch.int32, device=dev)
    scores = torch.empty((n, n_best), dtype=torch.float32, device=dev)
    ctc_scores = torch.empty((n, n_best), dtype=torch.float32, device=dev)
    return lse, ws, st, (labels, lengths, scores, ctc_scores)


@torch.library.custom_op('silent_speech::ctc_beam_search', mutates_args=())
def ctc_beam_search(logits: Tensor, utt: Tensor, V: int, blank: int, total_frames: int, max_len: int, beam_width: int, n_best: int,
                    lm: Optional[Tensor], alpha: float, beta: float) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """CTC prefix beam search (ss_ctc_beam_search in include/silent_speech_hip.h states the algorithm).  logits [M][ld >= V] f32 raw model
    outputs; utt [n][2] int64 on the device = (first frame, frames) per utterance, packed or slot layout; total_frames >= the sum of the
    frames, max_len >= the longest utterance; lm: optional (V, V, V - 1) f32 table of natural-log label probabilities, weights alpha, beta.
    Returns (labels [n][n_best][max_len] int32 with -1 behind the end, lengths [n][n_best] int32 (-1: no such rank), scores, CTC scores [n][n_best])."""
    _beam_search_checks('ctc_beam_search', 1, logits, utt, V, blank, total_frames, max_len, beam_width, n_best)
    if lm is not None and (lm.shape != (V, V, V - 1) or lm.dtype != torch.float32 or not lm.is_contiguous() or lm.device != logits.device):
        raise RuntimeError('ctc_beam_search: the label table must be a contiguous (%d, %d, %d) float32 tensor on the device of the logits' % (V, V, V - 1))
    lse, ws, st, out = _beam_search_buffers('ctc_beam_search', logits, utt, V, total_frames, max_len, beam_width, n_best, _L().ss_ctc_beam_workspace_bytes)
    n = utt.shape[0]
    _lib.check(_L().ss_ctc_beam_search(_p(logits), logits.shape[1], V, blank, logits.shape[0], _p(lse), _p(utt) if n else None, n, total_frames, beam_width, n_best,
                                       _p(lm), alpha, beta, _p(ws), max_len, *(_p(t) for t in out), st), 'ss_ctc_beam_search')
    return out


@ctc_beam_search.register_fake
def _(logits, utt, V, blank, total_frames, max_len, beam_width, n_best, lm, alpha, beta):
    n = utt.shape[0]
    return (logits.new_empty((n, n_best, max_len), dtype=torch.int32), logits.new_empty((n, n_best), dtype=torch.int32),
            logits.new_empty((n, n_best)), logits.new_empty((n, n_best)))


# ------------------------------------------------------------------------------------------------ ctc_word_beam_search / word_ngram_score (inference only)
def _word_tables(name, dev, uni, bi_keys, bi_val, tri_keys, tri_val, bi_probe, tri_probe):
    """Checks the n-gram tables of a WordNgramLM (ss_word_lm in include/silent_speech_hip.h) and fills the part of the struct they make up."""
    def bad(t, dtype, dim):
        return t.dtype != dtype or t.dim() != dim or not t.is_contiguous() or t.device != dev
    if bad(uni, torch.float32, 2) or uni.shape[0] != 2 or not (1 <= uni.shape[1] <= 1 << 21):
        raise RuntimeError('%s: the unigram table must be a contiguous (2, n <= 2^21) float32 tensor on the device of the input' % name)
    nb, nt = bi_keys.shape[0] if bi_keys.dim() == 1 else -1, tri_keys.shape[0] if tri_keys.dim() == 1 else -1
    if bad(bi_keys, torch.int64, 1) or bad(bi_val, torch.float32, 2) or tuple(bi_val.shape) != (2, nb) or nb & (nb - 1) or not (0 <= bi_probe <= nb):
        raise RuntimeError('%s: the bigram table must be int64 keys (slots) and float32 values (2, slots) on the device of the input, '
                           'slots 0 or a power of two, longest probe within them' % name)
    if bad(tri_keys, torch.int64, 1) or bad(tri_val, torch.float32, 1) or tri_val.shape[0] != nt or nt & (nt - 1) or not (0 <= tri_probe <= nt):
        raise RuntimeError('%s: the trigram table must be int64 keys (slots) and float32 values (slots) on the device of the input, '
                           'slots 0 or a power of two, longest probe within them' % name)
    n_uni = uni.shape[1]
    lm = _lib.WordLm()
    lm.uni_logp, lm.uni_bo = uni.data_ptr(), uni.data_ptr() + 4 * n_uni
    lm.bi_keys, lm.bi_logp, lm.bi_bo = (bi_keys.data_ptr(), bi_val.data_ptr(), bi_val.data_ptr() + 4 * nb) if nb else (None, None, None)
    lm.tri_keys, lm.tri_logp = (tri_keys.data_ptr(), tri_val.data_ptr()) if nt else (None, None)
    lm.n_uni, lm.n_vocab, lm.start, lm.n_nodes = n_uni, n_uni, 0, 0
    lm.bi_slots, lm.bi_probe, lm.tri_slots, lm.tri_probe = nb, bi_probe, nt, tri_probe
    _p(uni)                                                              # (the one place that refuses memory the kernels cannot read)
    return lm


@torch.library.custom_op('silent_speech::ctc_word_beam_search', mutates_args=())
def ctc_word_beam_search(logits: Tensor, utt: Tensor, V: int, blank: int, space: int, total_frames: int, max_len: int, beam_width: int, n_best: int,
                         lex_child: Tensor, lex_word: Tensor, uni: Tensor, bi_keys: Tensor, bi_val: Tensor, tri_keys: Tensor, tri_val: Tensor,
                         n_vocab: int, start: int, bi_probe: int, tri_probe: int, alpha: float, beta: float) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Lexicon-constrained CTC prefix beam search with a word n-gram (ss_ctc_word_beam_search in include/silent_speech_hip.h states the algorithm).
    logits, utt, V, blank, total_frames, max_len, beam_width, n_best as for ctc_beam_search; space: the class that ends a word.  The tables are
    the device form of recognition_model.WordNgramLM: lex_child [n_nodes][V - 1] int32, lex_word [n_nodes] int32, uni [2][n_uni] f32 (ln P, backoff),
    bi_keys [slots] int64 + bi_val [2][slots] f32, tri_keys [slots] int64 + tri_val [slots] f32, the word ids 0 .. n_vocab - 1 of the lexicon, the
    id of the start context and the longest probe sequence of each hash table.
    Returns (labels, lengths, scores, CTC scores) as ctc_beam_search and complete [n][n_best] int32 (1 / 0; -1: no such rank)."""
    dev = logits.device
    _beam_search_checks('ctc_word_beam_search', 2, logits, utt, V, blank, total_frames, max_len, beam_width, n_best)
    if not (0 <= space < V) or space == blank:
        raise RuntimeError('ctc_word_beam_search: space class %d (0 .. %d, not the blank %d)' % (space, V - 1, blank))
    if lex_child.dim() != 2 or lex_child.shape[0] < 1 or lex_child.shape[1] != V - 1 or lex_child.dtype != torch.int32 or not lex_child.is_contiguous() or \
            lex_child.device != dev or tuple(lex_word.shape) != (lex_child.shape[0],) or lex_word.dtype != torch.int32 or not lex_word.is_contiguous() or lex_word.device != dev:
        raise RuntimeError('ctc_word_beam_search: the lexicon must be contiguous int32 tensors (n_nodes >= 1, %d) and (n_nodes) on the device of the logits' % (V - 1))
    lm = _word_tables('ctc_word_beam_search', dev, uni, bi_keys, bi_val, tri_keys, tri_val, bi_probe, tri_probe)
    if not (0 <= n_vocab <= lm.n_uni) or not (0 <= start < lm.n_uni):
        raise RuntimeError('ctc_word_beam_search: %d words, start id %d, but %d word ids' % (n_vocab, start, lm.n_uni))
    lm.lex_child, lm.lex_word, lm.n_nodes, lm.n_vocab, lm.start = lex_child.data_ptr(), lex_word.data_ptr(), lex_child.shape[0], n_vocab, start
    lse, ws, st, out = _beam_search_buffers('ctc_word_beam_search', logits, utt, V, total_frames, max_len, beam_width, n_best, _L().ss_ctc_word_beam_workspace_bytes)
    n = utt.shape[0]
    complete = torch.empty((n, n_best), dtype=torch.int32, device=dev)
    _lib.check(_L().ss_ctc_word_beam_search(_p(logits), logits.shape[1], V, blank, space, logits.shape[0], _p(lse), _p(utt) if n else None, n, total_frames, beam_width,
                                            n_best, ctypes.byref(lm), alpha, beta, _p(ws), max_len, *(_p(t) for t in out), _p(complete), st), 'ss_ctc_word_beam_search')
    return out + (complete,)


@ctc_word_beam_search.register_fake
def _(logits, utt, V, blank, space, total_frames, max_len, beam_width, n_best, lex_child, lex_word, uni, bi_keys, bi_val, tri_keys, tri_val,
      n_vocab, start, bi_probe, tri_probe, alpha, beta):
    n = utt.shape[0]
    return (logits.new_empty((n, n_best, max_len), dtype=torch.int32), logits.new_empty((n, n_best), dtype=torch.int32),
            logits.new_empty((n, n_best)), logits.new_empty((n, n_best)), logits.new_empty((n, n_best), dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ ctc_forced_align (inference only: no autograd)
@torch.library.custom_op('silent_speech::ctc_forced_align', mutates_args=())
def ctc_forced_align(logits: Tensor, utt: Tensor, targets: Tensor, V: int, blank: int, total_frames: int,
                     max_target_len: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Best alignment of known label strings to the frame posteriors (ss_ctc_align in include/silent_speech_hip.h states the definition and the
    ties).  logits [M][ld >= V] f32 raw model outputs; utt [n][4] int64 on the device = (first frame, frames, first target index, target length)
    per utterance, packed or slot layout; targets flat int32; blank in [0, V), or -1 for the linear topology of a head without a blank;
    total_frames >= the sum of the frames, max_target_len >= the longest target (<= 511).
    Returns (score [n] f32, frame_token [M] int32: token index, -1 blank, -2 no utterance / no alignment, and parallel to targets token_first,
    token_frames int32 and token_logp f32: -1 / 0 / 0 where no alignment exists)."""
    dev = logits.device
    if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise RuntimeError('ctc_forced_align: logits must be a contiguous (frames, ld) float32 matrix')
    if utt.dim() != 2 or utt.shape[1] != 4 or utt.dtype != torch.int64 or not utt.is_contiguous() or utt.device != dev:
        raise RuntimeError('ctc_forced_align: utt must be a contiguous (n, 4) int64 table on the device of the logits')
    if targets.dim() != 1 or targets.dtype != torch.int32 or not targets.is_contiguous() or targets.device != dev:
        raise RuntimeError('ctc_forced_align: targets must be a contiguous flat int32 tensor on the device of the logits')
    # everything the launches below rely on is checked HERE: ss_frame_lse reads V columns at stride ld whatever it is told
    if not (1 <= V <= min(logits.shape[1], 4096)) or not (-1 <= blank < V):
        raise RuntimeError('ctc_forced_align: %d classes (1 .. min(row stride %d, 4096)), blank %d (-1: linear topology)' % (V, logits.shape[1], blank))
    if not (0 <= max_target_len <= 511) or total_frames < 0:
        raise RuntimeError('ctc_forced_align: max_target_len %d (0 .. 511), total_frames %d' % (max_target_len, total_frames))
    M, ld = logits.shape
    n, nt = utt.shape[0], targets.shape[0]
    st = _lib.stream_of(logits)
    ws_bytes = _L().ss_ctc_align_workspace_bytes(n, total_frames, max_target_len)
    if ws_bytes < 0:
        raise RuntimeError('ctc_forced_align: max_target_len %d (0 .. 511)' % max_target_len)
    lse = torch.empty(max(M, 1), dtype=torch.float32, device=dev)
    amax = torch.empty(max(M, 1), dtype=torch.int32, device=dev)
    if M:
        _lib.check(_L().ss_frame_lse(_p(logits), ld, 0, V, M, _p(lse), _p(amax), st), 'ss_frame_lse')
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    frame_token = torch.empty(M, dtype=torch.int32, device=dev)
    token_first = torch.empty(nt, dtype=torch.int32, device=dev)
    token_frames = torch.empty(nt, dtype=torch.int32, device=dev)
    token_logp = torch.empty(nt, dtype=torch.float32, device=dev)
    _lib.check(_L().ss_ctc_align(_p(logits), ld, V, blank, M, _p(lse), _p(utt) if n else None, n, total_frames, max_target_len,
                                 _p(targets) if nt else None, nt, _p(ws), _p(score) if n else None, _p(frame_token) if M else None,
                                 _p(token_first) if nt else None, _p(token_frames) if nt else None, _p(token_logp) if nt else None, st), 'ss_ctc_align')
    return score, frame_token, token_first, token_frames, token_logp


@ctc_forced_align.register_fake
def _(logits, utt, targets, V, blank, total_frames, max_target_len):
    n, nt = utt.shape[0], targets.shape[0]
    return (logits.new_empty((n,)), logits.new_empty((logits.shape[0],), dtype=torch.int32), logits.new_empty((nt,), dtype=torch.int32),
            logits.new_empty((nt,), dtype=torch.int32), logits.new_empty((nt,)))


# ------------------------------------------------------------------------------------------------ edit_distance / nbest_risk (scoring: no autograd)
MAX_EDIT_TOKENS = 1023
MAX_NBEST = 128


def _edit_tables(name, tokens, seqs):
    dev = tokens.device
    if tokens.dim() != 1 or tokens.dtype != torch.int32 or not tokens.is_contiguous():
        raise RuntimeError('%s: tokens must be a contiguous flat int32 tensor' % name)
    if seqs.dim() != 2 or seqs.shape[1] != 2 or seqs.dtype != torch.int64 or not seqs.is_contiguous() or seqs.device != dev:
        raise RuntimeError('%s: seqs must be a contiguous (n, 2) int64 table (first token, length) on the device of the tokens' % name)


@torch.library.custom_op('silent_speech::edit_distance', mutates_args=())
def edit_distance(tokens: Tensor, seqs: Tensor, pairs: Tensor, want_ops: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Levenshtein distance, error breakdown and (want_ops) alignment of a batch of pairs in one launch (ss_edit_distance in
    include/silent_speech_hip.h states the definition and the ties).  tokens flat int32; seqs [n_seq][2] int64 = (first token, length <= 1023);
    pairs [n][2] int32 = (reference sequence, hypothesis sequence).
    Returns (dist [n] int32, counts [n][4] int32 = hits, substitutions, deletions, insertions, ops int8, ops_first [n + 1] int64): pair p's
    alignment is ops[ops_first[p] : ops_first[p + 1]] (n_a + n_b bytes: 0 hit, 1 substitution, 2 deletion, 3 insertion from the beginning, then
    -1); both are empty without want_ops.  A pair with a bad table entry gets -1s (and no ops bytes)."""
    dev = tokens.device
    _edit_tables('edit_distance', tokens, seqs)
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int32 or not pairs.is_contiguous() or pairs.device != dev:
        raise RuntimeError('edit_distance: pairs must be a contiguous (n, 2) int32 table on the device of the tokens')
    n, n_seq, n_tok = pairs.shape[0], seqs.shape[0], tokens.shape[0]
    if n > 1 << 24:
        raise RuntimeError('edit_distance: %d pairs (at most 2^24 in one launch)' % n)
    dist = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty((n, 4), dtype=torch.int32, device=dev)
    ops = torch.empty(0, dtype=torch.int8, device=dev)
    ops_first = torch.empty(0, dtype=torch.int64, device=dev)
    ws = None
    n_ops = 0
    if want_ops:
        # the room of every pair, from the tables where they lie: n_a + n_b of the entries that are in range, none for the others
        ops_first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if n and n_seq:
            ln = seqs[:, 1]
            ln = torch.where((ln >= 0) & (ln <= MAX_EDIT_TOKENS), ln, torch.zeros_like(ln))
            ix = pairs.to(torch.int64)
            inside = ((ix >= 0) & (ix < n_seq)).all(1)
            room = ln[ix.clamp(0, n_seq - 1)].sum(1) * inside
            ops_first[1:] = torch.cumsum(room, 0)
            n_ops = int(ops_first[-1])
        ops = torch.empty(n_ops, dtype=torch.int8, device=dev)
        ws_bytes = _L().ss_edit_distance_workspace_bytes(n, n_ops)
        if ws_bytes < 0:
            raise RuntimeError('edit_distance: %d pairs with %d alignment bytes' % (n, n_ops))
        ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.int32, device=dev)
    if n:
        _lib.check(_L().ss_edit_distance(_p(tokens) if n_tok else None, n_tok, _p(seqs) if n_seq else None, n_seq, _p(pairs), n, _p(dist), _p(counts),
                                         _p(ops) if n_ops else None, _p(ops_first) if want_ops else None, n_ops, _p(ws), _lib.stream_of(tokens)), 'ss_edit_distance')
    return dist, counts, ops, ops_first


@edit_distance.register_fake
def _(tokens, seqs, pairs, want_ops):
    n = pairs.shape[0]
    n_ops = torch.library.get_ctx().new_dynamic_size() if want_ops else 0
    return (tokens.new_empty((n,)), tokens.new_empty((n, 4)), tokens.new_empty((n_ops,), dtype=torch.int8),
            tokens.new_empty((n + 1 if want_ops else 0,), dtype=torch.int64))


@torch.library.custom_op('silent_speech::nbest_risk', mutates_args=())
def nbest_risk(tokens: Tensor, seqs: Tensor, groups: Tensor, weights: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """Minimum-Bayes-risk selection from n-best lists (ss_nbest_risk in include/silent_speech_hip.h): tokens, seqs as for edit_distance; groups
    [n_groups][2] int64 = (first sequence, K <= 128 consecutive sequences, rank order); weights [n_seq] f32, the posterior of every sequence
    within its list.  Returns (dmat int32, group g's K x K distance matrix at the sum of the K^2 before it, risk [n_seq] f64 =
    sum_k weights[k] dmat[i][k] in ascending k (NaN outside every group), pick [n_groups] int32 = the smallest index of least risk; -1 and NaN
    risks for a group with a bad table entry).  The group sizes are read back once to size dmat."""
    dev = tokens.device
    _edit_tables('nbest_risk', tokens, seqs)
    if groups.dim() != 2 or groups.shape[1] != 2 or groups.dtype != torch.int64 or not groups.is_contiguous() or groups.device != dev:
        raise RuntimeError('nbest_risk: groups must be a contiguous (n, 2) int64 table (first sequence, K) on the device of the tokens')
    n_seq, n_tok, ng = seqs.shape[0], tokens.shape[0], groups.shape[0]
    if weights.dim() != 1 or weights.shape[0] != n_seq or weights.dtype != torch.float32 or not weights.is_contiguous() or weights.device != dev:
        raise RuntimeError('nbest_risk: weights must be a contiguous (%d) float32 tensor on the device of the tokens' % n_seq)
    if ng > 65535:
        raise RuntimeError('nbest_risk: %d groups (at most 65535 in one call)' % ng)
    K = groups[:, 1].cpu()
    if ng and (int(K.min()) < 1 or int(K.max()) > MAX_NBEST):
        raise RuntimeError('nbest_risk: groups of %d .. %d sequences (1 .. %d)' % (int(K.min()), int(K.max()), MAX_NBEST))
    n_dmat = int((K * K).sum())
    dmat = torch.empty(n_dmat, dtype=torch.int32, device=dev)
    risk = torch.full((n_seq,), float('nan'), dtype=torch.float64, device=dev)
    pick = torch.empty(ng, dtype=torch.int32, device=dev)
    if ng:
        _lib.check(_L().ss_nbest_risk(_p(tokens) if n_tok else None, n_tok, _p(seqs) if n_seq else None, n_seq, _p(groups), ng, int(K.max()),
                                      _p(weights) if n_seq else None, _p(dmat) if n_dmat else None, n_dmat, _p(risk) if n_seq else None, _p(pick),
                                      _lib.stream_of(tokens)), 'ss_nbest_risk')
    return dmat, risk, pick


@nbest_risk.register_fake
def _(tokens, seqs, groups, weights):
    return (tokens.new_empty((torch.library.get_ctx().new_dynamic_size(),)), tokens.new_empty((seqs.shape[0],), dtype=torch.float64),
            tokens.new_empty((groups.shape[0],)))


@torch.library.custom_op('silent_speech::word_ngram_score', mutates_args=())
def word_ngram_score(triples: Tensor, uni: Tensor, bi_keys: Tensor, bi_val: Tensor, tri_keys: Tensor, tri_val: Tensor, bi_probe: int, tri_probe: int) -> Tensor:
    """ln P(w | w2, w1) of every row (w2, w1, w) of triples [n][3] int32 (-1 = no such context word) by the backoff rule of ss_word_lm, with the
    device function the word beam search uses.  An id outside the tables gives NaN.  Returns [n] f32."""
    dev = triples.device
    if triples.dim() != 2 or triples.shape[1] != 3 or triples.dtype != torch.int32 or not triples.is_contiguous():
        raise RuntimeError('word_ngram_score: triples must be a contiguous (n, 3) int32 tensor')
    lm = _word_tables('word_ngram_score', dev, uni, bi_keys, bi_val, tri_keys, tri_val, bi_probe, tri_probe)
    out = torch.empty(triples.shape[0], dtype=torch.float32, device=dev)
    _lib.check(_L().ss_word_ngram_score(ctypes.byref(lm), _p(triples), triples.shape[0], _p(out), _lib.stream_of(triples)), 'ss_word_ngram_score')
    return out


@word_ngram_score.register_fake
def _(triples, uni, bi_keys, bi_val, tri_keys, tri_val, bi_probe, tri_probe):
    return triples.new_empty((triples.shape[0],), dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ ctc_word_state_beam_search / word_state_score (inference only)
def _word_state_tables(name, dev, uni_logp, st_bo, st_shorter, arc_keys, arc_logp, arc_next, arc_probe, order):
    """Checks the tables of a WordStateLM (ss_word_state_lm in include/silent_speech_hip.h) and fills the part of the struct they make up."""
    def bad(t, dtype):
        return t.dtype != dtype or t.dim() != 1 or not t.is_contiguous() or t.device != dev
    if not (1 <= order <= 6):
        raise RuntimeError('%s: order %d (1 .. 6)' % (name, order))
    if bad(uni_logp, torch.float32) or not (1 <= uni_logp.shape[0] <= 1 << 21):
        raise RuntimeError('%s: the unigram table must be a contiguous (n <= 2^21) float32 tensor on the device of the input' % name)
    n_uni = uni_logp.shape[0]
    if bad(st_bo, torch.float32) or bad(st_shorter, torch.int32) or st_bo.shape[0] != st_shorter.shape[0] or st_bo.shape[0] < n_uni + 1 or st_bo.shape[0] >= 1 << 31:
        raise RuntimeError('%s: the state tables must be float32 backoffs and int32 suffix links of one length >= %d (the empty context and one state per word id) '
                           'on the device of the input' % (name, n_uni + 1))
    slots = arc_keys.shape[0] if arc_keys.dim() == 1 else -1
    if bad(arc_keys, torch.int64) or bad(arc_logp, torch.float32) or bad(arc_next, torch.int32) or arc_logp.shape[0] != slots or arc_next.shape[0] != slots or \
            slots & (slots - 1) or not (0 <= arc_probe <= slots):
        raise RuntimeError('%s: the arc table must be int64 keys, float32 values and int32 next states (slots) on the device of the input, '
                           'slots 0 or a power of two, longest probe within them' % name)
    lm = _lib.WordStateLm()
    lm.uni_logp, lm.st_bo, lm.st_shorter = uni_logp.data_ptr(), st_bo.data_ptr(), st_shorter.data_ptr()
    lm.arc_keys, lm.arc_logp, lm.arc_next = (arc_keys.data_ptr(), arc_logp.data_ptr(), arc_next.data_ptr()) if slots else (None, None, None)
    lm.n_uni, lm.n_vocab, lm.n_states, lm.start_state, lm.n_nodes = n_uni, n_uni, st_bo.shape[0], 0, 0
    lm.arc_slots, lm.arc_probe, lm.order = slots, arc_probe, order
    _p(uni_logp)                                                         # (the one place that refuses memory the kernels cannot read)
    return lm


@torch.library.custom_op('silent_speech::ctc_word_state_beam_search', mutates_args=())
def ctc_word_state_beam_search(logits: Tensor, utt: Tensor, V: int, blank: int, space: int, total_frames: int, max_len: int, beam_width: int, n_best: int,
                               lex_child: Tensor, lex_word: Tensor, uni_logp: Tensor, st_bo: Tensor, st_shorter: Tensor, arc_keys: Tensor, arc_logp: Tensor,
                               arc_next: Tensor, n_vocab: int, start_state: int, arc_probe: int, order: int, alpha: float,
                               beta: float) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """ctc_word_beam_search with a word n-gram of any order 1 .. 6 held as context states (ss_ctc_word_state_beam_search in
    include/silent_speech_hip.h).  logits .. n_best, lex_child, lex_word as for ctc_word_beam_search.  The tables are the device form of
    recognition_model.WordStateLM: uni_logp [n_uni] f32, st_bo [n_states] f32 + st_shorter [n_states] int32, arc_keys [slots] int64 + arc_logp
    [slots] f32 + arc_next [slots] int32, the word ids 0 .. n_vocab - 1 of the lexicon, the state of the start context, the longest probe sequence
    of the arc table and the order.  Returns (labels, lengths, scores, CTC scores, complete) as ctc_word_beam_search."""
    dev = logits.device
    _beam_search_checks('ctc_word_state_beam_search', 2, logits, utt, V, blank, total_frames, max_len, beam_width, n_best)
    if not (0 <= space < V) or space == blank:
        raise RuntimeError('ctc_word_state_beam_search: space class %d (0 .. %d, not the blank %d)' % (space, V - 1, blank))
    if lex_child.dim() != 2 or lex_child.shape[0] < 1 or lex_child.shape[1] != V - 1 or lex_child.dtype != torch.int32 or not lex_child.is_contiguous() or \
            lex_child.device != dev or tuple(lex_word.shape) != (lex_child.shape[0],) or lex_word.dtype != torch.int32 or not lex_word.is_contiguous() or lex_word.device != dev:
        raise RuntimeError('ctc_word_state_beam_search: the lexicon must be contiguous int32 tensors (n_nodes >= 1, %d) and (n_nodes) on the device of the logits' % (V - 1))
    lm = _word_state_tables('ctc_word_state_beam_search', dev, uni_logp, st_bo, st_shorter, arc_keys, arc_logp, arc_next, arc_probe, order)
    if not (0 <= n_vocab <= lm.n_uni) or not (0 <= start_state < lm.n_states):
        raise RuntimeError('ctc_word_state_beam_search: %d words of %d word ids, start state %d of %d states' % (n_vocab, lm.n_uni, start_state, lm.n_states))
    lm.lex_child, lm.lex_word, lm.n_nodes, lm.n_vocab, lm.start_state = lex_child.data_ptr(), lex_word.data_ptr(), lex_child.shape[0], n_vocab, start_state
    lse, ws, st, out = _beam_search_buffers('ctc_word_state_beam_search', logits, utt, V, total_frames, max_len, beam_width, n_best,
                                            _L().ss_ctc_word_state_beam_workspace_bytes)
    n = utt.shape[0]
    complete = torch.empty((n, n_best), dtype=torch.int32, device=dev)
    _lib.check(_L().ss_ctc_word_state_beam_search(_p(logits), logits.shape[1], V, blank, space, logits.shape[0], _p(lse), _p(utt) if n else None, n, total_frames,
                                                  beam_width, n_best, ctypes.byref(lm), alpha, beta, _p(ws), max_len, *(_p(t) for t in out), _p(complete), st),
               'ss_ctc_word_state_beam_search')
    return out + (complete,)


@ctc_word_state_beam_search.register_fake
def _(logits, utt, V, blank, space, total_frames, max_len, beam_width, n_best, lex_child, lex_word, uni_logp, st_bo, st_shorter, arc_keys, arc_logp, arc_next,
      n_vocab, start_state, arc_probe, order, alpha, beta):
    n = utt.shape[0]
    return (logits.new_empty((n, n_best, max_len), dtype=torch.int32), logits.new_empty((n, n_best), dtype=torch.int32),
            logits.new_empty((n, n_best)), logits.new_empty((n, n_best)), logits.new_empty((n, n_best), dtype=torch.int32))


@torch.library.custom_op('silent_speech::word_state_score', mutates_args=())
def word_state_score(pairs: Tensor, uni_logp: Tensor, st_bo: Tensor, st_shorter: Tensor, arc_keys: Tensor, arc_logp: Tensor, arc_next: Tensor,
                     arc_probe: int, order: int) -> Tuple[Tensor, Tensor]:
    """ln P(word | state) and the state after the word of every row (state, word) of pairs [n][2] int32 by the rule of ss_word_state_lm, with the
    device function the word-state beam search uses.  An id outside the tables gives NaN and -1.  Returns ([n] f32, [n] int32)."""
    dev = pairs.device
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int32 or not pairs.is_contiguous():
        raise RuntimeError('word_state_score: pairs must be a contiguous (n, 2) int32 tensor')
    lm = _word_state_tables('word_state_score', dev, uni_logp, st_bo, st_shorter, arc_keys, arc_logp, arc_next, arc_probe, order)
    lnp = torch.empty(pairs.shape[0], dtype=torch.float32, device=dev)
    nxt = torch.empty(pairs.shape[0], dtype=torch.int32, device=dev)
    _lib.check(_L().ss_word_state_score(ctypes.byref(lm), _p(pairs), pairs.shape[0], _p(lnp), _p(nxt), _lib.stream_of(pairs)), 'ss_word_state_score')
    return lnp, nxt


@word_state_score.register_fake
def _(pairs, uni_logp, st_bo, st_shorter, arc_keys, arc_logp, arc_next, arc_probe, order):
    return pairs.new_empty((pairs.shape[0],), dtype=torch.float32), pairs.new_empty((pairs.shape[0],), dtype=torch.int32)


# ------------------------------------------------------------------------------------------------ stft_logmel
@torch.library.custom_op('silent_speech::stft_logmel', mutates_args=())
def stft_logmel(y: Tensor, n_fft: int, num_mels: int, sampling_rate: int, hop_size: int, win_size: int, fmin: int, fmax: int, center: bool) -> Tensor:
    """data_utils.py:39-62: (B, L) float32 -> (B, num_mels, F) log-mel."""
    from .data_utils import _mel_spectrogram_impl
    return _mel_spectrogram_impl(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center)


@stft_logmel.register_fake
def _(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center):
    Lp = y.shape[1] + 2 * int((n_fft - hop_size) / 2) + (2 * (n_fft // 2) if center else 0)
    return y.new_empty(y.shape[0], num_mels, 1 + (Lp - n_fft) // hop_size)


@torch.library.custom_op('silent_speech::stft_logmel_backward', mutates_args=())
def stft_logmel_backward(g: Tensor, y: Tensor, n_fft: int, num_mels: int, sampling_rate: int, hop_size: int, win_size: int, fmin: int, fmax: int, center: bool) -> Tensor:
    """d loss / d y (B, L) of stft_logmel from g = d loss / d mel (B, num_mels, F), read through its strides (csrc/mel_bwd.hip).  Only the direct FFT path
    (n_fft = 1024, center=False) has a gradient: anything else raises.  No autograd formula of its own (no second derivative)."""
    from .data_utils import _mel_spectrogram_backward_impl
    return _mel_spectrogram_backward_impl(g, y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center)


@stft_logmel_backward.register_fake
def _(g, y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center):
    return y.new_empty(y.shape)


def _stft_logmel_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0])
    ctx.params = tuple(inputs[1:])


def _stft_logmel_bwd(ctx, g):
    y, = ctx.saved_tensors
    return (torch.ops.silent_speech.stft_logmel_backward(g, y, *ctx.params),) + (None,) * 8


stft_logmel.register_autograd(_stft_logmel_bwd, setup_context=_stft_logmel_setup)


@torch.library.custom_op('silent_speech::stft_logmel_ragged', mutates_args=())
def stft_logmel_ragged(flat: Tensor, offsets: Tensor, lengths: Tensor, F: int, clip: bool, n_fft: int, num_mels: int, sampling_rate: int, hop_size: int,
                       win_size: int, fmin: int, fmax: int) -> Tensor:
    """load_audio's clip (when `clip`) + mel_spectrogram(center=False) of a ragged batch: signal b = flat[offsets[b] .. + lengths[b]) (offsets int64, lengths
    int32, on the device) -> buf (B, F, num_mels) f32, F >= the longest signal's frame count; rows behind a signal's own frames are filler.  n_fft = 1024
    only (the direct FFT kernel); differentiable with respect to flat."""
    from .data_utils import _mel_ragged_impl
    return _mel_ragged_impl(flat, offsets, lengths, F, clip, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax)


@stft_logmel_ragged.register_fake
def _(flat, offsets, lengths, F, clip, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax):
    return flat.new_empty((offsets.shape[0], F, num_mels))


@torch.library.custom_op('silent_speech::stft_logmel_ragged_backward', mutates_args=())
def stft_logmel_ragged_backward(g: Tensor, flat: Tensor, offsets: Tensor, lengths: Tensor, clip: bool, n_fft: int, num_mels: int, sampling_rate: int,
                                hop_size: int, win_size: int, fmin: int, fmax: int) -> Tensor:
    """d loss / d flat of stft_logmel_ragged from g = d loss / d buf (B, F, num_mels), any strides: filler rows are not read, samples outside every signal
    get 0, with `clip` samples beyond [-1, 1] get 0.  No autograd formula of its own."""
    from .data_utils import _mel_ragged_backward_impl
    return _mel_ragged_backward_impl(g, flat, offsets, lengths, clip, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax)


@stft_logmel_ragged_backward.register_fake
def _(g, flat, offsets, lengths, clip, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax):
    return flat.new_empty(flat.shape)


def _stft_logmel_ragged_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1], inputs[2])
    ctx.params = tuple(inputs[4:])


def _stft_logmel_ragged_bwd(ctx, g):
    flat, offsets, lengths = ctx.saved_tensors
    return (torch.ops.silent_speech.stft_logmel_ragged_backward(g, flat, offsets, lengths, *ctx.params),) + (None,) * 11


stft_logmel_ragged.register_autograd(_stft_logmel_ragged_bwd, setup_context=_stft_logmel_ragged_setup)


# ------------------------------------------------------------------------------------------------ emg_features
@torch.library.custom_op('silent_speech::emg_features', mutates_args=())
def emg_features(x: Tensor) -> Tensor:
    """data_utils.py:85-136: (n, C) EMG at 516.79 Hz (n >= 16) -> (1 + (n - 16) // 6, 14 C) float32 features, f64 arithmetic."""
    from .read_emg import emg_features_batch
    if x.dim() != 2 or x.shape[0] < 16:
        raise ValueError('emg_features: a (n >= 16, C) signal is expected')
    return emg_features_batch([x.to(torch.float64).contiguous()])[0]


@emg_features.register_fake
def _(x):
    if x.dim() != 2 or x.shape[0] < 16:
        raise ValueError('emg_features: a (n >= 16, C) signal is expected')
    return x.new_empty((1 + (x.shape[0] - 16) // 6, 14 * x.shape[1]), dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ stored audio (csrc/audio.hip; no autograd: data loading)
@torch.library.custom_op('silent_speech::audio_resample', mutates_args=('out',))
def audio_resample(flat: Tensor, out: Tensor, table: Tensor, coef: Tensor, gains: Optional[Tensor], up: int, down: int, half: int, taps_per_phase: int,
                   clip: bool, total_out: int) -> None:
    """scipy.signal.resample_poly(x, up, down) of every utterance of a ragged batch (ss_audio_resample_batch in include/silent_speech_hip.h).  flat / out:
    flat f32 buffers; table [R][4] int64 on their device = (first input sample, n, first output sample, n_out) per utterance, all inside the two
    buffers; coef [up][taps_per_phase] f32: the phase-major filter (data_utils._resample_table); gains: optional [R] f32 scale; clip: to [-1, 1];
    total_out: the sum of the n_out.  Writes the rows' outputs into `out` and nothing else."""
    dev = flat.device
    for t, dt, name in ((flat, torch.float32, 'flat'), (out, torch.float32, 'out'), (table, torch.int64, 'table'), (coef, torch.float32, 'coef')):
        if t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise RuntimeError('audio_resample: %s must be a contiguous %s tensor on the device of the input' % (name, dt))
    if flat.dim() != 1 or out.dim() != 1 or table.dim() != 2 or table.shape[1] != 4 or table.shape[0] < 1 or tuple(coef.shape) != (up, taps_per_phase):
        raise RuntimeError('audio_resample: flat buffers, a (R >= 1, 4) table and a (%d, %d) coefficient table are expected' % (up, taps_per_phase))
    if gains is not None and (gains.dtype != torch.float32 or tuple(gains.shape) != (table.shape[0],) or not gains.is_contiguous() or gains.device != dev):
        raise RuntimeError('audio_resample: gains must be a contiguous (R) float32 tensor on the device of the input')
    if not (0 <= total_out <= out.shape[0]):
        raise RuntimeError('audio_resample: %d outputs do not fit the output buffer of %d' % (total_out, out.shape[0]))
    if not _L().ss_audio_resample_supported(up, down, half, taps_per_phase):
        raise ValueError('audio_resample: ratio %d/%d is not supported' % (up, down))
    if total_out == 0:
        return
    _lib.check(_L().ss_audio_resample_batch(_p(flat), _p(out), _p(table), table.shape[0], up, down, half, taps_per_phase, _p(coef), _p(gains),
                                            1 if clip else 0, total_out, _lib.stream_of(flat)), 'ss_audio_resample_batch')


@audio_resample.register_fake
def _(flat, out, table, coef, gains, up, down, half, taps_per_phase, clip, total_out):
    return None


@torch.library.custom_op('silent_speech::audio_level', mutates_args=())
def audio_level(flat: Tensor, table: Tensor, total_blocks: int) -> Tuple[Tensor, Tensor]:
    """normalize_volume's two numbers and its gain per utterance (ss_audio_level_batch): flat f32; table [R][3] int64 = (first sample, n, first 512-sample
    block).  Returns (levels [R][2] f32 = {max frame RMS, max |x|}, gains [R] f32)."""
    dev = flat.device
    if flat.dim() != 1 or flat.dtype != torch.float32 or not flat.is_contiguous():
        raise RuntimeError('audio_level: a flat contiguous float32 buffer is expected')
    if table.dim() != 2 or table.shape[1] != 3 or table.shape[0] < 1 or table.dtype != torch.int64 or not table.is_contiguous() or table.device != dev:
        raise RuntimeError('audio_level: table must be a contiguous (R >= 1, 3) int64 tensor on the device of the input')
    R = table.shape[0]
    ws = torch.empty(max(2 * total_blocks, 1), dtype=torch.float32, device=dev)
    level = torch.empty((R, 2), dtype=torch.float32, device=dev)
    gains = torch.empty(R, dtype=torch.float32, device=dev)
    _lib.check(_L().ss_audio_level_batch(_p(flat), _p(table), R, total_blocks, _p(ws), ws.shape[0], _p(level), _p(gains), _lib.stream_of(flat)), 'ss_audio_level_batch')
    return level, gains


@audio_level.register_fake
def _(flat, table, total_blocks):
    return flat.new_empty((table.shape[0], 2)), flat.new_empty((table.shape[0],))


# ------------------------------------------------------------------------------------------------ spectral gating (csrc/spectral_gate.hip; no autograd: data preparation)
GATE_BINS, GATE_ROW_DWORDS, GATE_MAX_NF, GATE_MAX_NT = 513, 17, 32, 8


def _gate_check(name, flat, table, windows):
    dev = flat.device
    if flat.dim() != 1 or flat.dtype != torch.float32 or not flat.is_contiguous():
        raise RuntimeError('%s: a flat contiguous float32 buffer is expected' % name)
    if table.dim() != 2 or table.shape[1] != 4 or table.shape[0] < 1 or table.dtype != torch.int64 or not table.is_contiguous() or table.device != dev:
        raise RuntimeError('%s: table must be a contiguous (R >= 1, 4) int64 tensor on the device of the input' % name)
    if tuple(windows.shape) != (3, 1024) or windows.dtype != torch.float32 or not windows.is_contiguous() or windows.device != dev:
        raise RuntimeError('%s: windows must be a contiguous (3, 1024) float32 tensor on the device of the input' % name)


@torch.library.custom_op('silent_speech::spectral_gate_profile', mutates_args=())
def spectral_gate_profile(flat: Tensor, table: Tensor, windows: Tensor, frames: int, n_std: float) -> Tensor:
    """The stationary gate's threshold per frequency row from ONE noise clip (ss_spectral_gate_profile): flat f32 holding the clip; table (1, 4) int64 =
    (first sample, L, 0, F = ceil(L / 256) + 1); windows (3, 1024) f32 (data_utils._gate_windows); frames = F.  Returns thresh (513,) f32 in dB:
    mean + n_std * population std over the frames of 20 log10(|X| + eps) clamped at the row's maximum - 80."""
    _gate_check('spectral_gate_profile', flat, table, windows)
    if table.shape[0] != 1 or frames < 2:
        raise ValueError('spectral_gate_profile: one non-empty noise clip is expected')
    dev = flat.device
    db = torch.empty((frames, GATE_BINS), dtype=torch.float64, device=dev)
    rowmax = torch.empty(GATE_BINS, dtype=torch.int32, device=dev)
    thresh = torch.empty(GATE_BINS, dtype=torch.float32, device=dev)
    _lib.check(_L().ss_spectral_gate_profile(_p(flat), _p(table), frames, _p(windows), float(n_std), _p(db), _p(rowmax), _p(thresh), _lib.stream_of(flat)),
               'ss_spectral_gate_profile')
    return thresh


@spectral_gate_profile.register_fake
def _(flat, table, windows, frames, n_std):
    return flat.new_empty((GATE_BINS,))


@torch.library.custom_op('silent_speech::spectral_gate', mutates_args=('out',))
def spectral_gate(flat: Tensor, out: Tensor, table: Tensor, windows: Tensor, thresh: Tensor, total_frames: int, n_f: int, n_t: int, prop_decrease: float,
                  return_bits: bool) -> Tensor:
    """noisereduce's stationary gate over every signal of a ragged batch (ss_spectral_gate_batch in include/silent_speech_hip.h).  flat: f32 buffer; table
    (R, 4) int64 = (first sample, L, first frame, F) per signal; thresh (513,) f32 in dB; n_f / n_t: half widths of the mask's triangular smoothing over
    frequency rows / frames (0, 0 = none).  Writes the gated signals into `out` (flat's layout and size; nothing else of it is touched) and returns the
    final binary gate (total_frames, 17) int32 -- bit k & 31 of dword k >> 5 -- when return_bits, else an empty (0, 17) tensor."""
    _gate_check('spectral_gate', flat, table, windows)
    dev = flat.device
    if tuple(thresh.shape) != (GATE_BINS,) or thresh.dtype != torch.float32 or not thresh.is_contiguous() or thresh.device != dev:
        raise RuntimeError('spectral_gate: thresh must be a contiguous (513,) float32 tensor on the device of the input')
    if not (0 <= n_f <= GATE_MAX_NF and 0 <= n_t <= GATE_MAX_NT):
        raise ValueError('spectral_gate: mask smoothing over %d rows x %d frames is not supported (at most %d x %d)' % (n_f, n_t, GATE_MAX_NF, GATE_MAX_NT))
    if not (0.0 <= prop_decrease <= 1.0):
        raise ValueError('spectral_gate: prop_decrease must lie in [0, 1]')
    R = table.shape[0]
    if total_frames < 2 * R:
        raise ValueError('spectral_gate: every signal needs at least one sample')
    if out.shape != flat.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise RuntimeError('spectral_gate: out must be a contiguous float32 buffer of the size and on the device of the input')
    bits_ws = torch.empty((total_frames, GATE_ROW_DWORDS), dtype=torch.int32, device=dev)
    rowmax = torch.empty((R, GATE_BINS), dtype=torch.int32, device=dev)
    frames = torch.empty((total_frames, 1024), dtype=torch.float32, device=dev)
    bits = torch.empty((total_frames if return_bits else 0, GATE_ROW_DWORDS), dtype=torch.int32, device=dev)
    _lib.check(_L().ss_spectral_gate_batch(_p(flat), _p(out), _p(table), R, total_frames, _p(windows), _p(thresh), n_f, n_t, float(prop_decrease), _p(bits_ws),
                                           _p(rowmax), _p(frames), _p(bits) if return_bits else None, _lib.stream_of(flat)), 'ss_spectral_gate_batch')
    return bits


@spectral_gate.register_fake
def _(flat, out, table, windows, thresh, total_frames, n_f, n_t, prop_decrease, return_bits):
    return flat.new_empty((total_frames if return_bits else 0, GATE_ROW_DWORDS), dtype=torch.int32)


@torch.library.custom_op('silent_speech::spectral_gate_nonstationary', mutates_args=('out',))
def spectral_gate_nonstationary(flat: Tensor, out: Tensor, table: Tensor, windows: Tensor, total_frames: int, b: float, n_mult: float, slope: float, n_f: int,
                                n_t: int, prop_decrease: float, return_mask: bool) -> Tensor:
    """noisereduce's non-stationary gate over every signal of a ragged batch (ss_spectral_gate_ns_batch in include/silent_speech_hip.h): no noise clip, the
    level per frequency row is the signal's own magnitude smoothed forward and backward over time with the coefficient b
    (data_utils.nonstationary_coefficient), the mask a sigmoid of slope `slope` on the relative excess over n_mult.  flat, table, windows, n_f, n_t as for
    spectral_gate.  Writes the gated signals into `out` (flat's layout and size; nothing else of it is touched) and returns the UNSMOOTHED mask m0
    (total_frames, 513) f32 when return_mask, else an empty (0, 513) tensor."""
    name = 'spectral_gate_nonstationary'
    _gate_check(name, flat, table, windows)
    dev = flat.device
    if not (0.0 < b <= 1.0):
        raise ValueError('%s: the smoothing coefficient b must lie in (0, 1]' % name)
    if not (slope > 0.0) or n_mult != n_mult:
        raise ValueError('%s: the sigmoid slope must be positive' % name)
    if not (0 <= n_f <= GATE_MAX_NF and 0 <= n_t <= GATE_MAX_NT):
        raise ValueError('%s: mask smoothing over %d rows x %d frames is not supported (at most %d x %d)' % (name, n_f, n_t, GATE_MAX_NF, GATE_MAX_NT))
    if not (0.0 <= prop_decrease <= 1.0):
        raise ValueError('%s: prop_decrease must lie in [0, 1]' % name)
    R = table.shape[0]
    if total_frames < 2 * R:
        raise ValueError('%s: every signal needs at least one sample' % name)
    if out.shape != flat.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise RuntimeError('%s: out must be a contiguous float32 buffer of the size and on the device of the input' % name)
    mag = torch.empty((total_frames, GATE_BINS), dtype=torch.float32, device=dev)
    level = torch.empty((total_frames, GATE_BINS), dtype=torch.float32, device=dev)
    frames = torch.empty((total_frames, 1024), dtype=torch.float32, device=dev)
    mask = torch.empty((total_frames if return_mask else 0, GATE_BINS), dtype=torch.float32, device=dev)
    _lib.check(_L().ss_spectral_gate_ns_batch(_p(flat), _p(out), _p(table), R, total_frames, _p(windows), float(b), float(n_mult), float(slope), n_f, n_t,
                                              float(prop_decrease), _p(mag), _p(level), _p(frames), _p(mask) if return_mask else None, _lib.stream_of(flat)),
               'ss_spectral_gate_ns_batch')
    return mask


@spectral_gate_nonstationary.register_fake
def _(flat, out, table, windows, total_frames, b, n_mult, slope, n_f, n_t, prop_decrease, return_mask):
    return flat.new_empty((total_frames if return_mask else 0, GATE_BINS))


# ------------------------------------------------------------------------------------------------ fused_adamw
@torch.library.custom_op('silent_speech::fused_adamw', mutates_args=('p', 'm', 'v'))
def fused_adamw(p: Tensor, g: Tensor, m: Tensor, v: Tensor, n: int, lr: float, step: int, beta1: float, beta2: float, eps: float,
                weight_decay: float, grad_scale: float) -> None:
    """One decoupled-weight-decay Adam step over the first n floats of the flat arenas (torch.optim.AdamW semantics, bias correction from `step`)."""
    ops.adamw_step(p, g, m, v, n, lr, step, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale)


@fused_adamw.register_fake
def _(p, g, m, v, n, lr, step, beta1, beta2, eps, weight_decay, grad_scale):
    return None


# ------------------------------------------------------------------------------------------------ HiFi-GAN generator (inference only: no autograd)
# One op per kernel family over ONE utterance of L time steps, time-major (L, C) float32 -- the packed, multi-utterance form is what
# vocoder.Vocoder drives through ops.voc_* (one table for all ~80 launches of a call).  `blob` is the layer's weight blob (vocoder.conv_blob /
# vocoder.conv_transpose_blob / vocoder.tail_weights).
def _one_utterance(x):
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError('a time-major (L, C) float32 tensor is expected')
    return torch.tensor([[0, x.shape[0]]], dtype=torch.int64, device=x.device), x.contiguous()


@torch.library.custom_op('silent_speech::vocoder_conv1d', mutates_args=())
def vocoder_conv1d(x: Tensor, blob: Tensor, c_out: int, k: int, dilation: int, slope: float, residual: Optional[Tensor], x3: bool) -> Tensor:
    """conv1d(leaky_relu(x, slope), W, b, dilation=dilation, padding=(k - 1) * dilation // 2) [+ residual], (L, c_in) -> (L, c_out)."""
    table, x = _one_utterance(x)
    L, c_in = x.shape
    out = x.new_empty((L, c_out))
    if residual is not None:
        if residual.shape != out.shape or residual.dtype != torch.float32:
            raise ValueError('vocoder_conv1d: residual must be (L, c_out) float32')
        residual = residual.contiguous()
    return ops.voc_conv1d(x, blob, out, table, 1, L, L, 1, c_in, c_out, k, dilation, slope, residual=residual, x3=x3)


@vocoder_conv1d.register_fake
def _(x, blob, c_out, k, dilation, slope, residual, x3):
    return x.new_empty((x.shape[0], c_out))


@torch.library.custom_op('silent_speech::vocoder_conv_transpose1d', mutates_args=())
def vocoder_conv_transpose1d(x: Tensor, blob: Tensor, c_out: int, k: int, stride: int, slope: float, x3: bool) -> Tensor:
    """conv_transpose1d(leaky_relu(x, slope), W, b, stride=stride, padding=(k - stride) // 2), (L, c_in) -> (L * stride, c_out)."""
    table, x = _one_utterance(x)
    L, c_in = x.shape
    out = x.new_empty((L * stride, c_out))
    return ops.voc_conv_transpose1d(x, blob, out, table, 1, L, L, 1, c_in, c_out, k, stride, slope, x3=x3)


@vocoder_conv_transpose1d.register_fake
def _(x, blob, c_out, k, stride, slope, x3):
    return x.new_empty((x.shape[0] * stride, c_out))


@torch.library.custom_op('silent_speech::vocoder_tail', mutates_args=())
def vocoder_tail(x: Tensor, w: Tensor, k: int, slope: float) -> Tensor:
    """tanh(conv1d(leaky_relu(x, slope), W (1, c_in, k), b, padding=(k - 1) // 2)), (L, c_in) -> (L,)."""
    table, x = _one_utterance(x)
    L, c_in = x.shape
    out = x.new_empty((L,))
    return ops.voc_tail(x, w, out, table, 1, L, L, 1, c_in, k, slope)


@vocoder_tail.register_fake
def _(x, w, k, slope):
    return x.new_empty((x.shape[0],))


OPS = ('model_forward', 'model_forward_ragged', 'model_backward', 'dtw_loss', 'dtw_align', 'ctc_loss', 'ctc_beam_search', 'ctc_word_beam_search', 'ctc_word_state_beam_search', 'ctc_forced_align', 'word_ngram_score', 'word_state_score', 'stft_logmel', 'stft_logmel_backward', 'stft_logmel_ragged', 'stft_logmel_ragged_backward',
       'emg_features', 'audio_resample', 'audio_level', 'spectral_gate_profile', 'spectral_gate', 'spectral_gate_nonstationary', 'fused_adamw',
       'vocoder_conv1d', 'vocoder_conv_transpose1d', 'vocoder_tail')
