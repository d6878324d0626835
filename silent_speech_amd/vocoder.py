"""HiFi-GAN generator on the MI355X (reference: vocoder.py:16-36, which wraps hifi_gan's Generator).

    Vocoder(device)(mel)          (T, 80) de-normalised log-mel -> (T * hop,) float32 audio on the device
    Vocoder(device).batch(mels)   a list of utterances as ONE packed launch sequence -> list of 1-D tensors

The generator is rebuilt from its `config.json` and `state_dict` alone (the hifi_gan submodule is not needed): conv_pre, per stage
leaky_relu -> ConvTranspose1d -> the mean of num_kernels ResBlocks, then leaky_relu -> conv_post -> tanh.  Every convolution is one launch
of csrc/vocoder.hip (leaky ReLU, bias, residual add and the ResBlock mean are fused into it); weights are folded (weight norm) and re-laid
into the kernels' [tap][c_out][c_in] bf16 hi / lo planes once, here, at load time.  There is no CPU path: tensors that the kernels cannot
read raise (see _lib.ptr)."""
import json
import os

import torch

from . import _lib, ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.silent_speech.vocoder_*)
from .flags import FLAGS

LRELU_SLOPE = 0.1          # hifi_gan/models.py: LRELU_SLOPE; the activation before conv_post uses torch's default 0.01 instead
MATMUL_MODES = ('bf16x3', 'bf16')


def _planes(w):
    """float64 / float32 tensor -> (hi, lo) bf16 with hi + lo ~ w to 16-17 bits."""
    w32 = w.to(torch.float32)
    hi = w32.to(torch.bfloat16)
    lo = (w32 - hi.to(torch.float32)).to(torch.bfloat16)
    return hi, lo


def _blob(slots_w, bias):
    """slots_w: (slots, c_out, c_in) weights, bias (c_out,) -> the uint8 blob of ss_voc_blob_bytes (bias | hi planes | lo planes, zero padded)."""
    slots, c_out, c_in = slots_w.shape
    co_pad, ci_pad = -(-c_out // 16) * 16, -(-c_in // 32) * 32
    wp = torch.zeros(slots, co_pad, ci_pad, dtype=torch.float64)
    wp[:, :c_out, :c_in] = slots_w.to(torch.float64)
    hi, lo = _planes(wp)
    bp = torch.zeros(co_pad, dtype=torch.float32)
    bp[:c_out] = bias.to(torch.float32)
    blob = torch.cat([bp.view(torch.uint8), hi.reshape(-1).view(torch.uint8), lo.reshape(-1).view(torch.uint8)])
    assert blob.numel() == ops.voc_blob_bytes(slots, c_out, c_in)
    return blob


def conv_blob(weight, bias):
    """torch Conv1d weight (c_out, c_in, k) -> blob with slot j = weight[:, :, j]."""
    return _blob(weight.detach().cpu().permute(2, 0, 1), bias.detach().cpu())


def conv_transpose_blob(weight, bias, stride):
    """torch ConvTranspose1d weight (c_in, c_out, k) -> blob with slot r * ntap + m = weight[:, :, r + m * stride].T (polyphase: the taps of
    output phase r; zero where the tap index runs past k)."""
    w = weight.detach().cpu()
    c_in, c_out, k = w.shape
    ntap = -(-k // stride)
    slots = torch.zeros(stride * ntap, c_out, c_in, dtype=w.dtype)
    for r in range(stride):
        for m in range(ntap):
            if r + m * stride < k:
                slots[r * ntap + m] = w[:, :, r + m * stride].T
    return _blob(slots, bias.detach().cpu())


def tail_weights(weight, bias):
    """conv_post weight (1, c_in, k), bias (1,) -> float32 [k * c_in + 1]: tap-major weights, then the bias."""
    w = weight.detach().cpu().to(torch.float32)
    return torch.cat([w[0].T.reshape(-1), bias.detach().cpu().to(torch.float32).reshape(1)]).contiguous()


def fold_weight_norm(state_dict):
    """`*.weight_g` / `*.weight_v` pairs -> `*.weight` = v * g / ||v|| (norm over every dimension but 0, torch.nn.utils.weight_norm's
    default dim: the output channel of a Conv1d, the INPUT channel of a ConvTranspose1d); plain `*.weight` keys pass through."""
    out = {}
    for key, v in state_dict.items():
        if key.endswith('.weight_g'):
            continue
        if key.endswith('.weight_v'):
            stem = key[:-len('.weight_v')]
            g = state_dict[stem + '.weight_g'].to(torch.float64)
            v64 = v.to(torch.float64)
            norm = v64.reshape(v64.shape[0], -1).norm(dim=1).reshape([-1] + [1] * (v64.dim() - 1))
            out[stem + '.weight'] = v64 * (g / norm)
        else:
            out[key] = v
    return out


class _Conv(object):
    def __init__(self, blob, c_in, c_out, k, d):
        self.blob, self.c_in, self.c_out, self.k, self.d = blob, c_in, c_out, k, d


class Vocoder(object):
    def __init__(self, device='cuda', *, checkpoint_file=None, config=None, state_dict=None, matmul='bf16x3'):
        if matmul not in MATMUL_MODES:
            raise ValueError('matmul must be one of %s' % (MATMUL_MODES,))
        if state_dict is None:
            if checkpoint_file is None:
                checkpoint_file = FLAGS.lookup('hifigan_checkpoint', None)
                assert checkpoint_file is not None, 'no HiFi-GAN checkpoint: pass checkpoint_file / state_dict or set FLAGS.hifigan_checkpoint'
            state_dict = torch.load(checkpoint_file, map_location='cpu')['generator']
            if config is None:
                with open(os.path.join(os.path.split(checkpoint_file)[0], 'config.json')) as f:
                    config = json.load(f)
        if config is None:
            raise ValueError('Vocoder: a state_dict needs its config')
        self.device = torch.device(device)
        self.x3 = matmul == 'bf16x3'
        self.matmul = matmul
        self._load(dict(config), fold_weight_norm(state_dict))

    # ---- load time: validate the architecture against the kernels and build the weight blobs
    def _load(self, h, sd):
        rates, ukern = list(h['upsample_rates']), list(h['upsample_kernel_sizes'])
        rk, rd = list(h['resblock_kernel_sizes']), [list(d) for d in h['resblock_dilation_sizes']]
        C, kind = int(h['upsample_initial_channel']), str(h['resblock'])
        n_mels = int(h.get('num_mels', 80))
        if kind not in ('1', '2'):
            raise ValueError("resblock must be '1' or '2'")
        if len(rates) != len(ukern) or len(rk) != len(rd):
            raise ValueError('config lists of unequal length')
        for u, k in zip(rates, ukern):
            if (k - u) % 2 or k < u:
                raise ValueError('upsample kernel %d / rate %d: k - u must be even and non-negative (padding (k - u) // 2 keeps T * u samples)' % (k, u))
        dev = self.device

        def need(ok, what):
            if not ok:
                raise ValueError('Vocoder: the gfx950 kernels do not take %s (ss_voc_supported)' % what)

        def conv(stem, c_in, c_out, k, d):
            w, b = sd[stem + '.weight'], sd[stem + '.bias']
            if tuple(w.shape) != (c_out, c_in, k):
                raise ValueError('%s.weight has shape %s, the config implies %s' % (stem, tuple(w.shape), (c_out, c_in, k)))
            need(ops.voc_supported(c_in, c_out, k, d, 0), 'Conv1d(%d, %d, %d, dilation=%d)' % (c_in, c_out, k, d))
            return _Conv(conv_blob(w, b).to(dev), c_in, c_out, k, d)

        self.n_mels, self.C, self.rates, self.nk, self.kind = n_mels, C, rates, len(rk), kind
        self.hop = 1
        for u in rates:
            self.hop *= u
        self.conv_pre = conv('conv_pre', n_mels, C, 7, 1)
        self.ups, self.resblocks = [], []
        for i, (u, k) in enumerate(zip(rates, ukern)):
            c_in, c_out = C >> i, C >> (i + 1)
            w, b = sd['ups.%d.weight' % i], sd['ups.%d.bias' % i]
            if tuple(w.shape) != (c_in, c_out, k):
                raise ValueError('ups.%d.weight has shape %s, the config implies %s' % (i, tuple(w.shape), (c_in, c_out, k)))
            need(ops.voc_supported(c_in, c_out, k, u, 1), 'ConvTranspose1d(%d, %d, %d, stride=%d)' % (c_in, c_out, k, u))
            self.ups.append(_Conv(conv_transpose_blob(w, b, u).to(dev), c_in, c_out, k, u))
            for j, (kk, dil) in enumerate(zip(rk, rd)):
                n = i * len(rk) + j
                if kind == '1':
                    self.resblocks.append([(conv('resblocks.%d.convs1.%d' % (n, m), c_out, c_out, kk, d),
                                            conv('resblocks.%d.convs2.%d' % (n, m), c_out, c_out, kk, 1)) for m, d in enumerate(dil[:3])])
                else:
                    self.resblocks.append([(conv('resblocks.%d.convs.%d' % (n, m), c_out, c_out, kk, d),) for m, d in enumerate(dil[:2])])
        c_last = C >> len(rates)
        w, b = sd['conv_post.weight'], sd['conv_post.bias']
        if tuple(w.shape) != (1, c_last, 7):
            raise ValueError('conv_post.weight has shape %s, the config implies %s' % (tuple(w.shape), (1, c_last, 7)))
        need(ops.voc_supported(c_last, 1, 7, 1, 2), 'conv_post over %d channels' % c_last)
        self.tail_w = tail_weights(w, b).to(dev)

    # ---- the hot path
    def batch(self, mels):
        """list of (T_u, n_mels) tensors -> list of (T_u * hop,) float32 tensors (views of one packed buffer)."""
        if len(mels) == 0:
            return []
        dev = self.device
        lens = [int(m.shape[0]) for m in mels]
        for m in mels:
            if m.dim() != 2 or m.shape[1] != self.n_mels:
                raise ValueError('Vocoder: mel spectrograms are (T, %d)' % self.n_mels)
        total, longest, U = sum(lens), max(lens), len(lens)
        firsts = [sum(lens[:u]) for u in range(U)]
        if total == 0:
            return [torch.empty(0, dtype=torch.float32, device=dev) for _ in mels]
        x = torch.cat([m.to(device=dev, dtype=torch.float32) for m in mels], 0).contiguous()
        table = torch.tensor([[f, n] for f, n in zip(firsts, lens)], dtype=torch.int64).to(dev)
        one = ops.voc_workspace_bytes(total, self.C, self.rates) // 4
        ws = torch.empty(4 * one, dtype=torch.uint8, device=dev)
        X, T_, R, M = [ws[i * one:(i + 1) * one].view(torch.float32) for i in range(4)]
        x3 = self.x3

        def conv(c, src, dst, scale, slope=LRELU_SLOPE, residual=None, accumulate=False, out_scale=1.0):
            ops.timed('voc_conv_kernel c%d k%d' % (c.c_out, c.k), 2.0 * total * scale * c.c_in * c.c_out * c.k, 4.0 * total * scale * (c.c_in + c.c_out),
                      lambda: ops.voc_conv1d(src, c.blob, dst, table, U, total, longest, scale, c.c_in, c.c_out, c.k, c.d, slope, residual=residual,
                                             accumulate=accumulate, out_scale=out_scale, x3=x3))

        conv(self.conv_pre, x, M, 1, slope=1.0)
        scale = 1
        for i, up in enumerate(self.ups):
            ops.timed('voc_conv_kernel transposed c%d' % up.c_out, 2.0 * total * scale * up.c_in * up.c_out * up.k, 4.0 * total * scale * (up.c_in + up.d * up.c_out),
                      lambda: ops.voc_conv_transpose1d(M, up.blob, X, table, U, total, longest, scale, up.c_in, up.c_out, up.k, up.d, LRELU_SLOPE, x3=x3))
            scale *= up.d
            for j in range(self.nk):
                rb = self.resblocks[i * self.nk + j]
                cur = X
                for m, pair in enumerate(rb):
                    last = m == len(rb) - 1
                    # the ResBlock's last `+ x` lands in the multi-receptive-field sum: M = (M + block_j(x)), scaled by 1 / nk with the last block
                    fin = dict(accumulate=j > 0, out_scale=(1.0 / self.nk) if j == self.nk - 1 else 1.0) if last else {}
                    if len(pair) == 2:
                        conv(pair[0], cur, T_, scale)
                        conv(pair[1], T_, M if last else R, scale, residual=cur, **fin)
                    else:
                        conv(pair[0], cur, M if last else R, scale, residual=cur, **fin)
                    cur = R
        audio = torch.empty(total * scale, dtype=torch.float32, device=dev)
        c_last = self.C >> len(self.rates)
        ops.timed('voc_tail_kernel', 2.0 * total * scale * c_last * 7, 4.0 * total * scale * (c_last + 1),
                  lambda: ops.voc_tail(M, self.tail_w, audio, table, U, total, longest, scale, c_last, 7, 0.01))
        return [audio[f * scale:(f + n) * scale] for f, n in zip(firsts, lens)]

    def __call__(self, mel_spectrogram):
        """mel_spectrogram: (seq_len, 80) -> 1-D float32 audio of seq_len * hop samples on the device (vocoder.py:28-36)."""
        with torch.no_grad():
            return self.batch([mel_spectrogram])[0]
