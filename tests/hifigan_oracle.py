"""Arithmetic oracle of the HiFi-GAN generator: the forward pass written out in torch primitives (conv1d, conv_transpose1d,
leaky_relu, tanh) on the CPU, float64 by default.  `rounding` (optional) is applied to the input and the weight of every convolution --
that is how the tests emulate the kernels' operand formats -- and `dtype` sets the accumulation type.

Test material: random generators under the architecture and key schema of the issue (conv_pre, ups.{i}, resblocks.{n}.convs1/convs2/convs.{m},
conv_post), scaled so that the audio neither vanishes nor saturates."""
import torch
import torch.nn.functional as F

CONFIGS = {
    'S1': dict(upsample_initial_channel=64, upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], resblock_kernel_sizes=[3, 7, 11],
               resblock_dilation_sizes=[[1, 3, 5]] * 3, resblock='1', num_mels=80),
    'S2': dict(upsample_initial_channel=64, upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], resblock_kernel_sizes=[3, 5, 7],
               resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]], resblock='2', num_mels=80),
    'S3': dict(upsample_initial_channel=32, upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4], resblock_kernel_sizes=[3, 11],
               resblock_dilation_sizes=[[1, 3, 5]] * 2, resblock='1', num_mels=80),
    'V1': dict(upsample_initial_channel=512, upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], resblock_kernel_sizes=[3, 7, 11],
               resblock_dilation_sizes=[[1, 3, 5]] * 3, resblock='1', num_mels=80),
}


def round_bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def round_bf16x2(x):
    """hi + lo with hi = bf16(x), lo = bf16(x - hi): the operand format of the 'bf16x3' mode."""
    x32 = x.to(torch.float32)
    hi = x32.to(torch.bfloat16).to(torch.float32)
    lo = (x32 - hi).to(torch.bfloat16).to(torch.float32)
    return (hi.to(torch.float64) + lo.to(torch.float64)).to(x.dtype)


def hop(config):
    n = 1
    for u in config['upsample_rates']:
        n *= u
    return n


def _conv(x, w, b, rounding, dtype, **kw):
    if rounding is not None:
        x, w = rounding(x), rounding(w)
    return F.conv1d(x.to(dtype), w.to(dtype), b.to(dtype), **kw)


def forward(config, sd, mel, rounding=None, dtype=torch.float64, pre_tanh=False):
    """mel (T, num_mels) -> audio (T * hop,) in `dtype`; sd holds plain `*.weight` / `*.bias` tensors."""
    rates, uk = config['upsample_rates'], config['upsample_kernel_sizes']
    rk, rd = config['resblock_kernel_sizes'], config['resblock_dilation_sizes']
    nk = len(rk)
    x = mel.to(dtype).T[None]
    x = _conv(x, sd['conv_pre.weight'], sd['conv_pre.bias'], rounding, dtype, padding=3)
    for i, (u, k) in enumerate(zip(rates, uk)):
        x = F.leaky_relu(x, 0.1)
        w = sd['ups.%d.weight' % i]
        xi = x
        if rounding is not None:
            xi, w = rounding(xi), rounding(w)
        x = F.conv_transpose1d(xi.to(dtype), w.to(dtype), sd['ups.%d.bias' % i].to(dtype), stride=u, padding=(k - u) // 2)
        xs = None
        for j in range(nk):
            n, kk, dil = i * nk + j, rk[j], rd[j]
            y = x
            if config['resblock'] == '1':
                for m in range(3):
                    d = dil[m]
                    t = _conv(F.leaky_relu(y, 0.1), sd['resblocks.%d.convs1.%d.weight' % (n, m)], sd['resblocks.%d.convs1.%d.bias' % (n, m)],
                              rounding, dtype, dilation=d, padding=(kk * d - d) // 2)
                    t = _conv(F.leaky_relu(t, 0.1), sd['resblocks.%d.convs2.%d.weight' % (n, m)], sd['resblocks.%d.convs2.%d.bias' % (n, m)],
                              rounding, dtype, dilation=1, padding=(kk - 1) // 2)
                    y = t + y
            else:
                for m in range(2):
                    d = dil[m]
                    t = _conv(F.leaky_relu(y, 0.1), sd['resblocks.%d.convs.%d.weight' % (n, m)], sd['resblocks.%d.convs.%d.bias' % (n, m)],
                              rounding, dtype, dilation=d, padding=(kk * d - d) // 2)
                    y = t + y
            xs = y if xs is None else xs + y
        x = xs / nk
    x = F.leaky_relu(x)                     # slope 0.01: torch's default (upstream passes none here)
    x = _conv(x, sd['conv_post.weight'], sd['conv_post.bias'], rounding, dtype, padding=3)
    if pre_tanh:
        return x.reshape(-1)
    return torch.tanh(x).reshape(-1)


def random_generator(config, seed, calib_frames):
    """Seeded float64 weights: conv ~ N(0, 1 / (c_in k)), convs2 / type-2 convs additionally * 0.3, transposed ~ N(0, u / (c_in k)),
    biases ~ N(0, 0.05^2); conv_post is then scaled by 0.5 / rms(pre-tanh output) on a seeded N(0, 1) mel of calib_frames frames."""
    g = torch.Generator().manual_seed(seed)
    C, rates, uk = config['upsample_initial_channel'], config['upsample_rates'], config['upsample_kernel_sizes']
    rk, rd = config['resblock_kernel_sizes'], config['resblock_dilation_sizes']
    sd = {}

    def conv(stem, c_out, c_in, k, scale=1.0):
        sd[stem + '.weight'] = torch.randn(c_out, c_in, k, generator=g, dtype=torch.float64) * (scale / (c_in * k) ** 0.5)
        sd[stem + '.bias'] = torch.randn(c_out, generator=g, dtype=torch.float64) * 0.05

    conv('conv_pre', C, config['num_mels'], 7)
    for i, (u, k) in enumerate(zip(rates, uk)):
        c_in, c_out = C >> i, C >> (i + 1)
        sd['ups.%d.weight' % i] = torch.randn(c_in, c_out, k, generator=g, dtype=torch.float64) * (u / (c_in * k)) ** 0.5
        sd['ups.%d.bias' % i] = torch.randn(c_out, generator=g, dtype=torch.float64) * 0.05
        for j, kk in enumerate(rk):
            n = i * len(rk) + j
            if config['resblock'] == '1':
                for m in range(3):
                    conv('resblocks.%d.convs1.%d' % (n, m), c_out, c_out, kk)
                    conv('resblocks.%d.convs2.%d' % (n, m), c_out, c_out, kk, 0.3)
            else:
                for m in range(2):
                    conv('resblocks.%d.convs.%d' % (n, m), c_out, c_out, kk, 0.3)
    conv('conv_post', 1, C >> len(rates), 7)
    mel = random_mel(config, seed, calib_frames)
    pre = forward(config, sd, mel, pre_tanh=True)
    s = 0.5 / float(pre.pow(2).mean().sqrt())
    sd['conv_post.weight'] = sd['conv_post.weight'] * s
    sd['conv_post.bias'] = sd['conv_post.bias'] * s
    return sd


def random_mel(config, seed, frames):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(frames, config['num_mels'], generator=g, dtype=torch.float64)


def weight_normed(sd, seed):
    """The same generator in checkpoint form: every `*.weight` as `weight_g` (random positive) / `weight_v` with v * g / ||v|| == weight
    (norm over every dimension but 0), as torch.nn.utils.weight_norm stores it."""
    g = torch.Generator().manual_seed(2000 + seed)
    out = {}
    for key, w in sd.items():
        if not key.endswith('.weight'):
            out[key] = w.clone()
            continue
        stem = key[:-len('.weight')]
        shape = [w.shape[0]] + [1] * (w.dim() - 1)
        norm = w.reshape(w.shape[0], -1).norm(dim=1).reshape(shape)
        gain = torch.rand(shape, generator=g, dtype=torch.float64) + 0.5
        out[stem + '.weight_g'] = norm.clone()                  # g = ||w||, v = w * gain  ->  v * g / ||v|| = w
        out[stem + '.weight_v'] = w * gain
    return out
