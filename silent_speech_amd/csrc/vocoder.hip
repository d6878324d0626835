// vocoder.hip -- the HiFi-GAN generator that turns predicted mels into audio (vocoder.py:16-36 of the reference calls hifi_gan's Generator),
// for a ragged batch of utterances packed back to back.
//
// Storage: every activation is f32, time-major -- row = one time step, channels contiguous -- so a row of the packed buffer is what torch
// would call x[0, :, t].  Utterance u of the batch owns rows [off_u * scale, (off_u + len_u) * scale) of a buffer at `scale` samples per
// mel frame (the product of the upsampling rates so far); off_u / len_u (in mel frames) come from ONE device table shared by all launches.
//
// Arithmetic: bf16 MFMA 16x16x32, f32 accumulate.  Mode x3 (the default of the Python layer) splits both operands into hi = bf16(v) and
// lo = bf16(v - hi) and spends three MFMAs per product (hi hi + hi lo + lo hi; the lo lo term, 2^-18 relative, is dropped); mode x1 uses
// the hi plane only.  Weights arrive split and re-laid by the caller ([slot][c_out][c_in] planes, see ss_voc_blob_bytes); activations are
// split on their way into LDS.
//
// voc_conv_kernel is the one MFMA kernel.  A block owns TTB = 64 NTT consecutive output positions q of one utterance (and, for the
// transposed convolution, one output phase) and NCO * 16 output channels; its four waves split the positions.  Per 32-channel input chunk it
// stages rows [q0 + lo, q0 + TTB + hi) of the input ONCE -- leaky ReLU applied, split into planes, zero outside [0, L) of ITS utterance
// (predication: no padded copy exists, and a neighbour's rows are never read as padding) -- and then walks the taps as shifted reads of
// that tile:
//     A fragment = W[slot][co = lane & 15][ci = 8 (lane >> 4) ..]       16 bytes straight from global memory (the layout's reason)
//     B fragment = tile[q + shift(tap)][ci = 8 (lane >> 4) ..]          16 bytes from LDS, rows 80 bytes apart: 16 lanes, 16 distinct 4-bank groups
//     D          = out[q = lane & 15][co = 4 (lane >> 4) .. + 4]        one 16-byte store (and residual / accumulate load) per lane
// Time is the MFMA's N dimension and the block's large one, so the 32- and 64-channel stages (most of the samples) fill their tiles.
//     dilated convolution        input row = q + (tap - (k - 1) / 2) d,   output row = q
//     transposed, phase r        input row = q - m,                         output row = q u + r - p,  slot = r * ceil(k / u) + m  <->  tap r + m u
// i.e. the polyphase form: phase r of the output is a ceil(k / u)-tap convolution of the input, nothing zero-stuffed is ever written.
// Epilogue: + bias, + residual[t, co] (may be `out` itself: each element is read and written by the same lane), + the old out (accumulate:
// the multi-receptive-field sum), * out_scale (1 / nk on the sum's last term).
//
// voc_tail_kernel: leaky ReLU (slope 0.01 upstream) -> k-tap C -> 1 convolution -> tanh, exact f32 on the VALU: 2 k C flops per 4-byte
// sample, bandwidth-bound, one thread per sample over an LDS tile.
#include "common.h"
#include "silent_speech_hip.h"
#include <math.h>

namespace {
constexpr int VOC_THREADS = 256;
constexpr int VOC_CK = 32;             // input channels per LDS chunk = K of one MFMA
constexpr int VOC_LD = VOC_CK + 8;     // LDS row pitch in bf16 (80 bytes)
constexpr int VOC_MAX_SPAN = 128;      // (k - 1) d of the convolution: keeps the x3 tile of the widest block under 64 KiB
constexpr int TAIL_T = 128, TAIL_MAX_C = 64, TAIL_MAX_K = 15;

struct VocArgs {
    const float* x;            // packed input rows, c_in floats each
    const float* residual;     // packed like out, or null
    float* out;
    const float* bias;         // blob: [co_pad] f32
    const bf16_t* whi;         //       [slots][co_pad][ci_pad]
    const bf16_t* wlo;
    const long long* tab;      // [U][2] = first mel frame, mel frames
    long long in_scale, out_scale;      // rows per mel frame of x / out
    int c_in, c_out, ci_pad, co_pad;
    int ntap, tap_off0, tap_step, lo_off, span;      // input row of tap m = q + tap_off0 + m tap_step; lo_off = the smallest such offset
    int phases, ostride, p;                            // output row = q ostride + phase - p
    int q_extra;                                       // positions per utterance = its input rows + q_extra
    int accumulate;
    float slope, post_scale;
};

template <int NCO, int NTT, bool X3>
__global__ void __launch_bounds__(VOC_THREADS) voc_conv_kernel(VocArgs a)
{
    SS_DYN_SMEM(smem_raw);
    constexpr int TTB = NTT * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int u = blockIdx.z / a.phases, r = blockIdx.z - u * a.phases;
    const long long off = a.tab[2 * u], len = a.tab[2 * u + 1];
    const long long Lin = len * a.in_scale, Lout = len * a.out_scale, Q = Lin + a.q_extra;
    const long long q0 = (long long)blockIdx.x * TTB;
    if (q0 >= Q) return;                                              // uniform per block, before any barrier
    const int NR = TTB + a.span;
    bf16_t* shi = (bf16_t*)smem_raw;
    bf16_t* slo = shi + NR * VOC_LD;
    const float* xu = a.x + off * a.in_scale * a.c_in;
    const int cob = blockIdx.y * (NCO * 16);
    const int qw = wave * (NTT * 16);                                 // this wave's first position inside the block
    const int li = lane & 15, lg = lane >> 4;

    f32x4 acc[NCO][NTT];
#pragma unroll
    for (int i = 0; i < NCO; ++i)
#pragma unroll
        for (int j = 0; j < NTT; ++j) { f32x4 z = {0.f, 0.f, 0.f, 0.f}; acc[i][j] = z; }

    for (int c0 = 0; c0 < a.ci_pad; c0 += VOC_CK) {
        __syncthreads();                                              // the previous chunk's tile has been consumed
        for (int e = tid; e < NR * (VOC_CK / 8); e += VOC_THREADS) {
            const int i = e >> 2, g = e & 3, c = c0 + g * 8;
            const long long s = q0 + a.lo_off + i;
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (s >= 0 && s < Lin && c < a.c_in) {                    // c_in % 8 == 0: a group of 8 is inside or outside as a whole
                Vec8<float>::load(xu + s * a.c_in + c, v);
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = v[k] > 0.f ? v[k] : v[k] * a.slope;
            }
            u32x4 h, l;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                h[k] = pack_bf16(v[2 * k], v[2 * k + 1]);
                if (X3) l[k] = pack_bf16(v[2 * k] - __uint_as_float(h[k] << 16), v[2 * k + 1] - __uint_as_float(h[k] & 0xffff0000u));
            }
            *(u32x4*)(shi + i * VOC_LD + g * 8) = h;
            if (X3) *(u32x4*)(slo + i * VOC_LD + g * 8) = l;
        }
        __syncthreads();
        if (q0 + qw < Q) {                                            // uniform per wave: a wave past the utterance's end only helps staging
            for (int m = 0; m < a.ntap; ++m) {
                const long long wrow = ((long long)(r * a.ntap + m) * a.co_pad + cob + li) * a.ci_pad + c0 + lg * 8;
                bf16x8 ah[NCO], al[NCO];
#pragma unroll
                for (int i = 0; i < NCO; ++i) {
                    ah[i] = *(const bf16x8*)(a.whi + wrow + (long long)i * 16 * a.ci_pad);
                    if (X3) al[i] = *(const bf16x8*)(a.wlo + wrow + (long long)i * 16 * a.ci_pad);
                }
                const int shift = a.tap_off0 + m * a.tap_step - a.lo_off;
#pragma unroll
                for (int j = 0; j < NTT; ++j) {
                    if (q0 + qw + j * 16 >= Q) continue;              // uniform per wave
                    const int row = qw + j * 16 + li + shift;
                    const bf16x8 bh = *(const bf16x8*)(shi + row * VOC_LD + lg * 8);
                    if (X3) {
                        const bf16x8 bl = *(const bf16x8*)(slo + row * VOC_LD + lg * 8);
#pragma unroll
                        for (int i = 0; i < NCO; ++i) {
                            acc[i][j] = mfma_bf16_16x16x32(ah[i], bl, acc[i][j]);
                            acc[i][j] = mfma_bf16_16x16x32(al[i], bh, acc[i][j]);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < NCO; ++i) acc[i][j] = mfma_bf16_16x16x32(ah[i], bh, acc[i][j]);
                }
            }
        }
    }

    float* ou = a.out + off * a.out_scale * a.c_out;
    const float* ru = a.residual ? a.residual + off * a.out_scale * a.c_out : nullptr;
#pragma unroll
    for (int j = 0; j < NTT; ++j) {
        const long long q = q0 + qw + j * 16 + li;
        const long long t = q * a.ostride + r - a.p;
        if (q >= Q || t < 0 || t >= Lout) continue;
#pragma unroll
        for (int i = 0; i < NCO; ++i) {
            const int co = cob + i * 16 + lg * 4;
            if (co >= a.c_out) continue;                              // c_out % 4 == 0
            f32x4 v = acc[i][j] + *(const f32x4*)(a.bias + co);
            if (ru) v += *(const f32x4*)(ru + t * a.c_out + co);
            float* o = ou + t * a.c_out + co;
            if (a.accumulate) v += *(const f32x4*)o;
            *(f32x4*)o = v * a.post_scale;
        }
    }
}

__global__ void __launch_bounds__(TAIL_T) voc_tail_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ out,
                                                          const long long* __restrict__ tab, long long scale, int C, int k, float slope)
{
    SS_DYN_SMEM(smem_raw);
    float* ws = (float*)smem_raw;              // [k][C] weights, then the bias
    float* xs = ws + k * C + 1;                // [TAIL_T + k - 1][C + 1]: the odd pitch keeps the 64 lanes' rows on distinct banks
    const int u = blockIdx.y, tid = threadIdx.x, half = (k - 1) / 2, NR = TAIL_T + k - 1, P = C + 1;
    const long long off = tab[2 * u] * scale, L = tab[2 * u + 1] * scale;
    const long long t0 = (long long)blockIdx.x * TAIL_T;
    if (t0 >= L) return;
    for (int e = tid; e <= k * C; e += TAIL_T) ws[e] = w[e];
    for (int e = tid; e < NR * C; e += TAIL_T) {
        const int i = e / C, c = e - i * C;
        const long long s = t0 - half + i;
        float v = 0.f;
        if (s >= 0 && s < L) { v = x[(off + s) * C + c]; v = v > 0.f ? v : v * slope; }
        xs[i * P + c] = v;
    }
    __syncthreads();
    const long long t = t0 + tid;
    if (t < L) {
        float acc = ws[k * C];
        for (int j = 0; j < k; ++j)
            for (int c = 0; c < C; ++c) acc = fmaf(ws[j * C + c], xs[(tid + j) * P + c], acc);
        out[off + t] = tanhf(acc);
    }
}

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

template <int NCO, bool X3>
int launch_conv_ntt(const VocArgs& a, int ntt, dim3 grid, void* stream)
{
    const size_t smem = (size_t)(ntt * 64 + a.span) * VOC_LD * sizeof(bf16_t) * (X3 ? 2 : 1);
    if (ntt == 4) SS_LAUNCH(SS_KERNEL(voc_conv_kernel<NCO, 4, X3>), grid, dim3(VOC_THREADS), smem, stream, a);
    else if (ntt == 2) SS_LAUNCH(SS_KERNEL(voc_conv_kernel<NCO, 2, X3>), grid, dim3(VOC_THREADS), smem, stream, a);
    else SS_LAUNCH(SS_KERNEL(voc_conv_kernel<NCO, 1, X3>), grid, dim3(VOC_THREADS), smem, stream, a);
    return 0;
}

// max_q: positions of the longest utterance.  The block's time extent shrinks (256 -> 128 -> 64 positions) while the launch would leave
// compute units idle or the longest utterance would not fill half of it.
int launch_conv(VocArgs& a, long long max_q, int n_utt, int x3, void* stream)
{
    const int n16 = a.co_pad / 16;
    const int nco = (n16 % 4 == 0) ? 4 : (n16 % 2 == 0) ? 2 : 1;
    const int gy = n16 / nco, gz = n_utt * a.phases, cus = ss_cu_count(4);
    int ntt = 4;
    while (ntt > 1 && (max_q <= ntt * 32 || ((max_q + ntt * 64 - 1) / (ntt * 64)) * gy * gz < cus)) ntt /= 2;
    const long long gx = (max_q + ntt * 64 - 1) / (ntt * 64);
    SS_CHECK(gx >= 1 && gx < (1ll << 31) && gz <= 65535 && gy <= 65535, "ss_voc: launch grid out of range");
    const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)gz);
    if (x3) {
        if (nco == 4) return launch_conv_ntt<4, true>(a, ntt, grid, stream);
        if (nco == 2) return launch_conv_ntt<2, true>(a, ntt, grid, stream);
        return launch_conv_ntt<1, true>(a, ntt, grid, stream);
    }
    if (nco == 4) return launch_conv_ntt<4, false>(a, ntt, grid, stream);
    if (nco == 2) return launch_conv_ntt<2, false>(a, ntt, grid, stream);
    return launch_conv_ntt<1, false>(a, ntt, grid, stream);
}

void bind_blob(VocArgs& a, const void* blob, int slots)
{
    a.bias = (const float*)blob;
    a.whi = (const bf16_t*)((const char*)blob + (size_t)a.co_pad * sizeof(float));
    a.wlo = a.whi + (size_t)slots * a.co_pad * a.ci_pad;
}
}  // namespace

extern "C" int ss_voc_supported(int c_in, int c_out, int k, int dilation_or_stride, int kind)
{
    if (c_in < 8 || k < 1 || dilation_or_stride < 1) return 0;
    if (kind == 2) return c_in <= TAIL_MAX_C && c_out == 1 && (k & 1) && k <= TAIL_MAX_K && dilation_or_stride == 1;
    if (c_in % 8 || c_out < 4 || c_out % 4) return 0;
    if (kind == 0) return (k & 1) && (long long)(k - 1) * dilation_or_stride <= VOC_MAX_SPAN;
    if (kind == 1) return k >= dilation_or_stride && (k - dilation_or_stride) % 2 == 0 && (k + dilation_or_stride - 1) / dilation_or_stride - 1 <= VOC_MAX_SPAN;
    return 0;
}

extern "C" int64_t ss_voc_blob_bytes(int slots, int c_out, int c_in)
{
    if (slots < 1 || c_out < 1 || c_in < 1) return -1;
    const int64_t co_pad = round_up(c_out, 16), ci_pad = round_up(c_in, VOC_CK);
    return co_pad * (int64_t)sizeof(float) + 2 * (int64_t)slots * co_pad * ci_pad * (int64_t)sizeof(bf16_t);
}

extern "C" int64_t ss_voc_workspace_bytes(int64_t total_frames, int c_initial, const int* rates, int n_ups)
{
    if (total_frames < 0 || c_initial < 1 || n_ups < 0 || (n_ups > 0 && !rates)) return -1;
    int64_t rows = total_frames, widest = total_frames * c_initial;
    for (int i = 0; i < n_ups; ++i) {
        if (rates[i] < 1) return -1;
        rows *= rates[i];
        const int64_t e = rows * (c_initial >> (i + 1));
        if (e > widest) widest = e;
    }
    const int64_t one = (widest * (int64_t)sizeof(float) + 255) / 256 * 256;
    return 4 * one;
}

extern "C" int ss_voc_conv1d(const float* x, const void* blob, const float* residual, float* out, const int64_t* table_dev, int n_utt,
                             int64_t max_frames, int scale, int c_in, int c_out, int k, int dilation, float slope, int accumulate,
                             float out_scale, int x3, void* stream)
{
    SS_CHECK(x && blob && out && table_dev, "ss_voc_conv1d: null pointer");
    SS_CHECK(n_utt >= 1 && max_frames >= 0 && scale >= 1, "ss_voc_conv1d: bad sizes");
    SS_CHECK(ss_voc_supported(c_in, c_out, k, dilation, 0), "ss_voc_conv1d: unsupported shape (c_in %d, c_out %d, k %d, dilation %d): c_in %% 8 == 0, c_out %% 4 == 0, k odd, (k - 1) dilation <= %d",
             c_in, c_out, k, dilation, VOC_MAX_SPAN);
    SS_CHECK((const void*)x != (const void*)out, "ss_voc_conv1d: out must not alias x (blocks read each other's halo)");
    if (max_frames == 0) return 0;
    VocArgs a;
    a.x = x; a.residual = residual; a.out = out; a.tab = (const long long*)table_dev;
    a.in_scale = a.out_scale = scale;
    a.c_in = c_in; a.c_out = c_out; a.ci_pad = round_up(c_in, VOC_CK); a.co_pad = round_up(c_out, 16);
    a.ntap = k; a.tap_off0 = -((k - 1) / 2) * dilation; a.tap_step = dilation; a.lo_off = a.tap_off0; a.span = (k - 1) * dilation;
    a.phases = 1; a.ostride = 1; a.p = 0; a.q_extra = 0;
    a.accumulate = accumulate; a.slope = slope; a.post_scale = out_scale;
    bind_blob(a, blob, k);
    int rc = launch_conv(a, max_frames * scale, n_utt, x3, stream);
    if (rc) return rc;
    SS_LAUNCH_CHECK("ss_voc_conv1d");
    return 0;
}

extern "C" int ss_voc_conv_transpose1d(const float* x, const void* blob, float* out, const int64_t* table_dev, int n_utt, int64_t max_frames,
                                       int scale, int c_in, int c_out, int k, int stride, float slope, int x3, void* stream)
{
    SS_CHECK(x && blob && out && table_dev, "ss_voc_conv_transpose1d: null pointer");
    SS_CHECK(n_utt >= 1 && max_frames >= 0 && scale >= 1, "ss_voc_conv_transpose1d: bad sizes");
    SS_CHECK(ss_voc_supported(c_in, c_out, k, stride, 1), "ss_voc_conv_transpose1d: unsupported shape (c_in %d, c_out %d, k %d, stride %d): c_in %% 8 == 0, c_out %% 4 == 0, k >= stride, k - stride even",
             c_in, c_out, k, stride);
    SS_CHECK((const void*)x != (const void*)out, "ss_voc_conv_transpose1d: out must not alias x");
    if (max_frames == 0) return 0;
    const int ntap = (k + stride - 1) / stride, p = (k - stride) / 2;
    VocArgs a;
    a.x = x; a.residual = nullptr; a.out = out; a.tab = (const long long*)table_dev;
    a.in_scale = scale; a.out_scale = (long long)scale * stride;
    a.c_in = c_in; a.c_out = c_out; a.ci_pad = round_up(c_in, VOC_CK); a.co_pad = round_up(c_out, 16);
    a.ntap = ntap; a.tap_off0 = 0; a.tap_step = -1; a.lo_off = -(ntap - 1); a.span = ntap - 1;
    a.phases = stride; a.ostride = stride; a.p = p; a.q_extra = p / stride + 1;
    a.accumulate = 0; a.slope = slope; a.post_scale = 1.f;
    bind_blob(a, blob, stride * ntap);
    int rc = launch_conv(a, max_frames * scale + a.q_extra, n_utt, x3, stream);
    if (rc) return rc;
    SS_LAUNCH_CHECK("ss_voc_conv_transpose1d");
    return 0;
}

extern "C" int ss_voc_tail(const float* x, const float* w, float* out, const int64_t* table_dev, int n_utt, int64_t max_frames, int scale,
                           int c_in, int k, float slope, void* stream)
{
    SS_CHECK(x && w && out && table_dev, "ss_voc_tail: null pointer");
    SS_CHECK(n_utt >= 1 && n_utt <= 65535 && max_frames >= 0 && scale >= 1, "ss_voc_tail: bad sizes");
    SS_CHECK(ss_voc_supported(c_in, 1, k, 1, 2), "ss_voc_tail: unsupported shape (c_in %d <= %d, k %d odd <= %d)", c_in, TAIL_MAX_C, k, TAIL_MAX_K);
    if (max_frames == 0) return 0;
    const long long gx = (max_frames * scale + TAIL_T - 1) / TAIL_T;
    SS_CHECK(gx < (1ll << 31), "ss_voc_tail: launch grid out of range");
    const size_t smem = ((size_t)k * c_in + 1 + (size_t)(TAIL_T + k - 1) * (c_in + 1)) * sizeof(float);
    SS_LAUNCH(voc_tail_kernel, dim3((unsigned)gx, (unsigned)n_utt), dim3(TAIL_T), smem, stream, x, w, out, (const long long*)table_dev,
              (long long)scale, c_in, k, slope);
    SS_LAUNCH_CHECK("ss_voc_tail");
    return 0;
}
