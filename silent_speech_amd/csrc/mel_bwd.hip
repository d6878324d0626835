// mel_bwd.hip -- the gradient of the log-mel spectrogram of mel.hip with respect to the audio: what HiFi-GAN's generator loss 45 L1(mel(y), mel(y^)) sends
// back through meldataset.mel_spectrogram (the reference's data_utils.py:39-62).  Forward per frame f of signal b (mel.hip):
//     x~[n] = clip?(y_pad[f hop + n]) w[n],  X = rfft(x~),  mag[k] = sqrt(re^2 + im^2 + 1e-9),  mel[m] = sum_k basis[m, k] mag[k],  out[m] = log(max(mel[m], clamp))
// Backward, given g_out[b, m, f]:
//     g_mel[m]  = mel[m] > clamp ? g_out[m] / mel[m] : 0
//     g_mag[k]  = sum_m basis[m, k] g_mel[m]                       the TRANSPOSED sparse filterbank: a bin lies under at most two neighbouring triangles
//     G[k]      = g_mag[k] X[k] / mag[k]                           (mag >= sqrt(1e-9): never a division by zero)
//     g_frame[n] = w[n] sum_{k = 0 .. 512} Re(G[k] e^(+2 pi i k n / 1024)) = w[n] 512 irfft(S)[n],  S = G except S_0 = 2 Re G_0, S_512 = 2 Re G_512
//     g_ypad[t] = sum_f g_frame_f[t - f hop],   g_y[s] = sum of g_ypad over the padded indices that read sample s (itself and its reflections),
//     times [|y[s]| <= 1] with clip.
// Two launches:
//   frames   ONE WAVE per frame, as in the forward: the frame's spectrum is computed AGAIN from the samples (1 KB read, ~26 kFLOP; saving it in the forward
//            would cost 4 KB per frame written and read back), the magnitudes, the mel values of the lane's bands, g_mel into the wave's LDS, g_mag and G per
//            bin in place of X, the inverse transform as the forward passes of fft1024.h on the conjugated packed spectrum (spectral_gate.hip's synthesis),
//            times the window -> the windowed frame gradient into a workspace [B F][1024] f32.  No barrier inside a frame.
//   gather   one thread per signal sample: the workspace rows of the frames that cover the sample's padded index, in ASCENDING frame order, first for
//            the sample itself, then for its left reflection, then for its right one.  No floating-point atomics: a sample's gradient depends on its own
//            signal only and is bitwise reproducible, whatever the batch, the grid or the order in which waves finish.
// Rows f >= (the signal's own frame count) of a ragged batch's g_out are filler: they are neither read nor written into the workspace.
#include "common.h"
#include "fft1024.h"
#include "silent_speech_hip.h"
#include <math.h>

namespace {
constexpr int MB_WAVES = 4;
constexpr int MB_MAXW = 4096, MB_MAXB = 128;               // the forward's bounds of the packed filterbank
constexpr int MB_MAGPAD = 8;                               // zeroed magnitudes behind bin 512 (runs are padded to multiples of 4)
constexpr int MB_BINS = MF_H + 1, MB_BINS_PAD = MF_H + 8;
constexpr int MB_MAXTAPS = 2;                              // bands over one bin
constexpr int MB_NONE = 255;                               // "no band" in a packed bin entry
constexpr int MB_GATHER = 256;
// resident workgroups per CU the frames kernel is compiled and launched for.  At 3 (the forward's 168 registers) the compiler keeps 65 registers in scratch and
// the two launches take 138 us for 16 512 frames; at 2 it takes 234 registers, no scratch: 90 us (tools/mel_probe.py --backward under a kernel trace).
#ifndef MB_BLOCKS_PER_CU
#define MB_BLOCKS_PER_CU 2
#endif

__device__ __forceinline__ float mb_sqrt(float x) {
#if defined(SS_EMU)
    return sqrtf(x);
#else
    return __builtin_amdgcn_sqrtf(x);                        // as in the forward (mel.hip): the recomputed mel values are the forward's
#endif
}
// frames of a signal of L samples (<= 0: none)
__device__ __forceinline__ int mb_frames(int L, int pad, int hop) { const int n = L + 2 * pad - MF_N; return n < 0 ? 0 : 1 + n / hop; }
}

// LDS: 4 x (4608 tile + 4160 spectrum + 2080 magnitudes + 512 g_mel) + 6240 bin table = 51.7 KB (three workgroups would fit a CU's 160 KB; the registers decide)
__global__ __launch_bounds__(MB_WAVES * 64, MB_BLOCKS_PER_CU) void stft_logmel_bwd_frames_kernel(const float* __restrict__ y, const long long* __restrict__ offs, const int* __restrict__ lens,
                                                                                long long uniform_len, int B, int F, int pad, int clip, int hop, const float* __restrict__ window,
                                                                                const int* __restrict__ band_lo, const int* __restrict__ band_cnt, const int* __restrict__ band_off,
                                                                                const float* __restrict__ band_w, const int* __restrict__ lane_bands,
                                                                                const int* __restrict__ bin_band, const float* __restrict__ bin_w, float log_clamp,
                                                                                const float* __restrict__ g_out, long long sb, long long sf, long long sm, float* __restrict__ frames_ws)
{
    __shared__ cpx tile_s[MB_WAVES][MF_TILE];
    __shared__ cpx spec_s[MB_WAVES][MB_BINS_PAD];
    __shared__ float mag_s[MB_WAVES][MF_H + MB_MAGPAD];
    __shared__ float gmel_s[MB_WAVES][MB_MAXB];
    __shared__ cpx binw_s[MB_BINS_PAD];
    __shared__ int binm_s[MB_BINS_PAD];
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_uniform(tid >> 6);
    for (int i = tid; i < MB_BINS; i += MB_WAVES * 64) { binw_s[i] = cpx{bin_w[2 * i], bin_w[2 * i + 1]}; binm_s[i] = bin_band[i]; }
    cpx* tl = tile_s[wv]; cpx* sp = spec_s[wv]; float* mg = mag_s[wv]; float* gm = gmel_s[wv];
    if (lane < MB_MAGPAD) mg[MF_H + lane] = 0.f;
    __syncthreads();

    // ---- per-lane constants (the forward's)
    const int r = lane;
    cpx win[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { const int n = r + 64 * q; win[q] = cpx{window[2 * n], window[2 * n + 1]}; }
    cpx tw1[8], tw2[8], tw3[8];
    fft512_twiddles(lane, tw1, tw2, tw3);
    const cpx tw_nyq = twiddle(MF_H, MF_N);
    int bm[2], blo[2], bcnt[2], boff[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        bm[it] = lane_bands[it * 64 + lane];
        const int m = bm[it] >= 0 ? bm[it] : 0;
        blo[it] = band_lo[m]; bcnt[it] = bm[it] >= 0 ? band_cnt[m] : 0; boff[it] = band_off[m];
    }
    // G[k] = g_mag[k] X[k] / mag[k] of bin k, g_mag from the (at most two) bands over the bin
    auto bin_grad = [&](int k) -> cpx {
        const int pk = binm_s[k], m0 = pk & 255, m1 = (pk >> 8) & 255;
        const cpx w2 = binw_s[k];
        const float g0 = m0 != MB_NONE ? w2[0] * gm[m0 & (MB_MAXB - 1)] : 0.f, g1 = m1 != MB_NONE ? w2[1] * gm[m1 & (MB_MAXB - 1)] : 0.f;
        return sp[k] * ((g0 + g1) / mg[k]);
    };

    const long long total = (long long)B * F;
    const long long wave0 = (long long)blockIdx.x * MB_WAVES + wv, nwaves = (long long)gridDim.x * MB_WAVES;
    for (long long g = wave0; g < total; g += nwaves) {
        const int b = (int)(g / F), f = (int)(g - (long long)b * F);
        const float* x = y + (offs ? offs[b] : (long long)b * uniform_len);
        const int L = wave_uniform(offs ? lens[b] : (int)uniform_len);
        if (f >= wave_uniform(mb_frames(L, pad, hop))) continue;      // (wave-uniform) a filler row of a ragged batch
        const int i0 = wave_uniform(f * hop - pad);
        // ---- the frame's spectrum again: the forward's loads, clip, window and passes
        cpx v[8];
        if (i0 >= 0 && i0 + MF_N <= L) {
#pragma unroll
            for (int q = 0; q < 8; ++q) { const float* p = x + i0 + 2 * (r + 64 * q); v[q] = cpx{p[0], p[1]}; }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int t = i0 + 2 * (r + 64 * q) + h;
                    int s = t < 0 ? -t : (t >= L ? 2 * (L - 1) - t : t);
                    const bool in = t >= -pad && t < L + pad;
                    s = s < 0 ? 0 : (s > L - 1 ? L - 1 : s);
                    v[q][h] = in ? x[s] : 0.f;
                }
            }
        }
        if (clip) {
#pragma unroll
            for (int q = 0; q < 8; ++q) { v[q][0] = fminf(fmaxf(v[q][0], -1.f), 1.f); v[q][1] = fminf(fmaxf(v[q][1], -1.f), 1.f); }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] *= win[q];
        fft512(v, tl, lane, tw1, tw2);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = lane + 64 * j;
            const cpx xk = rfft_bin(tl, k, tw3[j]);
            mg[k] = mb_sqrt(xk[0] * xk[0] + xk[1] * xk[1] + 1e-9f);
            sp[k] = xk;
        }
        if (lane == 0) {
            const cpx xk = rfft_nyquist(tl, tw_nyq);
            mg[MF_H] = mb_sqrt(xk[0] * xk[0] + xk[1] * xk[1] + 1e-9f);
            sp[MF_H] = xk;
        }
        wave_lds_sync();
        // ---- the mel values of this lane's bands (the forward's sums) -> g_mel = g_out / mel above the clamp
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            float acc0 = 0.f, acc1 = 0.f;
            const float* wp = band_w + boff[it]; const float* mp = mg + blo[it];
            for (int j = 0; j < bcnt[it]; j += 4) {
                const f32x4 w4 = *(const f32x4*)(wp + j);              // runs start at multiples of 4 floats
                acc0 += w4[0] * mp[j]; acc1 += w4[1] * mp[j + 1];
                acc0 += w4[2] * mp[j + 2]; acc1 += w4[3] * mp[j + 3];
            }
            if (bm[it] >= 0) {
                const float mel = acc0 + acc1;
                const float go = g_out[(long long)b * sb + (long long)f * sf + (long long)bm[it] * sm];
                gm[bm[it]] = mel > log_clamp ? go / mel : 0.f;
            }
        }
        wave_lds_sync();
        // ---- G in place of X; bins 0 and 512 count with their real parts, once: S_0 = 2 Re G_0, S_512 = 2 Re G_512
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = lane + 64 * j;
            const cpx G = bin_grad(k);
            sp[k] = k ? G : cpx{2.f * G[0], 0.f};
        }
        if (lane == 0) { const cpx G = bin_grad(MF_H); sp[MF_H] = cpx{2.f * G[0], 0.f}; }
        wave_lds_sync();
        // ---- inverse: v[j] = conj Z[k], Z[k] = E + i O, E = (S[k] + conj S[512 - k]) / 2, O = (S[k] - conj S[512 - k]) / 2 conj W_1024^k, k = lane + 64 j
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = lane + 64 * j;
            const cpx a = sp[k], c0 = sp[MF_H - k], c = cpx{c0[0], -c0[1]};
            const cpx e = 0.5f * (a + c), o = cmul(0.5f * (a - c), cpx{tw3[j][0], -tw3[j][1]});
            v[j] = cpx{e[0] - o[1], -(e[1] + o[0])};
        }
        fft512(v, tl, lane, tw1, tw2);
        float* out = frames_ws + g * MF_N;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int n = lane + 64 * q;
            const cpx rr = tl[zpos(n)];                                // conj(512 z[n]), z[n] = irfft(S)[2n] + i irfft(S)[2n + 1]
            *(cpx*)(out + 2 * n) = cpx{rr[0] * win[q][0], -rr[1] * win[q][1]};
        }
    }
}

// one thread per sample s of signal blockIdx.y; workspace row b F + f = the windowed gradient of frame f
__global__ __launch_bounds__(MB_GATHER) void stft_logmel_bwd_gather_kernel(const float* __restrict__ frames_ws, const float* __restrict__ y, const long long* __restrict__ offs,
                                                                          const int* __restrict__ lens, long long uniform_len, int F, int pad, int clip, int hop,
                                                                          float* __restrict__ g_y)
{
    const int b = blockIdx.y;
    const int L = offs ? lens[b] : (int)uniform_len;
    const int s = blockIdx.x * MB_GATHER + threadIdx.x;
    if (s >= L) return;
    const long long base = offs ? offs[b] : (long long)b * uniform_len;
    int Fb = mb_frames(L, pad, hop);
    Fb = Fb < F ? Fb : F;
    const float* w = frames_ws + (long long)b * F * MF_N;
    float acc = 0.f;
    auto add = [&](int t) {                                          // the frames f with 0 <= t - f hop < 1024, ascending
        const int f0 = t >= MF_N ? (t - MF_N) / hop + 1 : 0;
        int f1 = t / hop;
        f1 = f1 < Fb - 1 ? f1 : Fb - 1;
        for (int f = f0; f <= f1; ++f) acc += w[(long long)f * MF_N + (t - f * hop)];
    };
    add(s + pad);
    if (s >= 1 && s <= pad) add(pad - s);                            // read again by the left reflection
    if (s >= L - 1 - pad && s <= L - 2) add(pad + 2 * (L - 1) - s);  // ... by the right one
    if (clip && fabsf(y[base + s]) > 1.f) acc = 0.f;                 // torch.clamp passes the gradient on the closed interval
    g_y[base + s] = acc;
}

extern "C" int64_t ss_stft_logmel_fft_backward_workspace_bytes(int B, int F)
{
    if (B < 0 || F < 0) return -1;
    return (int64_t)B * F * MF_N * (int64_t)sizeof(float);
}

extern "C" int ss_stft_logmel_fft_backward(const float* y, const int64_t* offsets_dev, const int32_t* lengths_dev, int64_t uniform_len, int64_t max_len, int B, int F, int pad,
                                           int clip, int n_fft, int hop, const float* window,
                                           const int32_t* band_lo, const int32_t* band_cnt, const int32_t* band_off, const float* band_w, const int32_t* lane_bands, int n_mels,
                                           int n_w, const int32_t* bin_band, const float* bin_w, int bin_taps, float log_clamp,
                                           const float* g_out, int64_t stride_b, int64_t stride_f, int64_t stride_m, float* workspace, int64_t workspace_bytes, float* g_y,
                                           void* stream)
{
    SS_CHECK(y && window && band_lo && band_cnt && band_off && band_w && lane_bands && bin_band && bin_w && g_out && workspace && g_y, "ss_stft_logmel_fft_backward: null pointer");
    SS_CHECK((offsets_dev != nullptr) == (lengths_dev != nullptr), "ss_stft_logmel_fft_backward: offsets and lengths come together (ragged batch) or not at all (rows of uniform_len samples)");
    SS_CHECK(n_fft == MF_N, "ss_stft_logmel_fft_backward: n_fft must be %d (the DFT-GEMM path has no gradient)", MF_N);
    SS_CHECK(hop > 0 && hop % 4 == 0 && pad >= 0 && (offsets_dev || uniform_len > pad), "ss_stft_logmel_fft_backward: bad hop %d / pad %d / length %lld (hop a multiple of 4, reflect needs pad < length)",
             hop, pad, (long long)uniform_len);
    SS_CHECK(B >= 0 && B <= 65535 && F >= 0, "ss_stft_logmel_fft_backward: %d signals x %d frames (0 .. 65535 signals)", B, F);
    SS_CHECK(max_len >= (offsets_dev ? 0 : uniform_len) && max_len <= 0x7fffffff - 2 * (int64_t)pad - MB_GATHER, "ss_stft_logmel_fft_backward: bad longest length %lld", (long long)max_len);
    SS_CHECK(offsets_dev || F <= (uniform_len + 2 * (int64_t)pad < MF_N ? 0 : 1 + (uniform_len + 2 * (int64_t)pad - MF_N) / hop),
             "ss_stft_logmel_fft_backward: %d frames, but rows of %lld samples have fewer", F, (long long)uniform_len);
    SS_CHECK(n_mels >= 1 && n_mels <= MB_MAXB && n_w >= 0 && n_w <= MB_MAXW, "ss_stft_logmel_fft_backward: %d bands / %d packed weights exceed the tables (%d / %d)", n_mels, n_w, MB_MAXB, MB_MAXW);
    SS_CHECK(bin_taps >= 0 && bin_taps <= MB_MAXTAPS, "ss_stft_logmel_fft_backward: %d bands over one bin exceed the per-bin table (%d)", bin_taps, MB_MAXTAPS);
    const long long total = (long long)B * F;
    SS_CHECK(workspace_bytes >= total * MF_N * (long long)sizeof(float), "ss_stft_logmel_fft_backward: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             total * MF_N * (long long)sizeof(float));
    if (B == 0 || max_len == 0) return 0;
    if (total) {
        long long blocks = (total + MB_WAVES - 1) / MB_WAVES;
        const long long cap = (long long)ss_cu_count(2) * MB_BLOCKS_PER_CU;      // workgroups of 4 waves per CU: what is resident
        if (blocks > cap) blocks = cap;
        SS_LAUNCH(stft_logmel_bwd_frames_kernel, dim3((unsigned)blocks), dim3(MB_WAVES * 64), 0, stream, y, (const long long*)offsets_dev, lengths_dev, (long long)uniform_len, B, F, pad, clip, hop,
                  window, band_lo, band_cnt, band_off, band_w, lane_bands, bin_band, bin_w, log_clamp, g_out, (long long)stride_b, (long long)stride_f, (long long)stride_m, workspace);
    }
    SS_LAUNCH(stft_logmel_bwd_gather_kernel, dim3((unsigned)((max_len + MB_GATHER - 1) / MB_GATHER), (unsigned)B), dim3(MB_GATHER), 0, stream, (const float*)workspace, y,
              (const long long*)offsets_dev, lengths_dev, (long long)uniform_len, F, pad, clip, hop, g_y);
    SS_LAUNCH_CHECK("ss_stft_logmel_fft_backward");
    return 0;
}
