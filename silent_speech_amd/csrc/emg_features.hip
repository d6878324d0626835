// emg_features.hip -- the 112-d hand-crafted EMG features of the reference's data_utils.get_emg_features (data_utils.py:85-136), computed
// on the 516.79 Hz signal that load_utterance hands it (read_emg.py:71-78), for a ragged batch of recordings in ONE launch.
//
// Per channel c of a recording x (n, C) f64:
//     xs = x - mean(x)                          over the whole recording
//     v  = convolve(xs, ones(9) / 9, 'same')    zero padding of xs
//     w  = convolve(v,  ones(9) / 9, 'same')    zero padding of v (NOT v extended past the ends)
//     p  = xs - w,  r = |p|
// and per frame f = samples [6 f, 6 f + 16) (librosa.util.frame(16, 6); F = 1 + (n - 16) / 6 frames) the 14 columns c * 14 + j:
//     mean(w), rms(w), rms(r), zero-crossing rate of p (|p| <= 1e-10 -> 0, signbit, 15 neighbour pairs / 16), mean(r),
//     |rfft(hann16 * xs[6 f : 6 f + 16])| (9 bins, periodic Hann window).
// Mean, box filters and p are f64 like numpy; the features are rounded to f32 on the store (data_utils.py:136).
//
// Work split: block (u, b) owns the frame tiles b, b + nb, b + 2 nb, .. of recording u (nb = min(tiles of u, EF_MAX_BLOCKS)), a tile being
// EF_THREADS / C frames, one (frame, channel) per thread.  Every block first reduces its recording's column means itself, in a fixed order
// (so every block of u, and a one-recording call, sees bit-identical means) -- the price of a single launch without a workspace is that
// each of the <= EF_MAX_BLOCKS blocks of a recording reads the recording once more, from L2.  It then stages xs of its tile with an
// 8-sample halo in LDS, forms v and w there, and every thread reduces its frame.
#include "common.h"
#include "silent_speech_hip.h"
#include <math.h>

// numpy evaluates the sums with separate multiplies and adds; keep the compiler from contracting them into FMAs (as filters.hip does)
#pragma clang fp contract(off)

namespace {
constexpr int EF_THREADS = 256;
constexpr int EF_FL = 16, EF_HOP = 6, EF_NF = 14;   // frame length, hop, features per channel
constexpr int EF_BOX = 9, EF_HALF = 4;               // np.ones(9) / 9, 'same' -> 4 samples each side
constexpr int EF_HALO = 2 * EF_HALF;                 // two passes
constexpr int EF_MAX_C = 32;
constexpr int EF_LOADS = 8;                          // mean reduction: loads per thread in flight
constexpr int EF_MAX_BLOCKS = 16;                    // per recording: bounds the re-reads of the mean; longer recordings loop over tiles

__host__ __device__ constexpr int ef_tile_frames(int C) { return EF_THREADS / C; }
__host__ __device__ constexpr int ef_tile_rows(int C) { return EF_HOP * (ef_tile_frames(C) - 1) + EF_FL; }
// LDS: xs (rows + 16) x C | v (rows + 8) x C | w rows x C | mean partials EF_THREADS | means C   (doubles)
__host__ __device__ constexpr int ef_smem_doubles(int C) { return (3 * ef_tile_rows(C) + 3 * EF_HALF * 2) * C + EF_THREADS + C; }

__global__ void __launch_bounds__(EF_THREADS) emg_features_kernel(const double* __restrict__ x, float* __restrict__ out,
                                                                  const long long* __restrict__ tab, int C)
{
    SS_DYN_SMEM(smem_raw);
    double* smem = (double*)smem_raw;
    const int TF = ef_tile_frames(C), S = ef_tile_rows(C);
    double* xs = smem;                                  // row j <-> sample s0 - 8 + j
    double* v = xs + (S + 2 * EF_HALO) * C;             // row j <-> sample s0 - 4 + j
    double* w = v + (S + EF_HALO) * C;                  // row j <-> sample s0 + j
    double* part = w + S * C;
    double* mean = part + EF_THREADS;

    const int u = blockIdx.x, t = threadIdx.x;
    const long long in0 = tab[u * 4], n = tab[u * 4 + 1], out0 = tab[u * 4 + 2], F = tab[u * 4 + 3];
    const long long tiles = (F + TF - 1) / TF;
    const long long nb = tiles < EF_MAX_BLOCKS ? tiles : EF_MAX_BLOCKS;
    if ((long long)blockIdx.y >= nb) return;            // uniform per block: no barrier has been reached yet
    const double* xr = x + in0 * C;

    // ---- column means: thread t sums rows t / C, t / C + RS, .. of channel t % C in order, then thread c adds the partials of its channel
    const int RS = EF_THREADS / C, used = RS * C;
    {
        double acc = 0.0;
        if (t < used) {
            const int c = t % C;
            for (long long i0 = t / C; i0 < n; i0 += (long long)RS * EF_LOADS) {
                double ld[EF_LOADS];                                      // all loads of a step in flight before the first add
#pragma unroll
                for (int k = 0; k < EF_LOADS; ++k) { const long long i = i0 + (long long)k * RS; ld[k] = i < n ? xr[i * C + c] : 0.0; }
#pragma unroll
                for (int k = 0; k < EF_LOADS; ++k) acc += ld[k];
            }
        }
        part[t] = acc;
        __syncthreads();
        if (t < C) {
            double s = 0.0;
            for (int k = t; k < used; k += C) s += part[k];
            mean[t] = n > 0 ? s / (double)n : 0.0;
        }
        __syncthreads();
    }

    const double box = 1.0 / 9.0;
    const int nx = (S + 2 * EF_HALO) * C, nv = (S + EF_HALO) * C, nw = S * C;
    for (long long tile = blockIdx.y; tile < tiles; tile += nb) {
        const long long f0 = tile * TF, s0 = f0 * EF_HOP;
        // xs with its 8-sample halo; zero outside [0, n) is the zero padding of the first box filter
        for (int e = t; e < nx; e += EF_THREADS) {
            const int j = e / C, c = e - j * C;
            const long long g = s0 - EF_HALO + j;
            xs[e] = (g >= 0 && g < n) ? xr[g * C + c] - mean[c] : 0.0;
        }
        __syncthreads();
        // v on [s0 - 4, s0 + S + 4); zero outside [0, n): the second filter pads ITS input with zeros
        for (int e = t; e < nv; e += EF_THREADS) {
            const int j = e / C, c = e - j * C;
            const long long g = s0 - EF_HALF + j;
            double acc = 0.0;
            if (g >= 0 && g < n) {
#pragma unroll
                for (int k = 0; k < EF_BOX; ++k) acc += xs[(j + k) * C + c] * box;
            }
            v[e] = acc;
        }
        __syncthreads();
        for (int e = t; e < nw; e += EF_THREADS) {
            const int j = e / C, c = e - j * C;
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < EF_BOX; ++k) acc += v[(j + k) * C + c] * box;
            w[e] = acc;
        }
        __syncthreads();
        // one (frame, channel) per thread
        const int fl = t / C, c = t - fl * C;
        const long long f = f0 + fl;
        if (t < TF * C && f < F) {
            const double cw[16] = {1.0, 0.9238795325112867, 0.7071067811865476, 0.38268343236508984, 6.123233995736766e-17, -0.3826834323650897,
                                   -0.7071067811865475, -0.9238795325112867, -1.0, -0.9238795325112868, -0.7071067811865477, -0.38268343236509034,
                                   -1.8369701987210297e-16, 0.38268343236509, 0.7071067811865474, 0.9238795325112865};        // cos(2 pi m / 16)
            const double sw[16] = {0.0, 0.3826834323650898, 0.7071067811865475, 0.9238795325112867, 1.0, 0.9238795325112867, 0.7071067811865476,
                                   0.3826834323650899, 1.2246467991473532e-16, -0.38268343236508967, -0.7071067811865475, -0.9238795325112865,
                                   -1.0, -0.9238795325112866, -0.7071067811865477, -0.3826834323650904};                      // sin(2 pi m / 16)
            const int r0 = fl * EF_HOP;
            double sw_ = 0.0, sww = 0.0, sr = 0.0, srr = 0.0, y[EF_FL];
            int crossings = 0;
            bool prev = false;
#pragma unroll
            for (int k = 0; k < EF_FL; ++k) {
                const double wk = w[(r0 + k) * C + c], xk = xs[(r0 + k + EF_HALO) * C + c];
                const double pk = xk - wk, rk = fabs(pk);
                sw_ += wk; sww += wk * wk; sr += rk; srr += rk * rk;
                const bool neg = rk <= 1e-10 ? false : signbit(pk);       // librosa.zero_crossings: |p| <= threshold -> 0, signbit (0 counts positive)
                if (k > 0 && neg != prev) ++crossings;
                prev = neg;
                y[k] = (0.5 - 0.5 * cw[k]) * xk;                           // periodic Hann window on xs
            }
            float* o = out + (out0 + f) * (long long)(EF_NF * C) + c * EF_NF;
            o[0] = (float)(sw_ / EF_FL);
            o[1] = (float)sqrt(sww / EF_FL);
            o[2] = (float)sqrt(srr / EF_FL);
            o[3] = (float)((double)crossings / EF_FL);
            o[4] = (float)(sr / EF_FL);
#pragma unroll
            for (int b = 0; b <= EF_FL / 2; ++b) {
                double re = 0.0, im = 0.0;
#pragma unroll
                for (int k = 0; k < EF_FL; ++k) {
                    const int m = (b * k) & (EF_FL - 1);
                    re += y[k] * cw[m];
                    im -= y[k] * sw[m];
                }
                o[5 + b] = (float)sqrt(re * re + im * im);
            }
        }
        __syncthreads();                                                  // the next tile overwrites xs / v / w
    }
}
}  // namespace

// table_dev: int64 [R][4] = {first input row, n, first output row, F} per recording (device memory); x packed (rows, C) f64,
// out packed (total_frames, 14 C) f32.  F must be 1 + (n - 16) / 6 (0 for n < 16).
extern "C" int ss_emg_features_batch(const double* x, float* out, const int64_t* table_dev, int R, int C, int64_t total_frames, void* stream)
{
    SS_CHECK(x && out && table_dev, "ss_emg_features_batch: null pointer");
    SS_CHECK(R >= 1 && C >= 1 && C <= EF_MAX_C && total_frames >= 0, "ss_emg_features_batch: bad sizes (R >= 1, 1 <= C <= %d)", EF_MAX_C);
    if (total_frames == 0) return 0;
    // no recording has more tiles than the whole batch: blocks beyond a recording's own count return at once
    const long long tf = ef_tile_frames(C), max_tiles = (total_frames + tf - 1) / tf;
    const int nb = (int)(max_tiles < EF_MAX_BLOCKS ? max_tiles : EF_MAX_BLOCKS);
    const size_t smem = (size_t)ef_smem_doubles(C) * sizeof(double);
    SS_LAUNCH(emg_features_kernel, dim3((unsigned)R, (unsigned)nb), dim3(EF_THREADS), smem, stream, x, out, (const long long*)table_dev, C);
    SS_LAUNCH_CHECK("ss_emg_features_batch");
    return 0;
}
