// spectral_gate_common.h -- what the stationary gate (spectral_gate.hip) and the non-stationary gate (spectral_gate_ns.hip) share: the ragged frame
// table, the framing of one wave's frame for the FFT of fft1024.h, the split of the frames over the waves, and the deterministic overlap-add.
#pragma once
#include "common.h"
#include "fft1024.h"
#include <math.h>

namespace {
constexpr int SG_WAVES = 4, SG_BINS = 513, SG_HOP = 256;
constexpr int SG_MAX_NF = 32, SG_MAX_NT = 8;
constexpr int SG_PAD = SG_MAX_NF;                                   // zeros on both sides of the time-combined counts
constexpr int SG_PER = 9;                                           // consecutive bins per lane in the frequency smoothing: 64 x 9 = 576 >= 513
constexpr int SG_CBUF = SG_PAD + 64 * SG_PER + SG_PAD + 4;          // (the lanes behind bin 512 read zeros up to n_f + 1 places past their last bin)

// tab[u] = {first sample, L, first frame, F}; the utterance that holds global frame g
__device__ __forceinline__ int sg_find(const long long* __restrict__ tab, int R, long long g) {
    int lo = 0, hi = R - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tab[mid * 4 + 2] <= g) lo = mid; else hi = mid - 1; }
    return lo;
}
// lane r's v[q] = z[r + 64 q] = (x[2n], x[2n + 1]) w of frame f, n = r + 64 q; zeros outside [0, L)
__device__ __forceinline__ void sg_load_frame(const float* __restrict__ x, int L, int f, int r, const cpx (&win)[8], cpx (&v)[8]) {
    const int i0 = wave_uniform(f * SG_HOP - MF_H);
    if (i0 >= 0 && i0 + MF_N <= L) {
#pragma unroll
        for (int q = 0; q < 8; ++q) { const float* p = x + i0 + 2 * (r + 64 * q); v[q] = cpx{p[0], p[1]}; }
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
#pragma unroll
            for (int h = 0; h < 2; ++h) { const int t = i0 + 2 * (r + 64 * q) + h; v[q][h] = (t >= 0 && t < L) ? x[t] : 0.f; }
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] *= win[q];
}
__device__ __forceinline__ float sg_mag(cpx x) { return sqrtf(x[0] * x[0] + x[1] * x[1]); }
// the frames [g0, g1) of wave `wave` out of `nwaves`: consecutive runs
__device__ __forceinline__ void sg_run(long long total, long long wave, long long nwaves, long long& g0, long long& g1) {
    const long long per = (total + nwaves - 1) / nwaves;
    g0 = wave * per; g1 = g0 + per < total ? g0 + per : total;
}

// one workgroup per hop of 256 output samples; hop h of utterance u is global hop (first frame of u) - u + h, since F = hops + 1
__global__ __launch_bounds__(SG_HOP) void sg_overlap_add_kernel(const float* __restrict__ frames, const long long* __restrict__ tab, int R,
                                                                const float* __restrict__ wsq, float* __restrict__ y)
{
    const long long gh = blockIdx.x;
    int lo = 0, hi = R - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tab[mid * 4 + 2] - mid <= gh) lo = mid; else hi = mid - 1; }
    const long long fr0 = tab[lo * 4 + 2], L = tab[lo * 4 + 1];
    const int F = (int)tab[lo * 4 + 3], h = (int)(gh - (fr0 - lo));
    const long long n = (long long)h * SG_HOP + threadIdx.x;
    if (n >= L) return;
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int d = -1; d <= 2; ++d) {                                   // ascending frame order
        const int f = h + d;
        if (f >= 0 && f < F) {
            const int i = (int)(n - (long long)f * SG_HOP) + MF_H;    // 0 <= i < 1024
            num += frames[(fr0 + f) * MF_N + i];
            den += wsq[i];
        }
    }
    y[tab[lo * 4] + n] = num / den;
}

int sg_grid(long long total) {
    long long blocks = (total + SG_WAVES - 1) / SG_WAVES;
    const long long cap = (long long)ss_cu_count(2) * 4;             // 4 workgroups of 4 waves per CU (LDS: 48 KB per workgroup in the synthesis)
    return (int)(blocks < cap ? blocks : cap);
}
}  // namespace
