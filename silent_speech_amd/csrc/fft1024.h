// fft1024.h -- the 1024-point real FFT of ONE WAVE, shared by mel.hip (log-mel targets) and spectral_gate.hip (spectral gating, forward and inverse).
// The 1024 real samples are packed into 512 complex numbers z[n] = x[2n] + i x[2n+1]; 512 = 8 x 8 x 8: three radix-8 passes in registers (lane = one
// butterfly of 8; complex numbers are float pairs, so adds / twiddle products are v_pk_add_f32 / v_pk_fma_f32), two transposes through the wave's own
// 4.6 KiB LDS tile (8-byte elements, pitches 72 / 9 and a skew of the last layout: every access of a pass is conflict-free), twiddles W_512^(r k0),
// W_64^(r0 k0') per lane in registers.  The spectrum of the real signal is recombined from Z[k] and conj Z[512 - k]; the inverse runs the same passes
// on conj Z (spectral_gate.hip).  No barrier inside a frame: LDS serves a wave's operations in order, wave_lds_sync is a compiler-level fence.
#pragma once
#include "common.h"
#include <math.h>

namespace {
constexpr int MF_N = 1024, MF_H = 512;
constexpr int MF_P1 = 72, MF_P2 = 9;                       // LDS pitches of the two transposes (complex elements)
constexpr int MF_TILE = 8 * MF_P1;                         // complex elements of a wave's tile

typedef float cpx __attribute__((ext_vector_type(2)));     // (re, im)
__device__ __forceinline__ cpx cmul(cpx a, cpx b) { const cpx bs = {-b[1], b[0]}; return a[0] * b + a[1] * bs; }      // two packed operations
__device__ __forceinline__ cpx mul_mi(cpx a) { return cpx{a[1], -a[0]}; }                                               // a * (-i)
// e^(-2 pi i num / den)
__device__ __forceinline__ cpx twiddle(int num, int den) {
#if defined(SS_EMU)
    const double a = -2.0 * 3.14159265358979323846 * (double)num / (double)den;
    return cpx{(float)cos(a), (float)sin(a)};
#else
    float s, c;
    sincospif(2.0f * (float)num / (float)den, &s, &c);      // the argument is exact (den a power of two)
    return cpx{c, -s};
#endif
}
// X[k] = sum_q x[q] e^(-2 pi i q k / 8), in place, natural order: one radix-2 split (decimation in frequency) and two 4-point transforms
__device__ __forceinline__ void dft4(cpx c0, cpx c1, cpx c2, cpx c3, cpx& y0, cpx& y1, cpx& y2, cpx& y3) {
    const cpx e0 = c0 + c2, e1 = c0 - c2, o0 = c1 + c3, o1 = mul_mi(c1 - c3);
    y0 = e0 + o0; y2 = e0 - o0; y1 = e1 + o1; y3 = e1 - o1;
}
__device__ __forceinline__ void dft8(cpx (&x)[8]) {
    constexpr float H = 0.70710678118654752f;
    cpx a[4], b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { a[q] = x[q] + x[q + 4]; b[q] = x[q] - x[q + 4]; }
    b[1] = cpx{b[1][0] + b[1][1], b[1][1] - b[1][0]} * H;            // (1 - i) / sqrt 2
    b[2] = mul_mi(b[2]);                                               // -i
    b[3] = cpx{b[3][1] - b[3][0], -(b[3][0] + b[3][1])} * H;         // (-1 - i) / sqrt 2
    dft4(a[0], a[1], a[2], a[3], x[0], x[2], x[4], x[6]);
    dft4(b[0], b[1], b[2], b[3], x[1], x[3], x[5], x[7]);
}
// position of Z[k] in the tile: a skew of 4 elements per 32, so that the pass-3 stores (k = k0 + 8 k0' + 64 k1' over the lanes (k0, k0')) and the
// recombination's reads (k = lane + 64 j, and 512 - k) both touch 32 distinct 8-byte bank pairs per half wave
__device__ __forceinline__ int zpos(int k) { return k + 4 * (k >> 5); }
static_assert(MF_H - 1 + 4 * ((MF_H - 1) >> 5) < MF_TILE, "the skewed spectrum fits the tile");

// the per-lane twiddles of the three passes and of the real-signal recombination: tw1[k] = W_512^(lane k), tw2[k] = W_64^((lane & 7) k), tw3[j] = W_1024^(lane + 64 j)
__device__ __forceinline__ void fft512_twiddles(int lane, cpx (&tw1)[8], cpx (&tw2)[8], cpx (&tw3)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) { tw1[k] = twiddle(lane * k, MF_H); tw2[k] = twiddle((lane & 7) * k, 64); tw3[k] = twiddle(lane + 64 * k, MF_N); }
}
// The 512-point complex FFT of a wave: lane r hands in v[q] = z[r + 64 q], q = 0 .. 7; Z[k] is left at tl[zpos(k)] (v is clobbered).
__device__ __forceinline__ void fft512(cpx (&v)[8], cpx* tl, int lane, const cpx (&tw1)[8], const cpx (&tw2)[8]) {
    const int r = lane, k0l = lane >> 3, r0 = lane & 7;            // pass 1: lane = r; pass 2: lane = (k0, r0); pass 3: lane = (k0, k0')
    // ---- pass 1: z[r + 64 q], q = 0 .. 7 -> radix 8 over q -> T[k0][r] = W_512^(r k0) sum_q z[r + 64 q] W_8^(q k0)
    dft8(v);
    wave_lds_sync();                                               // (the previous frame's reads of the tile are behind us)
#pragma unroll
    for (int k = 0; k < 8; ++k) tl[k * MF_P1 + r] = k ? cmul(v[k], tw1[k]) : v[k];
    wave_lds_sync();
    // ---- pass 2: lane (k0, r0): T[k0][r0 + 8 r1], r1 = 0 .. 7 -> radix 8 over r1 -> U[k0][r0][k0'] = W_64^(r0 k0') sum_r1 T W_8^(r1 k0')
#pragma unroll
    for (int r1 = 0; r1 < 8; ++r1) v[r1] = tl[k0l * MF_P1 + r0 + 8 * r1];
    dft8(v);
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < 8; ++k) tl[k0l * MF_P1 + r0 * MF_P2 + k] = k ? cmul(v[k], tw2[k]) : v[k];
    wave_lds_sync();
    // ---- pass 3: lane (k0, k0' = lane & 7): U[k0][r0][k0'], r0 = 0 .. 7 -> radix 8 over r0 -> Z[k0 + 8 k0' + 64 k1']
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = tl[k0l * MF_P1 + q * MF_P2 + r0];
    dft8(v);
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < 8; ++k) tl[zpos(k0l + 8 * r0 + 64 * k)] = v[k];
    wave_lds_sync();
}
// bin k = lane + 64 j (0 <= k < 512) of the real signal: X[k] = E + W_1024^k O, E = (Z[k] + conj Z[512 - k]) / 2, O = (Z[k] - conj Z[512 - k]) / (2 i); tw = W_1024^k
__device__ __forceinline__ cpx rfft_bin(const cpx* tl, int k, cpx tw) {
    const int km = (MF_H - k) & (MF_H - 1);
    const cpx a = tl[zpos(k)], c0 = tl[zpos(km)], c = cpx{c0[0], -c0[1]};
    const cpx e = 0.5f * (a + c), o = mul_mi(0.5f * (a - c));
    return e + cmul(o, tw);
}
// bin 512: Z[512] = Z[0]: E = re Z[0], O = im Z[0]; tw_nyq = W_1024^512
__device__ __forceinline__ cpx rfft_nyquist(const cpx* tl, cpx tw_nyq) {
    const cpx a = tl[0];
    return cpx{a[0], 0.f} + cmul(cpx{a[1], 0.f}, tw_nyq);
}
}  // namespace
