// spectral_gate_ns.hip -- NON-STATIONARY spectral gating of recorded audio (noisereduce 3's default mode, nr.reduce_noise(y, sr), restated in
// tests/spectral_gate_ns_oracle.py) for a RAGGED BATCH of signals on the MI355X: the threshold comes from the recording itself, so no noise clip is needed.
// Same STFT as the stationary gate (spectral_gate.hip): N = 1024, hop 256, w = periodic Hann, W = sum w, F = ceil(L / 256) + 1 centred frames.
//     A = |X|;  S = the per-bin level of A over time, a one-pole smoother run forward and then backward (scipy's filtfilt([b], [1, b - 1], A, padtype=None)):
//         s[f] = b A[f] + (1 - b) s[f - 1], s[-1] := A[0];  S[f] = b s[f] + (1 - b) S[f + 1], S[F] := s[F - 1]
//     r = (A - S) / S (0 where S == 0),  m0 = 1 / (1 + exp(-(r - n_mult) slope)),  m = smooth(m0) p + (1 - p)  with outer(tri(n_f), tri(n_t)) / sum and
//     zeros outside the 513 x F mask,  y_f = irfft(X m) W,  out[n] = sum_f w y_f / sum_f w^2.
// Four launches per batch, no floating-point atomics, a sample depends on its own signal only:
//   magnitudes  every frame ONE WAVE with the FFT of fft1024.h -> A[g][k] f32, a (total frames, 513) workspace.
//   level       ONE LANE per (signal, bin); the lanes of a wave take consecutive bins, so the row of a frame is one coalesced load.  The lane walks its
//               signal's F frames forward (s kept as f32 in a second workspace) and backward.  The recurrences, S, r and the sigmoid are f64: with
//               b ~ 0.006 an f32 recurrence loses u / b ~ 170 ulp, and the 2 F-step chain of dependent FMAs is latency-bound either way.  The loads do
//               not depend on the chain: the rows of the next SGN_AHEAD frames are requested before the current SGN_AHEAD are consumed.  m0 is rounded
//               to f32 once and replaces A in place.
//   synthesis   the FFT AGAIN (as in the stationary gate: a stored spectrum would cost 16 B per sample more), the m0 rows of the frames f - n_t .. f + n_t
//               combined over time into the wave's LDS row, then over frequency, both as plain f32 sums in ASCENDING tap order (the values are real:
//               no integer trick, no running sums), / the weights' sum, p, Y = X m, the inverse FFT, the windowed frame into the frames workspace.
//               The time taps accumulate in registers straight from the (cache-resident) rows instead of staging all 17 rows in LDS: 17 x 2 KB per
//               wave would leave one workgroup per CU.
//   overlap-add sg_overlap_add_kernel of the stationary gate, unchanged.
#include "spectral_gate_common.h"
#include "silent_speech_hip.h"

namespace {
constexpr int SGN_AHEAD = 8;                                        // frames whose rows are in flight while the chain consumes the previous SGN_AHEAD

__global__ __launch_bounds__(SG_WAVES * 64, 2) void sgn_magnitude_kernel(const float* __restrict__ x, const long long* __restrict__ tab, int R, long long total,
                                                                      const float* __restrict__ window, float* __restrict__ mag)
{
    __shared__ cpx tile_s[SG_WAVES][MF_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_uniform(tid >> 6);
    cpx* tl = tile_s[wv];
    cpx win[8], tw1[8], tw2[8], tw3[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { const int n = lane + 64 * q; win[q] = cpx{window[2 * n], window[2 * n + 1]}; }
    fft512_twiddles(lane, tw1, tw2, tw3);
    const cpx tw_nyq = twiddle(MF_H, MF_N);
    long long g0, g1;
    sg_run(total, (long long)blockIdx.x * SG_WAVES + wv, (long long)gridDim.x * SG_WAVES, g0, g1);
    int u = -1, L = 0;
    long long fr0 = 0, fr1 = 0;
    const float* xu = x;
    for (long long g = g0; g < g1; ++g) {
        if (u < 0 || g >= fr1) {
            u = wave_uniform(sg_find(tab, R, g));
            fr0 = tab[u * 4 + 2]; fr1 = fr0 + tab[u * 4 + 3];
            xu = x + tab[u * 4]; L = wave_uniform((int)tab[u * 4 + 1]);
        }
        const int f = wave_uniform((int)(g - fr0));
        cpx v[8];
        sg_load_frame(xu, L, f, lane, win, v);
        fft512(v, tl, lane, tw1, tw2);
        float* row = mag + g * SG_BINS;
#pragma unroll
        for (int j = 0; j < 8; ++j) row[lane + 64 * j] = sg_mag(rfft_bin(tl, lane + 64 * j, tw3[j]));
        if (lane == 0) row[MF_H] = sg_mag(rfft_nyquist(tl, tw_nyq));
    }
}

// grid (9, R): workgroup (bx, u) = one wave = the bins 64 bx .. 64 bx + 63 of signal u.  am: A in, m0 out (in place); sw: s between the passes.
__global__ __launch_bounds__(64) void sgn_level_kernel(const long long* __restrict__ tab, float* __restrict__ am, float* __restrict__ sw, double b, double n_mult,
                                                       double slope, float* __restrict__ mask_out)
{
    const int u = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
    if (k >= SG_BINS) return;
    const long long fr0 = tab[u * 4 + 2];
    const int F = (int)tab[u * 4 + 3];
    float* a = am + fr0 * SG_BINS + k;
    float* s_row = sw + fr0 * SG_BINS + k;
    float* mo = mask_out ? mask_out + fr0 * SG_BINS + k : nullptr;
    const double c = 1.0 - b;
    // ---- forward: s[f] = b A[f] + (1 - b) s[f - 1], s[-1] := A[0]
    float nxt[SGN_AHEAD], cur[SGN_AHEAD];
#pragma unroll
    for (int i = 0; i < SGN_AHEAD; ++i) nxt[i] = i < F ? a[(long long)i * SG_BINS] : 0.f;
    double s = (double)nxt[0];
    for (int f0 = 0; f0 < F; f0 += SGN_AHEAD) {
#pragma unroll
        for (int i = 0; i < SGN_AHEAD; ++i) { cur[i] = nxt[i]; const int f = f0 + SGN_AHEAD + i; nxt[i] = f < F ? a[(long long)f * SG_BINS] : 0.f; }
#pragma unroll
        for (int i = 0; i < SGN_AHEAD; ++i) {
            const int f = f0 + i;
            if (f < F) { s = fma(c, s, b * (double)cur[i]); s_row[(long long)f * SG_BINS] = (float)s; }
        }
    }
    // ---- backward over j = F - 1 - f: S[f] = b s[f] + (1 - b) S[f + 1], S[F] := s[F - 1]; then r, the sigmoid, one rounding
    float nxs[SGN_AHEAD], cus[SGN_AHEAD];
#pragma unroll
    for (int i = 0; i < SGN_AHEAD; ++i) {
        const int f = F - 1 - i;
        nxt[i] = f >= 0 ? a[(long long)f * SG_BINS] : 0.f; nxs[i] = f >= 0 ? s_row[(long long)f * SG_BINS] : 0.f;
    }
    double S = s;
    for (int j0 = 0; j0 < F; j0 += SGN_AHEAD) {
#pragma unroll
        for (int i = 0; i < SGN_AHEAD; ++i) {
            cur[i] = nxt[i]; cus[i] = nxs[i];
            const int f = F - 1 - (j0 + SGN_AHEAD + i);
            nxt[i] = f >= 0 ? a[(long long)f * SG_BINS] : 0.f; nxs[i] = f >= 0 ? s_row[(long long)f * SG_BINS] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < SGN_AHEAD; ++i) {
            const int f = F - 1 - (j0 + i);
            if (f >= 0) {
                S = fma(c, S, b * (double)cus[i]);
                const double r = S > 0.0 ? ((double)cur[i] - S) / S : 0.0;
                const float m0 = (float)(1.0 / (1.0 + exp(-(r - n_mult) * slope)));
                a[(long long)f * SG_BINS] = m0;
                if (mo) mo[(long long)f * SG_BINS] = m0;
            }
        }
    }
}

// window3 = [w / W | w W / 512 | w^2], 1024 floats each; pf = p, qf = 1 - p rounded to f32 on the host
__global__ __launch_bounds__(SG_WAVES * 64, 2) void sgn_synthesis_kernel(const float* __restrict__ x, const long long* __restrict__ tab, int R, long long total,
                                                                      const float* __restrict__ window3, const float* __restrict__ m0, int n_f, int n_t,
                                                                      float pf, float qf, float* __restrict__ frames)
{
    __shared__ cpx tile_s[SG_WAVES][MF_TILE];
    __shared__ cpx spec_s[SG_WAVES][SG_BINS + 7];
    __shared__ float row_s[SG_WAVES][SG_CBUF];
    __shared__ float mask_s[SG_WAVES][64 * SG_PER];
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_uniform(tid >> 6);
    cpx* tl = tile_s[wv]; cpx* sp = spec_s[wv]; float* cb = row_s[wv]; float* mk = mask_s[wv];
    for (int i = lane; i < SG_CBUF; i += 64) cb[i] = 0.f;            // the margins stay zero: only [SG_PAD, SG_PAD + 513) is written per frame
    cpx win[8], tw1[8], tw2[8], tw3[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { const int n = lane + 64 * q; win[q] = cpx{window3[2 * n], window3[2 * n + 1]}; }
    fft512_twiddles(lane, tw1, tw2, tw3);
    const cpx tw_nyq = twiddle(MF_H, MF_N);
    const float norm = (float)((n_f + 1) * (n_f + 1) * (n_t + 1) * (n_t + 1));       // sum of the integer weights: <= 33^2 9^2, exact

    long long g0, g1;
    sg_run(total, (long long)blockIdx.x * SG_WAVES + wv, (long long)gridDim.x * SG_WAVES, g0, g1);
    int u = -1, F = 0, L = 0;
    long long fr0 = 0, fr1 = 0;
    const float* xu = x;
    for (long long g = g0; g < g1; ++g) {
        if (u < 0 || g >= fr1) {
            u = wave_uniform(sg_find(tab, R, g));
            fr0 = tab[u * 4 + 2]; F = wave_uniform((int)tab[u * 4 + 3]); fr1 = fr0 + F;
            xu = x + tab[u * 4]; L = wave_uniform((int)tab[u * 4 + 1]);
        }
        const int f = wave_uniform((int)(g - fr0));
        // ---- the spectrum again
        cpx v[8];
        sg_load_frame(xu, L, f, lane, win, v);
        fft512(v, tl, lane, tw1, tw2);                                // (its fences order the row / mask buffers too)
#pragma unroll
        for (int j = 0; j < 8; ++j) sp[lane + 64 * j] = rfft_bin(tl, lane + 64 * j, tw3[j]);
        if (lane == 0) { sp[0][1] = 0.f; sp[MF_H] = cpx{rfft_nyquist(tl, tw_nyq)[0], 0.f}; }      // bins 0 and 512 of a real signal are real
        // ---- time taps, ascending dt: T[k] = sum_dt (n_t + 1 - |dt|) m0[k, f + dt] over the frames that exist (zeros outside the mask)
        {
            float T[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) T[j] = 0.f;
            for (int dt = -n_t; dt <= n_t; ++dt) {
                if (f + dt < 0 || f + dt >= F) continue;
                const float wt = (float)(n_t + 1 - (dt < 0 ? -dt : dt));
                const float* row = m0 + (g + dt) * SG_BINS;
#pragma unroll
                for (int j = 0; j < 8; ++j) T[j] = fmaf(wt, row[lane + 64 * j], T[j]);
                if (lane == 0) T[8] = fmaf(wt, row[MF_H], T[8]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) cb[SG_PAD + lane + 64 * j] = T[j];
            if (lane == 0) cb[SG_PAD + MF_H] = T[8];
        }
        wave_lds_sync();
        // ---- frequency taps, ascending dk, over SG_PER consecutive bins per lane: M[k] = sum_dk (n_f + 1 - |dk|) T[k + dk]; m = M / norm p + (1 - p)
        {
            const float* c = cb + SG_PAD + SG_PER * lane;
            float M[SG_PER];
#pragma unroll
            for (int i = 0; i < SG_PER; ++i) M[i] = 0.f;
            for (int dk = -n_f; dk <= n_f; ++dk) {
                const float wf = (float)(n_f + 1 - (dk < 0 ? -dk : dk));
#pragma unroll
                for (int i = 0; i < SG_PER; ++i) M[i] = fmaf(wf, c[i + dk], M[i]);
            }
#pragma unroll
            for (int i = 0; i < SG_PER; ++i) mk[SG_PER * lane + i] = fmaf(M[i] / norm, pf, qf);     // (bins behind 512: never read)
        }
        wave_lds_sync();
        // ---- Y = X m
#pragma unroll
        for (int j = 0; j < 8; ++j) sp[lane + 64 * j] *= mk[lane + 64 * j];
        if (lane == 0) sp[MF_H] *= mk[MF_H];
        wave_lds_sync();
        // ---- inverse: v[j] = conj Z[k], Z[k] = E + i O, k = lane + 64 j
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = lane + 64 * j;
            const cpx a = sp[k], c0 = sp[MF_H - k], c = cpx{c0[0], -c0[1]};
            const cpx e = 0.5f * (a + c), o = cmul(0.5f * (a - c), cpx{tw3[j][0], -tw3[j][1]});
            v[j] = cpx{e[0] - o[1], -(e[1] + o[0])};
        }
        fft512(v, tl, lane, tw1, tw2);
        float* out = frames + g * MF_N;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int n = lane + 64 * q;
            const cpx r = tl[zpos(n)];                                // the inverse comes out conjugated: z[n] = conj(R[n]) / 512
            out[2 * n] = r[0] * window3[MF_N + 2 * n]; out[2 * n + 1] = -r[1] * window3[MF_N + 2 * n + 1];
        }
    }
}
}  // namespace

extern "C" int ss_spectral_gate_ns_batch(const float* x, float* y, const int64_t* table_dev, int R, int64_t total_frames, const float* window_dev, double b,
                                         double n_mult, double slope, int n_f, int n_t, double prop_decrease, float* mag_workspace, float* level_workspace,
                                         float* frames_workspace, float* mask_out, void* stream)
{
    SS_CHECK(x && y && table_dev && window_dev && mag_workspace && level_workspace && frames_workspace, "ss_spectral_gate_ns_batch: null pointer");
    SS_CHECK(R >= 1 && R <= 65535 && total_frames >= 2 * (int64_t)R,
             "ss_spectral_gate_ns_batch: bad sizes (1 to 65535 signals, every signal has L >= 1 samples, i.e. at least 2 frames)");
    SS_CHECK(b > 0.0 && b <= 1.0, "ss_spectral_gate_ns_batch: the smoothing coefficient b must lie in (0, 1]");
    SS_CHECK(slope > 0.0 && n_mult == n_mult, "ss_spectral_gate_ns_batch: the sigmoid's slope must be positive");
    SS_CHECK(n_f >= 0 && n_f <= SG_MAX_NF && n_t >= 0 && n_t <= SG_MAX_NT, "ss_spectral_gate_ns_batch: mask smoothing of %d bins x %d frames exceeds the kernel's bounds (%d x %d)",
             n_f, n_t, SG_MAX_NF, SG_MAX_NT);
    SS_CHECK(prop_decrease >= 0.0 && prop_decrease <= 1.0, "ss_spectral_gate_ns_batch: prop_decrease must lie in [0, 1]");
    const int grid = sg_grid(total_frames);
    SS_LAUNCH(sgn_magnitude_kernel, dim3(grid), dim3(SG_WAVES * 64), 0, stream, x, (const long long*)table_dev, R, (long long)total_frames, window_dev, mag_workspace);
    SS_LAUNCH(sgn_level_kernel, dim3((SG_BINS + 63) / 64, R), dim3(64), 0, stream, (const long long*)table_dev, mag_workspace, level_workspace, b, n_mult, slope, mask_out);
    SS_LAUNCH(sgn_synthesis_kernel, dim3(grid), dim3(SG_WAVES * 64), 0, stream, x, (const long long*)table_dev, R, (long long)total_frames, window_dev,
              (const float*)mag_workspace, n_f, n_t, (float)prop_decrease, (float)(1.0 - prop_decrease), frames_workspace);
    SS_LAUNCH(sg_overlap_add_kernel, dim3((unsigned)(total_frames - R)), dim3(SG_HOP), 0, stream, (const float*)frames_workspace, (const long long*)table_dev, R,
              window_dev + 2 * MF_N, y);
    SS_LAUNCH_CHECK("ss_spectral_gate_ns_batch");
    return 0;
}
