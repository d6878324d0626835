// audio.hip -- the stored-audio half of the reference's load_audio (data_utils.py:64-83) on the MI355X: band-limited resampling of a ragged
// batch (16 000 -> 22 050 Hz for the corpus, 22 050 -> 16 000 Hz for ASR evaluation, any small rational ratio) and the two numbers
// normalize_volume (data_utils.py:19-27) needs, both per BATCH in one launch each.
//
// The resampler is scipy.signal.resample_poly(x, up, down) with its defaults, in closed form:
//     half = 10 max(up, down),  h = firwin(2 half + 1, 1 / max(up, down), window = ('kaiser', 5.0)) * up,  n_out = ceil(n up / down)
//     y[m] = sum_j x[j] h[m down + half - j up]        over 0 <= j < n, 0 <= m down + half - j up <= 2 half        (zeros outside the signal)
// Output m has phase ph = (m down + half) mod up and newest input jm = (m down + half) div up; its taps are h[ph + i up], i = 0, 1, .., against
// x[jm - i].  The host lays h out phase-major, [up][tpp] with tpp = the taps of the longest phase rounded up to a multiple of 4 (zero filled), in
// f32 (data_utils._resample_table), so that an output is ONE row of the table against a run of the staged input, four taps per 16-byte read.
// Accumulation is f32, one fma per tap, i ascending: an output depends on its own utterance's samples only -- not on the tile it falls into,
// not on what else is in the batch.
//
// A workgroup is persistent: it stages the table once (LDS variant), then walks tiles of AR_TILE consecutive outputs of ONE utterance, grid-stride
// over all tiles of the batch.  Lane l of a tile pass takes output l, l + AR_THREADS, ..: neighbouring lanes read neighbouring staged samples
// (down / up apart: no LDS bank conflict, equal addresses broadcast) and store neighbouring outputs.  Their table rows lie a phase step apart, so
// the LDS copy of the table uses a row stride of an ODD number of 16-byte units (tpp, or tpp + 4): the 16-byte reads of neighbouring lanes then fall
// into different bank groups instead of every second one.
#include "common.h"
#include "silent_speech_hip.h"
#include <math.h>

namespace {
constexpr int AR_THREADS = 512;
constexpr int AR_PER = 4;              // outputs per thread and tile: four independent fma chains
constexpr int AR_TILE = AR_PER * AR_THREADS;   // outputs per tile
constexpr int AR_SPAN = 8192;          // bound of the staged input samples per tile, (AR_TILE - 1) down / up + 1 + tpp
constexpr int AR_TAB_MAX = 12288;      // bound of the phase-major table, floats (48 KB)
constexpr int AR_LDS_MAX = 65536;      // span + tile counts + LDS copy of the table of one ratio must fit the LDS a workgroup gets without asking: bytes
constexpr int AR_RCACHE = 512;         // tile counts of the first utterances kept in LDS: the walk that finds a workgroup's tiles does not wait for memory

// staged samples of a tile for this ratio, rounded up so that the table behind them stays 16-byte aligned
static inline int ar_span_floats(int up, int down, int tpp) { return (int)(((long long)(AR_TILE - 1) * down / up + 1 + tpp + 3) / 4 * 4); }
// row stride of the LDS copy of the table: an odd number of 16-byte units
__host__ __device__ static inline int ar_lds_stride(int tpp) { return (tpp / 4) % 2 ? tpp : tpp + 4; }

__device__ __forceinline__ float ar_finish(float v, float g, bool scale, bool clip) {
    if (scale) v *= g;
    if (clip) v = v < -1.f ? -1.f : (v > 1.f ? 1.f : v);            // np.clip; NaN stays NaN
    return v;
}

// tab4[u] = {first input sample, n, first output sample, n_out}
template <bool TAB_LDS>
__global__ void __launch_bounds__(AR_THREADS) audio_resample_ragged_kernel(const float* __restrict__ x, float* __restrict__ y, const long long* __restrict__ tab4, int R,
                                                                           int up, int down, int half, int tpp, int span_floats,
                                                                           const float* __restrict__ coef, const float* __restrict__ gains, int clip)
{
    SS_DYN_SMEM(smem_raw);
    float* sx = (float*)smem_raw;              // span_floats: sample j_lo + i of the tile's utterance, zero outside [0, n)
    int* s_nt = (int*)(sx + span_floats);      // AR_RCACHE: tiles of utterance u
    float* stab = (float*)(s_nt + AR_RCACHE);  // TAB_LDS: the table, rows ar_lds_stride(tpp) apart
    const int t = threadIdx.x;
    const int ts = TAB_LDS ? ar_lds_stride(tpp) : tpp;
    auto tiles_of = [&](int u) -> long long { const long long n_out = tab4[u * 4 + 3]; return n_out <= 0 ? 0 : (n_out + AR_TILE - 1) / AR_TILE; };
    for (int u = t; u < R && u < AR_RCACHE; u += AR_THREADS) s_nt[u] = (int)tiles_of(u);
    if (TAB_LDS) {
        const unsigned n4 = (unsigned)(up * tpp) / 4u, q4 = (unsigned)tpp / 4u;      // 16-byte units of the table, of a row
        for (unsigned i0 = t; i0 < n4; i0 += AR_THREADS * 4) {                        // four 16-byte loads in flight per thread
            f32x4 r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { const unsigned i = i0 + k * AR_THREADS; if (i < n4) r[k] = *(const f32x4*)(coef + 4 * (size_t)i); }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned i = i0 + k * AR_THREADS, row = i / q4;
                if (i < n4) *(f32x4*)(stab + (size_t)row * ts + 4 * (i - row * q4)) = r[k];
            }
        }
    }
    __syncthreads();
    const float* ctab = TAB_LDS ? stab : coef;
    // AR_THREADS outputs further: AR_THREADS down = step_j up + step_ph
    const unsigned step_j = (unsigned)(AR_THREADS * down) / (unsigned)up, step_ph = (unsigned)(AR_THREADS * down) - step_j * (unsigned)up;
    long long tile_base = 0, next = blockIdx.x;
    for (int u = 0; u < R; ++u) {
        const long long nt = u < AR_RCACHE ? (long long)s_nt[u] : tiles_of(u);
        if (next < tile_base + nt) {
            const long long n = tab4[u * 4 + 1], n_out = tab4[u * 4 + 3];
            float* yu = y + tab4[u * 4 + 2];
            const float* xu = x + tab4[u * 4];
            const float g = gains ? gains[u] : 1.f;
            for (; next < tile_base + nt; next += gridDim.x) {
                const long long m_lo = (next - tile_base) * AR_TILE, m_hi = m_lo + AR_TILE < n_out ? m_lo + AR_TILE : n_out;
                const long long p_lo = m_lo * down + half, jq = p_lo / up;
                const unsigned r0 = (unsigned)(p_lo - jq * up);
                const long long j_lo = jq - (tpp - 1);
                const int count = (int)(m_hi - m_lo);
                const int span = (int)(((unsigned)(count - 1) * (unsigned)down + r0) / (unsigned)up) + tpp;
                __syncthreads();                                            // the previous tile has been read
                for (int i0 = t; i0 < span; i0 += AR_THREADS * 4) {          // four loads in flight per thread
                    float ld[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) { const int i = i0 + k * AR_THREADS; const long long j = j_lo + i; ld[k] = (i < span && j >= 0 && j < n) ? xu[j] : 0.f; }
#pragma unroll
                    for (int k = 0; k < 4; ++k) { const int i = i0 + k * AR_THREADS; if (i < span) sx[i] = ld[k]; }
                }
                __syncthreads();
                if (t < count) {
                    const unsigned pl = (unsigned)t * (unsigned)down + r0;
                    unsigned dj = pl / (unsigned)up, ph = pl - dj * (unsigned)up;
                    // the thread's outputs advance together, tap group by tap group: independent fma chains with their LDS reads in flight at once (each
                    // chain still takes its taps in ascending order).  An output that does not exist reads row 0 / sample 0 and is not stored.
                    const float* c[AR_PER];
                    const float* xs[AR_PER];
                    float v[AR_PER];
#pragma unroll
                    for (int r = 0; r < AR_PER; ++r) {
                        const bool ok = t + r * AR_THREADS < count;
                        if (r) { dj += step_j; ph += step_ph; if (ph >= (unsigned)up) { ph -= (unsigned)up; ++dj; } }
                        c[r] = ctab + (size_t)(ok ? ph : 0u) * ts;
                        xs[r] = sx + (ok ? dj : 0u) + (tpp - 1);            // sample jq + dj; tap i meets the sample i places earlier
                        v[r] = 0.f;
                    }
                    for (int i = 0; i < tpp; i += 4) {
                        f32x4 w[AR_PER];
                        float xv[AR_PER][4];
#pragma unroll
                        for (int r = 0; r < AR_PER; ++r) {
                            w[r] = *(const f32x4*)(c[r] + i);
#pragma unroll
                            for (int k = 0; k < 4; ++k) xv[r][k] = xs[r][-i - k];
                        }
#pragma unroll
                        for (int r = 0; r < AR_PER; ++r) {
#pragma unroll
                            for (int k = 0; k < 4; ++k) v[r] = fmaf(w[r][k], xv[r][k], v[r]);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < AR_PER; ++r)
                        if (t + r * AR_THREADS < count) yu[m_lo + t + r * AR_THREADS] = ar_finish(v[r], g, gains != nullptr, clip != 0);
                }
            }
        }
        tile_base += nt;
    }
}

// ---- normalize_volume: librosa.feature.rms(y = audio) with its defaults (frame_length 2048, hop_length 512, center = True with ZERO padding --
// librosa >= 0.10 --, 1 + n // 512 frames) and max |x|.  Frame f covers the 512-sample blocks f - 2 .. f + 1, so the sums of squares of the blocks are
// formed once (one wave per block) and four of them make a frame.
constexpr int AL_BLOCK = 512, AL_FRAME = 2048;

// tab3[u] = {first input sample, n, first block = sum over earlier utterances of ceil(n / 512)}; ws = [block sum of squares | block max |x|]
__global__ void __launch_bounds__(256) audio_level_ragged_kernel(const float* __restrict__ x, const long long* __restrict__ tab3, int R, long long total_blocks,
                                                                 float* __restrict__ ws)
{
    const int lane = threadIdx.x & 63;
    const long long gb = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gb >= total_blocks) return;                                       // whole waves; the kernel has no workgroup barrier
    int lo = 0, hi = R - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tab3[mid * 3 + 2] <= gb) lo = mid; else hi = mid - 1; }
    const long long b = gb - tab3[lo * 3 + 2], rem = tab3[lo * 3 + 1] - b * AL_BLOCK;
    const float* xb = x + tab3[lo * 3] + b * AL_BLOCK;
    float ld[AL_BLOCK / 64];
#pragma unroll
    for (int k = 0; k < AL_BLOCK / 64; ++k) { const int i = k * 64 + lane; ld[k] = i < rem ? xb[i] : 0.f; }
    float s = 0.f, mx = 0.f;
#pragma unroll
    for (int k = 0; k < AL_BLOCK / 64; ++k) { s = fmaf(ld[k], ld[k], s); mx = fmaxf(mx, fabsf(ld[k])); }
    s = wave_sum(s); mx = wave_max(mx);
    if (lane == 0) { ws[gb] = s; ws[total_blocks + gb] = mx; }
}

// one wave per utterance: level[u] = {max frame RMS, max |x|}, gains[u] = 0.2 / (max_rms + 0.01), or 1 / max |x| where that gain would leave the peak above 1
__global__ void __launch_bounds__(64) audio_level_finalize_kernel(const long long* __restrict__ tab3, long long total_blocks, const float* __restrict__ ws,
                                                                  float* __restrict__ level, float* __restrict__ gains)
{
    const int u = blockIdx.x, lane = threadIdx.x;
    const long long n = tab3[u * 3 + 1], nb = (n + AL_BLOCK - 1) / AL_BLOCK, nf = n / AL_BLOCK + 1;
    const float* S = ws + tab3[u * 3 + 2];
    const float* M = S + total_blocks;
    float best = 0.f, mx = 0.f;
    for (long long f = lane; f < nf; f += 64) {
        float s = 0.f;
#pragma unroll
        for (int d = -2; d <= 1; ++d) { const long long b = f + d; s += (b >= 0 && b < nb) ? S[b] : 0.f; }
        best = fmaxf(best, s);
    }
    for (long long b = lane; b < nb; b += 64) mx = fmaxf(mx, M[b]);
    best = wave_max(best); mx = wave_max(mx);
    if (lane == 0) {
        const float rms = sqrtf(best / (float)AL_FRAME);
        if (level) { level[u * 2] = rms; level[u * 2 + 1] = mx; }
        if (gains) {
            float g = 0.2f / (rms + 0.01f);
            if (g * mx > 1.f) g = 1.f / mx;
            gains[u] = g;
        }
    }
}
}  // namespace

extern "C" int ss_audio_resample_limits(int* tile, int* span, int* table_floats)
{
    if (tile) *tile = AR_TILE;
    if (span) *span = AR_SPAN;
    if (table_floats) *table_floats = AR_TAB_MAX;
    return 0;
}

extern "C" int ss_audio_resample_supported(int up, int down, int half, int taps_per_phase)
{
    if (up < 1 || down < 1 || half < 0 || taps_per_phase < 4 || taps_per_phase % 4) return 0;
    if ((long long)up * taps_per_phase > AR_TAB_MAX) return 0;
    if ((long long)(2 * (long long)half / up + 1) > taps_per_phase) return 0;                       // the longest phase (phase 0) has 2 half / up + 1 taps
    if ((long long)(AR_TILE - 1) * down / up + 1 + taps_per_phase > AR_SPAN) return 0;
    if ((long long)(ar_span_floats(up, down, taps_per_phase) + AR_RCACHE + up * ar_lds_stride(taps_per_phase)) * (long long)sizeof(float) > AR_LDS_MAX) return 0;
    return 1;
}

extern "C" int ss_audio_resample_batch(const float* x, float* y, const int64_t* table_dev, int R, int up, int down, int half, int taps_per_phase,
                                       const float* coef_dev, const float* gains_dev, int flags, int64_t total_out, void* stream)
{
    SS_CHECK(x && y && table_dev && coef_dev, "ss_audio_resample_batch: null pointer");
    SS_CHECK(R >= 1 && total_out >= 0 && up >= 1 && down >= 1, "ss_audio_resample_batch: bad sizes");
    SS_CHECK(ss_audio_resample_supported(up, down, half, taps_per_phase),
             "ss_audio_resample_batch: ratio %d/%d (half length %d, %d taps per phase) is not supported: the phase table is limited to %d floats, a tile's "
             "input span to %d samples and both together to %d bytes", up, down, half, taps_per_phase, AR_TAB_MAX, AR_SPAN, AR_LDS_MAX);
    SS_CHECK(((uintptr_t)coef_dev & 15) == 0, "ss_audio_resample_batch: the coefficient table must be 16-byte aligned");
    if (total_out == 0) return 0;
    const bool in_l2 = (flags & 2) != 0;
    const int span_floats = ar_span_floats(up, down, taps_per_phase);
    const size_t smem = (size_t)(span_floats + AR_RCACHE + (in_l2 ? 0 : up * ar_lds_stride(taps_per_phase))) * sizeof(float);
    // persistent workgroups: as many as stay resident (160 KB of LDS and 32 waves per compute unit), never more than there are tiles
    long long per_cu = (160 * 1024) / (long long)(smem + 512);
    if (per_cu > 2048 / AR_THREADS) per_cu = 2048 / AR_THREADS;
    const long long tiles = total_out / AR_TILE + R;                       // upper bound: every utterance adds at most one short tile
    const long long resident = (long long)ss_cu_count(2) * per_cu;
    const int grid = (int)(tiles < resident ? tiles : resident);
    if (in_l2)
        SS_LAUNCH(SS_KERNEL(audio_resample_ragged_kernel<false>), dim3(grid), dim3(AR_THREADS), smem, stream, x, y, (const long long*)table_dev, R, up, down, half,
                  taps_per_phase, span_floats, coef_dev, gains_dev, flags & 1);
    else
        SS_LAUNCH(SS_KERNEL(audio_resample_ragged_kernel<true>), dim3(grid), dim3(AR_THREADS), smem, stream, x, y, (const long long*)table_dev, R, up, down, half,
                  taps_per_phase, span_floats, coef_dev, gains_dev, flags & 1);
    SS_LAUNCH_CHECK("ss_audio_resample_batch");
    return 0;
}

extern "C" int ss_audio_level_batch(const float* x, const int64_t* table_dev, int R, int64_t total_blocks, float* workspace, int64_t workspace_floats,
                                    float* level, float* gains, void* stream)
{
    SS_CHECK(x && table_dev && workspace && (level || gains), "ss_audio_level_batch: null pointer");
    SS_CHECK(R >= 1 && total_blocks >= 0, "ss_audio_level_batch: bad sizes");
    SS_CHECK(workspace_floats >= 2 * total_blocks, "ss_audio_level_batch: workspace too small (%lld floats needed)", (long long)(2 * total_blocks));
    if (total_blocks > 0)
        SS_LAUNCH(audio_level_ragged_kernel, dim3((unsigned)((total_blocks + 3) / 4)), dim3(256), 0, stream, x, (const long long*)table_dev, R, (long long)total_blocks, workspace);
    SS_LAUNCH(audio_level_finalize_kernel, dim3(R), dim3(64), 0, stream, (const long long*)table_dev, (long long)total_blocks, (const float*)workspace, level, gains);
    SS_LAUNCH_CHECK("ss_audio_level_batch");
    return 0;
}
