// klatt_pitch.h -- the pitch period and a periodicity measure ESTIMATED FROM THE SIGNAL, per step of the spectrogram's grid, of a batch's PCM or
// of a signal's rows: the YIN difference function, its cumulative mean normalised form (CMND), the first dip below a threshold, a parabolic
// refinement (speechPlayer_batch_exportPitch / exportPitchOf, speechPlayer_pcmPitch / signalPitch).
//
// The definition is in include/speechPlayer_batch.h; this header is its one statement in code.  The functions marked KLATT_PITCH_HD are
// compiled for the host (plain C++17, no HIP) and for the device from the same source with -ffp-contract=off: the host entry points run them
// in plain loops, the kernel calls the same bodies, and nothing here changes arithmetic between the two sides.  tests/native/check_pitch.cpp
// models the kernel's walk on the host against brute force under the sanitizers.
//
//   The frame       N = W + lagMax samples, x[i] = sample c - N / 2 + i by the reader (klatt_tiles.h: tile_sample -- +0 outside the row,
//                   nothing loaded there).
//   d(tau)          u = x[i] - x[i + tau], one binary32 subtraction; (double)u * (double)u is EXACT in binary64 (24 x 24 bits), so
//                   pitch_term's fma adds it with one rounding whichever way it is written.  Chain i mod 4 sums its terms in ascending i
//                   over 0 <= i < W from +0.0; d = (c0 + c1) + (c2 + c3) (pitch_fold).  pitch_diff is that in a plain loop.
//   Lemma           A chain that starts from +0.0 is never -0.0 (klatt_lpc.h), so terms with u == 0 may be skipped or added alike, and
//                   adding a d of +0.0 to the running sum s changes no bit: the kernel's scan adds +0.0 for the lanes past lagMax.
//   m(tau)          s(tau) = s(tau - 1) + d(tau) in ascending tau, one rounding each (no parallel prefix: its order is not the
//                   definition's); pitch_cmnd: s > 0 ? (d * tau) / s : 1.0, one product and one division.
//   The choice      pitch_dip: m(tau) < threshold and (tau == lagMax or !(m(tau + 1) < m(tau))); the lowest such tau is voiced.  Otherwise
//                   the least m, ties to the lowest tau (pitch_better).  Both are minima under a total order (no m is a NaN inside the
//                   signal bound), so a lane may take any subset of the lags and the lanes be reduced in any order: only the choice
//                   crosses lanes, as in tempo_better.
//   Refinement      pitch_refine: the parabola through m(tau* - 1 .. tau* + 1), +0.0 at the range's edge (tau* - 1 < 1 or tau* + 1 >
//                   lagMax), for den <= 0 and for |delta| > 0.5.
//
//   klatt_pitch<F32, In>   pitch_rows<F32>, the one body it shares with klatt_stage_pitch (klatt_stage_frames.h), handed the row's own steps,
//                   the frame's first sample phase + j hop - N / 2 and the reader tile_sample.  A 256-lane workgroup takes kPitchGroup = 16 consecutive steps of the OUTPUT (located by dense_locate: a group
//                   may end one row and begin the next), each wavefront four of them, one at a time, in its own LDS region and at its own
//                   pace (lpc_wave_sync: there is no workgroup barrier in the kernel).  Per step:
//                     1  the frame into LDS by masked coalesced loads, zeros from N to the region's end;
//                     2  pitch_lane_pass<R>: in a pass of 64 R lags lane l keeps the R consecutive lags p0 + R l + 1 .. + R and their 4 R
//                        chains in registers; R is 6 where that takes fewer lag-passes (lagMax 257 .. 384: one pass against two), else 4
//                        (pitch_lane_lags).  Per four samples i it reads x[i .. i+3] (one 16-byte LDS load, the same address in every
//                        lane: a broadcast) and the next four words of its own sliding window x[i + p0 + R l ..] (consecutive lanes read
//                        consecutive pieces: no bank conflict; one 16-byte load with R 4, two 8-byte loads with R 6): they serve 4 R
//                        pairs, against as many one-word reads for a lane-per-lag loop.  Every d(tau) is one lane's, in the definition's
//                        order;
//                     3  the scan: 64 lags at a time, lane l holds d(base + l); s runs through the lanes in ascending order by
//                        v_readlane (every lane computes the same s; lane k keeps the k-th); each lane then forms its m and puts it where
//                        d was;
//                     4  pitch_lane_choice over the lags lagMin + lane, + 64, ..., the choice reduced by a butterfly of pitch_better; the
//                        refinement and the scalar fields by lane 0, the CMND curve by all lanes into the wavefront's staged values;
//                     5  the step's nCols values leave through the row writer (tile_store_lane), a lane per aligned 16 bytes: with the CMND
//                        field a group's output could not be staged at once.
//                   LDS per workgroup (pitch_lds_bytes): 4 * (4 * pitch_frame_words(W, lagMax) + 8 * pitch_curve_words(lagMax) +
//                   nCols * sizeof(out element) rounded up to 16) -- 115 072 B at W 2048, lags 2 .. 1024, float64, every field; 34 368 B
//                   at W 1024, lags 44 .. 368, float32, f0 + aperiodicity (four workgroups a compute unit).  167 VGPRs (float32 out)
//                   and 171 (float64), no scratch: three and two wavefronts a SIMD (docs/KERNELS.md 4.25).
// Out of scope: normalised cross-correlation and energies; smoothing or tracking across steps (the CMND field serves a tracker of the
// caller's own); octave-error correction; FFT or MFMA evaluation of the difference (their summation order is not the definition's);
// decimation inside the export (the chain is exportResampled to 16 kHz, then the signal form); live handles (their pulls go through the
// pitch stage of klatt_stage_frames.h); NodePlayer beyond speechPlayer_node_part.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "klatt_tiles.h"
#include "klatt_spectrum.h"
#include "klatt_lpc.h"      // lpc_wave_sync

#if defined(__HIPCC__)
#define KLATT_PITCH_HD __host__ __device__ __forceinline__
#define KLATT_PITCH_UNROLL _Pragma("unroll")      // (a hint to hipcc alone: the loops' arithmetic is the same rolled or unrolled)
#define KLATT_PITCH_UNROLL_Q _Pragma("unroll Q")
#else
#define KLATT_PITCH_HD inline
#define KLATT_PITCH_UNROLL
#define KLATT_PITCH_UNROLL_Q
#endif

namespace klatt {

constexpr int kPitchMinWin = 32, kPitchMaxWin = 2048, kPitchMaxLag = 1024;
constexpr int kPitchChains = 4;           // chains of a lag: i mod 4
constexpr int kPitchGroup = 16;           // consecutive steps of the output a workgroup of klatt_pitch takes at a time: four per wavefront
// `what`: the fields come in this order whatever the order of the bits
constexpr int kPitchF0 = 1, kPitchPeriod = 2, kPitchLag = 4, kPitchAperiodicity = 8, kPitchVoiced = 16, kPitchCmnd = 32, kPitchAllFields = 63;

// The values of a step
KLATT_PITCH_HD int pitch_columns(int what, int lagMin, int lagMax)
{
    return ((what & kPitchF0) ? 1 : 0) + ((what & kPitchPeriod) ? 1 : 0) + ((what & kPitchLag) ? 1 : 0) + ((what & kPitchAperiodicity) ? 1 : 0) +
           ((what & kPitchVoiced) ? 1 : 0) + ((what & kPitchCmnd) ? lagMax - lagMin + 1 : 0);
}

// acc + (double)u * (double)u with u = a - b in binary32: the product is exact, the sum rounded once
KLATT_PITCH_HD double pitch_term(float a, float b, double acc) { const double u = (double)(a - b); return fma(u, u, acc); }
// d of the four chains
KLATT_PITCH_HD double pitch_fold(const double* c) { return (c[0] + c[1]) + (c[2] + c[3]); }

// d(tau) of the frame x[0 .. W + lagMax): the definition in a plain loop
KLATT_PITCH_HD double pitch_diff(const float* x, int W, int tau)
{
    double c[kPitchChains] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < W; ++i) c[i & 3] = pitch_term(x[i], x[i + tau], c[i & 3]);
    return pitch_fold(c);
}

// m(tau) from d(tau) and s(tau)
KLATT_PITCH_HD double pitch_cmnd(double d, int tau, double s) { return s > 0.0 ? (d * (double)tau) / s : 1.0; }

// tau is a dip below the threshold: m[] is indexed by the lag, m[tau + 1] is read only where tau < lagMax
KLATT_PITCH_HD bool pitch_dip(const double* m, int tau, int lagMax, double threshold)
{
    return m[tau] < threshold && (tau == lagMax || !(m[tau + 1] < m[tau]));
}

// (ma, ta) comes before (mb, tb) among the unvoiced candidates: the less m, ties to the lower lag; lag 0 stands for "none"
KLATT_PITCH_HD bool pitch_better(double ma, int ta, double mb, int tb) { return ta != 0 && (tb == 0 || ma < mb || (ma == mb && ta < tb)); }

// What lane `lane` of `lanes` finds among the lags lagMin + lane, + lanes, ...: its lowest dip (0: none) and its best unvoiced candidate
KLATT_PITCH_HD void pitch_lane_choice(const double* m, int lagMin, int lagMax, double threshold, int lane, int lanes, int& dip, double& bestM, int& bestTau)
{
    dip = 0; bestM = 0.0; bestTau = 0;
    for (int tau = lagMin + lane; tau <= lagMax; tau += lanes) {
        if (dip == 0 && pitch_dip(m, tau, lagMax, threshold)) dip = tau;
        if (pitch_better(m[tau], tau, bestM, bestTau)) { bestM = m[tau]; bestTau = tau; }
    }
}

// delta of the parabola through m(tau - 1), m(tau), m(tau + 1); +0.0 at the edge of 1 .. lagMax, for den <= 0 and for |delta| > 0.5
KLATT_PITCH_HD double pitch_refine(const double* m, int tau, int lagMax)
{
    if (tau - 1 < 1 || tau + 1 > lagMax) return 0.0;
    const double y0 = m[tau - 1], y1 = m[tau], y2 = m[tau + 1];
    const double den = (y0 - y1) + (y2 - y1);
    if (!(den > 0.0)) return 0.0;
    const double delta = (0.5 * (y0 - y2)) / den;
    return fabs(delta) <= 0.5 ? delta : 0.0;
}

// A step's scalar fields to o[0 ..), in the fixed order, each rounded to T once; returns the column the CMND curve starts at
template <typename T> KLATT_PITCH_HD int pitch_put_fields(T* o, int what, int sampleRate, const double* m, int tau, bool voiced, int lagMax)
{
    const double period = (double)tau + pitch_refine(m, tau, lagMax);
    int col = 0;
    if (what & kPitchF0) o[col++] = (T)(voiced ? (double)sampleRate / period : 0.0);
    if (what & kPitchPeriod) o[col++] = (T)period;
    if (what & kPitchLag) o[col++] = (T)(double)tau;
    if (what & kPitchAperiodicity) o[col++] = (T)m[tau];
    if (what & kPitchVoiced) o[col++] = (T)(voiced ? 1.0 : 0.0);
    return col;
}

// ---- the kernel's tiling of d(tau), compiled for the host too (check_pitch.cpp) ------------------------------------------------------------
// A lane keeps R = 4 or 6 consecutive lags; a pass of a wavefront covers 64 R.  What a step costs goes with passes x R: 6 where that is
// less (lagMax 257 .. 384, the 60 Hz floor at 16 and 22.05 kHz: one pass of 6 against two of 4), else 4.
KLATT_PITCH_HD int pitch_lane_lags(int lagMax) { return (lagMax + 383) / 384 * 6 < (lagMax + 255) / 256 * 4 ? 6 : 4; }
// The aligned 4-word pieces of a lane's sliding window: the words 1 .. R + 3 past its base are used
constexpr int pitch_window_quads(int R) { return (R + 4 + 3) / 4; }
// The words of a wavefront's frame in LDS: the frame, then zeros up to where the last lane with a lag <= lagMax reads (word N + 9 with R 6)
constexpr int pitch_frame_words(int W, int lagMax) { return (W + lagMax + 10 + 3) / 4 * 4; }
// The doubles of a wavefront's curve d / m, indexed by the lag 0 .. lagMax, an even count
constexpr int pitch_curve_words(int lagMax) { return (lagMax + 1 + 1) / 2 * 2; }

struct alignas(16) PitchQuad { float v[4]; };
struct alignas(8) PitchPair { float v[2]; };

// Four words from p, which lies on a 16-byte boundary (R a multiple of 4: one 16-byte load) or on an 8-byte one (two 8-byte loads)
template <int R> KLATT_PITCH_HD void pitch_load4(float* w, const float* p)
{
    if constexpr (R % 4 == 0) {
        const PitchQuad q = *reinterpret_cast<const PitchQuad*>(p);
        w[0] = q.v[0]; w[1] = q.v[1]; w[2] = q.v[2]; w[3] = q.v[3];
    } else {
        static_assert(R % 2 == 0, "a lane's base lies on an 8-byte boundary");
        const PitchPair a = *reinterpret_cast<const PitchPair*>(p), b = *reinterpret_cast<const PitchPair*>(p + 2);
        w[0] = a.v[0]; w[1] = a.v[1]; w[2] = b.v[0]; w[3] = b.v[1];
    }
}

// d of the lags p0 + R lane + 1 .. + R of the frame xs (16-byte aligned, pitch_frame_words long) to d[0 .. R); a lane all of whose lags lie
// above lagMax reads the frame's start and its values are not used.  Chain k of lag r is acc[r][k]: sample i = i0 + k with i0 a multiple
// of 4 is chain k, and the blocks come in ascending i0, so every chain sums in ascending i.  The window w holds xl[i0 .. i0 + 4 Q): a
// block loads its last four words and hands the rest on (unrolled Q times the window only changes names).
template <int R> KLATT_PITCH_HD void pitch_lane_pass(const float* xs, int W, int lagMax, int p0, int lane, double* d)
{
    constexpr int Q = pitch_window_quads(R);
    const int tau0 = p0 + R * lane + 1;
    const float* xl = xs + (tau0 <= lagMax ? tau0 - 1 : 0);      // x[i + tau0 + r] is xl[i + r + 1]
    double acc[R][kPitchChains];
KLATT_PITCH_UNROLL
    for (int r = 0; r < R; ++r)
KLATT_PITCH_UNROLL
        for (int k = 0; k < kPitchChains; ++k) acc[r][k] = 0.0;
    float w[4 * Q], b[4];
KLATT_PITCH_UNROLL
    for (int q = 0; q < Q - 1; ++q) pitch_load4<R>(w + 4 * q, xl + 4 * q);
    const int nFull = W & ~3;
KLATT_PITCH_UNROLL_Q
    for (int i = 0; i < nFull; i += 4) {
        pitch_load4<4>(b, xs + i);
        pitch_load4<R>(w + 4 * (Q - 1), xl + i + 4 * (Q - 1));
KLATT_PITCH_UNROLL
        for (int k = 0; k < kPitchChains; ++k)
KLATT_PITCH_UNROLL
            for (int r = 0; r < R; ++r) acc[r][k] = pitch_term(b[k], w[k + r + 1], acc[r][k]);
KLATT_PITCH_UNROLL
        for (int j = 0; j < 4 * (Q - 1); ++j) w[j] = w[j + 4];
    }
    if (nFull < W) {      // the last one to three samples
        pitch_load4<4>(b, xs + nFull);
        pitch_load4<R>(w + 4 * (Q - 1), xl + nFull + 4 * (Q - 1));
KLATT_PITCH_UNROLL
        for (int k = 0; k < kPitchChains - 1; ++k)
KLATT_PITCH_UNROLL
            for (int r = 0; r < R; ++r)
                if (nFull + k < W) acc[r][k] = pitch_term(b[k], w[k + r + 1], acc[r][k]);
    }
KLATT_PITCH_UNROLL
    for (int r = 0; r < R; ++r) d[r] = pitch_fold(acc[r]);
}

// d(1 .. lagMax) of lane `lane`'s lags to dm[lag], pass after pass
template <int R> KLATT_PITCH_HD void pitch_lane_diff(const float* xs, double* dm, int W, int lagMax, int lane)
{
    for (int p0 = 0; p0 < lagMax; p0 += 64 * R) {
        double d[R];
        pitch_lane_pass<R>(xs, W, lagMax, p0, lane, d);
        const int tau0 = p0 + R * lane + 1;
KLATT_PITCH_UNROLL
        for (int u = 0; u < R; ++u)
            if (tau0 + u <= lagMax) dm[tau0 + u] = d[u];
    }
}

// ---- the request, as both entry points plan it on the host ------------------------------------------------------------------------------
struct PitchPlan {
    int nWin = 0, lagMin = 0, lagMax = 0, what = 0, nCols = 0, sampleRate = 0;
    double threshold = 0.0;
};

// The plan of a request, or false with `why` set (without the entry point's prefix).
inline bool pitch_plan(PitchPlan& P, int sampleRate, int nWin, int lagMin, int lagMax, double threshold, int what, std::string& why)
{
    char buf[200];
    if (sampleRate <= 0) { snprintf(buf, sizeof buf, "sampleRate %d", sampleRate); why = buf; return false; }
    if (nWin < kPitchMinWin || nWin > kPitchMaxWin) { snprintf(buf, sizeof buf, "nWin %d (%d .. %d)", nWin, kPitchMinWin, kPitchMaxWin); why = buf; return false; }
    if (lagMin < 2 || lagMin >= lagMax || lagMax > kPitchMaxLag) {
        snprintf(buf, sizeof buf, "lagMin %d, lagMax %d (2 <= lagMin < lagMax <= %d)", lagMin, lagMax, kPitchMaxLag); why = buf; return false;
    }
    if (!(threshold >= 0.0 && threshold <= 1.0)) { snprintf(buf, sizeof buf, "threshold %g (0 .. 1)", threshold); why = buf; return false; }      // (a NaN fails both)
    if (what <= 0 || what > kPitchAllFields) {
        snprintf(buf, sizeof buf, "what %d (a set of the bits 1 f0, 2 period, 4 lag, 8 aperiodicity, 16 voiced, 32 cmnd)", what); why = buf; return false;
    }
    P.nWin = nWin; P.lagMin = lagMin; P.lagMax = lagMax; P.what = what; P.sampleRate = sampleRate; P.threshold = threshold;
    P.nCols = pitch_columns(what, lagMin, lagMax);
    return true;
}

// ---- the host's statements: the shared functions in plain loops ----------------------------------------------------------------------------
// The fields of one frame x[W + lagMax] to o[nCols]; m is scratch of lagMax + 2 doubles
inline void pitch_frame_host(const float* x, const PitchPlan& P, double* m, double* o)
{
    double s = 0.0;
    m[0] = 0.0;
    for (int tau = 1; tau <= P.lagMax; ++tau) {
        const double d = pitch_diff(x, P.nWin, tau);
        s = s + d;
        m[tau] = pitch_cmnd(d, tau, s);
    }
    int dip = 0, bestTau = 0;
    double bestM = 0.0;
    pitch_lane_choice(m, P.lagMin, P.lagMax, P.threshold, 0, 1, dip, bestM, bestTau);
    const bool voiced = dip != 0;
    const int col = pitch_put_fields(o, P.what, P.sampleRate, m, voiced ? dip : bestTau, voiced, P.lagMax);
    if (P.what & kPitchCmnd)
        for (int tau = P.lagMin; tau <= P.lagMax; ++tau) o[col + tau - P.lagMin] = m[tau];
}

// out[step][col] of `length` samples; returns steps * P.nCols.  In: int16_t (PCM) or float (a signal's samples).
template <typename In>
inline long long pitch_host(const In* x, long long length, const PitchPlan& P, long long hop, long long phase, double* out)
{
    const long long steps = length > phase ? (length - phase + hop - 1) / hop : 0;
    const int N = P.nWin + P.lagMax;
    std::vector<float> frame((size_t)N);
    std::vector<double> m((size_t)P.lagMax + 2);
    for (long long j = 0; j < steps; ++j) {
        const long long t0 = phase + j * hop - N / 2;
        for (int i = 0; i < N; ++i) frame[(size_t)i] = tile_sample(x, t0 + i, length);
        pitch_frame_host(frame.data(), P, m.data(), out + (size_t)j * P.nCols);
    }
    return steps * P.nCols;
}

// The LDS of a wavefront of klatt_pitch: its frame, its curve, its staged values; and of the workgroup's four
constexpr size_t pitch_wave_bytes(int W, int lagMax, int nCols, int elSize)
{
    return (size_t)4 * pitch_frame_words(W, lagMax) + (size_t)8 * pitch_curve_words(lagMax) + ((size_t)nCols * elSize + 15) / 16 * 16;
}
constexpr size_t pitch_lds_bytes(int W, int lagMax, int nCols, int elSize) { return 4 * pitch_wave_bytes(W, lagMax, nCols, elSize); }
constexpr size_t kPitchLdsBudget = pitch_lds_bytes(kPitchMaxWin, kPitchMaxLag, 5 + kPitchMaxLag - 1, 8);      // (lagMin 2: the longest curve)
static_assert(kPitchLdsBudget <= 160 * 1024, "the worst case of klatt_pitch fits the 160 KiB of a gfx950 compute unit's LDS");

}  // namespace klatt

// ---- the device ---------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

namespace klatt {

struct PitchArgs {
    const void* in;                      // the pool, or a signal's data: int16_t or float, as the kernel's In says
    const SpecRow* rows;
    const long long *start, *chunk;      // the packed form's row table (rowStride 0)
    long long rowStride, nSteps;         // nSteps: the steps of the output, rows x rowStride or the rows' steps together
    long long hop, phase;
    double threshold;
    int nWin, lagMin, lagMax, what, nCols, sampleRate;
    void* out;
};

// v of lane k (wave-uniform), in every lane
__device__ __forceinline__ double pitch_lane_value(double v, int k)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

// The one body of klatt_pitch and of klatt_stage_pitch (klatt_stage_frames.h: the pitch fed chunk by chunk), its two entry points: `rows`,
// steps(row), first(row, j) and sample(row, t) as lpc_rows' (klatt_lpc.h).
template <bool F32, class Row, class Steps, class First, class Sample>
__device__ __forceinline__ void pitch_rows(const PitchArgs& A, const Row* __restrict__ rows, Steps steps, First first, Sample sample)
{
    using T = typename std::conditional<F32, float, double>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char pitch_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = A.nWin, lagMin = A.lagMin, lagMax = A.lagMax, nCols = A.nCols, N = W + lagMax;
    const int frameWords = pitch_frame_words(W, lagMax);
    unsigned char* const region = pitch_lds + (size_t)wave * pitch_wave_bytes(W, lagMax, nCols, (int)sizeof(T));
    float* const xs = reinterpret_cast<float*>(region);
    double* const dm = reinterpret_cast<double*>(region + (size_t)4 * frameWords);
    T* const staged = reinterpret_cast<T*>(region + (size_t)4 * frameWords + (size_t)8 * pitch_curve_words(lagMax));
    const int mis = tile_mis<T>(A.out);
    const long long nGroups = (A.nSteps + kPitchGroup - 1) / kPitchGroup;
    for (long long grp = blockIdx.x; grp < nGroups; grp += gridDim.x) {
        for (int s = 0; s < kPitchGroup / 4; ++s) {
            const long long gs = grp * kPitchGroup + wave * (kPitchGroup / 4) + s;      // the step's number in the output: wave-uniform
            if (gs >= A.nSteps) break;
            long long g, r, j;
            int q;
            dense_locate(gs, 1, A.rowStride, A.start, A.chunk, g, q, r, j);
            const Row row = rows[r];
            if (j < steps(row)) {
                // ---- 1: the frame ----
                const long long t0 = first(row, j);
                for (int i = lane; i < frameWords; i += 64) xs[i] = i < N ? sample(row, t0 + i) : 0.0f;
                lpc_wave_sync();
                // ---- 2: d(1 .. lagMax), four or six lags a lane ----
                if (pitch_lane_lags(lagMax) == 6) pitch_lane_diff<6>(xs, dm, W, lagMax, lane);
                else pitch_lane_diff<4>(xs, dm, W, lagMax, lane);
                lpc_wave_sync();
                // ---- 3: s in ascending tau through the lanes, then m where d was ----
                double carry = 0.0;
                for (int base = 0; base <= lagMax; base += 64) {
                    const int tau = base + lane;
                    const bool mineIn = tau >= 1 && tau <= lagMax;
                    const double dl = mineIn ? dm[tau] : 0.0;      // (+0.0 changes no bit of s)
                    const int n = lagMax - base + 1 < 64 ? lagMax - base + 1 : 64;
                    double mine = 0.0;
                    for (int k = 0; k < n; ++k) {
                        carry = carry + pitch_lane_value(dl, k);
                        if (lane == k) mine = carry;
                    }
                    if (mineIn) dm[tau] = pitch_cmnd(dl, tau, mine);
                }
                lpc_wave_sync();
                // ---- 4: the choice ----
                int dip, bestTau;
                double bestM;
                pitch_lane_choice(dm, lagMin, lagMax, A.threshold, lane, 64, dip, bestM, bestTau);
                int first = dip != 0 ? dip : 0x7FFFFFFF;
KLATT_PITCH_UNROLL
                for (int k = 1; k < 64; k <<= 1) {
                    const int of = __shfl_xor(first, k, 64), ot = __shfl_xor(bestTau, k, 64);
                    const double om = __shfl_xor(bestM, k, 64);
                    first = of < first ? of : first;
                    if (pitch_better(om, ot, bestM, bestTau)) { bestM = om; bestTau = ot; }
                }
                const bool voiced = first != 0x7FFFFFFF;
                int col = 0;
                if (lane == 0) col = pitch_put_fields(staged, A.what, A.sampleRate, dm, voiced ? first : bestTau, voiced, lagMax);
                col = __builtin_amdgcn_readfirstlane(col);
                if (A.what & kPitchCmnd)
                    for (int tau = lagMin + lane; tau <= lagMax; tau += 64) staged[col + tau - lagMin] = (T)dm[tau];
            } else {
                for (int i = lane; i < nCols; i += 64) staged[i] = (T)0;      // past the row's steps in the padded form
            }
            lpc_wave_sync();
            // ---- 5: the step's values through the row writer ----
            const long long e0 = gs * nCols;
            const int lanes = tile_lanes<T>(mis, e0, nCols);
            for (int i = lane; i < lanes; i += 64) tile_store_lane(static_cast<T*>(A.out), mis, e0, nCols, staged, i);
            lpc_wave_sync();      // the staged values are read before the next step's
        }
    }
}

template <bool F32, typename In = int16_t>
__global__ void __launch_bounds__(256) klatt_pitch(const PitchArgs A)
{
    pitch_rows<F32>(A, A.rows, [](const SpecRow& row) { return row.steps; },
                    [&](const SpecRow&, long long j) { return A.phase + j * A.hop - (A.nWin + A.lagMax) / 2; },
                    [&](const SpecRow& row, long long t) { return tile_sample(static_cast<const In*>(A.in) + row.src, t, row.len); });
}

}  // namespace klatt
#endif
