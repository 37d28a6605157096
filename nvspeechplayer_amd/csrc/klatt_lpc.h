// klatt_lpc.h -- linear prediction of a batch's PCM or of a signal's rows: the analysis (autocorrelation method, Levinson-Durbin recursion;
// speechPlayer_batch_exportLpc, speechPlayer_pcmLpc / signalLpc, speechPlayer_lpcFromAutocorrelation) and the inverse filter by the frames'
// own coefficients (the residual or the prediction; speechPlayer_batch_exportLpcResidual, speechPlayer_pcmLpcResidual / signalLpcResidual).
//
// The definition is in include/speechPlayer_batch.h; this header is its one statement in code.  The functions marked KLATT_LPC_HD are
// compiled for the host (plain C++17, no HIP) and for the device from the same source: the host entry points run them in plain loops, the
// kernels call the same bodies, and nothing here changes arithmetic between the two sides.  tests/native/check_lpc.cpp models both
// kernels' walks on the host against brute force under the sanitizers.
//
//   The frame       xw[i] = x[c - nWin / 2 + i] * w[i], one float32 product (klatt_spectrum.h: spec_windowed) of the reader's sample
//                   (klatt_tiles.h: tile_sample -- +0 outside the row, nothing loaded there) and the window rounded to float32 once.
//   r[k]            term(i, k) = (double)xw[i] * (double)xw[i - k] is EXACT in binary64 (24 x 24 bits), so lpc_term's fma adds it with one
//                   rounding whichever way it is written.  partial[q] (lpc_partial) sums the terms of i = q, q + 64, ... >= k in ascending
//                   i from +0.0; r[k] is the balanced tree over the 64 partials in natural order (lpc_tree: t[i] = t[2i] + t[2i+1], six
//                   levels).  A butterfly over lanes (v += v of lane ^ 1, ^ 2, ... ^ 32) evaluates that very tree in every lane:
//                   binary64 addition commutes, so which operand comes first changes no bit.
//   Lemma           A partial that starts from +0.0 is never -0.0: x + y is -0.0 only when both are -0.0 (round to nearest), and the
//                   first addend is +0.0; by induction no later sum is -0.0 either (a sum that cancels exactly is +0.0).  Adding +-0 to
//                   a value that is not -0.0 changes no bit.  So the terms with a zero factor -- samples outside the row, the exact
//                   zeros of a Klatt silence -- may be skipped or added alike.
//   The recursion   lpc_levinson, binary64 with explicit fma, written over compile-time indices (every loop runs to kLpcMaxOrder behind
//                   i <= order tests) so that on the device r[] and a[] stay in registers; the in-place update of a[] takes the pair
//                   (j, i - j) from the old values, which is the definition's a' "all from the old a".
//   The inverse     lpc_frame_of: the nearest centre, ties upward; lpc_inverse: the fma chain in ascending m from x(t) (residual) or
//   filter          +0.0 (prediction, negated), rounded to float32 once.
//
//   klatt_lpc<F32, In>   lpc_rows<F32>, the one body it shares with klatt_stage_lpc (klatt_stage_frames.h), handed the row's own steps, the
//                   frame's first sample phase + j hop - nWin / 2 and the reader tile_sample.  A 256-lane workgroup takes kLpcGroup = 64 consecutive steps of the OUTPUT (located by dense_locate: a group may
//                   end one row and begin the next).  Phase A: each wavefront takes 16 of them, one at a time and at its own pace (its LDS region is its own: lpc_wave_sync): coalesced masked loads
//                   of the frame, the window product, xw into its own LDS region; lane q then accumulates partial[q] of kLpcLagBlock
//                   lags at a time (xw[i] is read once per block; consecutive lanes read consecutive words: no bank conflict), the tree
//                   goes across lanes (six __shfl_xor of a double a lag), lane 0 applies the lag window and parks r[k] in LDS as
//                   rs[k][step].  Phase B: one barrier, then wavefront 0 runs 64 recursions side by side, a lane per step, r[] and
//                   a[] in registers; the step's fields are staged where xw was (all frames are spent) and the whole group's run of
//                   64 nCols elements leaves through the row writer (tile_store).  LDS per workgroup:
//                       max(4 * 4 * (nWin + order), 64 * nCols * sizeof(out element)) + 8 * 64 * (order + 1) bytes
//                   -- 82 944 B at nWin 4096, order 32, float64, every field; 17 152 B at nWin 512, order 16, float32, lpc + error.
//   klatt_lpc_residual<WHAT, F32, In, C32>   The tile walk of klatt_tiles.h, tiles of kLpcTile = 1024 outputs of one row: x(t0 - order ..
//                   t0 + n) staged by tile_read, the coefficient rows the tile's samples use staged in LDS as doubles when they number
//                   at most kLpcStageRows = 64 (hop >= 17 or so; a row serves hop samples) and read from memory by each lane otherwise
//                   (hop 1: every sample has a row of its own, staging would share nothing), one output per lane per pass, stored by
//                   tile_store.
// Out of scope: line spectral frequencies, Burg and covariance methods, the recursive synthesis filter 1 / A(z) (klatt_lpcsynth.h), order above 32,
// pre-emphasis inside the export, live handles (their pulls go through the LPC stage of klatt_stage_frames.h; the inverse filter has no
// stage: a sample's frame is the nearest centre, which may be a frame still to come), NodePlayer.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "klatt_tiles.h"
#include "klatt_spectrum.h"
#include "klatt_resample.h"

#if defined(__HIPCC__)
#define KLATT_LPC_HD __host__ __device__ __forceinline__
#define KLATT_LPC_UNROLL _Pragma("unroll")      // (a hint to hipcc alone: the loops' arithmetic is the same rolled or unrolled)
#else
#define KLATT_LPC_HD inline
#define KLATT_LPC_UNROLL
#endif

namespace klatt {

constexpr int kLpcMaxOrder = 32, kLpcMaxWin = 4096;
constexpr int kLpcPartials = 64;          // partial sums of a lag: a lane each
constexpr int kLpcGroup = 64;             // consecutive steps of the output a workgroup of klatt_lpc takes at a time
constexpr int kLpcLagBlock = 8;           // lags a lane accumulates side by side
constexpr int kLpcTile = 1024;            // consecutive outputs of one row a workgroup of klatt_lpc_residual takes at a time
constexpr int kLpcStageRows = 64;         // coefficient rows a tile stages in LDS at most
// `what` of the analysis: the fields come in this order whatever the order of the bits
constexpr int kLpcAutocorr = 1, kLpcCoeff = 2, kLpcReflection = 4, kLpcError = 8, kLpcStages = 16, kLpcAllFields = 31;
// `what` of the inverse filter
constexpr int kLpcResidual = 0, kLpcPrediction = 1;

// The values of a step
KLATT_LPC_HD int lpc_columns(int what, int order)
{
    return ((what & kLpcAutocorr) ? order + 1 : 0) + ((what & kLpcCoeff) ? order : 0) + ((what & kLpcReflection) ? order : 0) +
           ((what & kLpcError) ? 1 : 0) + ((what & kLpcStages) ? 1 : 0);
}

// acc + (double)a * (double)b: the product is exact, the sum rounded once
KLATT_LPC_HD double lpc_term(float a, float b, double acc) { return fma((double)a, (double)b, acc); }

// partial[q] of lag k over a frame of nWin windowed samples: the terms of i = q, q + 64, ... with i >= k, ascending, from +0.0
KLATT_LPC_HD double lpc_partial(const float* xw, int nWin, int k, int q)
{
    double acc = 0.0;
    for (int i = q; i < nWin; i += kLpcPartials)
        if (i >= k) acc = lpc_term(xw[i], xw[i - k], acc);
    return acc;
}

// The balanced tree over 64 values in natural order, in place: t[i] = t[2i] + t[2i+1], six levels; the root is t[0]
KLATT_LPC_HD double lpc_tree(double* t)
{
    for (int n = kLpcPartials / 2; n >= 1; n >>= 1)
        for (int i = 0; i < n; ++i) t[i] = t[2 * i] + t[2 * i + 1];
    return t[0];
}

// r[k] after the lag window: one binary64 product, or none at all
KLATT_LPC_HD double lpc_lagged(double r, const double* lagWindow, int k) { return lagWindow ? r * lagWindow[k] : r; }

// The Levinson-Durbin recursion on r[0 .. order]: a[1 .. order] and k[1 .. order] (index 0 unused), the error E and the stages done.
// Every array holds kLpcMaxOrder + 1 values; r beyond `order` is not read.
KLATT_LPC_HD void lpc_levinson(const double* r, int order, double* a, double* k, double& E, int& stages)
{
KLATT_LPC_UNROLL
    for (int j = 0; j <= kLpcMaxOrder; ++j) { a[j] = 0.0; k[j] = 0.0; }
    E = r[0];
    stages = 0;
    bool going = true;
KLATT_LPC_UNROLL
    for (int i = 1; i <= kLpcMaxOrder; ++i) {
        if (i <= order) {
            going = going && E > 0.0 && E <= 1.7976931348623157e308;      // (a NaN fails both)
            double acc = r[i];
KLATT_LPC_UNROLL
            for (int j = 1; j < i; ++j) acc = fma(a[j], r[i - j], acc);
            const double kappa = -acc / E;
            going = going && fabs(kappa) < 1.0;                             // (a NaN stops too)
            if (going) {
KLATT_LPC_UNROLL
                for (int j = 1; 2 * j <= i; ++j) {                          // the pair (j, i - j), both from the old a; the middle one once
                    const double lo = a[j], hi = a[i - j];
                    a[j] = fma(kappa, hi, lo);
                    if (2 * j != i) a[i - j] = fma(kappa, lo, hi);
                }
                a[i] = kappa; k[i] = kappa;
                E = fma(kappa, acc, E);
                stages = i;
            }
        }
    }
}

// A step's fields to o[0 .. lpc_columns): r after the lag window, a, k, E, stages, in this fixed order, each rounded to T once.  Written
// over compile-time indices, as lpc_levinson is: on the device r[], a[] and k[] are registers.
template <typename T> KLATT_LPC_HD void lpc_put_fields(T* o, int what, int order, const double* r, const double* a, const double* k, double E, int stages)
{
    int col = 0;
    if (what & kLpcAutocorr) {
KLATT_LPC_UNROLL
        for (int c = 0; c <= kLpcMaxOrder; ++c) if (c <= order) o[col + c] = (T)r[c];
        col += order + 1;
    }
    if (what & kLpcCoeff) {
KLATT_LPC_UNROLL
        for (int c = 1; c <= kLpcMaxOrder; ++c) if (c <= order) o[col + c - 1] = (T)a[c];
        col += order;
    }
    if (what & kLpcReflection) {
KLATT_LPC_UNROLL
        for (int c = 1; c <= kLpcMaxOrder; ++c) if (c <= order) o[col + c - 1] = (T)k[c];
        col += order;
    }
    if (what & kLpcError) o[col++] = (T)E;
    if (what & kLpcStages) o[col++] = (T)(double)stages;
}

// The frame of sample t of a row of `steps` > 0 steps: the nearest centre phase + j hop, ties upward
KLATT_LPC_HD long long lpc_frame_of(long long t, long long hop, long long phase, long long steps)
{
    const long long d = t > phase ? t - phase : 0, j = (d + hop / 2) / hop;
    return j < steps - 1 ? j : steps - 1;
}

// e(t) or p(t): xs[order] is x(t), xs[order - m] is x(t - m); a[m - 1] is a_m, binary64 or float32 widened exactly
KLATT_LPC_HD double lpc_widen(double c) { return c; }
KLATT_LPC_HD double lpc_widen(float c) { return (double)c; }
template <int WHAT, typename C> KLATT_LPC_HD float lpc_inverse(const float* xs, const C* a, int order)
{
    double s = WHAT == kLpcResidual ? (double)xs[order] : 0.0;
KLATT_LPC_UNROLL
    for (int m = 1; m <= kLpcMaxOrder; ++m)
        if (m <= order) s = fma(lpc_widen(a[m - 1]), (double)xs[order - m], s);
    return (float)(WHAT == kLpcResidual ? s : -s);
}

// ---- the request, as both entry points plan it on the host ------------------------------------------------------------------------------
struct LpcPlan {
    int order = 0, nWin = 0, what = 0, nCols = 0;
    bool hasLag = false;
    std::vector<float> window;       // [nWin]
    std::vector<double> lag;         // [order + 1] with a lag window
};

// The plan of a request, or false with `why` set (without the entry point's prefix).
inline bool lpc_plan(LpcPlan& P, int order, int nWin, const double* window, const double* lagWindow, int what, std::string& why)
{
    char buf[160];
    if (order < 1 || order > kLpcMaxOrder) { snprintf(buf, sizeof buf, "order %d (1 .. %d)", order, kLpcMaxOrder); why = buf; return false; }
    if (nWin <= order || nWin > kLpcMaxWin) { snprintf(buf, sizeof buf, "nWin %d (order + 1 = %d .. %d)", nWin, order + 1, kLpcMaxWin); why = buf; return false; }
    if (what <= 0 || what > kLpcAllFields) { snprintf(buf, sizeof buf, "what %d (a set of the bits 1 autocorr, 2 lpc, 4 reflection, 8 error, 16 stages)", what); why = buf; return false; }
    P.order = order; P.nWin = nWin; P.what = what; P.nCols = lpc_columns(what, order);
    P.window.resize((size_t)nWin);
    for (int i = 0; i < nWin; ++i) {
        const double w = window ? window[i] : 0.5 - 0.5 * cos(6.283185307179586 * (double)i / (double)nWin);
        if (!std::isfinite(w)) { snprintf(buf, sizeof buf, "window[%d] is not finite", i); why = buf; return false; }
        P.window[(size_t)i] = (float)w;
    }
    P.hasLag = lagWindow != nullptr;
    P.lag.clear();
    for (int k = 0; lagWindow && k <= order; ++k) {
        if (!std::isfinite(lagWindow[k])) { snprintf(buf, sizeof buf, "lagWindow[%d] is not finite", k); why = buf; return false; }
        P.lag.push_back(lagWindow[k]);
    }
    return true;
}

// ---- the host's statements: the shared functions in plain loops ----------------------------------------------------------------------------
// The fields of one frame whose windowed samples are xw[nWin], to o[nCols]
inline void lpc_frame_host(const float* xw, const LpcPlan& P, double* o)
{
    double r[kLpcMaxOrder + 1], a[kLpcMaxOrder + 1], k[kLpcMaxOrder + 1], t[kLpcPartials], E;
    int stages;
    for (int lag = 0; lag <= P.order; ++lag) {
        for (int q = 0; q < kLpcPartials; ++q) t[q] = lpc_partial(xw, P.nWin, lag, q);
        r[lag] = lpc_lagged(lpc_tree(t), P.hasLag ? P.lag.data() : nullptr, lag);
    }
    lpc_levinson(r, P.order, a, k, E, stages);
    lpc_put_fields(o, P.what, P.order, r, a, k, E, stages);
}

// out[step][col] of `length` samples; returns steps * P.nCols.  In: int16_t (PCM) or float (a signal's samples).
template <typename In>
inline long long lpc_host(const In* x, long long length, const LpcPlan& P, long long hop, long long phase, double* out)
{
    const long long steps = length > phase ? (length - phase + hop - 1) / hop : 0;
    std::vector<float> xw((size_t)P.nWin);
    for (long long j = 0; j < steps; ++j) {
        const long long t0 = phase + j * hop - P.nWin / 2;
        for (int i = 0; i < P.nWin; ++i) xw[(size_t)i] = spec_windowed(tile_sample(x, t0 + i, length), P.window[(size_t)i]);
        lpc_frame_host(xw.data(), P, out + (size_t)j * P.nCols);
    }
    return steps * P.nCols;
}

// The inverse filter of `length` samples by coeff[steps][order] (binary64), to out in `format` (0 int16 by res_int16, 1 float32)
template <typename In>
inline void lpc_inverse_host(const In* x, long long length, int order, long long hop, long long phase, const double* coeff, int what, int format, void* out)
{
    const long long steps = length > phase ? (length - phase + hop - 1) / hop : 0;
    const double none[kLpcMaxOrder] = {};
    float xs[kLpcMaxOrder + 1];
    for (long long t = 0; t < length; ++t) {
        for (int m = 0; m <= order; ++m) xs[order - m] = tile_sample(x, t - m, length);
        const double* a = steps > 0 ? coeff + (size_t)lpc_frame_of(t, hop, phase, steps) * order : none;
        res_store(out, format, t, what == kLpcResidual ? lpc_inverse<kLpcResidual>(xs, a, order) : lpc_inverse<kLpcPrediction>(xs, a, order));
    }
}

// The LDS of a workgroup of klatt_lpc: the four wavefronts' frames (each with `order` words of slack before it, so that no lane forms an address below
// the region), where the group's fields are staged afterwards; then rs[order + 1][64]
constexpr int lpc_frame_words(int nWin, int order) { return (nWin + order + 3) / 4 * 4; }
constexpr size_t lpc_front_bytes(int nWin, int order, int nCols, int elSize)
{
    const size_t frames = (size_t)4 * 4 * lpc_frame_words(nWin, order), staged = ((size_t)kLpcGroup * nCols * elSize + 15) / 16 * 16;
    return frames > staged ? frames : staged;
}
constexpr size_t lpc_lds_bytes(int nWin, int order, int nCols, int elSize) { return lpc_front_bytes(nWin, order, nCols, elSize) + (size_t)8 * kLpcGroup * (order + 1); }
constexpr size_t kLpcLdsBudget = lpc_lds_bytes(kLpcMaxWin, kLpcMaxOrder, 3 * kLpcMaxOrder + 3, 8);

}  // namespace klatt

// ---- the device ---------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

namespace klatt {

struct LpcArgs {
    const void* in;                      // the pool, or a signal's data: int16_t or float, as the kernel's In says
    const SpecRow* rows;
    const long long *start, *chunk;      // the packed form's row table (rowStride 0)
    long long rowStride, nSteps;         // nSteps: the steps of the output, rows x rowStride or the rows' steps together
    long long hop, phase;
    const float* window;
    const double* lag;                   // or null
    int order, nWin, what, nCols;
    void* out;
};

// Between a wavefront's LDS stores and its own lanes' loads of them: its LDS operations complete in the order issued, so no workgroup
// barrier is needed -- the compiler must only keep the order, and the four wavefronts need not run in step
__device__ __forceinline__ void lpc_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The one body of klatt_lpc and of klatt_stage_lpc (klatt_stage_frames.h: the analysis fed chunk by chunk), its two entry points: `rows` is
// the launch's row table, steps(row) the steps of a row in this output, first(row, j) the first sample of its step j's frame, and
// sample(row, t) sample t as the reader gives it -- of the row itself, or of a stage's virtual row.
template <bool F32, class Row, class Steps, class First, class Sample>
__device__ __forceinline__ void lpc_rows(const LpcArgs& A, const Row* __restrict__ rows, Steps steps, First first, Sample sample)
{
    using T = typename std::conditional<F32, float, double>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char lpc_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int order = A.order, nWin = A.nWin, nCols = A.nCols;
    const int frameWords = lpc_frame_words(nWin, order);
    float* const xw = reinterpret_cast<float*>(lpc_lds) + (size_t)wave * frameWords + order;      // xw[-order .. -1] is the slack
    T* const staged = reinterpret_cast<T*>(lpc_lds);
    double* const rs = reinterpret_cast<double*>(lpc_lds + lpc_front_bytes(nWin, order, nCols, (int)sizeof(T)));
    const long long nGroups = (A.nSteps + kLpcGroup - 1) / kLpcGroup;
    for (long long grp = blockIdx.x; grp < nGroups; grp += gridDim.x) {
        const long long g0 = grp * kLpcGroup;
        const int nInside = (int)(A.nSteps - g0 < kLpcGroup ? A.nSteps - g0 : kLpcGroup);
        // ---- phase A: r[0 .. order] of the group's steps, sixteen per wavefront ----
        for (int s = 0; s < kLpcGroup / 4; ++s) {
            const int step = wave * (kLpcGroup / 4) + s;
            bool live = false;
            Row row{};
            long long j = 0;
            if (step < nInside) {
                long long g, r;
                int q;
                dense_locate(g0 + step, 1, A.rowStride, A.start, A.chunk, g, q, r, j);
                row = rows[r];
                live = j < steps(row);
            }
            if (live) {
                const long long t0 = first(row, j);
                for (int i = lane; i < nWin; i += 64) xw[i] = spec_windowed(sample(row, t0 + i), A.window[i]);
            }
            lpc_wave_sync();
            if (live) {
                for (int kb = 0; kb <= order; kb += kLpcLagBlock) {
                    double acc[kLpcLagBlock];
KLATT_LPC_UNROLL
                    for (int u = 0; u < kLpcLagBlock; ++u) acc[u] = 0.0;
                    for (int i = lane; i < nWin; i += kLpcPartials) {
                        const float xi = xw[i];
KLATT_LPC_UNROLL
                        for (int u = 0; u < kLpcLagBlock; ++u)
                            if (i >= kb + u && kb + u <= order) acc[u] = lpc_term(xi, xw[i - kb - u], acc[u]);
                    }
KLATT_LPC_UNROLL
                    for (int u = 0; u < kLpcLagBlock; ++u) {
                        double v = acc[u];
KLATT_LPC_UNROLL
                        for (int m = 1; m < kLpcPartials; m <<= 1) v = v + __shfl_xor(v, m, 64);
                        if (lane == 0 && kb + u <= order) rs[(kb + u) * kLpcGroup + step] = lpc_lagged(v, A.lag, kb + u);
                    }
                }
            }
            lpc_wave_sync();      // the frame is spent before the next one's stores
        }
        __syncthreads();      // every wavefront's r[] is parked, every frame spent
        // ---- phase B: the recursions, a lane per step ----
        if (wave == 0 && lane < nInside) {
            long long g, rr, j;
            int q;
            dense_locate(g0 + lane, 1, A.rowStride, A.start, A.chunk, g, q, rr, j);
            const bool live = j < steps(rows[rr]);
            double r[kLpcMaxOrder + 1], a[kLpcMaxOrder + 1], k[kLpcMaxOrder + 1], E = 0.0;
            int stages = 0;
KLATT_LPC_UNROLL
            for (int c = 0; c <= kLpcMaxOrder; ++c) r[c] = live && c <= order ? rs[c * kLpcGroup + lane] : 0.0;
            lpc_levinson(r, order, a, k, E, stages);
            lpc_put_fields(staged + (size_t)lane * nCols, A.what, order, r, a, k, E, stages);
        }
        __syncthreads();
        tile_store<T>(A.out, g0 * nCols, nInside * nCols, staged, tid);
        __syncthreads();      // every lane has read the staged values before the next group's frames
    }
}

template <bool F32, typename In = int16_t>
__global__ void __launch_bounds__(256) klatt_lpc(const LpcArgs A)
{
    lpc_rows<F32>(A, A.rows, [](const SpecRow& row) { return row.steps; },
                  [&](const SpecRow&, long long j) { return A.phase + j * A.hop - A.nWin / 2; },
                  [&](const SpecRow& row, long long t) { return tile_sample(static_cast<const In*>(A.in) + row.src, t, row.len); });
}

struct LpcResRow { long long src, len, steps, dst, coeff; };      // a row's input, its steps, its first element in the output, its first STEP in the coefficients

struct LpcResArgs {
    const void* in;
    const LpcResRow* rows;
    TileOut tile;
    const void* coeff;                   // double or float, as the kernel's C32 says
    long long hop, phase;
    int order, coeffCols, col0;
};

template <int WHAT, bool F32, typename In = int16_t, bool C32 = false>
__global__ void __launch_bounds__(256) klatt_lpc_residual(const LpcResArgs A)
{
    using T = TileValue<F32>;
    using C = typename std::conditional<C32, float, double>::type;
    __shared__ __attribute__((aligned(16))) float xs[kLpcTile + kLpcMaxOrder];
    __shared__ __attribute__((aligned(16))) T staged[kLpcTile];
    __shared__ __attribute__((aligned(16))) double as[kLpcStageRows * kLpcMaxOrder];
    const int tid = threadIdx.x, order = A.order;
    const C* __restrict__ coeff = static_cast<const C*>(A.coeff);
    for (long long g = blockIdx.x; g < A.tile.nTiles; g += gridDim.x) {
        long long r, t0;
        tile_locate(A.tile, g, kLpcTile, r, t0);
        const LpcResRow row = A.rows[r];
        const int n = tile_n(A.tile.rowStride, row.len, t0, kLpcTile), live = tile_live(n, row.len, t0);
        long long j0 = 0;
        int nRows = 0;      // the coefficient rows staged (0: each lane reads its own from memory)
        if (live > 0) {
            tile_read<1>(xs, static_cast<const In*>(A.in) + row.src, row.len, t0 - order, live + order, tid);
            if (row.steps > 0) {
                j0 = lpc_frame_of(t0, A.hop, A.phase, row.steps);
                const long long rowsUsed = lpc_frame_of(t0 + live - 1, A.hop, A.phase, row.steps) - j0 + 1;
                nRows = rowsUsed <= kLpcStageRows ? (int)rowsUsed : 0;
                for (int i = tid; i < nRows * order; i += 256) {
                    const int jj = i / order, m = i - jj * order;
                    as[i] = lpc_widen(coeff[(row.coeff + j0 + jj) * A.coeffCols + A.col0 + m]);
                }
            } else {      // a row without steps: coefficients +0
                nRows = 1;
                for (int i = tid; i < order; i += 256) as[i] = 0.0;
            }
        }
        __syncthreads();
        for (int i = tid; i < n; i += 256) {
            float y = 0.0f;
            if (i < live) {
                const long long j = row.steps > 0 ? lpc_frame_of(t0 + i, A.hop, A.phase, row.steps) : 0;
                y = nRows > 0 ? lpc_inverse<WHAT>(xs + i, as + (int)(j - j0) * order, order)
                              : lpc_inverse<WHAT>(xs + i, coeff + (row.coeff + j) * A.coeffCols + A.col0, order);
            }
            staged[i] = i < live ? res_value<F32>(y) : (T)0;
        }
        __syncthreads();
        tile_store<T>(A.tile.out, row.dst + t0, n, staged, tid);
        __syncthreads();      // every lane has read the staged values before the next tile's
    }
}

}  // namespace klatt
#endif
