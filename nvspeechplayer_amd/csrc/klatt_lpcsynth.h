// klatt_lpcsynth.h -- LPC synthesis: a row of excitation samples through the recursive all-pole filter 1 / A(z) of its own frames' prediction
// coefficients (speechPlayer_batch_exportLpcSynthesis / exportLpcSynthesisOf, speechPlayer_pcmLpcSynthesis / signalLpcSynthesis), and the
// step-up recursion from reflection coefficients (speechPlayer_lpcFromReflection).  It is the inverse of klatt_lpc.h's inverse filter.
//
// The definition is in include/speechPlayer_batch.h ("LPC synthesis"); this header is its one statement in code.  The functions marked
// KLATT_LPC_HD are compiled for the host (plain C++17, no HIP) and for the device from the same source: the host entry points run them in
// plain loops, the kernel calls the same bodies.  tests/native/check_lpc_synth.cpp models the kernel's walk on the host against
// lpc_synth_host under the sanitizers.
//
//   The step        lpc_synth_step<B>: s = (double)e(t), then s = fma(-a_m, (double)y(t - m), s) for m = 1 .. order ascending behind
//                   m <= order tests (no coefficient is padded: fma(-0.0, y, s) can change the sign of a zero), y(t) = (float)s.  The
//                   history is a ring of B float32 values, y(t) in slot t mod B; B is 8, 16 or 32, the smallest >= order
//                   (lpc_synth_history), and the step reads slot (t - m) mod B BEFORE the caller writes slot t mod B, so B = order works.
//   The frames      lpc_frame_of(t) is the nearest centre, ties upward, clamped to steps - 1.  Unclamped it is the same number k for every
//                   row of a call: it turns from k - 1 to k at sample lpc_synth_change(k) = phase + k hop - floor(hop / 2), k = 1, 2, ...
//                   (check_lpc_synth.cpp holds this to lpc_frame_of).  Only the clamp differs from row to row.
//   The statement   lpc_synth_host: the plain loop, coeff[steps][order] binary64 on the host.
//   The packing     lpc_synth_pack: filter_pack (klatt_filter.h) over rows that carry their first coefficient step and their steps beside a
//                   FilterRow of one section: groups of 64 rows by length descending, fillers (all zeros: no section, no steps) behind
//                   the last, which read and write nothing.
//   klatt_lpc_synth<B, F32, In, C32>   The lane-per-row scheme of klatt_filter.h, its third user: one wavefront (a workgroup of 64 lanes)
//                   per group, lane r takes row r.  Tiles of 64 samples are loaded by filter_load_rows, converted by tile_x into the LDS
//                   region at a pitch of 65 dwords, staged in place in the output's type and stored by filter_store_rows; the next tile's
//                   loads are issued before the current tile's arithmetic and wait in registers.  Each lane keeps its row's current
//                   a_1 .. a_order as doubles and the ring of B float32 in registers: the sample loop is unrolled by B (64 is a multiple
//                   of every B), so slot t mod B and every coefficient index are compile-time constants.  The frame change is tested on
//                   t == lpc_synth_change(k), which is wave-uniform (one hop and phase per call); each lane clamps its own frame to its
//                   own steps - 1.  The coefficients of frame k + 1 are loaded (raw, float32 or float64) as soon as frame k is taken, so
//                   a load has hop samples of arithmetic to land; hop 1 runs the same code with a load per sample.  A row without steps,
//                   and so a filler, loads no coefficient and runs on +0.  A padded row's remainder past the group's longest row is
//                   written from a zeroed region without arithmetic.  LDS: 64 x 65 x 4 + 1 024 = 17 664 bytes per wavefront.
//                   VGPRs (B 32, float64 coefficients): 64 the next tile, 64 the coefficients, 64 the next frame's, 32 the ring; the
//                   workgroup is one wavefront and may take 512, so nothing goes to scratch (docs/KERNELS.md has the figures).
//                   A dependent binary64 chain of `order` fused multiply-adds per sample and lane: latency binds, not memory.
// Out of scope: initial conditions in or out, a pole-zero or weighting filter A(z/g1)/A(z/g2), order above 32, a live stage (a stage takes
// one input; this takes two), NodePlayer, time-parallel formulations (they cannot meet the sequential statement's bits).  Unstable
// coefficients cannot be refused (they live on the device): once a value of a row is not finite its later bits are unspecified; nothing
// faults and no value steers an address.
#pragma once

#include "klatt_lpc.h"
#include "klatt_filter.h"

namespace klatt {

constexpr int kLpcSynthMaxHistory = 32;

// The ring a request of `order` runs in: 8, 16 or 32 slots, the smallest that holds y(t - order)
KLATT_LPC_HD int lpc_synth_history(int order) { return order <= 8 ? 8 : order <= 16 ? 16 : 32; }

// One sample: e is e(t), a[m - 1] is a_m (binary64), ring[(t - m) mod B] is y(t - m) and `slot` is t mod B.  The caller writes the
// result to ring[slot] afterwards.
template <int B> KLATT_LPC_HD float lpc_synth_step(float e, const double* a, int order, const float* ring, int slot)
{
    static_assert(B >= 1 && (B & (B - 1)) == 0 && B <= kLpcSynthMaxHistory, "the ring is a power of two");
    double s = (double)e;
KLATT_LPC_UNROLL
    for (int m = 1; m <= B; ++m)
        if (m <= order) s = fma(-a[m - 1], (double)ring[(slot - m) & (B - 1)], s);
    return (float)s;
}

// The first sample whose unclamped frame is k (k >= 1)
KLATT_LPC_HD long long lpc_synth_change(long long k, long long hop, long long phase) { return phase + k * hop - hop / 2; }

// The frame a row of `steps` > 0 steps takes where the unclamped frame is k
KLATT_LPC_HD long long lpc_synth_clamp(long long k, long long steps) { return k < steps - 1 ? k : steps - 1; }

// a_1 .. a_order from the reflection coefficients k_1 .. k_order (the step-up recursion: lpc_levinson's update of a[]); both arrays hold
// kLpcMaxOrder + 1 values, index 0 unused
KLATT_LPC_HD void lpc_step_up(const double* k, int order, double* a)
{
KLATT_LPC_UNROLL
    for (int j = 0; j <= kLpcMaxOrder; ++j) a[j] = 0.0;
KLATT_LPC_UNROLL
    for (int i = 1; i <= kLpcMaxOrder; ++i) {
        if (i <= order) {
            const double kappa = k[i];
KLATT_LPC_UNROLL
            for (int j = 1; 2 * j <= i; ++j) {                              // the pair (j, i - j), both from the old a; the middle one once
                const double lo = a[j], hi = a[i - j];
                a[j] = fma(kappa, hi, lo);
                if (2 * j != i) a[i - j] = fma(kappa, lo, hi);
            }
            a[i] = kappa;
        }
    }
}

// ---- the request, as every entry point plans it on the host ------------------------------------------------------------------------------
struct LpcSynthPlan {
    int order = 0, history = 0, format = 0;
    long long hop = 0, phase = 0;
};

// The plan of a request, or false with `why` set (without the entry point's prefix)
inline bool lpc_synth_plan(LpcSynthPlan& P, int order, long long hop, long long phase, int format, std::string& why)
{
    char buf[160];
    if (order < 1 || order > kLpcMaxOrder) { snprintf(buf, sizeof buf, "order %d (1 .. %d)", order, kLpcMaxOrder); why = buf; return false; }
    if (format != 0 && format != 1) { snprintf(buf, sizeof buf, "format %d (0 int16, 1 float32)", format); why = buf; return false; }
    if (hop <= 0 || phase < 0) { snprintf(buf, sizeof buf, "hop %lld, phase %lld (hop > 0, phase >= 0)", hop, phase); why = buf; return false; }
    P.order = order; P.history = lpc_synth_history(order); P.format = format;
    P.hop = hop < (1ll << 40) ? hop : 1ll << 40;            // (beyond any row: one step, and the products stay in 64 bits)
    P.phase = phase < (1ll << 40) ? phase : 1ll << 40;
    return true;
}

// ---- the host's statement: the shared step in a plain loop ---------------------------------------------------------------------------------
// `length` samples through 1 / A(z) by coeff[steps][order] (binary64), to out in `format` (0 int16 by res_int16, 1 float32)
template <typename In>
inline void lpc_synth_host(const In* x, long long length, int order, long long hop, long long phase, const double* coeff, int format, void* out)
{
    constexpr int B = kLpcSynthMaxHistory;
    const long long steps = length > phase ? (length - phase + hop - 1) / hop : 0;
    const double none[kLpcMaxOrder] = {};
    float ring[B] = {};
    for (long long t = 0; t < length; ++t) {
        const double* a = steps > 0 ? coeff + (size_t)lpc_frame_of(t, hop, phase, steps) * order : none;
        const int slot = (int)(t & (B - 1));
        const float y = lpc_synth_step<B>(tile_x(x[t]), a, order, ring, slot);
        ring[slot] = y;
        res_store(out, format, t, y);
    }
}

// ---- the packing ------------------------------------------------------------------------------------------------------------------------
// A FilterRow of one section (a filler: none) with the row's first STEP in the coefficients and its steps
struct LpcSynthRow : FilterRow { long long coeff, steps; };

inline LpcSynthRow lpc_synth_row(long long src, long long len, long long dst, long long coeff, long long steps)
{
    LpcSynthRow r{};
    r.src = src; r.len = len; r.outLen = len; r.dst = dst; r.secAt = 0; r.sections = 1; r.coeff = coeff; r.steps = steps;
    return r;
}

inline void lpc_synth_pack(const std::vector<LpcSynthRow>& rows, std::vector<LpcSynthRow>& packed, std::vector<FilterGroup>& groups)
{
    filter_pack(rows, packed, groups);
}

}  // namespace klatt

// ---- the device ---------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

namespace klatt {

struct LpcSynthArgs {
    const void* in;                      // the pool, or a signal's data: int16_t or float, as the kernel's In says
    const LpcSynthRow* rows;             // the packed table
    const FilterGroup* groups;
    long long nGroups;
    long long rowStride;                 // the padded form: a row's width
    void* out;
    const void* coeff;                   // double or float, as the kernel's C32 says
    long long hop, phase;
    int order, coeffCols, col0;
};

template <int B, bool F32, typename In = int16_t, bool C32 = false>
__global__ void __launch_bounds__(kFilterLanes) klatt_lpc_synth(const LpcSynthArgs A)
{
    using T = TileValue<F32>;
    using C = typename std::conditional<C32, float, double>::type;
    constexpr int TILE = kFilterTile;
    static_assert(TILE % B == 0, "a tile is whole turns of the ring");
    __shared__ __attribute__((aligned(16))) float region[kFilterLanes * kFilterPitch];
    __shared__ __attribute__((aligned(16))) long long where[kFilterLanes][2];
    const int lane = threadIdx.x, order = A.order;
    float* const mine = region + lane * kFilterPitch;
    T* const staged = reinterpret_cast<T*>(mine);
    const In* __restrict__ in = static_cast<const In*>(A.in);
    const C* __restrict__ coeff = static_cast<const C*>(A.coeff);
    for (long long g = blockIdx.x; g < A.nGroups; g += gridDim.x) {
        const FilterGroup G = A.groups[g];
        const LpcSynthRow me = A.rows[G.first + lane];
        const bool framed = me.steps > 0;                          // (a filler, or a row without steps: coefficients +0, none loaded)
        // the lane's frame j is at at(j); only a framed lane forms the address
        const auto at = [&](long long k) { return coeff + (me.coeff + lpc_synth_clamp(k, me.steps)) * A.coeffCols + A.col0; };
        double a[B];
        C an[B];
        float ring[B];
        {
            const C* __restrict__ c0 = framed ? at(0) : nullptr;
            const C* __restrict__ c1 = framed ? at(1) : nullptr;
#pragma unroll
            for (int m = 0; m < B; ++m) {
                a[m] = framed && m < order ? lpc_widen(c0[m]) : 0.0;
                an[m] = framed && m < order ? c1[m] : (C)0;
                ring[m] = 0.0f;
            }
        }
        long long k = 0, turn = lpc_synth_change(1, A.hop, A.phase);      // the unclamped frame, and the sample at which it turns to k + 1
        where[lane][0] = me.sections ? me.dst : -1;
        where[lane][1] = me.outLen;
        const long long width = A.rowStride > 0 ? A.rowStride : G.outMost;
        In next[kFilterLanes];
        filter_load_rows(next, in, me.src, me.len, 0, lane);
        bool zeroed = false;
        for (long long t0 = 0; t0 < width; t0 += TILE) {
            if (t0 < G.outMost) {
                __syncthreads();                                   // the tile before has left the region
#pragma unroll
                for (int q = 0; q < kFilterLanes; ++q) region[q * kFilterPitch + lane] = tile_x(next[q]);
                // the next tile's loads, in flight during the recursion (none where no row of the group reaches it)
                if (t0 + TILE < G.inMost) filter_load_rows(next, in, me.src, me.len, t0 + TILE, lane);
                else {
#pragma unroll
                    for (int q = 0; q < kFilterLanes; ++q) next[q] = (In)0;
                }
                __syncthreads();
                const long long live = me.outLen - t0;             // outputs of the tile inside the lane's row; the rest is padding
                for (int tb = 0; tb < TILE; tb += B) {
#pragma unroll
                    for (int u = 0; u < B; ++u) {                  // sample t0 + tb + u, ring slot u
                        const int t = tb + u;
                        if (t0 + t == turn) {                      // wave-uniform: frame k + 1 from here, frame k + 2 on its way
                            ++k; turn += A.hop;
                            const C* __restrict__ c = framed ? at(k + 1) : nullptr;
#pragma unroll
                            for (int m = 0; m < B; ++m) {
                                if (m < order) {
                                    a[m] = lpc_widen(an[m]);
                                    an[m] = framed ? c[m] : (C)0;
                                }
                            }
                        }
                        const float y = lpc_synth_step<B>(mine[t], a, order, ring, u);
                        ring[u] = y;
                        staged[t] = t < live ? res_value<F32>(y) : (T)0;
                    }
                }
                __syncthreads();
            } else if (!zeroed) {                                  // (padded rows past the group's longest: +0 without arithmetic)
                __syncthreads();
                for (int t = 0; t < TILE; ++t) mine[t] = 0.0f;
                zeroed = true;
                __syncthreads();
            }
            filter_store_rows<T>(A.out, where, A.rowStride, t0, region, lane);
        }
        __syncthreads();                                           // the last tile has left before the next group's first
    }
}

}  // namespace klatt
#endif
