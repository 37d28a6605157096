// klatt_spectrum.h -- the STFT and band (mel) spectrogram of a batch's PCM (speechPlayer_batch_exportSpectrogram) and of plain PCM on the
// host (speechPlayer_pcmSpectrogram).
//
// The definition is in include/speechPlayer_batch.h; this header is its one statement in code.  The functions marked KLATT_SPEC_HD are
// compiled for the host and for the device from the same source, with -ffp-contract=off: every operation is a separately rounded float32
// operation on both (there is no fmaf anywhere), the window, the twiddles and the band weights are rounded to float32 once, on the host,
// for both, and sqrt / the widening to binary64 are IEEE.  Only log10 is a library call whose bits may differ between the two.
//
//   The transform   an nFft-point real DFT as an M = nFft / 2 point complex one of z[m] = xw[2m] + i xw[2m+1]: the input in bit-reversed
//                   order, log2 M radix-2 decimation-in-time passes in place (spec_butterfly_at says which two elements and which
//                   twiddle butterfly b of pass p takes; the M / 2 butterflies of a pass touch disjoint pairs, so their order -- and the
//                   number of lanes that share them -- changes nothing), then one unpacking pass (spec_unpack) for the bins 0 .. M:
//                     X[k] = E[k] + W^k O[k],  E[k] = (Z[k] + conj Z[M-k]) / 2,  O[k] = -i (Z[k] - conj Z[M-k]) / 2,  W = exp(-2 pi i / nFft).
//                   Twiddles: W^k for k = 0 .. M, cos and sin of the C library in binary64 rounded to float32, exact at k = 0, M / 2, M.
//   Its error       (what tests/test_spectrogram_host.py holds it to)  Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2:
//                   a radix-2 transform of t passes with twiddles of relative error mu has ||err||_2 <= t eta ||Z||_2,
//                   eta = mu + gamma_4 (sqrt 2 + mu) < 8 u for correctly rounded twiddles (u = 2^-24).  Here t = log2 nFft - 1, and the
//                   unpacking pass is one more butterfly with a twiddle (two halvings are exact), so it counts as a pass: log2 nFft
//                   passes in all, 8 u log2 nFft; the scaling by 1 / 32767 and the window product add 2 u, inside the 8 u the bound
//                   keeps for them.  ||Z||_2 <= sqrt(nFft) ||xw||_2 as for the full-length transform (Parseval on the even and odd halves).
//                   The constant of the full-length radix-2 transform therefore holds:  B = (8 log2 nFft + 8) u sqrt(nFft) ||xw||_2.
//
//   spec_rows       The one body of klatt_spectrogram and of klatt_stage_spectrogram (klatt_stage_window.h: the spectrogram fed chunk by chunk),
//                   its two entry points: a row's steps, a step's first sample and the sample reader are the entry point's, inlined.
//   klatt_spectrogram   One wavefront per step, four steps (consecutive in the output) per 256-lane workgroup, so that overlapping frames
//                   come from L1/L2.  A wavefront loads its frame's samples, int16 or float32, masked by 0 <= t < L (klatt_tiles.h:
//                   tile_sample), multiplies by the window and
//                   stores z bit-reversed into its own LDS region; the passes and the unpacking run there; v[k] goes to a float array
//                   beside it; one lane per band sums its column range from LDS; the values (after the binary64 log) are staged in LDS
//                   and stored by 16-byte stores where the output is aligned, element by element otherwise.  LDS addresses of z are
//                   XOR-swizzled with the index's top four bits (spec_slot): the bit-reversed store, whose 16-lane groups would fall on
//                   one bank, spreads over sixteen, and the passes keep their (at most two-way) pattern.  The swizzle moves data, not
//                   arithmetic.  LDS per workgroup: 4 (8 (M + 2) + 4 (M + 4)) bytes, 98 KB at nFft 4096, 24 KB at 1024.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "klatt_tiles.h"

#if defined(__HIPCC__)
#define KLATT_SPEC_HD __host__ __device__ __forceinline__
#else
#define KLATT_SPEC_HD inline
#endif

namespace klatt {

constexpr int kSpecMinFft = 64, kSpecMaxFft = 4096;
constexpr int kSpecWaves = 4;              // steps a workgroup takes at a time, one wavefront each

struct SpecCx { float re, im; };

// x[i] w[i]: the sample as the reader gives it (klatt_tiles.h: tile_x, tile_sample), times the window
KLATT_SPEC_HD float spec_windowed(float x, float w) { return x * w; }
KLATT_SPEC_HD float spec_input(int s, float w) { return spec_windowed(tile_x(s), w); }

// m's lowest `bits` bits in reverse order (bits >= 1)
KLATT_SPEC_HD uint32_t spec_reverse(uint32_t m, int bits)
{
    m = ((m & 0x55555555u) << 1) | ((m >> 1) & 0x55555555u);
    m = ((m & 0x33333333u) << 2) | ((m >> 2) & 0x33333333u);
    m = ((m & 0x0F0F0F0Fu) << 4) | ((m >> 4) & 0x0F0F0F0Fu);
    m = ((m & 0x00FF00FFu) << 8) | ((m >> 8) & 0x00FF00FFu);
    m = (m << 16) | (m >> 16);
    return m >> (32 - bits);
}

// Butterfly b (0 .. M / 2 - 1) of pass p (0 .. log2 M - 1) of the nFft = 1 << logN point transform: elements i0 and i1 = i0 + (1 << p), twiddle W^t.
KLATT_SPEC_HD void spec_butterfly_at(uint32_t b, int p, int logN, uint32_t& i0, uint32_t& i1, uint32_t& t)
{
    const uint32_t half = 1u << p, j = b & (half - 1u);
    i0 = ((b >> p) << (p + 1)) + j;
    i1 = i0 + half;
    t = j << (logN - 1 - p);
}

// (a, b) <- (a + w b, a - w b)
KLATT_SPEC_HD void spec_butterfly(SpecCx& a, SpecCx& b, SpecCx w)
{
    const float tr = b.re * w.re - b.im * w.im;
    const float ti = b.re * w.im + b.im * w.re;
    const SpecCx a0 = a;
    a.re = a0.re + tr; a.im = a0.im + ti;
    b.re = a0.re - tr; b.im = a0.im - ti;
}

// Bin k from zk = Z[k mod M], zm = Z[(M - k) mod M] and w = W^k
KLATT_SPEC_HD SpecCx spec_unpack(SpecCx zk, SpecCx zm, SpecCx w)
{
    const float er = (zk.re + zm.re) * 0.5f, ei = (zk.im - zm.im) * 0.5f;
    const float pr = (zk.im + zm.im) * 0.5f, pi = (zm.re - zk.re) * 0.5f;
    SpecCx x;
    x.re = er + (pr * w.re - pi * w.im);
    x.im = ei + (pr * w.im + pi * w.re);
    return x;
}

// power 2: re re + im im; power 1: its binary64 square root, rounded to float32
KLATT_SPEC_HD float spec_value(SpecCx x, int power)
{
    const float p = x.re * x.re + x.im * x.im;
    return power == 2 ? p : (float)sqrt((double)p);
}

// sum of w[k] v[k] over lo <= k <= hi, ascending, from +0 (lo > hi: a band without weights)
KLATT_SPEC_HD float spec_band(const float* w, const float* v, int lo, int hi)
{
    float acc = 0.0f;
    for (int k = lo; k <= hi; ++k) acc = acc + w[k] * v[k];
    return acc;
}

// the output value: linear (logScale == 0), or logScale log10(max(value, floor)) in binary64
KLATT_SPEC_HD double spec_scale(float value, double logScale, double floor)
{
    const double v = (double)value;
    if (logScale == 0.0) return v;
    return logScale * log10(v > floor ? v : floor);
}

// ---- the request, as both entry points plan it on the host ------------------------------------------------------------------------------
struct SpecPlan {
    int nFft = 0, logN = 0, M = 0;
    int nOut = 0;                    // values per step: the bands, or the nFft / 2 + 1 bins
    bool hasBank = false;
    int power = 2;
    double logScale = 0.0, floor = 0.0;
    std::vector<float> window;       // [nFft]
    std::vector<SpecCx> tw;          // [M + 1]
    std::vector<float> weights;      // [nOut][M + 1] with a bank
    std::vector<int> range;          // [nOut][2]: first and last non-zero column (first > last: none)
};

// The plan of a request, or false with `why` set (without the entry point's prefix).
inline bool spec_plan(SpecPlan& P, int nFft, const double* window, const double* bank, int nBands, int power, double logScale, double floor,
                      std::string& why)
{
    char buf[160];
    if (nFft < kSpecMinFft || nFft > kSpecMaxFft || (nFft & (nFft - 1))) {
        snprintf(buf, sizeof buf, "nFft %d (a power of two in %d .. %d)", nFft, kSpecMinFft, kSpecMaxFft); why = buf; return false;
    }
    if (power != 1 && power != 2) { snprintf(buf, sizeof buf, "power %d (1 or 2)", power); why = buf; return false; }
    if (bank && nBands <= 0) { snprintf(buf, sizeof buf, "%d bands", nBands); why = buf; return false; }
    if (!std::isfinite(logScale) || !std::isfinite(floor) || (logScale != 0.0 && !(floor > 0.0))) {
        snprintf(buf, sizeof buf, "logScale %g with floor %g (finite; a floor above 0 with a logScale)", logScale, floor); why = buf; return false;
    }
    P.nFft = nFft; P.M = nFft / 2; P.logN = 0;
    while ((1 << P.logN) < nFft) ++P.logN;
    P.power = power; P.logScale = logScale; P.floor = floor;
    P.hasBank = bank != nullptr;
    P.nOut = bank ? nBands : P.M + 1;
    const int K = P.M + 1;
    P.window.resize((size_t)nFft);
    for (int i = 0; i < nFft; ++i) {
        const double w = window ? window[i] : 0.5 - 0.5 * cos(6.283185307179586 * (double)i / (double)nFft);
        if (!std::isfinite(w)) { snprintf(buf, sizeof buf, "window[%d] is not finite", i); why = buf; return false; }
        P.window[(size_t)i] = (float)w;
    }
    P.tw.resize((size_t)K);
    for (int k = 0; k < K; ++k) {
        const double a = 6.283185307179586 * (double)k / (double)nFft;
        P.tw[(size_t)k] = SpecCx{(float)cos(a), (float)-sin(a)};
    }
    P.tw[0] = SpecCx{1.0f, -0.0f}; P.tw[(size_t)(P.M / 2)] = SpecCx{0.0f, -1.0f}; P.tw[(size_t)P.M] = SpecCx{-1.0f, -0.0f};
    P.weights.clear(); P.range.clear();
    if (bank) {
        P.weights.resize((size_t)nBands * K);
        P.range.resize((size_t)nBands * 2);
        for (int b = 0; b < nBands; ++b) {
            int lo = K, hi = -1;
            for (int k = 0; k < K; ++k) {
                const double w = bank[(size_t)b * K + k];
                if (!std::isfinite(w)) { snprintf(buf, sizeof buf, "bank[%d][%d] is not finite", b, k); why = buf; return false; }
                const float f = (float)w;
                P.weights[(size_t)b * K + k] = f;
                if (f != 0.0f) { lo = lo < k ? lo : k; hi = k; }
            }
            P.range[(size_t)b * 2] = lo; P.range[(size_t)b * 2 + 1] = hi;
        }
    }
    return true;
}

// ---- the host's statement (speechPlayer_pcmSpectrogram): the shared functions in plain loops --------------------------------------------
// out[step][value] of `length` samples; returns steps * P.nOut.  In: int16_t (PCM) or float (a signal's samples).
template <typename In>
inline long long spectrogram_host(const In* pcm, long long length, const SpecPlan& P, long long hop, long long phase, double* out)
{
    const int M = P.M, K = M + 1, logM = P.logN - 1;
    const long long steps = length > phase ? (length - phase + hop - 1) / hop : 0;
    std::vector<SpecCx> z((size_t)M);
    std::vector<float> v((size_t)K);
    for (long long j = 0; j < steps; ++j) {
        const long long t0 = phase + j * hop - M;
        for (int m = 0; m < M; ++m) {
            const long long ta = t0 + 2 * m, tb = ta + 1;
            z[spec_reverse((uint32_t)m, logM)] = SpecCx{spec_windowed(tile_sample(pcm, ta, length), P.window[(size_t)(2 * m)]),
                                                       spec_windowed(tile_sample(pcm, tb, length), P.window[(size_t)(2 * m + 1)])};
        }
        for (int p = 0; p < logM; ++p)
            for (uint32_t b = 0; b < (uint32_t)M / 2; ++b) {
                uint32_t i0, i1, t;
                spec_butterfly_at(b, p, P.logN, i0, i1, t);
                spec_butterfly(z[i0], z[i1], P.tw[t]);
            }
        for (int k = 0; k < K; ++k)
            v[(size_t)k] = spec_value(spec_unpack(z[(size_t)(k & (M - 1))], z[(size_t)((M - k) & (M - 1))], P.tw[(size_t)k]), P.power);
        double* o = out + (size_t)j * P.nOut;
        for (int b = 0; b < P.nOut; ++b) {
            const float value = P.hasBank ? spec_band(P.weights.data() + (size_t)b * K, v.data(), P.range[(size_t)b * 2], P.range[(size_t)b * 2 + 1]) : v[(size_t)b];
            o[b] = spec_scale(value, P.logScale, P.floor);
        }
    }
    return steps * P.nOut;
}

}  // namespace klatt

// ---- the device ---------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "klatt_timeline.h"

namespace klatt {

struct SpecRow { long long src, len, steps; };      // first element, samples and steps of a row's input (the pool's utterance, a signal's row)

struct SpecArgs {
    const void* in;                      // the pool, or a signal's data: int16_t or float, as the kernel's In says
    const SpecRow* rows;
    const long long *start, *chunk;      // the packed form's row table (rowStride 0)
    long long rowStride, nSteps;         // nSteps: the steps of the output, rows x rowStride or the rows' steps together
    long long hop, phase;
    const float* window;
    const SpecCx* tw;
    const float* weights;
    const int* range;
    int logN, nOut, hasBank, power;
    double logScale, floor;
    void* out;
    int vec;                             // the output is 16-byte aligned
};

constexpr int spec_lds_wave(int M) { return 8 * (M + 2) + 4 * (M + 4); }      // a wavefront's region: z (and the staged values), v; a multiple of 16
constexpr int kSpecLdsBudget = kSpecWaves * spec_lds_wave(kSpecMaxFft / 2);

// where element i of z lives: i with its low four bits XORed by its top four (i < M = 1 << logM, logM >= 5)
__device__ __forceinline__ uint32_t spec_slot(uint32_t i, int logM) { return i ^ (i >> (logM - 4)); }

// The one body of klatt_spectrogram and of klatt_stage_spectrogram (klatt_stage_window.h), its two entry points: `rows` is the launch's row
// table, steps(row) the steps of a row in this output, first(row, j) the first sample of its step j's frame, and sample(row, t) sample t
// as the reader gives it -- of the row itself, or of a stage's virtual row.
template <bool F32, class Row, class Steps, class First, class Sample>
__device__ __forceinline__ void spec_rows(const SpecArgs& A, const Row* __restrict__ rows, Steps steps, First first, Sample sample)
{
    using T = typename std::conditional<F32, float, double>::type;
    constexpr int EL = 16 / (int)sizeof(T);
    extern __shared__ __attribute__((aligned(16))) unsigned char spec_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int logM = A.logN - 1, M = 1 << logM, K = M + 1, nOut = A.nOut;
    unsigned char* mine = spec_lds + (size_t)wave * spec_lds_wave(M);
    SpecCx* z = reinterpret_cast<SpecCx*>(mine);
    T* staged = reinterpret_cast<T*>(mine);                                 // `room` values, once z is spent
    const int room = 8 * (M + 2) / (int)sizeof(T);
    float* v = reinterpret_cast<float*>(mine + 8 * (M + 2));
    const long long nGroups = (A.nSteps + kSpecWaves - 1) / kSpecWaves;
    for (long long grp = blockIdx.x; grp < nGroups; grp += gridDim.x) {
        const long long g = grp * kSpecWaves + wave;                         // the step's number in the output
        bool inside = g < A.nSteps, live = false;
        Row row{};
        long long j = 0;
        if (inside) {
            long long r;
            if (A.rowStride > 0) { r = g / A.rowStride; j = g - r * A.rowStride; }
            else { const long long c = g >> kTimelineChunkLog2; packed_locate(g, A.start, A.chunk[c], A.chunk[c + 1] + 1, r, j); }
            row = rows[r];
            live = j < steps(row);
        }
        // ---- the frame, windowed, in bit-reversed order ----
        if (live) {
            const long long t0 = first(row, j);
            for (int m = lane; m < M; m += 64) {      // (a lane takes a PAIR of samples: the reader's sample, not its run)
                const long long ta = t0 + 2 * m, tb = ta + 1;
                const float2 w = reinterpret_cast<const float2*>(A.window)[m];
                z[spec_slot(spec_reverse((uint32_t)m, logM), logM)] = SpecCx{spec_windowed(sample(row, ta), w.x), spec_windowed(sample(row, tb), w.y)};
            }
        }
        // ---- the passes ----
        for (int p = 0; p < logM; ++p) {
            __syncthreads();
            if (live)
                for (uint32_t b = lane; b < (uint32_t)M / 2; b += 64) {
                    uint32_t i0, i1, t;
                    spec_butterfly_at(b, p, A.logN, i0, i1, t);
                    const uint32_t s0 = spec_slot(i0, logM), s1 = spec_slot(i1, logM);
                    SpecCx x = z[s0], y = z[s1];
                    spec_butterfly(x, y, A.tw[t]);
                    z[s0] = x; z[s1] = y;
                }
        }
        __syncthreads();
        // ---- the bins ----
        if (live)
            for (int k = lane; k < K; k += 64)
                v[k] = spec_value(spec_unpack(z[spec_slot((uint32_t)(k & (M - 1)), logM)], z[spec_slot((uint32_t)((M - k) & (M - 1)), logM)], A.tw[k]), A.power);
        __syncthreads();
        // ---- the values of the step (a step past its row's end: zeros), as many at a time as fit where z was ----
        for (int c0 = 0; c0 < nOut; c0 += room) {
            const int n = min(room, nOut - c0);
            if (inside)
                for (int b = lane; b < n; b += 64) {
                    double d = 0.0;
                    if (live) {
                        const int band = c0 + b;
                        const float value = A.hasBank ? spec_band(A.weights + (size_t)band * K, v, A.range[2 * band], A.range[2 * band + 1]) : v[band];
                        d = spec_scale(value, A.logScale, A.floor);
                    }
                    staged[b] = (T)d;
                }
            __syncthreads();
            // the stores: a lane owns an aligned 16 bytes of the output
            if (inside) {
                T* __restrict__ out = static_cast<T*>(A.out);
                const long long e0 = g * nOut + c0, first = e0 - (e0 & (EL - 1));
                const int lanes = (int)((e0 + n - first + EL - 1) / EL);
                for (int i = lane; i < lanes; i += 64) {
                    const long long at = first + (long long)i * EL;
                    const int b0 = (int)(at - e0);                          // (negative in the first lane of a run that starts inside its 16 bytes)
                    if (A.vec && b0 >= 0 && b0 + EL <= n) {
                        struct alignas(16) Lane { T x[EL]; } l;
#pragma unroll
                        for (int q = 0; q < EL; ++q) l.x[q] = staged[b0 + q];
                        *reinterpret_cast<Lane*>(out + at) = l;
                    } else {
#pragma unroll
                        for (int q = 0; q < EL; ++q) if (b0 + q >= 0 && b0 + q < n) out[at + q] = staged[b0 + q];
                    }
                }
            }
            __syncthreads();
        }
    }
}

template <bool F32, typename In = int16_t>
__global__ void __launch_bounds__(64 * kSpecWaves) klatt_spectrogram(const SpecArgs A)
{
    const int M = 1 << (A.logN - 1);
    spec_rows<F32>(A, A.rows, [](const SpecRow& row) { return row.steps; },
                   [&](const SpecRow&, long long j) { return A.phase + j * A.hop - M; },
                   [&](const SpecRow& row, long long t) { return tile_sample(static_cast<const In*>(A.in) + row.src, t, row.len); });
}

}  // namespace klatt
#endif
