// klatt_resample.h -- a batch's PCM at another sample rate (speechPlayer_batch_exportResampled) and plain PCM resampled on the host
// (speechPlayer_pcmResample, speechPlayer_resampleKernel, speechPlayer_resampledLength).
//
// The definition is in include/speechPlayer_batch.h; this header is its one statement in code.  The functions marked KLATT_RES_HD are
// compiled for the host and for the device from the same source, with -ffp-contract=off: the input conversion, every product and
// every sum of the tap loop and the int16 conversion are separately rounded float32 operations on both sides (there is no fmaf
// anywhere), and the table is evaluated once, in binary64 on the host, and rounded to float32 for both.
//
//   The plan        res_plan: the ratio up / down, the cut-off c, the half-width Wd, Z = ceil(Wd), taps = 2 Z, the refusals and the table
//                   h[p][k] = c sinc(c t) w(t), t = (k - Z + 1) - p / up.  taps <= 1024 bounds the ratio as well: Z >= Wd >= down / up,
//                   so down <= 512 up <= 2^21, which is what lets the kernel count in 32 bits inside a tile.
//   The statement   resample_host: for every output m, res_locate gives n0 = floor(m down / up) and p = (m down) mod up, the taps'
//                   inputs are res_input of the samples n0 - Z + 1 .. n0 + Z (+0 outside the signal), res_taps sums them against row p
//                   in ascending k from +0, and res_int16 makes format 0.
//   klatt_resample  A 256-lane workgroup takes tiles of kResampleTile consecutive outputs of one row, a tile in spans whose inputs fit
//                   kResampleIn floats of LDS ((span - 1) down / up + 1 + taps <= kResampleIn: the whole tile wherever down / up < 6.9).
//                   Per span: the inputs n0(first) - Z + 1 .. n0(last) + Z are loaded once, masked by 0 <= n < Lin and converted, by the
//                   reader (klatt_tiles.h: tile_read, from int16 or float32) into LDS; lane i takes outputs i, i + 256, ... of the span, so consecutive lanes read LDS at stride
//                   down / up (conflict-free below 2, two-way at 2) and the table at consecutive addresses: it is uploaded reordered
//                   by use and transposed, hT[k][m mod up] = h[(m down) mod up][k] (phase has period `up` in m), 230 KB in the
//                   largest tested case and L2-resident.  The reordering moves data, not arithmetic.  The tiles are walked and the
//                   values written as klatt_tiles.h says, a span being a run of the writer: staged in LDS in the output's type, a
//                   padded row's tail as +0.
//   One body        The kernel is resample_rows<KEPT = false>: the loop is written once, and klatt_resample is the entry point that hands it
//                   the reader above.  A row fed chunk by chunk keeps 2 Z - 1 samples of history between calls (klatt_stage.h):
//                   klatt_stage_resample is the other entry point, resample_rows<KEPT = true> with the reader of the virtual row
//                   [history | chunk | +0] and a span's first output counted from the row's start.  Behind `if constexpr (KEPT)` is that
//                   one addition; with KEPT false nothing of a stage exists in the code.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "klatt_tiles.h"

namespace klatt {

constexpr int kResampleTile = 1024;          // consecutive outputs of one row a workgroup takes at a time (a power of two, at most 4096)
constexpr int kResampleIn = 8192;            // floats of LDS for a span's inputs
constexpr int kResampleMaxUp = 4096, kResampleMaxTaps = 1024;
constexpr long long kResampleMaxTable = 1ll << 20;
constexpr long long kResampleMaxLength = 1ll << 44;      // samples of plain PCM the host statement takes (index products stay in 64 bits)

// x[n]: the sample as speechPlayer_batch_exportPcm's format 1 gives it (klatt_tiles.h: the reader's conversion)
KLATT_RES_HD float res_input(int s) { return tile_x(s); }

// Output m reads inputs n0 - Z + 1 .. n0 + Z against row p of the table
KLATT_RES_HD void res_locate(long long m, int up, int down, long long& n0, int& p)
{
    const long long a = m * (long long)down;
    n0 = a / up;
    p = (int)(a - n0 * up);
}

// sum over k ascending, from +0, of x[k] h[k * hStride]: one float32 product and one float32 sum per term
KLATT_RES_HD float res_taps(const float* x, const float* h, int taps, int hStride)
{
    float acc = 0.0f;
#if defined(__clang__)
#pragma unroll 4
#endif
    for (int k = 0; k < taps; ++k) acc = acc + x[k] * h[(size_t)k * hStride];      // (unrolling hoists the loads; the sums keep their order)
    return acc;
}

// format 0: one float32 product, clipped, rounded to nearest even
KLATT_RES_HD int16_t res_int16(float y)
{
    const float q = y * 32767.0f;
    if (q >= 32767.0f) return (int16_t)32767;
    if (q <= -32768.0f) return (int16_t)-32768;
    return (int16_t)rintf(q);
}

// A finished sum in the output's type
template <bool F32> KLATT_RES_HD TileValue<F32> res_value(float y) { if (F32) return (TileValue<F32>)y; return (TileValue<F32>)res_int16(y); }
// The same into output m of a host statement: format 1 float[], format 0 int16_t[]
inline void res_store(void* out, int format, long long m, float y) { if (format) static_cast<float*>(out)[m] = y; else static_cast<int16_t*>(out)[m] = res_int16(y); }

// ---- the request, as every entry point plans it on the host -----------------------------------------------------------------------------
inline long long res_gcd(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }

// ceil(length * up / down), 0 for length 0 (length >= 0, up and down positive)
inline long long res_length(long long length, long long up, long long down)
{
    const unsigned __int128 a = (unsigned __int128)length * (unsigned __int128)up + (unsigned __int128)(down - 1);
    const unsigned __int128 q = a / (unsigned __int128)down;
    return q > (unsigned __int128)0x7FFFFFFFFFFFFFFFll ? 0x7FFFFFFFFFFFFFFFll : (long long)q;
}

// I0 by its power series, sum of ((x / 2)^2)^k / (k!)^2, in binary64
inline double res_bessel_i0(double x)
{
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 1000; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

struct ResPlan {
    int srcRate = 0, dstRate = 0, zeros = 0, window = 0;
    double rolloff = 0.0, beta = 0.0;
    int up = 0, down = 0, Z = 0, taps = 0;
    bool identity = false;           // equal rates: no filtering
    std::vector<float> table;        // [up][taps]
    std::vector<float> hT;           // [taps][up], column j holding row (j down) mod up: what the kernel reads (made by res_transpose)
    bool same(int s, int d, int z, double r, int w, double b) const
    {
        return up > 0 && s == srcRate && d == dstRate && z == zeros && r == rolloff && w == window && (w == 0 || b == beta);
    }
};

// The plan of a request, or false with `why` set (without the entry point's prefix).
inline bool res_plan(ResPlan& P, int srcRate, int dstRate, int zeros, double rolloff, int window, double beta, std::string& why)
{
    char buf[200];
    if (srcRate <= 0 || dstRate <= 0) { snprintf(buf, sizeof buf, "sample rates %d and %d (both above 0)", srcRate, dstRate); why = buf; return false; }
    if (zeros < 1) { snprintf(buf, sizeof buf, "zeros %d (at least 1)", zeros); why = buf; return false; }
    if (!std::isfinite(rolloff) || !(rolloff > 0.0) || rolloff > 1.0) { snprintf(buf, sizeof buf, "rolloff %g (in (0, 1])", rolloff); why = buf; return false; }
    if (window != 0 && window != 1) { snprintf(buf, sizeof buf, "window %d (0 Hann, 1 Kaiser)", window); why = buf; return false; }
    if (window == 1 && (!std::isfinite(beta) || beta < 0.0)) { snprintf(buf, sizeof buf, "Kaiser beta %g (finite, not negative)", beta); why = buf; return false; }
    const long long g = res_gcd(srcRate, dstRate), up = dstRate / g, down = srcRate / g;
    if (up > kResampleMaxUp) { snprintf(buf, sizeof buf, "%d to %d Hz is the ratio %lld / %lld: up is above %d", srcRate, dstRate, up, down, kResampleMaxUp); why = buf; return false; }
    const double c = rolloff * (up < down ? (double)up / (double)down : 1.0);
    const double Wd = (double)zeros / c;
    if (!(Wd <= (double)(kResampleMaxTaps / 2))) {
        snprintf(buf, sizeof buf, "zeros %d at the ratio %lld / %lld takes more than %d taps", zeros, up, down, kResampleMaxTaps); why = buf; return false;
    }
    const int Z = (int)ceil(Wd), taps = 2 * Z;
    if (up * taps > kResampleMaxTable) {
        snprintf(buf, sizeof buf, "a table of %lld phases of %d taps is above %lld values", up, taps, kResampleMaxTable); why = buf; return false;
    }
    P.srcRate = srcRate; P.dstRate = dstRate; P.zeros = zeros; P.window = window; P.rolloff = rolloff; P.beta = window == 1 ? beta : 0.0;
    P.up = (int)up; P.down = (int)down; P.Z = Z; P.taps = taps;
    P.identity = srcRate == dstRate;
    P.table.resize((size_t)up * taps);
    P.hT.clear();
    const double pi = 3.141592653589793;
    const double i0b = window == 1 ? res_bessel_i0(beta) : 1.0;
    for (int p = 0; p < (int)up; ++p)
        for (int k = 0; k < taps; ++k) {
            const double t = (double)(k - Z + 1) - (double)p / (double)up;
            double w = 0.0;
            if (fabs(t) < Wd) {
                if (window == 0) { const double cw = cos(pi * t / (2.0 * Wd)); w = cw * cw; }
                else { const double r = t / Wd; w = res_bessel_i0(beta * sqrt(1.0 - r * r)) / i0b; }
            }
            const double x = pi * (c * t);
            const double sinc = x == 0.0 ? 1.0 : sin(x) / x;
            P.table[(size_t)p * taps + k] = (float)(c * sinc * w);
        }
    return true;
}

// The table as the kernel reads it: hT[k][j] = h[(j down) mod up][k]
inline void res_transpose(ResPlan& P)
{
    if (!P.hT.empty()) return;
    P.hT.resize(P.table.size());
    for (int j = 0; j < P.up; ++j) {
        const int p = (int)(((long long)j * P.down) % P.up);
        for (int k = 0; k < P.taps; ++k) P.hT[(size_t)k * P.up + j] = P.table[(size_t)p * P.taps + k];
    }
}

// ---- the host's statement (speechPlayer_pcmResample): the shared functions in a plain loop ------------------------------------------------
// format 1: out is float[Lout]; format 0: int16_t[Lout].  Returns Lout.  In: int16_t (PCM) or float (a signal's samples).
// Equal rates: y[m] = x[m], and format 0 of an int16 is the sample itself (res_int16(tile_x(s)) == s for all 65 536 values).
template <typename In>
inline long long resample_host(const In* pcm, long long length, const ResPlan& P, int format, void* out)
{
    const long long Lout = res_length(length, P.up, P.down);
    if (P.identity) {
        for (long long m = 0; m < Lout; ++m) res_store(out, format, m, tile_x(pcm[m]));
        return Lout;
    }
    std::vector<float> x((size_t)P.taps);
    for (long long m = 0; m < Lout; ++m) {
        long long n0; int p;
        res_locate(m, P.up, P.down, n0, p);
        for (int k = 0; k < P.taps; ++k) {
            const long long n = n0 + k - P.Z + 1;
            x[(size_t)k] = tile_sample(pcm, n, length);
        }
        const float y = res_taps(x.data(), P.table.data() + (size_t)p * P.taps, P.taps, 1);
        res_store(out, format, m, y);
    }
    return Lout;
}

// Outputs of a tile whose inputs fit the kernel's LDS at once: the largest span with (span - 1) down / up + 1 + taps <= kResampleIn
inline int res_span(const ResPlan& P)
{
    const long long s = (long long)(kResampleIn - P.taps - 1) * P.up / P.down + 1;
    return (int)(s < kResampleTile ? s : kResampleTile);
}

}  // namespace klatt

// ---- the device ---------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
namespace klatt {

struct ResRow { long long src, len, outLen, dst; };      // first element and samples of a row's input (the pool's utterance, a signal's row); its outputs; its first element in the output

struct ResArgs {
    const void* in;                      // the pool, or a signal's data: int16_t or float, as the kernel's In says
    const ResRow* rows;
    TileOut tile;
    const float* hT;                     // [taps][up]
    int up, down, Z, span;
};

static_assert((kResampleTile & (kResampleTile - 1)) == 0 && kResampleTile <= 4096, "kResampleTile is a power of two, at most 4096");
static_assert(kResampleIn >= kResampleMaxTaps + 1 + kResampleMaxTaps / 2, "a span of one output fits at the largest ratio and filter");

// The one body of klatt_resample and of klatt_stage_resample (klatt_stage.h).  KEPT: the launch carries a row's state from push to push --
// A.rows are StageResRow, a span's first output is output row.M + e0 of the row's stream, and `read` fills LDS from the virtual row.
// read(xin, x, r, row, first, count, tid): samples first .. first + count - 1 of row r's stream into xin, +0 where the stream has none; x is
// the first of the row's samples in this call (the whole row's, or the chunk's).
template <bool KEPT, bool F32, typename In, class Args, class Read>
__device__ __forceinline__ void resample_rows(const Args& A, Read read)
{
    using T = TileValue<F32>;
    __shared__ float xin[kResampleIn];
    __shared__ __attribute__((aligned(16))) T staged[kResampleTile];
    const int tid = threadIdx.x;
    const int up = A.up, down = A.down, Z = A.Z, taps = 2 * Z;
    for (long long g = blockIdx.x; g < A.tile.nTiles; g += gridDim.x) {
        long long r, t0;
        tile_locate(A.tile, g, kResampleTile, r, t0);
        const auto row = A.rows[r];
        const int n = tile_n(A.tile.rowStride, row.outLen, t0, kResampleTile);
        const In* __restrict__ x = static_cast<const In*>(A.in) + row.src;
        for (int c0 = 0; c0 < n; c0 += A.span) {
            const int cn = min(A.span, n - c0);
            const long long e0 = t0 + c0;                        // the span's first output: of this call ...
            long long m0 = e0;                                   // ... and of the row
            if constexpr (KEPT) m0 += row.M;
            const int live = tile_live(cn, row.outLen, e0);      // outputs of the span inside the row's; the rest is padding
            long long nA = 0; int pA = 0;
            if (live > 0) {
                // ---- the span's inputs, once ----
                long long nB; int pB;
                res_locate(m0, up, down, nA, pA);
                res_locate(m0 + live - 1, up, down, nB, pB);
                read(xin, x, r, row, nA - Z + 1, (int)(nB - nA) + taps, tid);
            }
            __syncthreads();
            // ---- the outputs: lane i takes i, i + 256, ... ----
            const uint32_t jA = (uint32_t)(m0 % up);
            for (int i = tid; i < cn; i += 256) {
                T v = (T)0;
                if (i < live) {
                    const uint32_t a = (uint32_t)pA + (uint32_t)i * (uint32_t)down;      // (below 2^12 + 2^10 2^21)
                    const uint32_t col = (jA + (uint32_t)i) % (uint32_t)up;
                    const float y = res_taps(xin + a / (uint32_t)up, A.hT + col, taps, up);
                    v = res_value<F32>(y);
                }
                staged[i] = v;
            }
            __syncthreads();
            tile_store<T>(A.tile.out, row.dst + e0, cn, staged, tid);
            // (the next span's loads and values are behind its own barriers: every lane has read `staged` before any lane passes the first)
        }
    }
}

template <bool F32, typename In = int16_t>
__global__ void __launch_bounds__(256) klatt_resample(const ResArgs A)
{
    resample_rows<false, F32, In>(A, [](float* xin, const In* __restrict__ pcm, long long, const ResRow& row, long long first, int count, int tid) {
        tile_read<1>(xin, pcm, row.len, first, count, tid);
    });
}

// Equal rates of a signal: y[m] = x[m] in the output's type, tile by tile: the reader's sample into the writer's staging
template <bool F32, typename In>
__global__ void __launch_bounds__(256) klatt_signal_copy(const ResArgs A)
{
    using T = TileValue<F32>;
    __shared__ __attribute__((aligned(16))) T staged[kResampleTile];
    const int tid = threadIdx.x;
    for (long long g = blockIdx.x; g < A.tile.nTiles; g += gridDim.x) {
        long long r, t0;
        tile_locate(A.tile, g, kResampleTile, r, t0);
        const ResRow row = A.rows[r];
        const int n = tile_n(A.tile.rowStride, row.outLen, t0, kResampleTile);
        const In* __restrict__ x = static_cast<const In*>(A.in) + row.src;
        for (int i = tid; i < n; i += 256) staged[i] = res_value<F32>(tile_sample(x, tile_source<1>(t0, i), row.len));      // (past the row: +0, the padding)
        __syncthreads();
        tile_store<T>(A.tile.out, row.dst + t0, n, staged, tid);
        __syncthreads();      // every lane has read `staged` before the next tile's values
    }
}

}  // namespace klatt
#endif
