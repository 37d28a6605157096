// klatt_tempo.h -- a batch's PCM, or a signal's rows, at another tempo by waveform-similarity overlap-add (WSOLA), with the time map
// (speechPlayer_batch_exportTempoPositions, speechPlayer_batch_exportTempo; speechPlayer_pcmTempo, signalTempo, tempoLength, tempoFrames).
//
// The definition is in include/speechPlayer_batch.h; the function bodies below are its one statement in code.  The functions marked
// KLATT_RES_HD are compiled for the host (plain C++17, no HIP) and for the device from the same source, with -ffp-contract=off;
// tests/native/check_tempo.cpp holds both kernels' walks to brute force under the sanitizers.
//
//   Lengths         tempo_out_length: Lout = ceil(L / tempo), one binary64 division (host only); tempo_frames: K = ceil(Lout / Hs) + 1.
//   Positions       p[0] = 0; for k >= 1 the nominal a = floor((k Hs) tempo) (tempo_nominal: one binary64 product, exact floor), the
//                   template T[i] = x(p[k-1] + i), the candidates C_d[i] = x(a - Hs + d + i), d = -D .. D.
//   Score           term(i) = (double)T[i] * (double)C_d[i] is EXACT in binary64 (24 x 24 bits), so tempo_term's fma adds it with one
//                   rounding whichever way it is written.  Four chains c_j, j = i mod 4, each summed in ascending i from +0.0;
//                   score = (c_0 + c_1) + (c_2 + c_3) (tempo_score).  A chain from +0.0 is never -0.0: a term with a zero factor (a
//                   sample outside the row, a silence) changes no bit, so the masked reader's +0 is as good as skipping it.
//   Choice          tempo_better: the greater score, then the lower rank 2|d| - (d < 0) (tempo_rank): the order 0, -1, +1, -2, ...  It is
//                   a TOTAL order on (finite score, rank), ranks being distinct: the best of a set is the same in whatever order a scan
//                   or a butterfly visits it.  That is the whole argument for bit equality of the positions: each score is computed by
//                   ONE lane in the definition's order, and only the choice crosses lanes.
//   Render          y(m) = fmaf(w[Hs + i], x(P[q] + i), w[i] * x(P[q+1] - Hs + i)) + 0.0f with q = m / Hs, i = m - q Hs (tempo_render: one
//                   product, one fused multiply-add, one sum, each correctly rounded in binary32); P = tempo_clamp(p), so that a
//                   caller's positions of any value form no index that wraps.  A position steers an address only behind tile_inside.
//   klatt_tempo_search   One 256-lane workgroup per row, rows longest first.  Per frame: T and the N + 2 D values of the search region
//                   go to LDS through tile_read (masked, coalesced); lane t scores the lags t, t + 256, ... -- consecutive lanes read
//                   consecutive LDS words of the region and one broadcast word of T --; the (score, rank) pairs are reduced by
//                   tempo_better with shuffles inside a wavefront and through LDS across the four; lane 0 stores p[k] and hands it
//                   to the next frame through LDS.  LDS: 4 (2048 + 4096) bytes and three small words.
//   klatt_tempo_render   The tile walk of klatt_tiles.h, kTempoTile outputs of one row per tile; the tile's positions, at most
//                   kTempoTilePositions, are clamped into LDS; a lane takes one output per pass -- both of its samples are loaded by the
//                   masked reader, consecutive lanes at consecutive addresses -- and the values leave through tile_store.
// Out of scope: normalised cross-correlation; custom windows or hops other than N / 2; phase-vocoder and PSOLA methods; pitch shifting
// (this export followed by the resampler does it); warping label grids on the device (tempoMap of the binding does it on the host);
// live handles; NodePlayer beyond speechPlayer_node_part; filling the chip with few rows -- a row's frames are sequential.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "klatt_tiles.h"
#include "klatt_resample.h"

namespace klatt {

constexpr int kTempoMinWin = 64, kTempoMaxWin = 2048;      // nWin: even
constexpr int kTempoMaxSearch = 1024;                      // search: lags -D .. D
constexpr int kTempoTile = 1024;                           // consecutive outputs of one row a workgroup of the render takes at a time
constexpr int kTempoTilePositions = kTempoTile / (kTempoMinWin / 2) + 2;      // positions a tile reads, at most
constexpr double kTempoMin = 0.25, kTempoMax = 4.0;
constexpr long long kTempoClamp = 1ll << 45;               // |P| of the render

// ---- the shared statements -------------------------------------------------------------------------------------------------------------
// The nominal input sample of frame k: floor((k Hs) tempo), one binary64 product
KLATT_RES_HD long long tempo_nominal(long long k, int Hs, double tempo) { return (long long)floor((double)(k * (long long)Hs) * tempo); }
// 0, -1, +1, -2, +2, ... are ranks 0, 1, 2, 3, 4, ...
KLATT_RES_HD int tempo_rank(int d) { return d < 0 ? -2 * d - 1 : 2 * d; }
KLATT_RES_HD long long tempo_lag(int rank) { return (rank & 1) ? -(((long long)rank + 1) >> 1) : (long long)(rank >> 1); }
KLATT_RES_HD double tempo_term(float t, float c, double acc) { return fma((double)t, (double)c, acc); }
// Four chains over i mod 4, each ascending from +0.0; N is even
KLATT_RES_HD double tempo_score(const float* T, const float* C, int N)
{
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
    int i = 0;
    for (; i + 4 <= N; i += 4) {
        c0 = tempo_term(T[i], C[i], c0);
        c1 = tempo_term(T[i + 1], C[i + 1], c1);
        c2 = tempo_term(T[i + 2], C[i + 2], c2);
        c3 = tempo_term(T[i + 3], C[i + 3], c3);
    }
    if (i < N) {      // (N mod 4 == 2)
        c0 = tempo_term(T[i], C[i], c0);
        c1 = tempo_term(T[i + 1], C[i + 1], c1);
    }
    return (c0 + c1) + (c2 + c3);
}
// Whether candidate (s, r) is chosen before (bestS, bestR): the greater score, then the lower rank
KLATT_RES_HD bool tempo_better(double s, int r, double bestS, int bestR) { return s > bestS || (s == bestS && r < bestR); }
KLATT_RES_HD long long tempo_clamp(long long p) { return p < -kTempoClamp ? -kTempoClamp : (p > kTempoClamp ? kTempoClamp : p); }
// wHi = w[Hs + i] weighs the segment that fades out, wLo = w[i] the one that fades in
KLATT_RES_HD float tempo_render(float wHi, float xHi, float wLo, float xLo) { return __builtin_fmaf(wHi, xHi, wLo * xLo) + 0.0f; }
// The candidate nobody has scored yet: every finite score is better
constexpr int kTempoNoRank = 0x7FFFFFFF;
KLATT_RES_HD double tempo_no_score() { return -HUGE_VAL; }

// ---- the request, as every entry point plans it on the host ---------------------------------------------------------------------------------
inline bool tempo_valid(double tempo) { return std::isfinite(tempo) && tempo >= kTempoMin && tempo <= kTempoMax; }
// Lout = ceil(L / tempo): one binary64 division (L >= 0, tempo valid)
inline long long tempo_out_length(long long L, double tempo) { return L > 0 ? (long long)ceil((double)L / tempo) : 0; }
inline long long tempo_frames(long long Lout, int Hs) { return Lout > 0 ? (Lout + Hs - 1) / Hs + 1 : 0; }

// The tempo of output row i of a HOST array, or false with `why` set
inline bool tempo_of_row(const double* tempo, long long i, std::string& why)
{
    char buf[160];
    if (!tempo) { why = "no tempo (a HOST array, one double per output row)"; return false; }
    if (!tempo_valid(tempo[i])) { snprintf(buf, sizeof buf, "tempo[%lld] = %g: row %lld takes a finite tempo in 0.25 .. 4", i, tempo[i], i); why = buf; return false; }
    return true;
}

struct TempoPlan {
    int nWin = 0, Hs = 0, search = 0;
    std::vector<float> window;      // [nWin]
};

// The plan of a request, or false with `why` set (without the entry point's prefix).  search < 0: the request renders only.
inline bool tempo_plan(TempoPlan& P, int nWin, int search, bool searches, std::string& why)
{
    char buf[160];
    if (nWin < kTempoMinWin || nWin > kTempoMaxWin || (nWin & 1)) {
        snprintf(buf, sizeof buf, "nWin %d (even, %d .. %d)", nWin, kTempoMinWin, kTempoMaxWin); why = buf; return false;
    }
    if (searches && (search < 0 || search > kTempoMaxSearch)) { snprintf(buf, sizeof buf, "search %d (0 .. %d)", search, kTempoMaxSearch); why = buf; return false; }
    P.nWin = nWin; P.Hs = nWin / 2; P.search = searches ? search : 0;
    P.window.resize((size_t)nWin);
    const double pi = 3.141592653589793;
    for (int i = 0; i < nWin; ++i) P.window[(size_t)i] = (float)(0.5 - 0.5 * cos(2.0 * pi * (double)i / (double)nWin));
    return true;
}

// ---- the host's statements: the shared functions in plain loops -----------------------------------------------------------------------------
// p[0 .. K): the positions of a row of L samples
template <typename In>
inline void tempo_positions_host(const In* x, long long L, const TempoPlan& P, double tempo, long long K, long long* p)
{
    const int N = P.nWin, Hs = P.Hs, D = P.search;
    std::vector<float> T((size_t)N), R((size_t)N + 2 * (size_t)D);
    if (K > 0) p[0] = 0;
    for (long long k = 1; k < K; ++k) {
        const long long a = tempo_nominal(k, Hs, tempo);
        tile_read_lane<1>(T.data(), x, L, p[k - 1], N, 0, 1);
        tile_read_lane<1>(R.data(), x, L, a - Hs - D, N + 2 * D, 0, 1);
        double best = tempo_no_score();
        int bestRank = kTempoNoRank;
        for (int j = 0; j <= 2 * D; ++j) {
            const double s = tempo_score(T.data(), R.data() + j, N);
            const int r = tempo_rank(j - D);
            if (tempo_better(s, r, best, bestRank)) { best = s; bestRank = r; }
        }
        p[k] = a + tempo_lag(bestRank);
    }
}

// y[0 .. Lout) from the positions p[0 .. K): format 1 float[], format 0 int16_t[]
template <typename In>
inline void tempo_render_host(const In* x, long long L, const TempoPlan& P, long long Lout, const long long* p, int format, void* out)
{
    const int Hs = P.Hs;
    const float* w = P.window.data();
    for (long long m = 0; m < Lout; ++m) {
        const long long q = m / Hs;
        const int i = (int)(m - q * Hs);
        const long long pa = tempo_clamp(p[q]), pb = tempo_clamp(p[q + 1]);
        res_store(out, format, m, tempo_render(w[Hs + i], tile_sample(x, pa + i, L), w[i], tile_sample(x, pb - Hs + i, L)));
    }
}

}  // namespace klatt

// ---- the device ---------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
namespace klatt {

// A row's input (first element, samples), its outputs, its first element in the output, its first FRAME in the positions, its frames, its tempo
struct TempoRow { long long src, len, outLen, dst, pos, frames; double tempo; };

struct TempoSearchArgs {
    const void* in;                      // the pool, or a signal's data: int16_t or float, as the kernel's In says
    const TempoRow* rows;
    const long long* order;              // the rows, longest first
    long long nRows, rowStride;          // rowStride in frames: 0 packed
    int nWin, search;
    long long* pos;
};

template <typename In = int16_t>
__global__ void __launch_bounds__(256) klatt_tempo_search(const TempoSearchArgs A)
{
    __shared__ __attribute__((aligned(16))) float Ts[kTempoMaxWin];
    __shared__ __attribute__((aligned(16))) float Rs[kTempoMaxWin + 2 * kTempoMaxSearch];
    __shared__ double waveScore[4];
    __shared__ int waveRank[4];
    __shared__ long long previous;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = A.nWin, D = A.search, Hs = N / 2, nLags = 2 * D + 1;
    for (long long b = blockIdx.x; b < A.nRows; b += gridDim.x) {
        const TempoRow row = A.rows[A.order[b]];
        long long* __restrict__ p = A.pos + row.pos;
        const long long width = A.rowStride > 0 ? A.rowStride : row.frames;
        for (long long k = row.frames + tid; k < width; k += 256) p[k] = 0;      // a padded row's remainder
        if (row.frames == 0) continue;
        if (tid == 0) { p[0] = 0; previous = 0; }
        const In* __restrict__ x = static_cast<const In*>(A.in) + row.src;
        for (long long k = 1; k < row.frames; ++k) {
            __syncthreads();      // p[k-1] is in `previous`; every lane has left the last frame's T and region
            const long long a = tempo_nominal(k, Hs, row.tempo);
            tile_read<1>(Ts, x, row.len, previous, N, tid);
            tile_read<1>(Rs, x, row.len, a - Hs - D, N + 2 * D, tid);
            __syncthreads();
            double best = tempo_no_score();
            int bestRank = kTempoNoRank;
            for (int j = tid; j < nLags; j += 256) {
                const double s = tempo_score(Ts, Rs + j, N);
                const int r = tempo_rank(j - D);
                if (tempo_better(s, r, best, bestRank)) { best = s; bestRank = r; }
            }
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const double s = __shfl_xor(best, m, 64);
                const int r = __shfl_xor(bestRank, m, 64);
                if (tempo_better(s, r, best, bestRank)) { best = s; bestRank = r; }
            }
            if (lane == 0) { waveScore[wave] = best; waveRank[wave] = bestRank; }
            __syncthreads();
            if (tid == 0) {
                for (int v = 1; v < 4; ++v)
                    if (tempo_better(waveScore[v], waveRank[v], best, bestRank)) { best = waveScore[v]; bestRank = waveRank[v]; }
                const long long pk = a + tempo_lag(bestRank);
                p[k] = pk;
                previous = pk;
            }
        }
        // (the next row's first barrier stands between lane 0's stores here and any other lane's loads)
    }
}

struct TempoArgs {
    const void* in;
    const TempoRow* rows;
    TileOut tile;
    const long long* pos;                // [row][frame], rows at TempoRow.pos
    const float* window;                 // [nWin]
    int nWin;
};

static_assert(kTempoTile % 256 == 0 && kTempoMinWin % 2 == 0, "a lane takes whole passes of a tile");

template <bool F32, typename In = int16_t>
__global__ void __launch_bounds__(256) klatt_tempo_render(const TempoArgs A)
{
    using T = TileValue<F32>;
    __shared__ __attribute__((aligned(16))) T staged[kTempoTile];
    __shared__ long long Ps[kTempoTilePositions];
    const int tid = threadIdx.x, Hs = A.nWin / 2;
    const float* __restrict__ w = A.window;
    for (long long g = blockIdx.x; g < A.tile.nTiles; g += gridDim.x) {
        long long r, t0;
        tile_locate(A.tile, g, kTempoTile, r, t0);
        const TempoRow row = A.rows[r];
        const int n = tile_n(A.tile.rowStride, row.outLen, t0, kTempoTile), live = tile_live(n, row.outLen, t0);
        long long q0 = 0;
        if (live > 0) {
            q0 = t0 / Hs;
            const int count = (int)((t0 + live - 1) / Hs - q0) + 2;      // frames q0 .. q(last) + 1 <= K - 1
            for (int c = tid; c < count && c < kTempoTilePositions; c += 256) Ps[c] = tempo_clamp(A.pos[row.pos + q0 + c]);
        }
        __syncthreads();
        const In* __restrict__ x = static_cast<const In*>(A.in) + row.src;
        const int base = (int)(t0 - q0 * Hs);
        for (int i = tid; i < n; i += 256) {
            T v = (T)0;
            if (i < live) {
                const int local = base + i, q = local / Hs, ii = local - q * Hs;
                v = res_value<F32>(tempo_render(w[Hs + ii], tile_sample(x, Ps[q] + ii, row.len), w[ii], tile_sample(x, Ps[q + 1] - Hs + ii, row.len)));
            }
            staged[i] = v;
        }
        __syncthreads();
        tile_store<T>(A.tile.out, row.dst + t0, n, staged, tid);
        __syncthreads();      // every lane has read the staged values and positions before the next tile's
    }
}

}  // namespace klatt
#endif
