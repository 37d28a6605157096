// klatt_tiles.h -- the tile walk, the row reader and the row writer of the exports derived from a batch's PCM or from a caller's signal
// (klatt_resample.h, klatt_convolve.h, klatt_mix.h; klatt_spectrum.h takes the reader's sample).  The functions marked KLATT_RES_HD are
// compiled for the host (plain C++17, no HIP) and for the device from the same source; tests/native/check_tiles.cpp and check_signal.cpp
// hold them to brute force under the sanitizers.
//   The walk     One row per chosen utterance; a 256-lane workgroup takes tiles of `tile` consecutive outputs of one row.  Padded
//                (rowStride > 0): every row has rowStride elements and tile_count(rowStride) tiles, tile g is tile_row's (r, j).  Packed
//                (rowStride 0): a row has its outputs and their tiles -- none where it has none --, the row table counts TILES
//                (klatt_export.h: tile_row_table) and tile_locate bisects it within the chunk table's bounds.  The tile at output t0
//                holds tile_n elements, of which the first tile_live lie inside the row; the rest is padding, stored as +0.
//   The reader   A row is `len` samples from a pointer, int16 or float32 (the pool's utterances; a signal's rows: signal_plan).  tile_sample
//                is sample s of it as float32 -- (float)s / 32767.0f of an int16, a float32 as it is -- and +0 for every s outside
//                0 .. len-1: the mask decides whether the address is formed at all, so what lies either side of a row -- a padded row's
//                remainder, the next row, a guard -- is never loaded, and no sample's VALUE ever reaches an address.  A run is `count`
//                staged values, element i standing for sample tile_source<DIR>(s0, i): upwards (the resampler's span) or downwards (the
//                convolution's reversed inputs).  tile_read holds NO barrier.  Lane i loads element i, i + 256, ...: consecutive lanes
//                load consecutive elements, 128 or 256 contiguous bytes per wavefront, whatever the row's first element is.
//   The writer   `count` values staged in LDS in the output's type go to the elements e0 .. e0 + count - 1.  Lane i owns the i-th
//                ALIGNED 16 bytes the run touches -- by ADDRESS: `mis` is what out[0] lies past a 16-byte boundary, so a buffer aligned
//                to the element only still gets 16-byte stores -- and stores them at once where the run covers them all; the run's
//                two ends, which share their 16 bytes with the neighbouring run or row, go element by element.  tile_store holds NO
//                barrier: the caller stages the values before it and keeps `staged` until all lanes have left it.
#pragma once

#include <stdint.h>
#include <type_traits>

#if defined(__HIPCC__)
#define KLATT_RES_HD __host__ __device__ __forceinline__
#else
#define KLATT_RES_HD inline
#endif

namespace klatt {

// Where a tile-wise kernel finds its tiles and its output
struct TileOut {
    const long long *start, *chunk;      // the packed form's row table over TILES (rowStride 0)
    long long rowStride, tilesPerRow;    // the padded form: a row's width and its tiles
    long long nTiles;                    // of the launch
    void* out;
};
template <bool F32> using TileValue = typename std::conditional<F32, float, int16_t>::type;      // format 1 float32, format 0 int16
template <typename T> constexpr int kTileLane = 16 / (int)sizeof(T);                             // elements of 16 bytes

// ---- the walk ----------------------------------------------------------------------------------------------------------------------------
KLATT_RES_HD long long tile_count(long long width, int tile) { return (width + tile - 1) / tile; }
// Tile g of the padded form: row r, tile j of the row
KLATT_RES_HD void tile_row(long long g, long long tilesPerRow, long long& r, long long& j) { r = g / tilesPerRow; j = g - r * tilesPerRow; }
// The elements of the tile at t0 of a row of outLen outputs, rowStride elements wide where padded
KLATT_RES_HD int tile_n(long long rowStride, long long outLen, long long t0, int tile) { const long long left = (rowStride > 0 ? rowStride : outLen) - t0; return (int)(left < tile ? left : tile); }
// Of the n elements from output t0, those inside the row; the rest is padding
KLATT_RES_HD int tile_live(int n, long long outLen, long long t0) { const long long left = outLen - t0; return (int)(left < n ? (left > 0 ? left : 0) : n); }

// ---- the locators (tests/native/check_locate.cpp) --------------------------------------------------------------------------------------------
constexpr int kTimelineChunkLog2 = 15;      // steps per chunk of the packed form's row table

// The row of entry g of a packed output and the entry's place in it: the last row among [lo, hi) whose start is <= g.
KLATT_RES_HD void packed_locate(long long g, const long long* __restrict__ start, long long lo, long long hi, long long& r, long long& j)
{
    while (hi - lo > 1) { const long long mid = (lo + hi) >> 1; if (start[mid] <= g) lo = mid; else hi = mid; }
    r = lo; j = g - start[r];
}
KLATT_RES_HD void packed_locate(long long g, const long long* __restrict__ start, long long nRows, long long& r, long long& j)
{
    packed_locate(g, start, 0, nRows, r, j);
}

// Element e0 of a [row][step][column] output is (r, j, q): g = e0 / nCols is the step's number in the output, the row g / rowStride
// (padded) or by bisection over stepStart within the chunk table's bounds (packed: rowStride 0).  32-bit divisions where they do.
KLATT_RES_HD void dense_locate(long long e0, int nCols, long long rowStride, const long long* __restrict__ stepStart,
                               const long long* __restrict__ chunkRow, long long& g, int& q, long long& r, long long& j)
{
    if (nCols == 1) { g = e0; q = 0; }
    else if ((unsigned long long)e0 >> 32) { g = e0 / nCols; q = (int)(e0 - g * nCols); }
    else { const uint32_t g32 = (uint32_t)e0 / (uint32_t)nCols; g = g32; q = (int)((uint32_t)e0 - g32 * (uint32_t)nCols); }
    if (rowStride > 0) {
        if (((unsigned long long)g | (unsigned long long)rowStride) >> 32) r = g / rowStride;
        else r = (uint32_t)g / (uint32_t)rowStride;
        j = g - r * rowStride;
    } else {
        const long long c = g >> kTimelineChunkLog2;
        packed_locate(g, stepStart, chunkRow[c], chunkRow[c + 1] + 1, r, j);
    }
}

// ---- the reader ----------------------------------------------------------------------------------------------------------------------------
// x of a sample: an int16 as speechPlayer_batch_exportPcm's format 1 gives it, a float32 as it is
KLATT_RES_HD float tile_x(int s) { return (float)s / 32767.0f; }
KLATT_RES_HD float tile_x(float s) { return s; }
KLATT_RES_HD bool tile_inside(long long s, long long len) { return s >= 0 && s < len; }
// Sample s of a row of len samples: +0 outside it, and nothing is loaded there
template <typename In> KLATT_RES_HD float tile_sample(const In* x, long long s, long long len) { return tile_x(tile_inside(s, len) ? x[s] : (In)0); }
// The sample that element i of a run from s0 stands for: DIR 1 upwards, -1 downwards
template <int DIR> KLATT_RES_HD long long tile_source(long long s0, int i) { return s0 + (long long)(DIR * i); }
// Lane `lane` of `lanes`: elements lane, lane + lanes, ... of the run's `count`
template <int DIR, typename In> KLATT_RES_HD void tile_read_lane(float* xs, const In* x, long long len, long long s0, int count, int lane, int lanes)
{
    for (int i = lane; i < count; i += lanes) xs[i] = tile_sample(x, tile_source<DIR>(s0, i), len);
}

// ---- the writer ----------------------------------------------------------------------------------------------------------------------------
// Elements past a 16-byte boundary at out[0]
template <typename T> KLATT_RES_HD int tile_mis(const void* out) { return (int)((reinterpret_cast<uintptr_t>(out) / sizeof(T)) & (kTileLane<T> - 1)); }
// The first element of the aligned 16 bytes that hold element e0
template <typename T> KLATT_RES_HD long long tile_first(int mis, long long e0) { return e0 - ((e0 + mis) & (kTileLane<T> - 1)); }
// The aligned 16 bytes that the elements e0 .. e0 + count - 1 touch: a lane each
template <typename T> KLATT_RES_HD int tile_lanes(int mis, long long e0, int count) { return (int)((e0 + count - tile_first<T>(mis, e0) + kTileLane<T> - 1) / kTileLane<T>); }
// Lane i of the run: staged[0 .. count) are the values of the elements e0 .. e0 + count - 1
template <typename T> KLATT_RES_HD void tile_store_lane(T* out, int mis, long long e0, int count, const T* staged, int i)
{
    constexpr int EL = kTileLane<T>;
    const long long at = tile_first<T>(mis, e0) + (long long)i * EL;
    const int b0 = (int)(at - e0);                          // (negative in the first lane of a run that starts inside its 16 bytes)
    if (b0 >= 0 && b0 + EL <= count) {
        struct alignas(16) Lane { T x[EL]; } l;
        for (int q = 0; q < EL; ++q) l.x[q] = staged[b0 + q];
        *reinterpret_cast<Lane*>(out + at) = l;
    } else {
        for (int q = 0; q < EL; ++q) if (b0 + q >= 0 && b0 + q < count) out[at + q] = staged[b0 + q];
    }
}

}  // namespace klatt

// ---- a caller's signal (speechPlayer_signal_t), as every entry point plans it on the host -----------------------------------------------------
#include <stdio.h>
#include <math.h>
#include <string>

namespace klatt {

constexpr long long kSignalMaxLength = 1ll << 44;      // samples of a row (index products stay in 64 bits)
constexpr long long kSignalMaxElements = 1ll << 60;    // elements of a signal, padded or packed: its bytes stay in 64 bits (need * elSize <= 2^62)
constexpr float kSignalMaxValue = 65536.0f;            // |x| <= 2^16: the bound of the bit-for-bit promise (the noise bank's)

// The rows of a signal: row r is len(r) samples from element at(r); `need` elements hold them all
struct SignalPlan {
    int format = 0, elSize = 2;
    long long nRows = 0, rowStride = 0, need = 0;
    const long long* extent = nullptr;
    long long at(long long r) const { return rowStride > 0 ? r * rowStride : extent[r]; }
    long long len(long long r) const { return rowStride > 0 ? extent[r] : extent[r + 1] - extent[r]; }
};

// The plan of a signal's table, or false with `why` set (without the entry point's prefix): every refusal that needs no device.
inline bool signal_plan(SignalPlan& P, int format, long long nRows, long long rowStride, const long long* extent, std::string& why)
{
    char buf[200];
    if (format != 0 && format != 1) { snprintf(buf, sizeof buf, "signal format %d (0 int16, 1 float32)", format); why = buf; return false; }
    if (nRows < 0) { snprintf(buf, sizeof buf, "signal nRows %lld", nRows); why = buf; return false; }
    if (rowStride < 0) { snprintf(buf, sizeof buf, "signal rowStride %lld", rowStride); why = buf; return false; }
    if (nRows > 0 && !extent) { why = "signal without extent (the rows' lengths or offsets, on the host)"; return false; }
    P.format = format; P.elSize = format ? 4 : 2; P.nRows = nRows; P.rowStride = rowStride; P.extent = extent; P.need = 0;
    if (nRows == 0) return true;
    if (rowStride > 0) {
        if ((unsigned __int128)nRows * (unsigned __int128)rowStride > (unsigned __int128)kSignalMaxElements) {
            snprintf(buf, sizeof buf, "signal of %lld rows of rowStride %lld (at most 2^60 elements)", nRows, rowStride); why = buf; return false;
        }
        for (long long r = 0; r < nRows; ++r) {
            const long long L = extent[r];
            if (L < 0 || L > rowStride) { snprintf(buf, sizeof buf, "signal extent[%lld] = %lld: row %lld has 0 .. rowStride = %lld samples", r, L, r, rowStride); why = buf; return false; }
            if (L > kSignalMaxLength) { snprintf(buf, sizeof buf, "signal extent[%lld] = %lld: row %lld has more than 2^44 samples", r, L, r); why = buf; return false; }
            if (L > 0 && r * rowStride + L > P.need) P.need = r * rowStride + L;
        }
        return true;
    }
    if (extent[0] != 0) { snprintf(buf, sizeof buf, "signal extent[0] = %lld (row 0 of a packed signal starts at 0)", extent[0]); why = buf; return false; }
    for (long long r = 0; r < nRows; ++r) {
        const long long a = extent[r], b = extent[r + 1];
        if (b < a) { snprintf(buf, sizeof buf, "signal extent[%lld] = %lld is below extent[%lld] = %lld: row %lld ends before it starts", r + 1, b, r, a, r); why = buf; return false; }
        if (b - a > kSignalMaxLength) { snprintf(buf, sizeof buf, "signal extent[%lld] = %lld: row %lld has more than 2^44 samples", r + 1, b, r); why = buf; return false; }
        if (b > kSignalMaxElements) {      // (rows of 2^44 samples each may add up to anything: the bytes of `need` must not wrap)
            snprintf(buf, sizeof buf, "signal extent[%lld] = %lld: row %lld ends past 2^60 elements, the most a signal has", r + 1, b, r); why = buf; return false;
        }
    }
    P.need = extent[nRows];
    return true;
}

// The values a host statement takes: finite, at most 2^16 in magnitude; or false with the first other sample in `why`
inline bool signal_values(const float* x, long long length, std::string& why)
{
    for (long long n = 0; n < length; ++n)
        if (!(fabsf(x[n]) <= kSignalMaxValue)) {      // (a NaN fails the comparison)
            char buf[160];
            snprintf(buf, sizeof buf, "sample %lld is %g (finite, at most 2^16 in magnitude)", n, (double)x[n]); why = buf; return false;
        }
    return true;
}

}  // namespace klatt

#if defined(__HIPCC__)      // ---- the device ----

namespace klatt {

// Tile g of the launch: row r, and the tile's first output t0
__device__ __forceinline__ void tile_locate(const TileOut& O, long long g, int tile, long long& r, long long& t0)
{
    long long j;
    if (O.rowStride > 0) tile_row(g, O.tilesPerRow, r, j);
    else { const long long c = g >> kTimelineChunkLog2; packed_locate(g, O.start, O.chunk[c], O.chunk[c + 1] + 1, r, j); }
    t0 = j * tile;
}

// The workgroup's loads of a run
template <int DIR, typename In> __device__ __forceinline__ void tile_read(float* xs, const In* __restrict__ x, long long len, long long s0, int count, int tid)
{
    tile_read_lane<DIR>(xs, x, len, s0, count, tid, 256);
}

// The workgroup's stores of a run
template <typename T> __device__ __forceinline__ void tile_store(void* out, long long e0, int count, const T* staged, int tid)
{
    const int mis = tile_mis<T>(out), lanes = tile_lanes<T>(mis, e0, count);
    for (int i = tid; i < lanes; i += 256) tile_store_lane(static_cast<T*>(out), mis, e0, count, staged, i);
}

}  // namespace klatt
#endif
