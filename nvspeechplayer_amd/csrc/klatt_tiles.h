// klatt_tiles.h -- the tile walk and the row writer of the exports derived from a batch's PCM (klatt_resample.h, klatt_convolve.h,
// klatt_mix.h).  The functions marked KLATT_RES_HD are compiled for the host (plain C++17, no HIP) and for the device from the same
// source; tests/native/check_tiles.cpp holds them to brute force under the sanitizers.
//   The walk     One row per chosen utterance; a 256-lane workgroup takes tiles of `tile` consecutive outputs of one row.  Padded
//                (rowStride > 0): every row has rowStride elements and tile_count(rowStride) tiles, tile g is tile_row's (r, j).  Packed
//                (rowStride 0): a row has its outputs and their tiles -- none where it has none --, the row table counts TILES
//                (klatt_export.h: tile_row_table) and tile_locate bisects it within the chunk table's bounds.  The tile at output t0
//                holds tile_n elements, of which the first tile_live lie inside the row; the rest is padding, stored as +0.
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

#if defined(__HIPCC__)      // ---- the device ----
#include "klatt_timeline.h"

namespace klatt {

// Tile g of the launch: row r, and the tile's first output t0
__device__ __forceinline__ void tile_locate(const TileOut& O, long long g, int tile, long long& r, long long& t0)
{
    long long j;
    if (O.rowStride > 0) tile_row(g, O.tilesPerRow, r, j);
    else { const long long c = g >> kTimelineChunkLog2; packed_locate(g, O.start, O.chunk[c], O.chunk[c + 1] + 1, r, j); }
    t0 = j * tile;
}

// The workgroup's stores of a run
template <typename T> __device__ __forceinline__ void tile_store(void* out, long long e0, int count, const T* staged, int tid)
{
    const int mis = tile_mis<T>(out), lanes = tile_lanes<T>(mis, e0, count);
    for (int i = tid; i < lanes; i += 256) tile_store_lane(static_cast<T*>(out), mis, e0, count, staged, i);
}

}  // namespace klatt
#endif
