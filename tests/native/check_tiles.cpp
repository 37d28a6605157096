// check_tiles.cpp -- the tile walk and the row writer of the PCM-derived exports (nvspeechplayer_amd/csrc/klatt_tiles.h, and tile_row_table
// of klatt_export.h) against brute force.  The writer: every lane of a run is run into a guarded buffer, and what it wrote is found by
// comparing the buffer with its filling, not by restating the writer's index arithmetic.  The walk: every tile of a launch is located
// as the kernels locate it, and the tiles of every row are counted.
// Built with AddressSanitizer + UBSan by tests/test_host_logic.py; prints "ok <checks>" or the first failure.
#include "../../nvspeechplayer_amd/csrc/klatt_export.h"

#include <stdlib.h>

using namespace klatt;

static long long checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

// ---- the writer ----------------------------------------------------------------------------------------------------------------------------
// out[0] lies `mis` elements past a 16-byte boundary; the run is out[e0 .. e0 + count), everything else in the buffer is guard.
template <typename T> static void check_run(std::vector<T>& raw, T* base, int guard, int mis, long long e0, int count)
{
    constexpr int EL = 16 / (int)sizeof(T);
    const T filling = (T)-7;
    T* out = base + guard + mis;
    CHECK(reinterpret_cast<uintptr_t>(out - mis) % 16 == 0 && tile_mis<T>(out) == mis, "out[0] is %d elements past a boundary, tile_mis says %d", mis, tile_mis<T>(out));
    std::vector<T> staged((size_t)count);      // (exactly `count` values: the sanitizer guards both ends)
    for (int k = 0; k < count; ++k) staged[(size_t)k] = (T)(k + 1);
    std::vector<int> writes((size_t)count, 0);
    const long long origin = out - raw.data();      // raw[origin + e] is out[e]
    CHECK(origin + e0 >= guard && origin + e0 + count + guard <= (long long)raw.size(), "the buffer holds the run and its guards");
    const int lanes = tile_lanes<T>(mis, e0, count);
    CHECK(lanes >= 0 && lanes <= count / EL + 2, "%d lanes for %d elements", lanes, count);
    for (int i = 0; i < lanes; ++i) {
        tile_store_lane(out, mis, e0, count, staged.data(), i);
        int wrote = 0;
        uintptr_t block = 0;
        for (size_t k = 0; k < raw.size(); ++k) {
            if (raw[k] == filling) continue;
            const long long e = (long long)k - origin - e0;      // the element of the run that raw[k] is
            CHECK(e >= 0 && e < count, "lane %d wrote element %lld of a run of %d (mis %d, e0 %lld)", i, e, count, mis, e0);
            CHECK(raw[k] == staged[(size_t)e], "lane %d wrote %g at element %lld", i, (double)raw[k], e);
            const uintptr_t in = reinterpret_cast<uintptr_t>(&raw[k]) / 16;
            CHECK(wrote == 0 || in == block, "lane %d wrote in two 16-byte blocks", i);
            block = in;
            ++writes[(size_t)e];
            ++wrote;
            raw[k] = filling;
        }
        CHECK(wrote <= EL && (count == 0 || wrote >= 1), "lane %d of %d wrote %d elements (count %d, mis %d, e0 %lld)", i, lanes, wrote, count, mis, e0);
    }
    for (int k = 0; k < count; ++k) CHECK(writes[(size_t)k] == 1, "element %d of %d was written %d times (mis %d, e0 %lld)", k, count, writes[(size_t)k], mis, e0);
}

template <typename T> static void check_writer()
{
    constexpr int EL = 16 / (int)sizeof(T);
    const int guard = 4 * EL;      // (a multiple of EL: base + guard is a 16-byte boundary)
    std::vector<int> counts;
    for (int c = 0; c <= 3 * EL + 1; ++c) counts.push_back(c);
    for (int c : {1023, 1024, 1025}) counts.push_back(c);
    std::vector<T> raw((size_t)(guard + EL + 2 * EL + 1 + 1025 + guard + EL), (T)-7);
    T* base = raw.data();
    while (reinterpret_cast<uintptr_t>(base) % 16) ++base;      // (at most EL - 1 elements in)
    for (int mis = 0; mis < EL; ++mis)
        for (long long e0 = 0; e0 <= 2 * EL + 1; ++e0)
            for (int count : counts) check_run<T>(raw, base, guard, mis, e0, count);
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------------------
// Rows of lens[i] outputs in tiles of T, packed (rowStride 0) or padded: every tile of the launch, located as the kernels do.
static void check_walk(const std::vector<long long>& lens, long long rowStride, int T, int log2)
{
    const long long n = (long long)lens.size();
    std::vector<long long> words{-7, -7};      // (appended to: what is there stays)
    const TileTable t = tile_row_table(lens.data(), n, T, rowStride, log2, words);
    CHECK(words[0] == -7 && words[1] == -7 && (rowStride == 0 || words.size() == 2), "the words before");
    const long long* start = words.data() + t.table.startOff;
    const long long* chunk = words.data() + t.table.chunkOff;
    // brute force: the tiles of a row are its starts 0, T, 2 T, ... below its width
    std::vector<std::vector<int>> seen((size_t)n);
    long long all = 0;
    for (long long r = 0; r < n; ++r) {
        const long long width = rowStride > 0 ? rowStride : lens[(size_t)r];
        long long tiles = 0;
        for (long long t0 = 0; t0 < width; t0 += T) ++tiles;
        CHECK(tile_count(width, T) == tiles, "a row of %lld elements has %lld tiles", width, tiles);
        seen[(size_t)r].assign((size_t)tiles, 0);
        all += tiles;
    }
    CHECK(t.nTiles == all, "%lld tiles, the rows have %lld", t.nTiles, all);
    if (rowStride > 0) CHECK(t.tilesPerRow * n == all, "%lld tiles per row", t.tilesPerRow);
    std::vector<long long> sumN((size_t)n, 0), sumLive((size_t)n, 0);
    for (long long g = 0; g < t.nTiles; ++g) {
        long long r, j;
        if (rowStride > 0) tile_row(g, t.tilesPerRow, r, j);
        else {      // tile_locate: the bisection within the chunk table's bounds
            const long long c = g >> log2;
            long long lo = chunk[c], hi = chunk[c + 1] + 1;
            while (hi - lo > 1) { const long long mid = (lo + hi) >> 1; if (start[mid] <= g) lo = mid; else hi = mid; }
            r = lo; j = g - start[r];
        }
        CHECK(r >= 0 && r < n && j >= 0 && j < (long long)seen[(size_t)r].size(), "tile %lld is tile %lld of row %lld", g, j, r);
        ++seen[(size_t)r][(size_t)j];
        const long long t0 = j * T;
        const int count = tile_n(rowStride, lens[(size_t)r], t0, T), live = tile_live(count, lens[(size_t)r], t0);
        CHECK(count >= 1 && count <= T && live >= 0 && live <= count, "tile %lld: %d elements, %d live", g, count, live);
        sumN[(size_t)r] += count;
        sumLive[(size_t)r] += live;
        // the resampler's spans: runs of the tile, their live outputs are the tile's
        for (int span : {1, 7, 1000, T}) {
            int spanLive = 0;
            for (int c0 = 0; c0 < count; c0 += span) spanLive += tile_live(std::min(span, count - c0), lens[(size_t)r], t0 + c0);
            CHECK(spanLive == live, "tile %lld in spans of %d: %d live of %d", g, span, spanLive, live);
        }
    }
    for (long long r = 0; r < n; ++r) {
        for (size_t j = 0; j < seen[(size_t)r].size(); ++j) CHECK(seen[(size_t)r][j] == 1, "tile %zu of row %lld was met %d times", j, r, seen[(size_t)r][j]);
        CHECK(sumN[(size_t)r] == (rowStride > 0 ? rowStride : lens[(size_t)r]), "row %lld: the tiles hold %lld elements", r, sumN[(size_t)r]);
        CHECK(sumLive[(size_t)r] == lens[(size_t)r], "row %lld: %lld live of %lld", r, sumLive[(size_t)r], lens[(size_t)r]);
        if (rowStride == 0 && lens[(size_t)r] == 0) CHECK(seen[(size_t)r].empty() && start[r] == start[r + 1], "a row of no outputs has no tile");
    }
}

int main()
{
    check_writer<int16_t>();
    check_writer<float>();
    const int T = 1024;
    // the count sets of check_export_plan.cpp as output lengths, the small ones also scaled to a tile less one, a tile and a tile and one
    std::vector<std::vector<long long>> lengthSets{
        {}, {0}, {5}, {0, 0, 0, 4, 2}, {4, 2, 0, 0, 0}, {3, 0, 0, 0, 9, 1}, {0, 0, 0},
        {32767, 1, 0, 0, 1, 32768, 65537}, {32768, 32768, 32768}, {16384, 16384, 0, 32768}, {98304}, {1, 98303}, {70000, 0, 1, 0, 0, 70000, 3},
        {1023, 1024, 1025, 2049}, {0, 2049, 0, 0, 1025, 1023, 0}, {3, 4, 5, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1},
    };
    for (size_t k = 1; k < 7; ++k)
        for (long long scale : {1023, 1024, 1025, 2049}) {
            std::vector<long long> scaled = lengthSets[k];
            for (long long& L : scaled) L *= scale;
            lengthSets.push_back(scaled);
        }
    for (const auto& lens : lengthSets) {
        const long long most = lens.empty() ? 0 : *std::max_element(lens.begin(), lens.end());
        for (int log2 : {15, 2, 0}) check_walk(lens, 0, T, log2);      // (chunks of 4 tiles and of 1: many chunk boundaries)
        if (most > 0) check_walk(lens, most, T, 15);
        check_walk(lens, most + 3, T, 15);
    }
    printf("ok %lld checks\n", checks);
    return 0;
}
