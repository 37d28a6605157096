// check_locate.cpp -- the locators the dense and the tile-wise exports address their outputs with (nvspeechplayer_amd/csrc/klatt_tiles.h:
// packed_locate, dense_locate) against a restatement in plain 128-bit division and a linear scan, at and beyond 2^31, 2^32, 2^33 and
// 2^49 elements: the three magnitude branches of dense_locate -- 32-bit divisions while e0 and g | rowStride are below 2^32, 64-bit ones
// beyond -- are counted in the restatement's own terms and each must have been taken.
// Built with AddressSanitizer + UBSan by tests/test_host_logic.py; prints "ok <checks>" or the first failure.
#include "../../nvspeechplayer_amd/csrc/klatt_export.h"

#include <stdlib.h>

using namespace klatt;

static long long g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

typedef unsigned __int128 u128;

// the branches by the magnitudes that choose them: [0] nCols 1, [1] e0 below 2^32, [2] e0 beyond; [3] g | rowStride below 2^32, [4] beyond
static long long g_taken[5] = {0, 0, 0, 0, 0};

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()      // splitmix64
{
    uint64_t z = (g_seed += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static void check_padded(long long e0, int nCols, long long rowStride)
{
    const u128 G = (u128)e0 / (u128)nCols, Q = (u128)e0 % (u128)nCols, R = G / (u128)rowStride, J = G % (u128)rowStride;
    ++g_taken[nCols == 1 ? 0 : ((unsigned long long)e0 >> 32) ? 2 : 1];
    ++g_taken[(((unsigned long long)G | (unsigned long long)rowStride) >> 32) ? 4 : 3];
    long long g = -1, r = -1, j = -1;
    int q = -1;
    dense_locate(e0, nCols, rowStride, nullptr, nullptr, g, q, r, j);
    CHECK((u128)g == G && (u128)q == Q && (u128)r == R && (u128)j == J);
    CHECK((r * rowStride + j) * nCols + q == e0 && 0 <= q && q < nCols && 0 <= j && j < rowStride);      // and back again
}

static void check_padded_form()
{
    const long long limit = 1ll << 50;
    const int cols[] = {1, 2, 3, 7, 45, 4096};
    const long long strides[] = {1, 2, (1ll << 16) - 1, (1ll << 31) - 1, 1ll << 31, (1ll << 32) - 1, 1ll << 32, (1ll << 32) + 1, (1ll << 40) + 3};
    const long long bounds[] = {1ll << 31, 1ll << 32, 1ll << 33, 1ll << 49};
    for (int nCols : cols)
        for (long long rowStride : strides) {
            check_padded(0, nCols, rowStride);
            const u128 P = (u128)nCols * (u128)rowStride;      // a row's elements
            long long windows = 0;
            for (long long B : bounds) {
                const u128 below = (u128)B / P * P;
                for (u128 m : {below, below + P, (u128)B})      // the row starts either side of the bound, and the bound itself
                    for (long long d = -64; d <= 64; ++d) {
                        if ((d < 0 && m < (u128)(-d)) || m + (u128)(d + 64) >= (u128)limit + 64) continue;
                        check_padded((long long)m + d, nCols, rowStride);
                        ++windows;
                    }
            }
            CHECK(windows >= 4 * 65);
            for (int i = 0; i < 100000; ++i) check_padded((long long)(rnd() & (uint64_t)(limit - 1)), nCols, rowStride);
        }
}

// The packed form over rows of `counts` steps: entry g by linear scan, then both overloads of packed_locate and dense_locate with 1
// and 3 columns (the 64-bit e0 / nCols with a row table behind it).
struct Packed {
    std::vector<long long> words;
    const long long *start, *chunk;
    long long nRows, total;
    explicit Packed(const std::vector<long long>& counts) : nRows((long long)counts.size())
    {
        const RowTable t = packed_row_table(counts.data(), 0, nRows, kTimelineChunkLog2, words);
        start = words.data() + t.startOff; chunk = words.data() + t.chunkOff; total = start[nRows];
        CHECK((long long)words.size() == t.chunkOff + (total >> kTimelineChunkLog2) + 2);
    }
    void probe(long long g) const
    {
        if (g < 0 || g >= total) return;
        long long row = -1;
        for (long long i = 0; i < nRows; ++i) if (start[i] <= g && g < start[i + 1]) { CHECK(row < 0); row = i; }
        CHECK(row >= 0);
        long long r = -1, j = -1;
        packed_locate(g, start, nRows, r, j);
        CHECK(r == row && j == g - start[row]);
        const long long c = g >> kTimelineChunkLog2;
        r = j = -1;
        packed_locate(g, start, chunk[c], chunk[c + 1] + 1, r, j);
        CHECK(r == row && j == g - start[row]);
        for (int nCols : {1, 3})
            for (int col = 0; col < nCols; ++col) {
                const long long e0 = g * nCols + col;
                ++g_taken[nCols == 1 ? 0 : ((unsigned long long)e0 >> 32) ? 2 : 1];
                long long gg = -1;
                int q = -1;
                r = j = -1;
                dense_locate(e0, nCols, 0, start, chunk, gg, q, r, j);
                CHECK(gg == g && q == col && r == row && j == g - start[row]);
            }
    }
};

static void check_packed_form()
{
    const long long K = 1ll << kTimelineChunkLog2;
    const std::vector<std::vector<long long>> countSets{
        {0, 5, 0, 0, (1ll << 31) - 40, 7, 0, 1, (1ll << 31) + 3, K, 1ll << 33, 9, 0},      // a leading and a trailing row of nothing; rows end either side of 2^31 and 2^32
        {0, 1ll << 33, 3, 0, 5, 0},                                                        // a row ends on 2^33
        {(1ll << 31) - 1, 2, (1ll << 31) - 1, 0, 1ll << 32, 1, K - 1, 1ll << 33},          // rows start on 2^31 + 1, 2^32 and 2^33 + K
        {1ll << 33}, {0, 0, 1ll << 33, 0, 0},
    };
    for (const auto& counts : countSets) {
        const Packed p(counts);
        long long acc = 0, zeros = 0, big = 0;
        for (long long n : counts) { acc += n; zeros += n == 0; big += n == (1ll << 33); }
        CHECK(p.total == acc && acc > (1ll << 33) - 1 && big == 1);
        CHECK(counts.size() == 1 || zeros > 0);
        for (long long i = 0; i < p.nRows; ++i)      // every row's first and last step, and their neighbours
            for (long long d = -2; d <= 2; ++d) { p.probe(p.start[i] + d); p.probe(p.start[i + 1] - 1 + d); }
        for (long long c = 0; c <= acc >> kTimelineChunkLog2; ++c) { p.probe(c * K - 1); p.probe(c * K); }      // every chunk's first step, and the step before
        for (long long B : {1ll << 31, 1ll << 32, 1ll << 33})
            for (long long d = -64; d <= 64; ++d) p.probe(B + d);
        for (int i = 0; i < 20000; ++i) p.probe((long long)(rnd() % (uint64_t)acc));
    }
}

int main()
{
    check_padded_form();
    check_packed_form();
    for (long long n : g_taken) CHECK(n > 0);      // every branch of dense_locate was taken
    printf("ok %lld checks (nCols 1: %lld, e0 below 2^32: %lld, beyond: %lld; g | rowStride below 2^32: %lld, beyond: %lld)\n", g_checks,
           g_taken[0], g_taken[1], g_taken[2], g_taken[3], g_taken[4]);
    return 0;
}
