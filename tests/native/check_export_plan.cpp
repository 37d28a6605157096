// check_export_plan.cpp -- the export path's host planning (nvspeechplayer_amd/csrc/klatt_export.h) against a brute-force restatement.
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

// packed_row_table over rows [r0, r1) of `counts`: every output entry g is located by a linear scan, and the bounds the device
// bisects within (chunk[g >> log2], chunk[(g >> log2) + 1]) must bracket that row and lead the bisection to it.  every: all g (the
// whole selection); else those within two of a row start or a chunk boundary (the runs of rows a piece can be).
static void check_row_table(const std::vector<long long>& counts, long long r0, long long r1, int log2, bool every)
{
    std::vector<long long> words{-7, -7, -7};      // (appended to: what is there stays)
    const RowTable t = packed_row_table(counts.data(), r0, r1, log2, words);
    const long long nr = r1 - r0;
    CHECK(t.startOff == 3 && words[0] == -7 && words[2] == -7);
    CHECK(t.chunkOff == t.startOff + nr + 1);
    const long long* start = words.data() + t.startOff;
    long long acc = 0;
    for (long long i = 0; i < nr; ++i) { CHECK(start[i] == acc); acc += counts[(size_t)(r0 + i)]; }
    CHECK(start[nr] == acc);
    if (log2 < 0) { CHECK((long long)words.size() == t.chunkOff); return; }
    const long long nChunks = (acc >> log2) + 1;
    CHECK((long long)words.size() == t.chunkOff + nChunks + 1);
    const long long* chunk = words.data() + t.chunkOff;
    CHECK(chunk[nChunks] == std::max<long long>(nr - 1, 0));
    auto check_entry = [&](long long g) {
        if (g < 0 || g >= acc) return;
        long long row = -1;      // the row that holds entry g, by linear scan
        for (long long i = 0; i < nr; ++i) if (start[i] <= g && g < start[i + 1]) row = i;
        CHECK(row >= 0);
        const long long c = g >> log2;
        CHECK(c < nChunks && 0 <= chunk[c] && chunk[c] <= row && row <= chunk[c + 1] && chunk[c + 1] < nr);
        // the device's bisection inside those bounds: the last row whose start is <= g
        long long lo = chunk[c], hi = chunk[c + 1] + 1;
        while (hi - lo > 1) { const long long mid = (lo + hi) >> 1; if (start[mid] <= g) lo = mid; else hi = mid; }
        CHECK(lo == row);
    };
    if (every) for (long long g = 0; g < acc; ++g) check_entry(g);
    for (long long i = 0; i <= nr; ++i) for (long long d = -2; d <= 2; ++d) check_entry(start[i] + d);
    for (long long c = 0; c <= nChunks && c < 4096; ++c) for (long long d = -2; d <= 2; ++d) check_entry((c << log2) + d);
}

// list_pieces: the pieces cover [0, n) in order, hold at most slotsPerPiece lists, every row's slot is its list's within the piece and
// unique among the piece's lists, `fresh` marks the first row of a list in a piece, skipped rows are not placed; and the greedy rule
// itself: a piece ends only where the next row's list would be one too many.
static void check_pieces(const std::vector<long long>& listOf, const std::vector<long long>& counts, bool skip, long long nLists, long long slotsPerPiece)
{
    const long long n = (long long)listOf.size();
    std::vector<long long> slot((size_t)n, -1), freshAt((size_t)n, 0);
    long long placed = 0, lastPlaced = -1;
    const std::vector<ExportPiece> pieces = list_pieces(
        n, [&](long long i) { return listOf[(size_t)i]; }, [&](long long i) { return skip && counts[(size_t)i] == 0; }, nLists, slotsPerPiece,
        [&](long long i, uint32_t s, bool fresh) {
            CHECK(i > lastPlaced);
            lastPlaced = i; ++placed;
            slot[(size_t)i] = s; freshAt[(size_t)i] = fresh;
        });
    CHECK(!pieces.empty() && pieces.front().r0 == 0 && pieces.back().r1 == n);
    long long expectPlaced = 0;
    for (size_t p = 0; p < pieces.size(); ++p) {
        const ExportPiece& pc = pieces[p];
        CHECK(pc.r0 <= pc.r1 && (p == 0 || pc.r0 == pieces[p - 1].r1));
        CHECK(pc.nLists <= slotsPerPiece);
        std::vector<long long> listOfSlot;      // brute force: the distinct lists of the piece in order of appearance
        for (long long i = pc.r0; i < pc.r1; ++i) {
            if (skip && counts[(size_t)i] == 0) { CHECK(slot[(size_t)i] == -1); continue; }
            ++expectPlaced;
            long long s = -1;
            for (size_t k = 0; k < listOfSlot.size(); ++k) if (listOfSlot[k] == listOf[(size_t)i]) s = (long long)k;
            const bool fresh = s < 0;
            if (fresh) { s = (long long)listOfSlot.size(); listOfSlot.push_back(listOf[(size_t)i]); }
            CHECK(slot[(size_t)i] == s && freshAt[(size_t)i] == (long long)fresh);
        }
        CHECK((long long)listOfSlot.size() == pc.nLists);
        if (p + 1 < pieces.size()) {      // the piece was full, and the row that ended it brought a list it did not hold
            CHECK(pc.nLists == slotsPerPiece);
            CHECK(std::find(listOfSlot.begin(), listOfSlot.end(), listOf[(size_t)pc.r1]) == listOfSlot.end());
            CHECK(!(skip && counts[(size_t)pc.r1] == 0));
        }
    }
    CHECK(placed == expectPlaced);
}

static long long extent(const ExportNouns& nouns, long long most, long long total, long long n, long long rowStride, long long per, long long capacity,
                        std::string& why)
{
    why = "(untouched)";
    const long long e = export_extent(nouns, most, total, n, rowStride, per, capacity, why);
    CHECK((e < 0) == (why != "(untouched)"));
    return e;
}

static void check_extents()
{
    std::string why;
    // rowStride one below and equal to the largest count
    CHECK(extent(kStepNouns, 10, 25, 3, 9, 4, kNoCapacity, why) == -1 && why == "rowStride 9 is below the largest step count (10)");
    CHECK(extent(kStepNouns, 10, 25, 3, 10, 4, kNoCapacity, why) == 120);
    CHECK(extent(kEntryNouns, 10, 25, 3, 9, 7, kNoCapacity, why) == -1 && why == "rowStride 9 is below the largest count (10)");
    CHECK(extent(kEntryNouns, 10, 25, 3, 10, 7, kNoCapacity, why) == 210);
    CHECK(extent(kStepNouns, 10, 25, 3, 0, 4, kNoCapacity, why) == 100);      // packed: the total counts
    CHECK(extent(kStepNouns, 0, 0, 0, 0, 4, kNoCapacity, why) == 0 && extent(kStepNouns, 0, 0, 0, 5, 4, kNoCapacity, why) == 0);
    // products one below, equal to and one above 2^50: padded (n * rowStride * per) and packed (total * per)
    const long long lim = 1ll << 50;
    CHECK(extent(kStepNouns, 1, 1, lim / 8, 2, 4, kNoCapacity, why) == lim);
    CHECK(extent(kStepNouns, 1, 1, lim / 8 + 1, 2, 4, kNoCapacity, why) == -1 && why == "140737488355329 rows of 2 steps of 4 columns");
    CHECK(extent(kStepNouns, 1, 1, (lim - 1) / 3, 1, 3, kNoCapacity, why) == (lim - 1) / 3 * 3);      // 2^50 - 1 = 3 * 375299968947541
    CHECK((lim - 1) % 3 == 0 && extent(kStepNouns, 1, 1, (lim - 1) / 3 + 1, 1, 3, kNoCapacity, why) == -1);
    CHECK(extent(kStepNouns, 1, lim / 4, 1, 0, 4, kNoCapacity, why) == lim);
    CHECK(extent(kStepNouns, 1, lim / 4 + 1, 1, 0, 4, kNoCapacity, why) == -1 && why == "281474976710657 steps of 4 columns");
    CHECK(extent(kStepNouns, 1, lim - 1, 1, 0, 1, kNoCapacity, why) == lim - 1 && extent(kStepNouns, 1, lim + 1, 1, 0, 1, kNoCapacity, why) == -1);
    // entries: the limit is on n * rowStride, whatever an entry holds
    CHECK(extent(kEntryNouns, 1, 1, lim / 2, 2, 7, kNoCapacity, why) == lim * 7);
    CHECK(extent(kEntryNouns, 1, 1, lim / 2 + 1, 2, 7, kNoCapacity, why) == -1 && why == "562949953421313 rows of 2 entries");
    CHECK(extent(kEntryNouns, 1, lim + 1, 1, 0, 7, kNoCapacity, why) == (lim + 1) * 7);      // (packed entries have no limit of their own)
    // a hostile rowStride overflows nothing
    CHECK(extent(kStepNouns, 1, 1, 3, 0x7FFFFFFFFFFFFFFFll, 49, kNoCapacity, why) == -1);
    // capacity: after the extents, before the count is answered
    CHECK(extent(kStepNouns, 10, 25, 3, 10, 4, 120, why) == 120);
    CHECK(extent(kStepNouns, 10, 25, 3, 10, 4, 119, why) == -1 && why == "the output takes 120 elements, capacity is 119");
    CHECK(extent(kStepNouns, 10, 25, 3, 9, 4, 0, why) == -1 && why == "rowStride 9 is below the largest step count (10)");
    CHECK(extent(kStepNouns, 0, 0, 0, 0, 4, -1, why) == -1 && why == "the output takes 0 elements, capacity is -1");
}

static void check_block()
{
    StageBlock empty;
    CHECK(empty.bytes() == 0);
    const std::vector<int> cols{3, 1, 4};
    const std::vector<long long> none, words{5, 6, 7};
    struct Row24 { long long a; uint32_t b, c; long long d; };
    const std::vector<Row24> rows{{1, 2, 3, 4}, {5, 6, 7, 8}, {9, 10, 11, 12}};      // 72 bytes: the next section is padded to 80
    StageBlock b;
    const int c = b.add(cols.data(), cols.size() * sizeof(int)), r = b.add(rows), e = b.add(none), w = b.add(words);
    CHECK(c == 0 && r == 1 && e == 2 && w == 3);
    CHECK(b.offset(c) == 0 && b.offset(r) == 16 && b.offset(e) == 96 && b.offset(w) == 96 && b.bytes() == 96 + 32);
    std::vector<unsigned char> host(b.bytes(), 0xAB);
    b.copy_to(host.data());
    CHECK(memcmp(host.data(), cols.data(), 12) == 0 && host[12] == 0xAB);
    CHECK(memcmp(host.data() + 16, rows.data(), 72) == 0 && host[88] == 0xAB);
    CHECK(memcmp(host.data() + 96, words.data(), 24) == 0 && host[120] == 0xAB);
    CHECK(b.device<long long>(w, host.data()) == reinterpret_cast<const long long*>(host.data() + 96) && b.device<long long>(w, host.data())[2] == 7);
    CHECK(b.device<Row24>(r, host.data())[2].d == 12);
    // every section of any sizes starts on a 16-byte boundary, after the one before, and the block ends on one
    StageBlock many;
    size_t end = 0;
    for (size_t bytes = 0; bytes < 70; ++bytes) {
        const int s = many.add(host.data(), bytes);
        CHECK(many.offset(s) % 16 == 0 && many.offset(s) >= end && many.offset(s) < end + 16);
        end = many.offset(s) + bytes;
        CHECK(many.bytes() % 16 == 0 && many.bytes() >= end && many.bytes() < end + 16);
    }
}

int main()
{
    const int log2 = 15;
    const std::vector<std::vector<long long>> countSets{
        {}, {0}, {5}, {0, 0, 0, 4, 2}, {4, 2, 0, 0, 0}, {3, 0, 0, 0, 9, 1}, {0, 0, 0},
        {32767, 1, 0, 0, 1, 32768, 65537},      // starts on, one before and one after a chunk boundary; one row spans two chunks
        {32768, 32768, 32768}, {16384, 16384, 0, 32768}, {98304}, {1, 98303},      // totals that are exact multiples of 32768
        {70000, 0, 1, 0, 0, 70000, 3},
    };
    for (const auto& counts : countSets) {
        const long long n = (long long)counts.size();
        const bool small = counts.empty() || *std::max_element(counts.begin(), counts.end()) < 1000;
        for (int lg : {log2, 2, 0, -1}) {
            if (!small && (lg == 2 || lg == 0)) continue;      // (chunks of 4 and of 1: the small sets meet many boundaries that way)
            check_row_table(counts, 0, n, lg, true);
            for (long long r0 = 0; r0 <= n; ++r0)      // the pieces' tables: every run of rows
                for (long long r1 = r0; r1 <= n; ++r1) check_row_table(counts, r0, r1, lg, small);
        }
    }
    // pieces: the same list chosen by rows 0, 2 and 5; rows without entries first, last and three in a row
    const std::vector<std::vector<long long>> listSets{{}, {0}, {4, 1, 4, 2, 3, 4, 0}, {0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6}, {6, 5, 6, 5, 4, 4, 3}};
    const std::vector<std::vector<long long>> pieceCounts{{3, 1, 2, 5, 1, 1, 2}, {0, 1, 0, 0, 0, 1, 0}, {0, 0, 0, 0, 0, 0, 0}, {32767, 1, 0, 0, 1, 32768, 65537}};
    for (const auto& lists : listSets)
        for (const auto& counts : pieceCounts)
            for (bool skip : {false, true})
                for (long long slots : {1, 2, 3, 64}) {
                    check_pieces(lists, std::vector<long long>(counts.begin(), counts.begin() + (long)lists.size()), skip, 7, slots);
                }
    check_extents();
    check_block();
    printf("ok %lld checks\n", g_checks);
    return 0;
}
