// klatt_export.h -- the host half of the batch exports' one path (klatt_engine.hip, "the export path"): what every export of a batch
// "as set" plans before it touches the device.  Plain C++17, no HIP: tests/native/check_export_plan.cpp holds it to a brute-force
// restatement under the sanitizers.
//
//   export_extent      the extent refusals every export makes, and its element count
//   packed_row_table   the packed form's row table: step starts, chunk rows, the closing entry
//   tile_row_table     the same over the TILES of rows of outputs (klatt_tiles.h), with the padded form's tiles per row
//   list_pieces        runs of rows whose distinct lists fit a table
//   StageBlock         the sections of a staging block, each on a 16-byte boundary
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "klatt_tiles.h"

namespace klatt {

constexpr long long kExportLimit = 1ll << 50;            // no output has more elements
constexpr long long kNoCapacity = 0x7FFFFFFFFFFFFFFFll;  // the entry point takes no capacity

// The nouns an entry point's extent messages use: "rowStride 3 is below the <most> (5)", "4 rows of 3 <unit> of 2 <per>".
// per == nullptr: the limit is on the rows times rowStride of the padded form alone, and the messages end at the unit.
struct ExportNouns { const char *most, *unit, *per; };
constexpr ExportNouns kStepNouns{"largest step count", "steps", "columns"};
constexpr ExportNouns kEntryNouns{"largest count", "entries", nullptr};

// The elements of an export of n rows -- rowStride entries each (padded) or `total` entries in all (packed: rowStride 0), perEntry
// elements per entry -- or -1 with `error` set (without the entry point's prefix): rowStride below the largest count `most`, more
// than kExportLimit elements, more than `capacity`.
inline long long export_extent(const ExportNouns& nouns, long long most, long long total, long long n, long long rowStride, long long perEntry,
                               long long capacity, std::string& error)
{
    char buf[256], per[64] = "";
    const bool packed = rowStride == 0;
    const long long limit = kExportLimit / (nouns.per ? perEntry : 1);
    if (nouns.per) snprintf(per, sizeof per, " of %lld %s", perEntry, nouns.per);
    if (!packed && rowStride < most) snprintf(buf, sizeof buf, "rowStride %lld is below the %s (%lld)", rowStride, nouns.most, most);
    else if (!packed && n > 0 && n > limit / rowStride) snprintf(buf, sizeof buf, "%lld rows of %lld %s%s", n, rowStride, nouns.unit, per);
    else if (packed && nouns.per && total > limit) snprintf(buf, sizeof buf, "%lld %s%s", total, nouns.unit, per);
    else {
        const long long elements = (packed ? total : n * rowStride) * perEntry;
        if (elements <= capacity) return elements;
        snprintf(buf, sizeof buf, "the output takes %lld elements, capacity is %lld", elements, capacity);
    }
    error = buf;
    return -1;
}

// The row table of the packed form for rows [r0, r1) with counts[i] entries each, appended to `words`: the rows' starts and the total
// (nr + 1 words), then -- chunkLog2 >= 0 -- for every chunk of 1 << chunkLog2 output entries the last row that starts on or before
// the chunk's first entry ((total >> chunkLog2) + 1 words) and the closing max(nr - 1, 0): the row an entry g belongs to lies in
// [chunk[g >> chunkLog2], chunk[(g >> chunkLog2) + 1]].
struct RowTable { long long startOff, chunkOff; };
inline RowTable packed_row_table(const long long* counts, long long r0, long long r1, int chunkLog2, std::vector<long long>& words)
{
    RowTable t{(long long)words.size(), 0};
    long long acc = 0;
    for (long long i = r0; i < r1; ++i) { words.push_back(acc); acc += counts[i]; }
    words.push_back(acc);
    t.chunkOff = (long long)words.size();
    if (chunkLog2 < 0) return t;
    const long long nr = r1 - r0, nChunks = (acc >> chunkLog2) + 1;
    long long r = 0;
    for (long long c = 0; c < nChunks; ++c) {
        while (r + 1 < nr && words[(size_t)(t.startOff + r + 1)] <= (c << chunkLog2)) ++r;
        words.push_back(r);
    }
    words.push_back(std::max<long long>(nr - 1, 0));
    return t;
}

// The tiles of an export whose n rows have outLen[i] outputs each, in tiles of `tile` (klatt_tiles.h).  Packed (rowStride 0): the row
// table over the rows' tiles is appended to `words`.  Padded: every row has the tiles of rowStride elements, nothing is appended.
struct TileTable { RowTable table; long long tilesPerRow, nTiles; };
inline TileTable tile_row_table(const long long* outLen, long long n, int tile, long long rowStride, int chunkLog2, std::vector<long long>& words)
{
    const long long perRow = tile_count(rowStride, tile);
    if (rowStride > 0) return TileTable{{0, 0}, perRow, n * perRow};
    std::vector<long long> tiles((size_t)n);
    for (long long i = 0; i < n; ++i) tiles[(size_t)i] = tile_count(outLen[i], tile);
    const RowTable table = packed_row_table(tiles.data(), 0, n, chunkLog2, words);
    return TileTable{table, perRow, words[(size_t)(table.startOff + n)]};
}

// Rows [r0, r1) whose nLists distinct lists hold slots 0 .. nLists - 1 of a table; `table` is the caller's to fill.
struct ExportPiece { long long r0, r1, nLists; RowTable table; };

// The rows 0 .. n - 1 in runs whose distinct lists number at most slotsPerPiece (>= 1).  listOfRow(i) < nLists is the list row i
// speaks; a row with skipRow(i) takes no slot.  place(i, slot, fresh) hands every other row its slot within its piece, fresh for the
// first row of its list there.  The pieces cover [0, n) in order; there is always at least one.
template <class ListOfRow, class SkipRow, class Place>
std::vector<ExportPiece> list_pieces(long long n, ListOfRow listOfRow, SkipRow skipRow, long long nLists, long long slotsPerPiece, Place place)
{
    std::vector<ExportPiece> pieces;
    std::vector<long long> stamp((size_t)nLists, -1);     // the piece that last gave the list a slot
    std::vector<uint32_t> slotOf((size_t)nLists, 0);
    ExportPiece pc{0, 0, 0, {0, 0}};
    for (long long i = 0; i < n; ++i) {
        if (skipRow(i)) continue;
        const size_t l = (size_t)listOfRow(i);
        const bool fresh = stamp[l] != (long long)pieces.size();
        if (fresh) {
            if (pc.nLists == slotsPerPiece) {
                pc.r1 = i; pieces.push_back(pc);
                pc = ExportPiece{i, i, 0, {0, 0}};
            }
            stamp[l] = (long long)pieces.size();
            slotOf[l] = (uint32_t)pc.nLists++;
        }
        place(i, slotOf[l], fresh);
    }
    pc.r1 = n; pieces.push_back(pc);
    return pieces;
}

// A staging block: sections of host memory that cross the link in one copy, each on a 16-byte boundary of the block (whatever a
// kernel reads by vector loads may follow whatever else).  add() does not copy: the memory must live until copy_to().  reserve() makes a
// section without contents -- device scratch a kernel fills before another reads it: nothing is copied into it on the host, and the
// reserved sections at the block's END do not cross the link either (upload_bytes).
class StageBlock {
    struct Section { const void* from; size_t bytes, at; };
    std::vector<Section> sections;
    size_t total = 0;
public:
    int add(const void* from, size_t bytes)
    {
        sections.push_back(Section{from, bytes, total});
        total = (total + bytes + 15) / 16 * 16;
        return (int)sections.size() - 1;
    }
    template <class T> int add(const std::vector<T>& v) { return add(v.data(), v.size() * sizeof(T)); }
    int reserve(size_t bytes) { return add(nullptr, bytes); }
    size_t bytes() const { return total; }
    // The bytes from the block's start that hold contents: what the upload copies
    size_t upload_bytes() const
    {
        size_t end = 0;
        for (const Section& s : sections)
            if (s.from && s.bytes) end = (s.at + s.bytes + 15) / 16 * 16;
        return end;
    }
    size_t offset(int section) const { return sections[(size_t)section].at; }
    void copy_to(void* host) const
    {
        for (const Section& s : sections)
            if (s.bytes && s.from) memcpy(static_cast<char*>(host) + s.at, s.from, s.bytes);
    }
    template <class T> const T* device(int section, const unsigned char* base) const
    {
        static_assert(alignof(T) <= 16, "a section starts on a 16-byte boundary");
        return reinterpret_cast<const T*>(base + offset(section));
    }
};

}  // namespace klatt
