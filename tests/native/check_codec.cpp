// check_codec.cpp -- models of the two kernels of the codec export (nvspeechplayer_amd/csrc/klatt_codec.h) written from the shared functions
// alone.  klatt_code_g711: the tile walk (tile_row_table, tile_row and the bisection of the packed form, tile_n), the masked read, the
// values staged from codec_lead and codec_store_block for the decoded samples and for the codes, a one-byte element.  klatt_code_adpcm: the packing
// (filter_pack with one section a row), the masked loads of a tile of 64 rows, the int32 samples at the row pitch, the in-place staging
// of the decoded samples and the codes -- codes alone, decoded alone, and both with the codes' own run at the wider pitch -- and
// codec_store_row with 32, 16 or 8 lanes a row.  For 0, 1, 63, 64, 65 and 130 rows of lengths around both tiles, padded and packed, int16
// and float32 in and out, outputs 0, 1 and 3 elements past a 16-byte boundary: every load stays inside the input, every element of
// each output is written exactly once, the guards stay, and the bits are the statement's (code_host), +0 and code 0 in the padding.
// Built with AddressSanitizer + UBSan by tests/test_codec_host.py; prints "ok <checks>" or the first failure.
#include "../../nvspeechplayer_amd/csrc/klatt_codec.h"
#include "../../nvspeechplayer_amd/csrc/klatt_export.h"

#include <stdlib.h>
#include <string.h>

using namespace klatt;

static long long checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static uint32_t rng_state = 2463534242u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

template <typename In> static In random_sample();
template <> int16_t random_sample<int16_t>() { return (rng() % 9u) == 0 ? (int16_t)0 : (int16_t)((int)(rng() % 65536u) - 32768); }
template <> float random_sample<float>() { return (rng() % 9u) == 0 ? ((rng() & 1u) ? 0.0f : -0.0f) : (float)((int)(rng() % 65535u) - 32767) / 20000.0f; }

constexpr int GUARD = 32;

// An output of `elements` elements of T between guards, its first element `shift` elements past a 16-byte boundary
template <typename T>
struct Guarded {
    void* block;
    T* all;
    long long elements;
    int shift;
    std::vector<int> written;
    Guarded(long long elements, int shift) : elements(elements), shift(shift), written((size_t)elements, 0)
    {
        block = aligned_alloc(16, ((size_t)(elements + 2 * GUARD + shift) * sizeof(T) + 15) / 16 * 16);
        all = static_cast<T*>(block);
        for (long long e = 0; e < elements + 2 * GUARD + shift; ++e) all[e] = (T)-7;
    }
    ~Guarded() { free(block); }
    T* out() { return all + GUARD + shift; }
    void mark(long long e0, int n)
    {
        CHECK(e0 >= 0 && e0 + n <= elements, "store of %d elements from %lld of %lld", n, e0, elements);
        for (int e = 0; e < n; ++e) ++written[(size_t)(e0 + e)];
    }
    void finished(const char* what)
    {
        for (long long e = 0; e < GUARD + shift; ++e) CHECK(all[e] == (T)-7, "%s: the guard before, element %lld", what, e);
        for (long long e = 0; e < GUARD; ++e) CHECK(all[GUARD + shift + elements + e] == (T)-7, "%s: the guard behind, element %lld", what, e);
        for (long long e = 0; e < elements; ++e) CHECK(written[(size_t)e] == 1, "%s: element %lld of %lld written %d times", what, e, elements, written[(size_t)e]);
    }
};

struct Rows {
    std::vector<FilterRow> rows;      // (a section each)
    long long rowStride, inputs, outputs;
};

// n rows of the lengths given in turn from a seeded start, the inputs back to back from element 3 with gaps, the outputs padded or back to back
static Rows make_rows(int n, const int* lengths, int nLengths, bool padded)
{
    Rows R;
    long long src = 3, most = 0;
    for (int i = 0; i < n; ++i) {
        const long long L = lengths[rng() % (uint32_t)nLengths];
        R.rows.push_back(FilterRow{src, L, L, 0, 0, 1});
        src += L + (long long)(rng() % 3u);
        most = std::max(most, L);
    }
    R.inputs = src + 2;
    R.rowStride = padded ? most + (long long)(rng() % 5u) : 0;
    long long before = 0;
    for (int i = 0; i < n; ++i) { R.rows[(size_t)i].dst = padded ? i * R.rowStride : before; before += R.rows[(size_t)i].outLen; }
    R.outputs = padded ? n * R.rowStride : before;
    return R;
}

// The outputs against the statement: row by row, and the padding
template <bool F32, typename In>
static void compare(const Rows& R, const In* in, int codec, const TileValue<F32>* decoded, const uint8_t* codes, const char* what)
{
    using T = TileValue<F32>;
    for (size_t i = 0; i < R.rows.size(); ++i) {
        const FilterRow& r = R.rows[i];
        std::vector<T> wantD((size_t)r.len + 1);
        std::vector<uint8_t> wantC((size_t)r.len + 1);
        code_host(in + r.src, r.len, codec, F32 ? 1 : 0, wantD.data(), wantC.data(), nullptr);
        const long long span = R.rowStride > 0 ? R.rowStride : r.len;
        if (decoded) {
            CHECK(memcmp(decoded + r.dst, wantD.data(), sizeof(T) * (size_t)r.len) == 0, "%s: decoded row %zu of %lld samples", what, i, r.len);
            const T zero = (T)0;
            for (long long e = r.len; e < span; ++e) CHECK(memcmp(decoded + r.dst + e, &zero, sizeof zero) == 0, "%s: row %zu: decoded padding element %lld", what, i, e);
        }
        if (codes) {
            CHECK(memcmp(codes + r.dst, wantC.data(), (size_t)r.len) == 0, "%s: codes of row %zu of %lld samples", what, i, r.len);
            for (long long e = r.len; e < span; ++e) CHECK(codes[r.dst + e] == 0, "%s: row %zu: code padding element %lld", what, i, e);
        }
    }
}

// ---- klatt_code_g711 ------------------------------------------------------------------------------------------------------------------------
template <int LAW, bool F32, typename In>
static void model_g711(int n, bool padded, int outputs, int shift)
{
    using T = TileValue<F32>;
    static const int lengths[] = {0, 1, 2, kCodeTile - 1, kCodeTile, kCodeTile + 1, 3 * kCodeTile + 5, 130};
    const Rows R = make_rows(n, lengths, 8, padded);
    std::vector<In> in((size_t)R.inputs);
    for (auto& v : in) v = random_sample<In>();
    std::vector<long long> counts, words;
    for (const FilterRow& r : R.rows) counts.push_back(r.outLen);
    const TileTable tiles = tile_row_table(counts.data(), n, kCodeTile, R.rowStride, 4, words);
    Guarded<T> D(R.outputs, shift);
    Guarded<uint8_t> C(R.outputs, shift);
    const bool wantD = (outputs & kCodeDecoded) != 0, wantC = (outputs & kCodeCodes) != 0;
    for (long long g = 0; g < tiles.nTiles; ++g) {
        long long r, j;
        if (R.rowStride > 0) tile_row(g, tiles.tilesPerRow, r, j);
        else {      // (packed_locate of klatt_timeline.h, device only, restated: the last row that starts on or before tile g, within the chunk's bounds)
            const long long* start = words.data() + tiles.table.startOff, * chunk = words.data() + tiles.table.chunkOff;
            long long lo = chunk[g >> 4], hi = chunk[(g >> 4) + 1] + 1;
            while (hi - lo > 1) { const long long mid = (lo + hi) >> 1; if (start[mid] <= g) lo = mid; else hi = mid; }
            r = lo; j = g - start[r];
        }
        CHECK(r >= 0 && r < n, "tile %lld lies in row %lld of %d", g, r, n);
        const long long t0 = j * kCodeTile;
        const FilterRow row = R.rows[(size_t)r];
        const int cnt = tile_n(R.rowStride, row.outLen, t0, kCodeTile);
        CHECK(cnt > 0 && cnt <= kCodeTile, "tile %lld holds %d elements", g, cnt);
        // staged as the kernel stages: 16-byte aligned, the run from codec_lead
        struct alignas(16) StagedD { T x[kCodeTile + kTileLane<T>]; } staged;
        struct alignas(16) StagedC { uint8_t x[kCodeTile + kTileLane<uint8_t>]; } stagedCodes;
        for (T& v : staged.x) v = (T)-3;
        for (uint8_t& v : stagedCodes.x) v = (uint8_t)0xEE;
        const long long e0 = row.dst + t0;
        const int misD = tile_mis<T>(D.out()), misC = tile_mis<uint8_t>(C.out());
        const int leadD = wantD ? codec_lead<T>(misD, e0) : 0, leadC = wantC ? codec_lead<uint8_t>(misC, e0) : 0;
        CHECK(leadD >= 0 && leadD < kTileLane<T> && leadC >= 0 && leadC < 16, "leads %d and %d", leadD, leadC);
        for (int i = 0; i < cnt; ++i) {
            const long long s = t0 + i;
            const bool inside = tile_inside(s, row.len);
            T d = (T)0;
            uint8_t c = 0;
            if (t0 < row.len) {
                const long long at = codec_within(s, row.len);
                CHECK(at >= t0 && at < row.len && (at == s) == inside, "sample %lld of a row of %lld loads %lld", s, row.len, at);
                const int code = g711_encode<LAW>(codec_sample(in[(size_t)(row.src + at)]));
                d = inside ? codec_value<F32>(g711_decode<LAW>(code)) : (T)0;
                c = inside ? (uint8_t)code : (uint8_t)0;
            }
            staged.x[leadD + i] = d;
            stagedCodes.x[leadC + i] = c;
        }
        if (wantD) {
            D.mark(e0, cnt);
            CHECK((reinterpret_cast<uintptr_t>(D.out() + (e0 - leadD)) & 15) == 0, "block 0 of the decoded run is not aligned");
            for (int i = 0; i < codec_blocks<T>(leadD, cnt); ++i) codec_store_block(D.out(), e0, leadD, cnt, staged.x, i);
        }
        if (wantC) {
            C.mark(e0, cnt);
            CHECK(misC == shift, "the codes lie %d bytes past a 16-byte boundary", misC);
            CHECK((reinterpret_cast<uintptr_t>(C.out() + (e0 - leadC)) & 15) == 0, "block 0 of the codes' run is not aligned");
            for (int i = 0; i < codec_blocks<uint8_t>(leadC, cnt); ++i) codec_store_block(C.out(), e0, leadC, cnt, stagedCodes.x, i);
        }
    }
    if (wantD) D.finished("g711 decoded");
    if (wantC) C.finished("g711 codes");
    compare<F32, In>(R, in.data(), LAW, wantD ? D.out() : nullptr, wantC ? C.out() : nullptr, "g711");
}

// ---- klatt_code_adpcm -----------------------------------------------------------------------------------------------------------------------
// The stores of one tile of one output: lane by lane, as codec_store_rows walks the rows
template <typename T>
static void model_store(Guarded<T>& G, const FilterRow* rows, long long rowStride, long long t0, const int* region, int pitch, int at)
{
    constexpr int PER = kCodecStoreLanes<T>;
    const int mis = tile_mis<T>(G.out());
    for (int lane = 0; lane < kFilterLanes; ++lane) {
        const int sub = lane / PER, i = lane % PER;
        for (int q0 = 0; q0 < kFilterLanes; q0 += kFilterLanes / PER) {
            const int q = q0 + sub;
            const FilterRow row = rows[q];
            if (row.sections == 0) continue;
            const int n = tile_n(rowStride, row.outLen, t0, kFilterTile);
            if (n <= 0) continue;
            CHECK(tile_lanes<T>(mis, row.dst + t0, n) <= PER, "%d lanes for a row's run", tile_lanes<T>(mis, row.dst + t0, n));
            if (i == 0) G.mark(row.dst + t0, n);
            T values[kFilterTile];
            memcpy(values, region + q * pitch + at, sizeof values);      // (inside the row's pitch: the run is at most 64 dwords from `at`)
            codec_store_row(G.out(), mis, row.dst, row.outLen, rowStride, t0, values, i);
        }
    }
}

template <int OUT, bool F32, typename In>
static void model_adpcm(int n, bool padded, int shift)
{
    using T = TileValue<F32>;
    constexpr int PITCH = codec_pitch(OUT), CODES_AT = codec_codes_at(OUT);
    constexpr bool DECODED = (OUT & kCodeDecoded) != 0, CODES = (OUT & kCodeCodes) != 0;
    static_assert(CODES_AT * 4 + kFilterTile <= PITCH * 4 && (!DECODED || !CODES || CODES_AT >= kFilterTile), "the codes' run lies inside the row and behind the decoded samples");
    static const int lengths[] = {0, 1, 2, kFilterTile - 1, kFilterTile, kFilterTile + 1, 3 * kFilterTile + 5, 5};
    const Rows R = make_rows(n, lengths, 8, padded);
    std::vector<In> in((size_t)R.inputs);
    for (auto& v : in) v = random_sample<In>();
    std::vector<FilterRow> packed;
    std::vector<FilterGroup> groups;
    filter_pack(R.rows, packed, groups);
    CHECK(groups.size() == (size_t)(n + kFilterLanes - 1) / kFilterLanes, "%zu groups for %d rows: one bucket", groups.size(), n);
    Guarded<T> D(R.outputs, shift);
    Guarded<uint8_t> C(R.outputs, shift);
    for (const FilterGroup& G : groups) {
        CHECK(G.bucket == 1, "bucket %lld", G.bucket);
        const FilterRow* rows = packed.data() + G.first;
        std::vector<int> region((size_t)kFilterLanes * PITCH, 0x7A7A7A7A);
        int val[kFilterLanes], idx[kFilterLanes];
        for (int lane = 0; lane < kFilterLanes; ++lane) val[lane] = idx[lane] = 0;
        const long long width = R.rowStride > 0 ? R.rowStride : G.outMost;
        bool zeroed = false;
        for (long long t0 = 0; t0 < width; t0 += kFilterTile) {
            if (t0 < G.outMost) {
                for (int q = 0; q < kFilterLanes; ++q)
                    for (int lane = 0; lane < kFilterLanes; ++lane) {      // filter_load_rows, then the region's int32 samples
                        const long long left = rows[q].len - t0;
                        const int has = (int)(left < 0 ? 0 : left < kFilterTile ? left : kFilterTile);
                        In v = (In)0;
                        if (t0 < G.inMost && tile_inside(lane, has)) {
                            CHECK(rows[q].src + t0 + lane >= 0 && rows[q].src + t0 + lane < R.inputs, "load of element %lld", rows[q].src + t0 + lane);
                            v = in[(size_t)(rows[q].src + t0 + lane)];
                        }
                        region[(size_t)(q * PITCH + lane)] = codec_sample(v);
                    }
                for (int lane = 0; lane < kFilterLanes; ++lane) {
                    int* mine = region.data() + lane * PITCH;
                    unsigned char* bytes = reinterpret_cast<unsigned char*>(mine);
                    const long long live = rows[lane].outLen - t0;
                    for (int t = 0; t < kFilterTile; ++t) {
                        int s;
                        memcpy(&s, bytes + 4 * t, 4);
                        CHECK(s >= -32768 && s <= 32767, "lane %d read %d at %d: a staged value was written over a sample not yet read", lane, s, t);
                        const int code = adpcm_encode(s, kAdpcmTable.step[idx[lane]], val[lane], idx[lane]);
                        if (DECODED) { const T v = t < live ? codec_value<F32>(val[lane]) : (T)0; memcpy(bytes + sizeof(T) * (size_t)t, &v, sizeof v); }
                        if (CODES) bytes[4 * CODES_AT + t] = t < live ? (unsigned char)code : (unsigned char)0;
                    }
                }
            } else if (!zeroed) {
                for (int lane = 0; lane < kFilterLanes; ++lane)
                    for (int t = 0; t < PITCH; ++t) region[(size_t)(lane * PITCH + t)] = 0;
                zeroed = true;
            }
            if (DECODED) model_store<T>(D, rows, R.rowStride, t0, region.data(), PITCH, 0);
            if (CODES) model_store<uint8_t>(C, rows, R.rowStride, t0, region.data(), PITCH, CODES_AT);
        }
    }
    if (DECODED) D.finished("adpcm decoded");
    if (CODES) C.finished("adpcm codes");
    compare<F32, In>(R, in.data(), kCodecAdpcm, DECODED ? D.out() : nullptr, CODES ? C.out() : nullptr, "adpcm");
}

// The statements among themselves: the decoder rebuilds the encoder's samples and state; a float32 row is the int16 row it rounds to
static void statements()
{
    std::vector<int16_t> x(3000);
    for (auto& v : x) v = random_sample<int16_t>();
    std::vector<float> xf(x.size());
    for (size_t i = 0; i < x.size(); ++i) xf[i] = tile_x(x[i]);
    for (int codec = 0; codec < kCodecCount; ++codec) {
        std::vector<int16_t> d(x.size()), d2(x.size()), back(x.size());
        std::vector<uint8_t> c(x.size()), c2(x.size());
        int st[2], st2[2], st3[2];
        code_host(x.data(), (long long)x.size(), codec, 0, d.data(), c.data(), st);
        code_host(xf.data(), (long long)x.size(), codec, 0, d2.data(), c2.data(), st2);
        CHECK(d == d2 && c == c2 && st[0] == st2[0] && st[1] == st2[1], "codec %d: the float32 row", codec);
        CHECK(decode_bad_code(c.data(), (long long)c.size(), codec) == -1, "codec %d: a code above 15", codec);
        decode_host(c.data(), (long long)c.size(), codec, 0, back.data(), st3);
        CHECK(back == d && st3[0] == st[0] && st3[1] == st[1], "codec %d: the decoder alone", codec);
    }
    for (int s = -32768; s <= 32767; ++s) CHECK(codec_sample(tile_x(s)) == s, "res_int16(tile_x(%d))", s);
}

int main()
{
    statements();
    const int counts[] = {0, 1, 63, 64, 65, 130}, shifts[] = {0, 1, 3};
    int variant = 0;
    // ADPCM: the ten instantiations at every row count and form, the shifts in turn
    for (int padded = 0; padded < 2; ++padded)
        for (int n : counts)
            for (int each = 0; each < 10; ++each, ++variant) {
                const int shift = shifts[(variant / 10) % 3];
                const bool p = padded != 0;
                constexpr int D = kCodeDecoded, C = kCodeCodes;
                switch (variant % 10) {
                    case 0: model_adpcm<D, false, int16_t>(n, p, shift); break;
                    case 1: model_adpcm<D, true, int16_t>(n, p, shift); break;
                    case 2: model_adpcm<C, false, int16_t>(n, p, shift); break;
                    case 3: model_adpcm<D | C, false, int16_t>(n, p, shift); break;
                    case 4: model_adpcm<D | C, true, int16_t>(n, p, shift); break;
                    case 5: model_adpcm<D, false, float>(n, p, shift); break;
                    case 6: model_adpcm<D, true, float>(n, p, shift); break;
                    case 7: model_adpcm<C, false, float>(n, p, shift); break;
                    case 8: model_adpcm<D | C, false, float>(n, p, shift); break;
                    default: model_adpcm<D | C, true, float>(n, p, shift); break;
                }
            }
    // G.711: law, formats and outputs in turn
    variant = 0;
    for (int padded = 0; padded < 2; ++padded)
        for (int n : counts)
            for (int each = 0; each < 3; ++each, ++variant) {
                const int shift = shifts[(variant / 8) % 3], outputs = 1 + variant % 3;
                const bool p = padded != 0;
                switch (variant % 8) {
                    case 0: model_g711<kCodecUlaw, false, int16_t>(n, p, outputs, shift); break;
                    case 1: model_g711<kCodecAlaw, true, int16_t>(n, p, outputs, shift); break;
                    case 2: model_g711<kCodecUlaw, true, float>(n, p, outputs, shift); break;
                    case 3: model_g711<kCodecAlaw, false, float>(n, p, outputs, shift); break;
                    case 4: model_g711<kCodecUlaw, true, int16_t>(n, p, outputs, shift); break;
                    case 5: model_g711<kCodecAlaw, false, int16_t>(n, p, outputs, shift); break;
                    case 6: model_g711<kCodecUlaw, false, float>(n, p, outputs, shift); break;
                    default: model_g711<kCodecAlaw, true, float>(n, p, outputs, shift); break;
                }
            }
    printf("ok %lld\n", checks);
    return 0;
}
