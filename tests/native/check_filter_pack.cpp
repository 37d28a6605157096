// check_filter_pack.cpp -- the packing of the filter export (nvspeechplayer_amd/csrc/klatt_filter.h: filter_pack, filter_bucket) held to
// its properties -- every row once, one bucket per group, outputs non-increasing within a group, the rows themselves untouched -- and a
// model of the kernel written from the shared functions alone (the masked loads, the in-place staging at the row pitch, the row writer
// of klatt_tiles.h): for every group and tile it stays inside the input, the region and the output, writes every element of the output
// exactly once and arrives at the statement's bits, padded and packed, both formats, at an output aligned to 16 bytes and 1 and 3
// elements past.  Built with AddressSanitizer + UBSan by tests/test_filter_host.py; prints "ok <checks>" or the first failure.
#include "../../nvspeechplayer_amd/csrc/klatt_filter.h"

#include <stdlib.h>
#include <string.h>

using namespace klatt;

static long long checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static uint32_t rng_state = 2463534242u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static const int kLengths[] = {0, 1, kFilterTile - 1, kFilterTile, kFilterTile + 1, 2 * kFilterTile + 3, 200, 5};
static const int kSections[] = {1, 2, 3, 5, 8, 9, 16};

// n rows of mixed K and lengths, the inputs back to back from element 3, the outputs padded (rowStride) or back to back
static std::vector<FilterRow> make_rows(int n, long long tail, long long& rowStride, bool padded, long long& inputs, long long& outputs)
{
    std::vector<FilterRow> rows;
    long long src = 3, most = 0;
    for (int i = 0; i < n; ++i) {
        const long long L = kLengths[rng() % 8u], K = kSections[rng() % 7u];
        rows.push_back(FilterRow{src, L, filter_length(L, tail), 0, (long long)(rng() % 100u), K});
        src += L + (long long)(rng() % 3u);
        most = std::max(most, L + tail);
    }
    inputs = src + 2;
    rowStride = padded ? most + (long long)(rng() % 5u) : 0;
    long long before = 0;
    for (int i = 0; i < n; ++i) { rows[(size_t)i].dst = padded ? i * rowStride : before; before += rows[(size_t)i].outLen; }
    outputs = padded ? n * rowStride : before;
    return rows;
}

static bool same_row(const FilterRow& a, const FilterRow& b) { return memcmp(&a, &b, sizeof a) == 0; }

static void properties(int n, long long tail, bool padded)
{
    long long rowStride, inputs, outputs;
    const std::vector<FilterRow> rows = make_rows(n, tail, rowStride, padded, inputs, outputs);
    std::vector<FilterRow> packed;
    std::vector<FilterGroup> groups;
    filter_pack(rows, packed, groups);
    CHECK(packed.size() == groups.size() * (size_t)kFilterLanes, "%zu rows in %zu groups", packed.size(), groups.size());
    CHECK(groups.size() >= (size_t)(n + kFilterLanes - 1) / kFilterLanes && (n > 0 || groups.empty()), "%zu groups for %d rows", groups.size(), n);
    std::vector<int> seen((size_t)n, 0);
    long long lastBucket = 0;
    for (size_t g = 0; g < groups.size(); ++g) {
        const FilterGroup& G = groups[g];
        CHECK(G.first == (long long)g * kFilterLanes, "group %zu starts at %lld", g, G.first);
        CHECK(G.bucket >= lastBucket && (G.bucket == 1 || G.bucket == 2 || G.bucket == 4 || G.bucket == 8 || G.bucket == 16), "group %zu bucket %lld", g, G.bucket);
        lastBucket = G.bucket;
        long long before = -1, outMost = 0, inMost = 0;
        bool filler = false;
        for (int q = 0; q < kFilterLanes; ++q) {
            const FilterRow& r = packed[(size_t)G.first + (size_t)q];
            if (r.sections == 0) { filler = true; CHECK(r.len == 0 && r.outLen == 0 && q > 0, "filler %d of group %zu", q, g); continue; }
            CHECK(!filler, "row %d of group %zu lies behind a filler", q, g);
            CHECK(filter_bucket(r.sections) == G.bucket && r.sections <= G.bucket, "row %d of group %zu has %lld sections in bucket %lld", q, g, r.sections, G.bucket);
            CHECK(before < 0 || r.outLen <= before, "row %d of group %zu has %lld outputs behind %lld", q, g, r.outLen, before);
            before = r.outLen; outMost = std::max(outMost, r.outLen); inMost = std::max(inMost, r.len);
            // the row is one of the caller's, untouched (dst identifies it: padded rows differ in it; packed rows of no outputs may share it)
            int which = -1;
            for (int i = 0; i < n && which < 0; ++i) if (!seen[(size_t)i] && same_row(rows[(size_t)i], r)) which = i;
            CHECK(which >= 0, "row %d of group %zu is none of the caller's", q, g);
            seen[(size_t)which] = 1;
        }
        CHECK(G.outMost == outMost && G.inMost == inMost, "group %zu: outMost %lld inMost %lld", g, G.outMost, G.inMost);
    }
    for (int i = 0; i < n; ++i) CHECK(seen[(size_t)i] == 1, "row %d of %d is in no group", i, n);
}

static FilterSection random_section()
{
    const float r = 0.5f + (float)(rng() % 400u) / 1000.0f, c = (float)((int)(rng() % 2001u) - 1000) / 1000.0f;
    const float u = (float)((int)(rng() % 2001u) - 1000) / 1000.0f;
    return FilterSection{0.3f + 0.2f * u, 0.1f * c, -0.05f * u, 2.0f * r * c, -(r * r)};      // poles at r exp(+-i acos c)
}

template <typename In> static In random_sample();
template <> int16_t random_sample<int16_t>() { return (rng() % 9u) == 0 ? (int16_t)0 : (int16_t)((int)(rng() % 65535u) - 32767); }
template <> float random_sample<float>() { return (rng() % 9u) == 0 ? ((rng() & 1u) ? 0.0f : -0.0f) : (float)((int)(rng() % 65535u) - 32767) / 8192.0f; }

// One group as the kernel takes it, a lane at a time where the kernel's lanes are independent between its barriers
template <bool F32, typename In>
static void model_group(const int K, const In* in, long long inputs, const FilterRow* rows, const FilterGroup& G, const FilterSection* sections, long long rowStride, void* out,
                        long long outFirst, long long outputs, std::vector<int>& written)
{
    using T = TileValue<F32>;
    constexpr int PER = sizeof(T) == 4 ? 32 : 16;
    std::vector<float> region((size_t)kFilterLanes * kFilterPitch, 7.0f);
    FilterSection c[kFilterLanes][kFilterMaxSections];
    float s1[kFilterLanes][kFilterMaxSections], s2[kFilterLanes][kFilterMaxSections];
    for (int lane = 0; lane < kFilterLanes; ++lane)
        for (int j = 0; j < K; ++j) {
            const FilterRow& me = rows[lane];
            c[lane][j] = j < me.sections ? sections[me.secAt + j] : kFilterIdentity;
            s1[lane][j] = s2[lane][j] = 0.0f;
        }
    const long long width = rowStride > 0 ? rowStride : G.outMost;
    bool zeroed = false;
    const int mis = tile_mis<T>(static_cast<T*>(out) + outFirst);
    for (long long t0 = 0; t0 < width; t0 += kFilterTile) {
        if (t0 < G.outMost) {
            for (int q = 0; q < kFilterLanes; ++q)
                for (int lane = 0; lane < kFilterLanes; ++lane) {
                    const long long s = t0 + lane;
                    In v = (In)0;
                    if (t0 < G.inMost && tile_inside(s, rows[q].len)) {
                        CHECK(rows[q].src + s >= 0 && rows[q].src + s < inputs, "load of element %lld", rows[q].src + s);
                        v = in[rows[q].src + s];
                    }
                    region[(size_t)(q * kFilterPitch + lane)] = tile_x(v);
                }
            for (int lane = 0; lane < kFilterLanes; ++lane) {
                float* mine = region.data() + lane * kFilterPitch;
                T* staged = reinterpret_cast<T*>(mine);
                const long long live = rows[lane].outLen - t0;
                for (int t = 0; t < kFilterTile; ++t) {
                    float x;
                    memcpy(&x, mine + t, 4);
                    for (int j = 0; j < K; ++j) x = filter_section(c[lane][j], x, s1[lane][j], s2[lane][j]);
                    const T v = t < live ? res_value<F32>(filter_finish(x)) : (T)0;
                    memcpy(staged + t, &v, sizeof v);
                }
            }
        } else if (!zeroed) {
            for (int lane = 0; lane < kFilterLanes; ++lane)
                for (int t = 0; t < kFilterTile; ++t) region[(size_t)(lane * kFilterPitch + t)] = 0.0f;
            zeroed = true;
        }
        for (int lane = 0; lane < kFilterLanes; ++lane) {
            const int sub = lane / PER, i = lane % PER;
            for (int q0 = 0; q0 < kFilterLanes; q0 += kFilterLanes / PER) {
                const int q = q0 + sub;
                const FilterRow row = rows[q];
                if (row.sections == 0) continue;
                const int n = tile_n(rowStride, row.outLen, t0, kFilterTile);
                if (n <= 0) continue;
                CHECK(tile_lanes<T>(mis, row.dst + t0, n) <= PER, "%d lanes", tile_lanes<T>(mis, row.dst + t0, n));
                if (i >= tile_lanes<T>(mis, row.dst + t0, n)) continue;
                CHECK(row.dst + t0 >= 0 && row.dst + t0 + n <= outputs, "store of %d elements from %lld", n, row.dst + t0);
                if (i == 0) for (int e = 0; e < n; ++e) ++written[(size_t)(row.dst + t0 + e)];
                std::vector<T> values((size_t)kFilterTile);
                memcpy(values.data(), region.data() + q * kFilterPitch, sizeof(T) * (size_t)kFilterTile);
                tile_store_lane(static_cast<T*>(out) + outFirst, mis, row.dst + t0, n, values.data(), i);
            }
        }
    }
}

template <bool F32, typename In>
static void model(int n, long long tail, bool padded, int shift)
{
    using T = TileValue<F32>;
    long long rowStride, inputs, outputs;
    std::vector<FilterRow> rows = make_rows(n, tail, rowStride, padded, inputs, outputs);
    std::vector<FilterSection> sections(120);
    for (auto& s : sections) s = random_section();
    std::vector<In> in((size_t)inputs);
    for (auto& v : in) v = random_sample<In>();
    std::vector<FilterRow> packed;
    std::vector<FilterGroup> groups;
    filter_pack(rows, packed, groups);
    // the output between guards, its first element `shift` elements past a 16-byte boundary
    constexpr int GUARD = 16;
    void* block = aligned_alloc(16, ((size_t)(outputs + 2 * GUARD + shift) * sizeof(T) + 15) / 16 * 16);
    T* all = static_cast<T*>(block);
    for (long long e = 0; e < outputs + 2 * GUARD + shift; ++e) all[e] = (T)-7;
    std::vector<int> written((size_t)outputs, 0);
    for (const FilterGroup& G : groups) {
        const FilterRow* r = packed.data() + G.first;
        model_group<F32, In>((int)G.bucket, in.data(), inputs, r, G, sections.data(), rowStride, all, GUARD + shift, outputs, written);
    }
    for (long long e = 0; e < GUARD + shift; ++e) CHECK(all[e] == (T)-7, "the guard before, element %lld", e);
    for (long long e = 0; e < GUARD; ++e) CHECK(all[GUARD + shift + outputs + e] == (T)-7, "the guard behind, element %lld", e);
    for (long long e = 0; e < outputs; ++e) CHECK(written[(size_t)e] == 1, "element %lld of %lld written %d times (%d rows, padded %d)", e, outputs, written[(size_t)e], n, (int)padded);
    const T* got = all + GUARD + shift;
    for (int i = 0; i < n; ++i) {
        const FilterRow& r = rows[(size_t)i];
        std::vector<T> want((size_t)r.outLen + 1);
        CHECK(filter_host(in.data() + r.src, r.len, sections.data() + r.secAt, r.sections, tail, F32 ? 1 : 0, want.data()) == r.outLen, "row %d", i);
        CHECK(memcmp(got + r.dst, want.data(), sizeof(T) * (size_t)r.outLen) == 0, "row %d of %d: %lld samples, %lld sections", i, n, r.len, r.sections);
        const long long span = padded ? rowStride : r.outLen;
        for (long long e = r.outLen; e < span; ++e) {
            T zero = (T)0;
            CHECK(memcmp(got + r.dst + e, &zero, sizeof zero) == 0, "row %d: padding element %lld", i, e);
        }
    }
    free(block);
}

int main()
{
    for (long long K = 1; K <= kFilterMaxSections; ++K) {
        const int b = filter_bucket(K);
        CHECK(b >= K && (b == 1 || b / 2 < K), "bucket %d of %lld sections", b, K);
    }
    const int counts[] = {0, 1, 63, 64, 65, 130}, shifts[] = {0, 1, 3};
    int variant = 0;      // the twelve (formats, shift) variants in turn: each meets several row counts, tails and forms
    for (long long tail : {0ll, 1ll, (long long)kFilterTile + 3})
        for (int padded = 0; padded < 2; ++padded)
            for (int n : counts) {
                properties(n, tail, padded != 0);
                for (int twice = 0; twice < 2; ++twice, ++variant) {
                    const int shift = shifts[(variant / 4) % 3];
                    switch (variant % 4) {
                        case 0: model<true, int16_t>(n, tail, padded != 0, shift); break;
                        case 1: model<false, int16_t>(n, tail, padded != 0, shift); break;
                        case 2: model<true, float>(n, tail, padded != 0, shift); break;
                        default: model<false, float>(n, tail, padded != 0, shift); break;
                    }
                }
            }
    // the lemma, on the statement: identity sections in front, in the middle and behind
    {
        std::vector<float> x(500);
        for (auto& v : x) v = random_sample<float>();
        for (int i = 100; i < 140; ++i) x[(size_t)i] = (i & 1) ? 0.0f : -0.0f;
        const FilterSection a = random_section(), b = random_section();
        const FilterSection plain[2] = {a, b}, padded[5] = {kFilterIdentity, a, kFilterIdentity, b, kFilterIdentity};
        std::vector<float> y0(520), y1(520);
        filter_host(x.data(), 500, plain, 2, 20, 1, y0.data());
        filter_host(x.data(), 500, padded, 5, 20, 1, y1.data());
        CHECK(memcmp(y0.data(), y1.data(), 520 * 4) == 0, "the lemma");
    }
    printf("ok %lld\n", checks);
    return 0;
}
