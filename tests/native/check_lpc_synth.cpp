// check_lpc_synth.cpp -- a model of the LPC synthesis kernel's walk (nvspeechplayer_amd/csrc/klatt_lpcsynth.h: klatt_lpc_synth) written from
// the shared functions alone, against the statement lpc_synth_host: groups of 64 rows with fillers (lpc_synth_pack), 64-sample tiles with
// masked loads, the LDS region at the row pitch, the ring of B slots written after it is read, the wave-uniform frame change at
// lpc_synth_change with the per-row clamp and the next frame's coefficients fetched one frame ahead, frame changes inside tiles and on
// their edges, in-place staging in the output's type and the row writer of klatt_tiles.h.  For every group and tile it stays inside the
// input, the coefficients, the region and the output, writes every element of the output exactly once and arrives at the statement's
// bits: 1 .. 130 rows of 0 .. 200 samples, orders at both edges of every ring, hop 1 to beyond the rows, padded and packed, float64 and
// float32 coefficients at a column of their own, both sample formats in and out, the output 0, 1 and 3 elements past a 16-byte boundary.
// lpc_synth_change is held to lpc_frame_of, and lpc_step_up to lpc_levinson.
// Built with AddressSanitizer + UBSan by tests/test_lpc_synthesis_host.py; prints "ok <checks>" or the first failure.
#include "../../nvspeechplayer_amd/csrc/klatt_lpcsynth.h"

#include <stdlib.h>
#include <string.h>

using namespace klatt;

static long long checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static uint32_t rng_state = 2463534242u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

template <typename In> static In random_sample();
template <> int16_t random_sample<int16_t>() { return (rng() % 9u) == 0 ? (int16_t)0 : (int16_t)((int)(rng() % 65535u) - 32767); }
template <> float random_sample<float>() { return (rng() % 9u) == 0 ? ((rng() & 1u) ? 0.0f : -0.0f) : (float)((int)(rng() % 65535u) - 32767) / 8192.0f; }

// a_1 .. a_order of a stable 1 / A(z): reflection coefficients in (-0.9, 0.9) through the step-up recursion; now and then all zeros
static void random_frame(int order, double* a)
{
    double k[kLpcMaxOrder + 1] = {}, aa[kLpcMaxOrder + 1];
    if (rng() % 7u) for (int i = 1; i <= order; ++i) k[i] = (double)((int)(rng() % 1801u) - 900) / 1000.0;
    lpc_step_up(k, order, aa);
    for (int i = 1; i <= order; ++i) a[i - 1] = aa[i];
}

static const int kLengths[] = {0, 1, 3, kFilterTile - 1, kFilterTile, kFilterTile + 1, 2 * kFilterTile, 2 * kFilterTile + 1, 200};

// One group as the kernel takes it: the samples in order, the lanes one after another where the kernel's lanes are independent
template <int B, bool F32, typename In, typename C>
static void model_group(const In* in, long long inputs, const LpcSynthRow* rows, const FilterGroup& G, const C* coeff, long long coeffElements, int coeffCols, int col0, int order,
                        long long hop, long long phase, long long rowStride, void* out, long long outFirst, long long outputs, std::vector<int>& written)
{
    using T = TileValue<F32>;
    constexpr int PER = sizeof(T) == 4 ? 32 : 16;
    static_assert(kFilterTile % B == 0, "a tile is whole turns of the ring");
    std::vector<float> region((size_t)kFilterLanes * kFilterPitch, 7.0f);
    static double a[kFilterLanes][B];
    static C an[kFilterLanes][B];
    static float ring[kFilterLanes][B];
    const auto at = [&](const LpcSynthRow& me, long long k, int m) {
        const long long e = (me.coeff + lpc_synth_clamp(k, me.steps)) * coeffCols + col0 + m;
        CHECK(me.steps > 0 && e >= 0 && e < coeffElements, "coefficient element %lld of %lld", e, coeffElements);
        return coeff[e];
    };
    for (int lane = 0; lane < kFilterLanes; ++lane) {
        const LpcSynthRow& me = rows[lane];
        const bool framed = me.steps > 0;
        for (int m = 0; m < B; ++m) {
            a[lane][m] = framed && m < order ? lpc_widen(at(me, 0, m)) : 0.0;
            an[lane][m] = framed && m < order ? at(me, 1, m) : (C)0;
            ring[lane][m] = 0.0f;
        }
    }
    long long k = 0, turn = lpc_synth_change(1, hop, phase);
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
                        CHECK(rows[q].sections == 1 && rows[q].src + s >= 0 && rows[q].src + s < inputs, "load of element %lld", rows[q].src + s);
                        v = in[rows[q].src + s];
                    }
                    region[(size_t)(q * kFilterPitch + lane)] = tile_x(v);
                }
            for (int tb = 0; tb < kFilterTile; tb += B)
                for (int u = 0; u < B; ++u) {
                    const int t = tb + u;
                    const bool change = t0 + t == turn;
                    if (change) { ++k; turn += hop; }
                    for (int lane = 0; lane < kFilterLanes; ++lane) {
                        const LpcSynthRow& me = rows[lane];
                        const bool framed = me.steps > 0;
                        if (change)
                            for (int m = 0; m < B; ++m)
                                if (m < order) {
                                    a[lane][m] = lpc_widen(an[lane][m]);
                                    an[lane][m] = framed ? at(me, k + 1, m) : (C)0;
                                }
                        float* mine = region.data() + lane * kFilterPitch;
                        T* staged = reinterpret_cast<T*>(mine);
                        const long long live = me.outLen - t0;
                        float x;
                        memcpy(&x, mine + t, 4);
                        const float y = lpc_synth_step<B>(x, a[lane], order, ring[lane], u);
                        ring[lane][u] = y;
                        const T v = t < live ? res_value<F32>(y) : (T)0;
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
                const LpcSynthRow row = rows[q];
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

template <bool F32, typename In, typename C>
static void model(int n, int order, long long hop, long long phase, bool padded, bool coeffPadded, int shift)
{
    using T = TileValue<F32>;
    // the rows: inputs from element 3 with gaps, outputs and coefficient steps padded or back to back
    std::vector<LpcSynthRow> rows;
    std::vector<long long> lens;
    long long src = 3, most = 0, mostSteps = 0, stepsBefore = 0, before = 0;
    for (int i = 0; i < n; ++i) {
        const long long L = (rng() & 1u) ? kLengths[rng() % 9u] : (long long)(rng() % 201u);
        lens.push_back(L);
        most = std::max(most, L);
        mostSteps = std::max(mostSteps, L > phase ? (L - phase + hop - 1) / hop : 0);
    }
    const long long rowStride = padded ? most + (long long)(rng() % 5u) : 0, coeffStride = coeffPadded ? mostSteps + (long long)(rng() % 2u) : 0;
    for (int i = 0; i < n; ++i) {
        const long long L = lens[(size_t)i], steps = L > phase ? (L - phase + hop - 1) / hop : 0;
        rows.push_back(lpc_synth_row(src, L, padded ? i * rowStride : before, coeffPadded ? i * coeffStride : stepsBefore, steps));
        src += L + (long long)(rng() % 3u);
        before += L; stepsBefore += steps;
    }
    const long long inputs = src + 2, outputs = padded ? n * rowStride : before, coeffSteps = coeffPadded ? n * coeffStride : stepsBefore;
    const int col0 = (int)(rng() % 3u), coeffCols = col0 + order + (int)(rng() % 2u);
    std::vector<In> in((size_t)inputs);
    for (auto& v : in) v = random_sample<In>();
    // the coefficients: every row's steps at its place in the tensor, in C, and as the statement takes them (binary64, the widened values)
    std::vector<C> coeff((size_t)(coeffSteps * coeffCols), (C)7);
    std::vector<std::vector<double>> host((size_t)n);
    for (int i = 0; i < n; ++i) {
        const LpcSynthRow& r = rows[(size_t)i];
        host[(size_t)i].resize((size_t)(r.steps * order));
        for (long long j = 0; j < r.steps; ++j) {
            double a[kLpcMaxOrder];
            random_frame(order, a);
            for (int m = 0; m < order; ++m) {
                const C c = (C)a[m];
                coeff[(size_t)((r.coeff + j) * coeffCols + col0 + m)] = c;
                host[(size_t)i][(size_t)(j * order + m)] = lpc_widen(c);
            }
        }
    }
    std::vector<LpcSynthRow> packed;
    std::vector<FilterGroup> groups;
    lpc_synth_pack(rows, packed, groups);
    CHECK(packed.size() == groups.size() * (size_t)kFilterLanes && groups.size() == (size_t)(n + kFilterLanes - 1) / kFilterLanes, "%zu rows in %zu groups for %d", packed.size(), groups.size(), n);
    for (size_t q = (size_t)n; q < packed.size(); ++q) CHECK(packed[q].sections == 0 && packed[q].len == 0 && packed[q].steps == 0, "filler %zu", q);
    // the output between guards, its first element `shift` elements past a 16-byte boundary
    constexpr int GUARD = 16;
    void* block = aligned_alloc(16, ((size_t)(outputs + 2 * GUARD + shift) * sizeof(T) + 15) / 16 * 16);
    T* all = static_cast<T*>(block);
    for (long long e = 0; e < outputs + 2 * GUARD + shift; ++e) all[e] = (T)-7;
    std::vector<int> written((size_t)outputs, 0);
    for (const FilterGroup& G : groups) {
        const LpcSynthRow* r = packed.data() + G.first;
        const long long ce = (long long)coeff.size();
        switch (lpc_synth_history(order)) {
            case 8: model_group<8, F32, In, C>(in.data(), inputs, r, G, coeff.data(), ce, coeffCols, col0, order, hop, phase, rowStride, all, GUARD + shift, outputs, written); break;
            case 16: model_group<16, F32, In, C>(in.data(), inputs, r, G, coeff.data(), ce, coeffCols, col0, order, hop, phase, rowStride, all, GUARD + shift, outputs, written); break;
            default: model_group<32, F32, In, C>(in.data(), inputs, r, G, coeff.data(), ce, coeffCols, col0, order, hop, phase, rowStride, all, GUARD + shift, outputs, written); break;
        }
    }
    for (long long e = 0; e < GUARD + shift; ++e) CHECK(all[e] == (T)-7, "the guard before, element %lld", e);
    for (long long e = 0; e < GUARD; ++e) CHECK(all[GUARD + shift + outputs + e] == (T)-7, "the guard behind, element %lld", e);
    for (long long e = 0; e < outputs; ++e) CHECK(written[(size_t)e] == 1, "element %lld of %lld written %d times (%d rows, padded %d)", e, outputs, written[(size_t)e], n, (int)padded);
    const T* got = all + GUARD + shift;
    for (int i = 0; i < n; ++i) {
        const LpcSynthRow& r = rows[(size_t)i];
        std::vector<T> want((size_t)r.len + 1);
        lpc_synth_host(in.data() + r.src, r.len, order, hop, phase, host[(size_t)i].data(), F32 ? 1 : 0, want.data());
        for (long long e = 0; e < r.len; ++e)
            CHECK(memcmp(got + r.dst + e, want.data() + e, sizeof(T)) == 0, "row %d of %d: sample %lld of %lld, order %d hop %lld phase %lld", i, n, e, r.len, order, hop, phase);
        const long long span = padded ? rowStride : r.len;
        for (long long e = r.len; e < span; ++e) {
            T zero = (T)0;
            CHECK(memcmp(got + r.dst + e, &zero, sizeof zero) == 0, "row %d: padding element %lld", i, e);
        }
    }
    free(block);
}

int main()
{
    // the ring of an order
    for (int order = 1; order <= kLpcMaxOrder; ++order) {
        const int b = lpc_synth_history(order);
        CHECK(b >= order && (b == 8 || b / 2 < order) && (b == 8 || b == 16 || b == 32), "ring %d of order %d", b, order);
    }
    // the unclamped frame turns to k exactly at lpc_synth_change(k)
    for (long long hop : {1ll, 2ll, 3ll, 7ll, 64ll, 160ll, 1000ll})
        for (long long phase : {0ll, 1ll, 7ll, 32ll, 500ll}) {
            long long k = 0, turn = lpc_synth_change(1, hop, phase);
            for (long long t = 0; t < 2100; ++t) {
                if (t == turn) { ++k; turn += hop; }
                CHECK(lpc_frame_of(t, hop, phase, 1ll << 40) == k, "frame of %lld at hop %lld phase %lld", t, hop, phase);
                for (long long steps : {1ll, 2ll, 5ll}) CHECK(lpc_frame_of(t, hop, phase, steps) == lpc_synth_clamp(k, steps), "clamped frame of %lld", t);
            }
        }
    // the step-up recursion is the Levinson-Durbin update: from the k of a recursion that ran to the end, its a
    for (int order = 1; order <= kLpcMaxOrder; ++order) {
        double r[kLpcMaxOrder + 1], a[kLpcMaxOrder + 1], k[kLpcMaxOrder + 1], up[kLpcMaxOrder + 1], E;
        int stages;
        for (int i = 0; i <= kLpcMaxOrder; ++i) r[i] = (i == 0 ? 1.001 : 0.0) + 0.9 * pow(0.7, i) * cos(0.9 * i) + 0.05 * pow(0.95, i) * cos(2.1 * i);
        lpc_levinson(r, order, a, k, E, stages);
        CHECK(stages == order, "order %d stopped at stage %d", order, stages);
        lpc_step_up(k, order, up);
        CHECK(memcmp(a + 1, up + 1, sizeof(double) * (size_t)order) == 0, "step-up of order %d", order);
    }
    const int orders[] = {1, 8, 9, 16, 17, 32, 5, 24}, shifts[] = {0, 1, 3};
    const long long hops[] = {1, 7, 64, 160, 8192, 3, 32}, phases[] = {0, 7, 32};
    int variant = 0;
    for (int n = 1; n <= 130; ++n, ++variant) {
        const int order = orders[(variant + variant / 8) % 8], shift = shifts[(variant / 8) % 3];
        const long long hop = hops[variant % 7], phase = phases[(variant / 7) % 3];
        const bool padded = (variant / 2) % 2 != 0, coeffPadded = (variant / 3) % 2 != 0;
        switch (variant % 8) {
            case 0: model<true, int16_t, double>(n, order, hop, phase, padded, coeffPadded, shift); break;
            case 1: model<false, int16_t, float>(n, order, hop, phase, padded, coeffPadded, shift); break;
            case 2: model<true, float, float>(n, order, hop, phase, padded, coeffPadded, shift); break;
            case 3: model<false, float, double>(n, order, hop, phase, padded, coeffPadded, shift); break;
            case 4: model<true, int16_t, float>(n, order, hop, phase, padded, coeffPadded, shift); break;
            case 5: model<false, int16_t, double>(n, order, hop, phase, padded, coeffPadded, shift); break;
            case 6: model<true, float, double>(n, order, hop, phase, padded, coeffPadded, shift); break;
            default: model<false, float, float>(n, order, hop, phase, padded, coeffPadded, shift); break;
        }
    }
    printf("ok %lld\n", checks);
    return 0;
}
