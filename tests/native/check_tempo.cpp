// check_tempo.cpp -- models of the two kernels of the tempo exports (nvspeechplayer_amd/csrc/klatt_tempo.h) written from the shared
// functions alone, against brute force written here from the definition in include/speechPlayer_batch.h.  klatt_tempo_search: per frame
// the template and the region staged lane by lane (tile_read_lane), lane t of 256 over the lags t, t + 256, ..., the butterfly over the 64
// lanes of a wavefront (partner lane ^ m, as the shuffle pairs them), the four wavefronts' winners reduced by lane 0, p[k] handed to the
// next frame -- held to a linear scan over d = -D .. D with tempo_better and to the host statement, on rows with silences, constant
// stretches and exact periods (planted ties), and on (score, rank) sets with equal scores reduced in every rotation.
// klatt_tempo_render: the tile walk (tile_row_table, tile_row and the bisection of the packed form, tile_n, tile_live), the tile's
// positions staged (at most kTempoTilePositions), padded and packed positions, wild positions, the row writer with first elements 0, 1
// and 3 past a 16-byte boundary, rows around the tile's length, and row offsets beyond 2^32 (the output's and the positions' base pointers
// moved back by as much, so that only 64-bit arithmetic finds the elements): every element written exactly once, the guards stay, the
// bits are brute force's and the host statement's.
// Built with AddressSanitizer + UBSan by tests/test_tempo_host.py; prints "ok <checks>" or the first failure.
#include "../../nvspeechplayer_amd/csrc/klatt_tempo.h"
#include "../../nvspeechplayer_amd/csrc/klatt_tiles.h"
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

// ---- brute force, from the header's text ---------------------------------------------------------------------------------------------------
template <typename In> static float brute_x(const In* x, long long L, long long s) { return s >= 0 && s < L ? tile_x(x[s]) : 0.0f; }

template <typename In>
static double brute_score(const In* x, long long L, long long t0, long long c0, int N)
{
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < N; ++i) c[i % 4] += (double)brute_x(x, L, t0 + i) * (double)brute_x(x, L, c0 + i);      // (the product is exact: no fma needed)
    return (c[0] + c[1]) + (c[2] + c[3]);
}

template <typename In>
static std::vector<long long> brute_positions(const In* x, long long L, int N, int D, double tempo, long long K, long long& ties)
{
    const int Hs = N / 2;
    std::vector<long long> p((size_t)K, 0);
    for (long long k = 1; k < K; ++k) {
        const long long a = (long long)floor((double)(k * Hs) * tempo);
        // the order of the ties, 0, -1, +1, -2, ...: the first of the greatest wins
        double best = 0.0;
        int bestD = 0, equal = 0;
        for (int r = 0; r <= 2 * D; ++r) {
            const int d = r == 0 ? 0 : (r % 2 ? -(r + 1) / 2 : r / 2);
            const double s = brute_score(x, L, p[(size_t)(k - 1)], a - Hs + d, N);
            if (r == 0 || s > best) { best = s; bestD = d; equal = 0; }
            else if (s == best) ++equal;
        }
        ties += equal;
        p[(size_t)k] = a + bestD;
    }
    return p;
}

// ---- klatt_tempo_search ---------------------------------------------------------------------------------------------------------------------
struct Pick { double score; int rank; };

// The workgroup's reduction of its 256 lanes' candidates: the butterfly inside each wavefront, then lane 0 over the four
static Pick model_reduce(std::vector<Pick> lane)
{
    for (int wave = 0; wave < 4; ++wave)
        for (int m = 1; m < 64; m <<= 1) {
            std::vector<Pick> next(lane.begin() + wave * 64, lane.begin() + wave * 64 + 64);
            for (int l = 0; l < 64; ++l) {
                const Pick mine = lane[(size_t)(wave * 64 + l)], other = lane[(size_t)(wave * 64 + (l ^ m))];
                next[(size_t)l] = tempo_better(other.score, other.rank, mine.score, mine.rank) ? other : mine;
            }
            for (int l = 0; l < 64; ++l) lane[(size_t)(wave * 64 + l)] = next[(size_t)l];
        }
    for (int wave = 0; wave < 4; ++wave)
        for (int l = 1; l < 64; ++l)
            CHECK(lane[(size_t)(wave * 64 + l)].rank == lane[(size_t)(wave * 64)].rank, "the butterfly leaves every lane of wavefront %d the same winner", wave);
    Pick best = lane[0];
    for (int v = 1; v < 4; ++v)
        if (tempo_better(lane[(size_t)(v * 64)].score, lane[(size_t)(v * 64)].rank, best.score, best.rank)) best = lane[(size_t)(v * 64)];
    return best;
}

template <typename In>
static void model_search(const std::vector<In>& row, int N, int D, double tempo, const char* kind)
{
    char name[160];
    snprintf(name, sizeof name, "search %s L %zu N %d D %d tempo %g in %zu", kind, row.size(), N, D, tempo, sizeof(In));
    const long long L = (long long)row.size();
    const int Hs = N / 2, nLags = 2 * D + 1;
    const long long Lout = tempo_out_length(L, tempo), K = tempo_frames(Lout, Hs);
    std::vector<float> Ts((size_t)N), Rs((size_t)N + 2 * (size_t)D);      // exactly the LDS a frame uses: a read past it is past the vector
    std::vector<long long> p((size_t)K, -1);
    long long previous = 0;
    if (K > 0) p[0] = 0;
    for (long long k = 1; k < K; ++k) {
        const long long a = tempo_nominal(k, Hs, tempo);
        for (int lane = 0; lane < 256; ++lane) {
            tile_read_lane<1>(Ts.data(), row.data(), L, previous, N, lane, 256);
            tile_read_lane<1>(Rs.data(), row.data(), L, a - Hs - D, N + 2 * D, lane, 256);
        }
        std::vector<Pick> lanes(256);
        for (int lane = 0; lane < 256; ++lane) {
            Pick best{tempo_no_score(), kTempoNoRank};
            for (int j = lane; j < nLags; j += 256) {
                const double s = tempo_score(Ts.data(), Rs.data() + j, N);
                const int r = tempo_rank(j - D);
                if (tempo_better(s, r, best.score, best.rank)) best = Pick{s, r};
            }
            lanes[(size_t)lane] = best;
        }
        const Pick won = model_reduce(lanes);
        // the linear scan
        Pick scan{tempo_no_score(), kTempoNoRank};
        for (int j = 0; j < nLags; ++j) {
            const double s = tempo_score(Ts.data(), Rs.data() + j, N);
            if (tempo_better(s, tempo_rank(j - D), scan.score, scan.rank)) scan = Pick{s, tempo_rank(j - D)};
        }
        CHECK(won.rank == scan.rank && memcmp(&won.score, &scan.score, 8) == 0, "%s: frame %lld: rank %d against the scan's %d", name, k, won.rank, scan.rank);
        CHECK(won.rank >= 0 && won.rank <= 2 * D && tempo_rank((int)tempo_lag(won.rank)) == won.rank, "%s: frame %lld: rank %d", name, k, won.rank);
        p[(size_t)k] = previous = a + tempo_lag(won.rank);
    }
    long long ties = 0;
    const std::vector<long long> want = brute_positions(row.data(), L, N, D, tempo, K, ties);
    TempoPlan P;
    std::string why;
    CHECK(tempo_plan(P, N, D, true, why), "%s: %s", name, why.c_str());
    std::vector<long long> host((size_t)K + 1, -3);
    tempo_positions_host(row.data(), L, P, tempo, K, host.data());
    for (long long k = 0; k < K; ++k) {
        CHECK(p[(size_t)k] == want[(size_t)k], "%s: frame %lld: %lld against brute force's %lld", name, k, p[(size_t)k], want[(size_t)k]);
        CHECK(host[(size_t)k] == want[(size_t)k], "%s: the statement, frame %lld: %lld against %lld", name, k, host[(size_t)k], want[(size_t)k]);
    }
    CHECK(host[(size_t)K] == -3, "%s: the statement wrote past its frames", name);
    if (D > 0 && K > 3 && (!strcmp(kind, "period") || !strcmp(kind, "constant"))) CHECK(ties > 0, "%s: no frame had a tie", name);
}

template <typename In>
static std::vector<In> make_row(const char* kind, long long L)
{
    std::vector<In> row((size_t)L);
    for (long long t = 0; t < L; ++t) {
        In v = random_sample<In>();
        if (!strcmp(kind, "period")) v = (In)(std::is_same<In, float>::value ? 0.25 * (double)((t % 16) - 8) : (double)(1000 * ((t % 16) - 8)));      // exact period 16: equal scores 16 lags apart
        if (!strcmp(kind, "constant")) v = (In)(std::is_same<In, float>::value ? 0.375 : 1234.0);
        if (!strcmp(kind, "silence") && t > L / 4 && t < 3 * L / 4) v = (In)(std::is_same<In, float>::value && (t & 1) ? -0.0 : 0.0);
        row[(size_t)t] = v;
    }
    return row;
}

// ---- klatt_tempo_render ---------------------------------------------------------------------------------------------------------------------
constexpr int GUARD = 32;
constexpr long long FAR = (1ll << 32) + (1ll << 31) + 64;      // elements the fake offsets add (a multiple of 8: the alignment stays)

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

// A pointer `far` elements before p, by integer arithmetic: only p + (far + e) is ever formed again
template <typename T> static T* moved_back(T* p, long long far) { return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) - (uintptr_t)far * sizeof(T)); }

struct Row { long long src, len, outLen, dst, pos, frames; double tempo; };

template <bool F32, typename In>
static void model_render(const std::vector<long long>& lengths, int N, bool padded, bool posPadded, int shift, bool far, int wild)
{
    using T = TileValue<F32>;
    char name[200];
    snprintf(name, sizeof name, "render %zu rows N %d padded %d positions padded %d shift %d far %d wild %d f32 %d in %zu", lengths.size(), N, (int)padded, (int)posPadded, shift,
             (int)far, wild, (int)F32, sizeof(In));
    const int Hs = N / 2;
    const double tempos[5] = {0.25, 0.8, 1.0, 1.1, 4.0};
    const long long n = (long long)lengths.size();
    std::vector<Row> rows;
    std::vector<long long> outLen;
    long long src = 3, most = 0, mostFrames = 0, total = 0, totalFrames = 0;
    for (long long i = 0; i < n; ++i) {
        const long long L = lengths[(size_t)i];
        const double tempo = tempos[i % 5];
        const long long Lout = tempo_out_length(L, tempo), K = tempo_frames(Lout, Hs);
        rows.push_back(Row{src, L, Lout, 0, 0, K, tempo});
        outLen.push_back(Lout);
        src += L + (long long)(rng() % 3u);
        most = std::max(most, Lout); mostFrames = std::max(mostFrames, K); total += Lout; totalFrames += K;
    }
    std::vector<In> in((size_t)src + 2);
    for (In& v : in) v = random_sample<In>();
    const long long rowStride = padded ? most + 1 + (long long)(rng() % 5u) : 0, posStride = posPadded ? mostFrames + 1 : 0;
    long long before = 0, framesBefore = 0;
    const long long fake = far ? FAR : 0;
    for (long long i = 0; i < n; ++i) {
        rows[(size_t)i].dst = fake + (padded ? i * rowStride : before);
        rows[(size_t)i].pos = fake + (posPadded ? i * posStride : framesBefore);
        before += rows[(size_t)i].outLen; framesBefore += rows[(size_t)i].frames;
    }
    // exactly the positions the rows' frames need: a read past them is past the vector
    std::vector<long long> pos((size_t)(posPadded ? n * posStride : totalFrames), 0);
    TempoPlan P;
    std::string why;
    CHECK(tempo_plan(P, N, 0, false, why), "%s: %s", name, why.c_str());
    for (long long i = 0; i < n; ++i) {
        const Row& r = rows[(size_t)i];
        long long* p = pos.data() + (r.pos - fake);
        for (long long k = 0; k < r.frames; ++k) {
            p[k] = tempo_nominal(k, Hs, r.tempo) + (long long)(rng() % 41u) - 20;
            if (wild && rng() % (unsigned)wild == 0) p[k] = (rng() & 1u) ? (rng() & 2u ? 0x7FFFFFFFFFFFFFFFll : 1ll << 62) : (rng() & 2u ? -0x7FFFFFFFFFFFFFFFll - 1 : -(1ll << 62));
        }
    }
    std::vector<long long> words;
    const TileTable tiles = tile_row_table(outLen.data(), n, kTempoTile, rowStride, kTimelineChunkLog2, words);
    Guarded<T> G(padded ? n * rowStride : total, shift);
    T* const out = moved_back(G.out(), fake);
    const long long* const posBase = moved_back(pos.data(), fake);
    std::vector<T> staged((size_t)kTempoTile);
    std::vector<long long> Ps((size_t)kTempoTilePositions);
    int mostStaged = 0;
    for (long long g = 0; g < tiles.nTiles; ++g) {
        long long r, j;
        if (rowStride > 0) tile_row(g, tiles.tilesPerRow, r, j);
        else { const long long c = g >> kTimelineChunkLog2; packed_locate(g, words.data() + tiles.table.startOff, words[(size_t)(tiles.table.chunkOff + c)], words[(size_t)(tiles.table.chunkOff + c + 1)] + 1, r, j); }
        const long long t0 = j * kTempoTile;
        const Row row = rows[(size_t)r];
        const int nn = tile_n(rowStride, row.outLen, t0, kTempoTile), live = tile_live(nn, row.outLen, t0);
        CHECK(nn > 0 && nn <= kTempoTile, "%s: tile %lld of %d elements", name, g, nn);
        long long q0 = 0;
        if (live > 0) {
            q0 = t0 / Hs;
            const int count = (int)((t0 + live - 1) / Hs - q0) + 2;
            CHECK(count >= 2 && count <= kTempoTilePositions && q0 + count <= row.frames, "%s: tile %lld stages %d positions from %lld of %lld", name, g, count, q0, row.frames);
            mostStaged = std::max(mostStaged, count);
            for (int c = 0; c < count; ++c) Ps[(size_t)c] = tempo_clamp(posBase[row.pos + q0 + c]);
        }
        const int base = (int)(t0 - q0 * Hs);
        for (int i = 0; i < nn; ++i) {
            T v = (T)0;
            if (i < live) {
                const int local = base + i, q = local / Hs, ii = local - q * Hs;
                CHECK(q + 1 < kTempoTilePositions, "%s: output %lld reads staged position %d", name, t0 + i, q + 1);
                v = res_value<F32>(tempo_render(P.window[(size_t)(Hs + ii)], tile_sample(in.data() + row.src, Ps[(size_t)q] + ii, row.len), P.window[(size_t)ii],
                                                tile_sample(in.data() + row.src, Ps[(size_t)(q + 1)] - Hs + ii, row.len)));
            }
            staged[(size_t)i] = v;
        }
        const int mis = tile_mis<T>(out), lanes = tile_lanes<T>(mis, row.dst + t0, nn);
        CHECK(mis == shift % kTileLane<T>, "%s: mis %d of shift %d", name, mis, shift);
        for (int i = 0; i < lanes; ++i) tile_store_lane(out, mis, row.dst + t0, nn, staged.data(), i);
        G.mark(row.dst - fake + t0, nn);
    }
    G.finished(name);
    if (N == kTempoMinWin && most >= kTempoTile) CHECK(mostStaged >= kTempoTile / Hs + 1, "%s: at most %d positions staged", name, mostStaged);

    // against brute force and the statement
    const T zero = (T)0;
    const double pi = 3.141592653589793;
    for (long long i = 0; i < n; ++i) {
        const Row& r = rows[(size_t)i];
        const long long* p = pos.data() + (r.pos - fake);
        const T* got = G.out() + (r.dst - fake);
        std::vector<T> host((size_t)r.outLen + 1, (T)-3);
        tempo_render_host(in.data() + r.src, r.len, P, r.outLen, p, F32 ? 1 : 0, host.data());
        for (long long m = 0; m < r.outLen; ++m) {
            const long long q = m / Hs, ii = m - q * Hs;
            const long long pa = std::min(std::max(p[q], -(1ll << 45)), 1ll << 45), pb = std::min(std::max(p[q + 1], -(1ll << 45)), 1ll << 45);
            const float wHi = (float)(0.5 - 0.5 * cos(2.0 * pi * (double)(Hs + ii) / (double)N)), wLo = (float)(0.5 - 0.5 * cos(2.0 * pi * (double)ii / (double)N));
            const float lo = wLo * brute_x(in.data() + r.src, r.len, pb - Hs + ii);
            const float y = fmaf(wHi, brute_x(in.data() + r.src, r.len, pa + ii), lo) + 0.0f;
            const T w = F32 ? (T)y : (T)res_int16(y);
            CHECK(memcmp(&w, &host[(size_t)m], sizeof w) == 0, "%s: the statement against brute force, row %lld output %lld", name, i, m);
            CHECK(memcmp(&w, got + m, sizeof w) == 0, "%s: row %lld output %lld", name, i, m);
        }
        CHECK(host[(size_t)r.outLen] == (T)-3, "%s: the statement wrote past row %lld", name, i);
        for (long long m = r.outLen; padded && m < rowStride; ++m) CHECK(memcmp(&zero, got + m, sizeof zero) == 0, "%s: row %lld: padding element %lld", name, i, m);
    }
}

int main()
{
    // the order of the choice
    for (int d = -kTempoMaxSearch; d <= kTempoMaxSearch; ++d) {
        CHECK(tempo_rank(d) == 2 * abs(d) - (d < 0 ? 1 : 0) && tempo_lag(tempo_rank(d)) == d, "rank of %d", d);
    }
    CHECK(tempo_better(1.0, 5, 0.5, 0) && !tempo_better(0.5, 0, 1.0, 5) && tempo_better(1.0, 1, 1.0, 2) && !tempo_better(1.0, 2, 1.0, 1) && !tempo_better(1.0, 2, 1.0, 2), "tempo_better");
    CHECK(tempo_better(-1e300, 2048, tempo_no_score(), kTempoNoRank) && tempo_better(0.0, 0, -0.0, 1) && !tempo_better(-0.0, 1, 0.0, 0), "tempo_better at the ends");
    CHECK(tempo_clamp(0x7FFFFFFFFFFFFFFFll) == 1ll << 45 && tempo_clamp(-0x7FFFFFFFFFFFFFFFll - 1) == -(1ll << 45) && tempo_clamp(-5) == -5, "tempo_clamp");
    // planted ties: equal scores at chosen ranks, the candidates dealt to the lanes in every rotation
    for (int pass = 0; pass < 64; ++pass) {
        const int nLags = 1 + (int)(rng() % 2049u);
        std::vector<double> score((size_t)nLags);
        for (double& s : score) s = (double)((int)(rng() % 7u) - 3);      // few values: many ties, the greatest among them
        Pick scan{tempo_no_score(), kTempoNoRank};
        for (int j = 0; j < nLags; ++j)
            if (tempo_better(score[(size_t)j], j, scan.score, scan.rank)) scan = Pick{score[(size_t)j], j};
        for (int rot = 0; rot < 256; rot += 1 + (int)(rng() % 37u)) {
            std::vector<Pick> lanes(256, Pick{tempo_no_score(), kTempoNoRank});
            for (int j = 0; j < nLags; ++j) {
                Pick& mine = lanes[(size_t)((j + rot) % 256)];
                if (tempo_better(score[(size_t)j], j, mine.score, mine.rank)) mine = Pick{score[(size_t)j], j};
            }
            const Pick won = model_reduce(lanes);
            CHECK(won.rank == scan.rank && won.score == scan.score, "planted ties: %d lags rotated by %d: rank %d against %d", nLags, rot, won.rank, scan.rank);
        }
    }
    // the search on rows with ties: an exact period, a constant, a silence inside noise; and noise alone
    for (const char* kind : {"period", "constant", "silence", "noise"}) {
        model_search(make_row<int16_t>(kind, 1500), 64, 40, 0.8, kind);
        model_search(make_row<float>(kind, 1500), 66, 31, 1.1, kind);
        model_search(make_row<int16_t>(kind, 700), 128, 160, 4.0, kind);      // more lags than lanes
        model_search(make_row<float>(kind, 300), 64, 0, 0.25, kind);
        model_search(make_row<float>(kind, 900), 256, 300, 1.0, kind);
    }
    model_search(make_row<int16_t>("period", 5000), 2048, 1024, 1.1, "period");      // the widest: 2049 lags of 2048 samples
    for (long long L : {0ll, 1ll, 31ll, 32ll, 33ll, 64ll}) model_search(make_row<int16_t>("noise", L), 64, 5, 0.8, "noise");
    // the render: rows around the tile's length (tempo 1 is every third row of five), outputs 0, 1 and 3 elements past a 16-byte boundary
    const std::vector<long long> lengths = {kTempoTile + 1, 0, kTempoTile, 1, 5, 3 * kTempoTile - 1, 31, kTempoTile - 1, 2 * kTempoTile + 17, 300, 4 * kTempoTile, 33, kTempoTile + 1};
    for (int N : {64, 66, 512, 2048})
        for (int padded = 0; padded < 2; ++padded) {
            model_render<true, int16_t>(lengths, N, padded, padded, 1, false, 0);
            model_render<false, float>(lengths, N, padded, !padded, 3, false, 7);
            model_render<false, int16_t>(lengths, N, padded, true, 0, true, 0);
            model_render<true, float>(lengths, N, padded, false, 2, true, 5);
        }
    model_render<true, float>({}, 64, false, false, 0, false, 0);
    model_render<false, int16_t>({0, 0}, 64, true, true, 0, false, 0);
    printf("ok %lld\n", checks);
    return 0;
}
