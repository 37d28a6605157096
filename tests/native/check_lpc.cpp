// check_lpc.cpp -- models of the two kernels of the linear-prediction exports (nvspeechplayer_amd/csrc/klatt_lpc.h) written from the shared
// functions alone, against brute force written here from the definition in include/speechPlayer_batch.h.  klatt_lpc: groups of 64
// consecutive steps of the output located by dense_locate (padded and packed, a group that ends one row and begins the next), sixteen
// steps per wavefront, the frame in the wavefront's LDS region, lane-strided partials in blocks of kLpcLagBlock lags, the tree as a
// butterfly over the lanes, rs[lag][step], a lane per step for the recursion, the fields staged where the frames were and stored by
// tile_store_lane -- the LDS model has exactly lpc_lds_bytes bytes.  klatt_lpc_residual: the tile walk (tile_row_table, tile_row and the
// bisection of the packed form, tile_n, tile_live), the staged run x(t0 - order ..), the coefficient rows staged (at most kLpcStageRows)
// or read per lane, float64 and float32, at a column offset, padded and packed, and the row writer.  Rows of 0, 1, 63, 64 and 65 steps and
// of the tile's length and one either side; outputs 0, 1 and 3 elements past a 16-byte boundary: every element of each output is
// written exactly once, the guards stay, and the bits are brute force's and the host statement's.
// Built with AddressSanitizer + UBSan by tests/test_lpc_host.py; prints "ok <checks>" or the first failure.
#include "../../nvspeechplayer_amd/csrc/klatt_lpc.h"
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

// The workgroup's stores of a run, lane by lane (klatt_tiles.h: tile_store)
template <typename T> static void store_run(Guarded<T>& G, long long e0, int count, const T* staged)
{
    const int mis = tile_mis<T>(G.out()), lanes = tile_lanes<T>(mis, e0, count);
    CHECK(mis == G.shift % kTileLane<T>, "mis %d of shift %d", mis, G.shift);
    for (int i = 0; i < lanes; ++i) tile_store_lane(G.out(), mis, e0, count, staged, i);
    G.mark(e0, count);
}

struct Row { long long src, len, steps; };

// n rows of the lengths given in turn, the inputs from element 3 with gaps between them
template <typename In>
static std::vector<Row> make_rows(const std::vector<long long>& lengths, long long hop, long long phase, std::vector<In>& in)
{
    std::vector<Row> rows;
    long long src = 3;
    for (long long L : lengths) {
        rows.push_back(Row{src, L, L > phase ? (L - phase + hop - 1) / hop : 0});
        src += L + (long long)(rng() % 3u);
    }
    in.resize((size_t)src + 2);
    for (In& v : in) v = random_sample<In>();
    // a silence inside the first long row: exact zeros
    for (const Row& r : rows)
        if (r.len > 200) { for (long long t = 60; t < 160; ++t) in[(size_t)(r.src + t)] = (In)0; break; }
    return rows;
}

// ---- brute force, from the header's text ---------------------------------------------------------------------------------------------------
static double tree_sum(const double* p, int n) { return n == 1 ? p[0] : tree_sum(p, n / 2) + tree_sum(p + n / 2, n / 2); }

template <typename In>
static void brute_step(const In* x, long long L, long long c, int order, int nWin, const std::vector<float>& w, const double* lag, int what, double* o)
{
    std::vector<float> xw((size_t)nWin);
    for (int i = 0; i < nWin; ++i) {
        const long long t = c - nWin / 2 + i;
        const float v = t >= 0 && t < L ? tile_x(x[t]) : 0.0f;
        xw[(size_t)i] = v * w[(size_t)i];
    }
    std::vector<double> r((size_t)order + 1), a((size_t)order + 1, 0.0), k((size_t)order + 1, 0.0), next((size_t)order + 1);
    for (int lagK = 0; lagK <= order; ++lagK) {
        double partial[64];
        for (int q = 0; q < 64; ++q) {
            double acc = 0.0;
            for (int i = lagK; i < nWin; ++i)
                if (i % 64 == q) acc += (double)xw[(size_t)i] * (double)xw[(size_t)(i - lagK)];      // (the product is exact: no fma needed)
            partial[q] = acc;
        }
        r[(size_t)lagK] = tree_sum(partial, 64);
        if (lag) r[(size_t)lagK] = r[(size_t)lagK] * lag[lagK];
    }
    double E = r[0];
    int stages = 0;
    for (int i = 1; i <= order; ++i) {
        if (!(E > 0.0 && std::isfinite(E))) break;
        double acc = r[(size_t)i];
        for (int j = 1; j < i; ++j) acc = fma(a[(size_t)j], r[(size_t)(i - j)], acc);
        const double kappa = -acc / E;
        if (!(fabs(kappa) < 1.0)) break;
        for (int j = 1; j < i; ++j) next[(size_t)j] = fma(kappa, a[(size_t)(i - j)], a[(size_t)j]);
        for (int j = 1; j < i; ++j) a[(size_t)j] = next[(size_t)j];
        a[(size_t)i] = kappa; k[(size_t)i] = kappa;
        E = fma(kappa, acc, E);
        stages = i;
    }
    int col = 0;
    if (what & 1) for (int j = 0; j <= order; ++j) o[col++] = r[(size_t)j];
    if (what & 2) for (int j = 1; j <= order; ++j) o[col++] = a[(size_t)j];
    if (what & 4) for (int j = 1; j <= order; ++j) o[col++] = k[(size_t)j];
    if (what & 8) o[col++] = E;
    if (what & 16) o[col++] = (double)stages;
}

// ---- klatt_lpc --------------------------------------------------------------------------------------------------------------------------------
template <bool F32, typename In>
static void model_analysis(const std::vector<long long>& lengths, int order, int nWin, long long hop, long long phase, int what, bool withLag, bool padded, int shift)
{
    using T = typename std::conditional<F32, float, double>::type;
    char name[200];
    snprintf(name, sizeof name, "analysis %zu rows order %d nWin %d hop %lld phase %lld what %d lag %d padded %d shift %d f32 %d in %zu", lengths.size(), order, nWin, hop, phase, what,
             (int)withLag, (int)padded, shift, (int)F32, sizeof(In));
    std::vector<double> window((size_t)nWin), lagW;
    for (int i = 0; i < nWin; ++i) window[(size_t)i] = 0.54 - 0.46 * cos(6.283185307179586 * i / nWin) - ((i % 7) == 3 ? 1.0 : 0.0);      // (some negative values)
    for (int k = 0; withLag && k <= order; ++k) lagW.push_back(k == 0 ? 1.0 + 1.0 / 1024 : exp(-0.001 * k * k));
    LpcPlan P;
    std::string why;
    CHECK(lpc_plan(P, order, nWin, window.data(), withLag ? lagW.data() : nullptr, what, why), "%s: %s", name, why.c_str());
    const int nCols = P.nCols;
    CHECK(nCols == lpc_columns(what, order), "%s", name);
    std::vector<In> in;
    const std::vector<Row> rows = make_rows(lengths, hop, phase, in);
    const long long n = (long long)rows.size();
    std::vector<long long> counts;
    long long most = 0, total = 0;
    for (const Row& r : rows) { counts.push_back(r.steps); most = std::max(most, r.steps); total += r.steps; }
    const long long rowStride = padded ? most + 1 + (long long)(rng() % 3u) : 0;
    std::vector<long long> words;
    const RowTable table = padded ? RowTable{0, 0} : packed_row_table(counts.data(), 0, n, kTimelineChunkLog2, words);
    const long long* start = padded ? nullptr : words.data() + table.startOff;
    const long long* chunk = padded ? nullptr : words.data() + table.chunkOff;
    const long long nSteps = padded ? n * rowStride : total;
    Guarded<T> G(nSteps * nCols, shift);

    // the workgroup's LDS: exactly what the launch asks for
    const size_t front = lpc_front_bytes(nWin, order, nCols, (int)sizeof(T)), ldsBytes = lpc_lds_bytes(nWin, order, nCols, (int)sizeof(T));
    unsigned char* lds = static_cast<unsigned char*>(aligned_alloc(16, (ldsBytes + 15) / 16 * 16));
    const int frameWords = lpc_frame_words(nWin, order);
    T* const staged = reinterpret_cast<T*>(lds);
    double* const rs = reinterpret_cast<double*>(lds + front);
    const double* lag = P.hasLag ? P.lag.data() : nullptr;

    const long long nGroups = (nSteps + kLpcGroup - 1) / kLpcGroup;
    for (long long grp = 0; grp < nGroups; ++grp) {
        const long long g0 = grp * kLpcGroup;
        const int nInside = (int)std::min<long long>(nSteps - g0, kLpcGroup);
        for (int s = 0; s < kLpcGroup / 4; ++s)
            for (int wave = 0; wave < 4; ++wave) {      // (the wavefronts run side by side between two barriers: each in its own region)
                float* const xw = reinterpret_cast<float*>(lds) + (size_t)wave * frameWords + order;
                const int step = wave * (kLpcGroup / 4) + s;
                if (step >= nInside) continue;
                long long g, r, j;
                int q;
                dense_locate(g0 + step, 1, rowStride, start, chunk, g, q, r, j);
                CHECK(g == g0 + step && q == 0 && r >= 0 && r < n, "%s: step %lld located in row %lld", name, g0 + step, r);
                const Row row = rows[(size_t)r];
                if (!(j < row.steps)) continue;
                const long long t0 = phase + j * hop - nWin / 2;
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = lane; i < nWin; i += 64) xw[i] = spec_windowed(tile_sample(in.data() + row.src, t0 + i, row.len), P.window[(size_t)i]);
                for (int kb = 0; kb <= order; kb += kLpcLagBlock) {
                    double acc[64][kLpcLagBlock];
                    for (int lane = 0; lane < 64; ++lane) {
                        for (int u = 0; u < kLpcLagBlock; ++u) acc[lane][u] = 0.0;
                        for (int i = lane; i < nWin; i += kLpcPartials) {
                            const float xi = xw[i];
                            for (int u = 0; u < kLpcLagBlock; ++u)
                                if (i >= kb + u && kb + u <= order) acc[lane][u] = lpc_term(xi, xw[i - kb - u], acc[lane][u]);
                        }
                    }
                    for (int u = 0; u < kLpcLagBlock; ++u) {
                        double v[64], next[64];
                        for (int lane = 0; lane < 64; ++lane) v[lane] = acc[lane][u];
                        for (int m = 1; m < kLpcPartials; m <<= 1) {      // the butterfly: every lane ends with the tree's root
                            for (int lane = 0; lane < 64; ++lane) next[lane] = v[lane] + v[lane ^ m];
                            memcpy(v, next, sizeof v);
                        }
                        if (kb + u <= order) {
                            for (int lane = 1; lane < 64; ++lane) CHECK(memcmp(&v[lane], &v[0], 8) == 0, "%s: lane %d of the butterfly", name, lane);
                            double t[64];
                            for (int lane = 0; lane < 64; ++lane) t[lane] = acc[lane][u];
                            const double root = lpc_tree(t);
                            CHECK(memcmp(&root, &v[0], 8) == 0, "%s: the butterfly against lpc_tree", name);
                            rs[(kb + u) * kLpcGroup + step] = lpc_lagged(v[0], lag, kb + u);
                        }
                    }
                }
            }
        // phase B: a lane per step; the staged fields take the frames' place
        std::vector<T> fields((size_t)nInside * nCols);
        for (int lane = 0; lane < nInside; ++lane) {
            long long g, r, j;
            int q;
            dense_locate(g0 + lane, 1, rowStride, start, chunk, g, q, r, j);
            const bool live = j < rows[(size_t)r].steps;
            double rr[kLpcMaxOrder + 1], a[kLpcMaxOrder + 1], k[kLpcMaxOrder + 1], E;
            int stages;
            for (int c = 0; c <= kLpcMaxOrder; ++c) rr[c] = live && c <= order ? rs[c * kLpcGroup + lane] : 0.0;
            lpc_levinson(rr, order, a, k, E, stages);
            lpc_put_fields(fields.data() + (size_t)lane * nCols, what, order, rr, a, k, E, stages);
        }
        for (size_t e = 0; e < fields.size(); ++e) staged[e] = fields[e];      // (all lanes have read rs before: it lies behind the front)
        store_run(G, g0 * nCols, nInside * nCols, staged);
    }
    G.finished(name);
    free(lds);

    // against brute force and the statement
    std::vector<double> want((size_t)nCols), host;
    const T zero = (T)0;
    for (long long i = 0; i < n; ++i) {
        const Row& r = rows[(size_t)i];
        const long long first = padded ? i * rowStride : words[(size_t)(table.startOff + i)];
        host.assign((size_t)(r.steps * nCols) + 1, -3.0);
        CHECK(lpc_host(in.data() + r.src, r.len, P, hop, phase, host.data()) == r.steps * nCols, "%s: row %lld", name, i);
        for (long long j = 0; j < r.steps; ++j) {
            brute_step(in.data() + r.src, r.len, phase + j * hop, order, nWin, P.window, lag, what, want.data());
            CHECK(memcmp(want.data(), host.data() + j * nCols, 8 * (size_t)nCols) == 0, "%s: the statement against brute force, row %lld step %lld", name, i, j);
            for (int c = 0; c < nCols; ++c) {
                const T w = (T)want[(size_t)c];
                CHECK(memcmp(&w, G.out() + (first + j) * nCols + c, sizeof w) == 0, "%s: row %lld step %lld column %d: %a against %a", name, i, j, c, (double)w,
                      (double)G.out()[(first + j) * nCols + c]);
            }
        }
        for (long long j = r.steps; padded && j < rowStride; ++j)
            for (int c = 0; c < nCols; ++c) CHECK(memcmp(&zero, G.out() + (first + j) * nCols + c, sizeof zero) == 0, "%s: row %lld: padding step %lld", name, i, j);
    }
}

// ---- klatt_lpc_residual -------------------------------------------------------------------------------------------------------------------
template <int WHAT, bool F32, typename In, typename C>
static void model_residual(const std::vector<long long>& lengths, int order, long long hop, long long phase, bool padded, bool coeffPadded, int shift)
{
    using T = TileValue<F32>;
    char name[200];
    snprintf(name, sizeof name, "residual what %d %zu rows order %d hop %lld phase %lld padded %d coeff padded %d shift %d f32 %d in %zu c %zu", WHAT, lengths.size(), order, hop, phase,
             (int)padded, (int)coeffPadded, shift, (int)F32, sizeof(In), sizeof(C));
    std::vector<In> in;
    const std::vector<Row> rows = make_rows(lengths, hop, phase, in);
    const long long n = (long long)rows.size();
    std::vector<long long> outLen;
    long long most = 0, mostSteps = 0, totalSteps = 0, total = 0;
    for (const Row& r : rows) { outLen.push_back(r.len); most = std::max(most, r.len); mostSteps = std::max(mostSteps, r.steps); total += r.len; totalSteps += r.steps; }
    const long long rowStride = padded ? most + 1 + (long long)(rng() % 5u) : 0;
    const int coeffCols = order + 3, col0 = 2;
    const long long coeffStride = coeffPadded ? mostSteps + 1 : 0, coeffSteps = coeffPadded ? n * coeffStride : totalSteps;
    // exactly the elements the rows' steps need: a read past them is past the vector
    std::vector<C> coeff((size_t)(coeffSteps * coeffCols));
    for (C& c : coeff) c = (C)((double)((int)(rng() % 20001u) - 10000) / 10000.0);
    std::vector<long long> words;
    const TileTable tiles = tile_row_table(outLen.data(), n, kLpcTile, rowStride, kTimelineChunkLog2, words);
    Guarded<T> G(padded ? n * rowStride : total, shift);
    std::vector<long long> dst, cfirst;
    long long before = 0, stepsBefore = 0;
    for (long long i = 0; i < n; ++i) {
        dst.push_back(padded ? i * rowStride : before); cfirst.push_back(coeffPadded ? i * coeffStride : stepsBefore);
        before += rows[(size_t)i].len; stepsBefore += rows[(size_t)i].steps;
    }
    std::vector<float> xs((size_t)kLpcTile + kLpcMaxOrder);
    std::vector<T> staged((size_t)kLpcTile);
    std::vector<double> as((size_t)kLpcStageRows * kLpcMaxOrder);
    long long stagedTiles = 0, directTiles = 0;
    for (long long g = 0; g < tiles.nTiles; ++g) {
        long long r, j;
        if (rowStride > 0) tile_row(g, tiles.tilesPerRow, r, j);
        else { const long long c = g >> kTimelineChunkLog2; packed_locate(g, words.data() + tiles.table.startOff, words[(size_t)(tiles.table.chunkOff + c)], words[(size_t)(tiles.table.chunkOff + c + 1)] + 1, r, j); }
        const long long t0 = j * kLpcTile;
        const Row row = rows[(size_t)r];
        const int nn = tile_n(rowStride, row.len, t0, kLpcTile), live = tile_live(nn, row.len, t0);
        CHECK(nn > 0 && nn <= kLpcTile, "%s: tile %lld of %d elements", name, g, nn);
        long long j0 = 0;
        int nRows = 0;
        if (live > 0) {
            for (int lane = 0; lane < 256; ++lane) tile_read_lane<1>(xs.data(), in.data() + row.src, row.len, t0 - order, live + order, lane, 256);
            if (row.steps > 0) {
                j0 = lpc_frame_of(t0, hop, phase, row.steps);
                const long long used = lpc_frame_of(t0 + live - 1, hop, phase, row.steps) - j0 + 1;
                CHECK(used >= 1 && used <= (kLpcTile + hop - 1) / hop + 2, "%s: %lld coefficient rows in a tile", name, used);
                nRows = used <= kLpcStageRows ? (int)used : 0;
                for (int i = 0; i < nRows * order; ++i) {
                    const int jj = i / order, m = i - jj * order;
                    as[(size_t)i] = lpc_widen(coeff[(size_t)((cfirst[(size_t)r] + j0 + jj) * coeffCols + col0 + m)]);
                }
                ++(nRows ? stagedTiles : directTiles);
            } else {
                nRows = 1;
                for (int i = 0; i < order; ++i) as[(size_t)i] = 0.0;
            }
        }
        for (int i = 0; i < nn; ++i) {
            float y = 0.0f;
            if (i < live) {
                const long long jf = row.steps > 0 ? lpc_frame_of(t0 + i, hop, phase, row.steps) : 0;
                CHECK(jf >= j0 && (nRows == 0 || jf - j0 < nRows), "%s: sample %lld takes row %lld of %d from %lld", name, t0 + i, jf, nRows, j0);
                y = nRows > 0 ? lpc_inverse<WHAT>(xs.data() + i, as.data() + (int)(jf - j0) * order, order)
                              : lpc_inverse<WHAT>(xs.data() + i, coeff.data() + (cfirst[(size_t)r] + jf) * coeffCols + col0, order);
            }
            staged[(size_t)i] = i < live ? res_value<F32>(y) : (T)0;
        }
        store_run(G, dst[(size_t)r] + t0, nn, staged.data());
    }
    G.finished(name);
    if (hop == 1 && most > kLpcStageRows) CHECK(directTiles > 0, "%s: no tile read its rows directly", name);
    if (hop >= 32 && totalSteps > 0) CHECK(stagedTiles > 0, "%s: no tile staged its rows", name);

    // against brute force and the statement
    const T zero = (T)0;
    for (long long i = 0; i < n; ++i) {
        const Row& r = rows[(size_t)i];
        std::vector<double> c64((size_t)(r.steps * order) + 1);
        for (long long j = 0; j < r.steps; ++j)
            for (int m = 0; m < order; ++m) c64[(size_t)(j * order + m)] = (double)coeff[(size_t)((cfirst[(size_t)i] + j) * coeffCols + col0 + m)];
        std::vector<T> host((size_t)r.len + 1);
        lpc_inverse_host(in.data() + r.src, r.len, order, hop, phase, c64.data(), WHAT, F32 ? 1 : 0, host.data());
        for (long long t = 0; t < r.len; ++t) {
            long long jf = 0;
            if (r.steps > 0) {      // the nearest centre, ties upward, by search
                for (long long j = 1; j < r.steps; ++j) {
                    const long long da = llabs(t - (phase + jf * hop)), db = llabs(t - (phase + j * hop));
                    if (db <= da) jf = j;
                }
            }
            double s = WHAT == kLpcResidual ? (double)(t < r.len ? tile_x(in[(size_t)(r.src + t)]) : 0.0f) : 0.0;
            for (int m = 1; m <= order; ++m) {
                const double am = r.steps > 0 ? c64[(size_t)(jf * order + m - 1)] : 0.0;
                s = fma(am, t - m >= 0 ? (double)tile_x(in[(size_t)(r.src + t - m)]) : 0.0, s);
            }
            const float y = (float)(WHAT == kLpcResidual ? s : -s);
            const T w = F32 ? (T)y : (T)res_int16(y);
            CHECK(memcmp(&w, &host[(size_t)t], sizeof w) == 0, "%s: the statement against brute force, row %lld sample %lld", name, i, t);
            CHECK(memcmp(&w, G.out() + dst[(size_t)i] + t, sizeof w) == 0, "%s: row %lld sample %lld", name, i, t);
        }
        for (long long t = r.len; padded && t < rowStride; ++t) CHECK(memcmp(&zero, G.out() + dst[(size_t)i] + t, sizeof zero) == 0, "%s: row %lld: padding element %lld", name, i, t);
    }
}

int main()
{
    // the recursion's exact cases
    {
        double r[kLpcMaxOrder + 1] = {}, a[kLpcMaxOrder + 1], k[kLpcMaxOrder + 1], E;
        int stages;
        for (int i = 0; i <= 8; ++i) r[i] = ldexp(1.0, -i);
        lpc_levinson(r, 8, a, k, E, stages);
        CHECK(a[1] == -0.5 && E == 0.75 && stages == 8, "2^-k: a1 %g E %g stages %d", a[1], E, stages);
        for (int i = 2; i <= 8; ++i) CHECK(a[i] == 0.0 && k[i] == 0.0, "2^-k: a[%d] %g k %g", i, a[i], k[i]);
        const double silent[kLpcMaxOrder + 1] = {};
        lpc_levinson(silent, 32, a, k, E, stages);
        CHECK(stages == 0 && E == 0.0 && !std::signbit(E), "silence: stages %d", stages);
        for (int i = 0; i <= 32; ++i) CHECK(a[i] == 0.0 && !std::signbit(a[i]) && k[i] == 0.0 && !std::signbit(k[i]), "silence: a[%d]", i);
    }
    // steps of a row: 0, 1, 63, 64, 65 (hop h, phase p: L = p + (steps - 1) h + 1), and a null row
    for (int pass = 0; pass < 2; ++pass) {
        const long long hop = pass ? 3 : 10, phase = pass ? 7 : 0;
        auto len = [&](long long steps) { return steps ? phase + (steps - 1) * hop + 1 : phase; };
        const std::vector<long long> lengths = {len(65), 0, len(1), len(63), len(64), len(0), len(64), len(2) + hop - 1, len(130)};
        const int order = pass ? 32 : 5, nWin = pass ? 33 : 100;
        for (int padded = 0; padded < 2; ++padded)
            for (int shift : {0, 1, 3}) {
                model_analysis<false, int16_t>(lengths, order, nWin, hop, phase, kLpcAllFields, pass == 1, padded, shift);
                model_analysis<true, float>(lengths, order, nWin, hop, phase, pass ? kLpcCoeff | kLpcError : kLpcStages, pass == 0, padded, shift);
            }
        model_analysis<false, float>({len(64)}, 1, 2, hop, phase, kLpcReflection, false, true, 1);
        model_analysis<true, int16_t>({}, 2, 64, hop, phase, kLpcAutocorr, false, false, 0);
        model_analysis<true, int16_t>({0, 0}, 2, 65, hop, phase, kLpcAutocorr, false, true, 0);
    }
    // the residual: rows of the tile's length and one either side, hops that stage the coefficient rows and hops that do not
    const std::vector<long long> lengths = {kLpcTile + 1, 0, 1, kLpcTile - 1, 5, kLpcTile, 2 * kLpcTile + 17, 31};
    for (long long hop : {1ll, 16ll, 17ll, 160ll, 5000ll})
        for (int padded = 0; padded < 2; ++padded) {
            const long long phase = hop == 160 ? 7 : 0;
            model_residual<kLpcResidual, true, int16_t, double>(lengths, 16, hop, phase, padded, padded, 1);
            model_residual<kLpcPrediction, false, float, float>(lengths, 32, hop, phase, padded, !padded, 3);
            model_residual<kLpcResidual, false, int16_t, float>(lengths, 1, hop, phase, padded, true, 0);
            model_residual<kLpcPrediction, true, float, double>(lengths, 7, hop, phase + 40, padded, false, 2);
        }
    model_residual<kLpcResidual, true, float, double>({}, 4, 3, 0, false, false, 0);
    printf("ok %lld\n", checks);
    return 0;
}
