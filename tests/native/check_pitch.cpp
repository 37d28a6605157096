// check_pitch.cpp -- a model of the kernel of the pitch export (nvspeechplayer_amd/csrc/klatt_pitch.h) written from the shared functions
// alone, against brute force written here from the definition in include/speechPlayer_batch.h.  klatt_pitch: groups of kPitchGroup
// consecutive steps of the output located by dense_locate (padded and packed, a group that ends one row and begins the next), four steps
// per wavefront, the frame in the wavefront's LDS region with zeros behind it, passes of 64 R lags with R = 4 or 6 lags a lane
// (pitch_lane_lags, pitch_lane_diff, pitch_lane_pass), the scan through the lanes 64 lags at a time, a lane's share of the choice and the butterfly of pitch_better, the
// scalar fields by lane 0 and the CMND curve by all lanes into the wavefront's staged values, each step's values stored by
// tile_store_lane with 64 lanes -- the LDS model has exactly pitch_lds_bytes bytes, so AddressSanitizer sees every read past a region.
// W in {32, 33, 34, 35, 2048}, lagMax in {3, 63, 64, 65, 1024} and (six lags a lane) {257, 379, 384}, lagMin in {2, lagMax - 1}, rows shorter than a frame, of 0 and 1 samples,
// phase > 0, hop 1 and N + 1; outputs 0, 1 and 3 elements past a 16-byte boundary: every element of each output is written exactly once,
// the guards stay, and the bits are brute force's and the host statement's.
// Built with AddressSanitizer + UBSan by tests/test_pitch_host.py; prints "ok <checks>" or the first failure.
#include "../../nvspeechplayer_amd/csrc/klatt_pitch.h"
#include "../../nvspeechplayer_amd/csrc/klatt_tiles.h"
#include "../../nvspeechplayer_amd/csrc/klatt_export.h"

#include <stdlib.h>
#include <string.h>

using namespace klatt;

static long long checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static uint32_t rng_state = 2463534242u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

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

struct Row { long long src, len, steps; };

// Rows of the lengths given in turn, the inputs from element 3 with gaps between them.  A row is a pulse train of a period of its own with
// noise on it (so that some steps are voiced at threshold 0.3 and some are not), then exact zeros for a stretch, signed zeros among them.
template <typename In> static In as_sample(float v);
template <> int16_t as_sample<int16_t>(float v) { return (int16_t)(v * 12000.0f); }
template <> float as_sample<float>(float v) { return v == 0.0f && (rng() & 1u) ? -0.0f : v * 1.7f; }

template <typename In>
static std::vector<Row> make_rows(const std::vector<long long>& lengths, long long hop, long long phase, std::vector<In>& in)
{
    std::vector<Row> rows;
    long long src = 3;
    for (long long L : lengths) {
        rows.push_back(Row{src, L, L > phase ? (L - phase + hop - 1) / hop : 0});
        src += L + (long long)(rng() % 3u);
    }
    in.assign((size_t)src + 2, as_sample<In>(0.5f));      // (what lies between the rows is not zero: a load outside a row would show)
    int period = 5;
    for (const Row& r : rows) {
        period = period * 3 % 61 + 2;
        for (long long t = 0; t < r.len; ++t) {
            const bool silent = t % 700 >= 600, noisy = t % 1400 >= 900;
            const float tone = (float)(t % period) / (float)period - 0.5f, noise = (float)((int)(rng() % 2001u) - 1000) / 1000.0f;
            in[(size_t)(r.src + t)] = as_sample<In>(silent ? 0.0f : noisy ? noise : tone + 0.02f * noise);
        }
    }
    return rows;
}

// ---- brute force, from the header's text ---------------------------------------------------------------------------------------------------
template <typename In>
static void brute_step(const In* x, long long L, long long c, int sampleRate, int W, int lagMin, int lagMax, double threshold, int what, double* o)
{
    const int N = W + lagMax;
    std::vector<float> f((size_t)N);
    for (int i = 0; i < N; ++i) {
        const long long t = c - N / 2 + i;
        f[(size_t)i] = t >= 0 && t < L ? tile_x(x[t]) : 0.0f;
    }
    std::vector<double> m((size_t)lagMax + 2, 0.0);
    double s = 0.0;
    for (int tau = 1; tau <= lagMax; ++tau) {
        double c4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < 4; ++j)
            for (int i = j; i < W; i += 4) {
                const float u = f[(size_t)i] - f[(size_t)(i + tau)];
                if (u != 0.0f) c4[j] += (double)u * (double)u;      // (the product is exact: no fma needed; a zero term is skipped)
            }
        const double d = (c4[0] + c4[1]) + (c4[2] + c4[3]);
        s = s + d;
        m[(size_t)tau] = s > 0.0 ? (d * (double)tau) / s : 1.0;
    }
    int star = 0;
    bool voiced = false;
    for (int tau = lagMin; tau <= lagMax && !voiced; ++tau)
        if (m[(size_t)tau] < threshold && (tau == lagMax || !(m[(size_t)tau + 1] < m[(size_t)tau]))) { star = tau; voiced = true; }
    if (!voiced) {
        star = lagMin;
        for (int tau = lagMin + 1; tau <= lagMax; ++tau)
            if (m[(size_t)tau] < m[(size_t)star]) star = tau;
    }
    double delta = 0.0;
    if (star - 1 >= 1 && star + 1 <= lagMax) {
        const double y0 = m[(size_t)star - 1], y1 = m[(size_t)star], y2 = m[(size_t)star + 1], den = (y0 - y1) + (y2 - y1);
        if (den > 0.0) {
            const double dd = (0.5 * (y0 - y2)) / den;
            if (fabs(dd) <= 0.5) delta = dd;
        }
    }
    const double period = (double)star + delta;
    int col = 0;
    if (what & 1) o[col++] = voiced ? (double)sampleRate / period : 0.0;
    if (what & 2) o[col++] = period;
    if (what & 4) o[col++] = (double)star;
    if (what & 8) o[col++] = m[(size_t)star];
    if (what & 16) o[col++] = voiced ? 1.0 : 0.0;
    if (what & 32) for (int tau = lagMin; tau <= lagMax; ++tau) o[col++] = m[(size_t)tau];
}

// ---- klatt_pitch ------------------------------------------------------------------------------------------------------------------------------
static long long voicedSteps = 0, unvoicedSteps = 0;

template <bool F32, typename In>
static void model(const std::vector<long long>& lengths, int W, int lagMin, int lagMax, double threshold, long long hop, long long phase, int what, bool padded, int shift)
{
    using T = typename std::conditional<F32, float, double>::type;
    char name[240];
    snprintf(name, sizeof name, "pitch %zu rows W %d lags %d .. %d threshold %g hop %lld phase %lld what %d padded %d shift %d f32 %d in %zu", lengths.size(), W, lagMin, lagMax,
             threshold, hop, phase, what, (int)padded, shift, (int)F32, sizeof(In));
    const int sampleRate = 22050;
    PitchPlan P;
    std::string why;
    CHECK(pitch_plan(P, sampleRate, W, lagMin, lagMax, threshold, what, why), "%s: %s", name, why.c_str());
    const int nCols = P.nCols, N = W + lagMax;
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
    const size_t waveBytes = pitch_wave_bytes(W, lagMax, nCols, (int)sizeof(T)), ldsBytes = pitch_lds_bytes(W, lagMax, nCols, (int)sizeof(T));
    CHECK(ldsBytes == 4 * waveBytes && waveBytes % 16 == 0 && ldsBytes <= kPitchLdsBudget, "%s: %zu bytes of LDS", name, ldsBytes);
    unsigned char* lds = static_cast<unsigned char*>(aligned_alloc(16, ldsBytes));
    memset(lds, 0xFF, ldsBytes);      // (NaNs: what a lane reads before it is written shows)
    const int frameWords = pitch_frame_words(W, lagMax);
    const int mis = tile_mis<T>(G.out());

    const long long nGroups = (nSteps + kPitchGroup - 1) / kPitchGroup;
    for (long long grp = 0; grp < nGroups; ++grp)
        for (int wave = 0; wave < 4; ++wave) {      // (the wavefronts run at their own pace, each in its own region)
            unsigned char* const region = lds + (size_t)wave * waveBytes;
            float* const xs = reinterpret_cast<float*>(region);
            double* const dm = reinterpret_cast<double*>(region + (size_t)4 * frameWords);
            T* const staged = reinterpret_cast<T*>(region + (size_t)4 * frameWords + (size_t)8 * pitch_curve_words(lagMax));
            for (int s = 0; s < kPitchGroup / 4; ++s) {
                const long long gs = grp * kPitchGroup + wave * (kPitchGroup / 4) + s;
                if (gs >= nSteps) break;
                long long g, r, j;
                int q;
                dense_locate(gs, 1, rowStride, start, chunk, g, q, r, j);
                CHECK(g == gs && q == 0 && r >= 0 && r < n, "%s: step %lld located in row %lld", name, gs, r);
                const Row row = rows[(size_t)r];
                if (j < row.steps) {
                    const long long t0 = phase + j * hop - N / 2;
                    for (int lane = 0; lane < 64; ++lane)
                        for (int i = lane; i < frameWords; i += 64) xs[i] = i < N ? tile_sample(in.data() + row.src, t0 + i, row.len) : 0.0f;
                    for (int lane = 0; lane < 64; ++lane) {
                        if (pitch_lane_lags(lagMax) == 6) pitch_lane_diff<6>(xs, dm, W, lagMax, lane);
                        else pitch_lane_diff<4>(xs, dm, W, lagMax, lane);
                    }
                    // the scan: s through the lanes, 64 lags at a time
                    double carry = 0.0;
                    for (int base = 0; base <= lagMax; base += 64) {
                        double dl[64], mine[64];
                        for (int lane = 0; lane < 64; ++lane) {
                            const int tau = base + lane;
                            dl[lane] = tau >= 1 && tau <= lagMax ? dm[tau] : 0.0;
                            mine[lane] = 0.0;
                        }
                        const int nk = lagMax - base + 1 < 64 ? lagMax - base + 1 : 64;
                        for (int k = 0; k < nk; ++k) { carry = carry + dl[k]; mine[k] = carry; }
                        CHECK(!(carry == 0.0 && std::signbit(carry)), "%s: s is -0.0", name);
                        for (int lane = 0; lane < 64; ++lane) {
                            const int tau = base + lane;
                            if (tau >= 1 && tau <= lagMax) dm[tau] = pitch_cmnd(dl[lane], tau, mine[lane]);
                        }
                    }
                    // the choice: a lane's share, then the butterfly
                    int dip[64], bestTau[64], first[64];
                    double bestM[64];
                    for (int lane = 0; lane < 64; ++lane) {
                        pitch_lane_choice(dm, lagMin, lagMax, threshold, lane, 64, dip[lane], bestM[lane], bestTau[lane]);
                        first[lane] = dip[lane] != 0 ? dip[lane] : 0x7FFFFFFF;
                    }
                    for (int k = 1; k < 64; k <<= 1) {
                        int nf[64], nt[64];
                        double nm[64];
                        for (int lane = 0; lane < 64; ++lane) {
                            const int of = first[lane ^ k], ot = bestTau[lane ^ k];
                            const double om = bestM[lane ^ k];
                            nf[lane] = of < first[lane] ? of : first[lane];
                            const bool take = pitch_better(om, ot, bestM[lane], bestTau[lane]);
                            nm[lane] = take ? om : bestM[lane]; nt[lane] = take ? ot : bestTau[lane];
                        }
                        memcpy(first, nf, sizeof first); memcpy(bestTau, nt, sizeof bestTau); memcpy(bestM, nm, sizeof bestM);
                    }
                    for (int lane = 1; lane < 64; ++lane)
                        CHECK(first[lane] == first[0] && bestTau[lane] == bestTau[0] && memcmp(&bestM[lane], &bestM[0], 8) == 0, "%s: lane %d of the butterfly", name, lane);
                    const bool voiced = first[0] != 0x7FFFFFFF;
                    ++(voiced ? voicedSteps : unvoicedSteps);
                    const int col = pitch_put_fields(staged, what, sampleRate, dm, voiced ? first[0] : bestTau[0], voiced, lagMax);
                    if (what & kPitchCmnd)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int tau = lagMin + lane; tau <= lagMax; tau += 64) staged[col + tau - lagMin] = (T)dm[tau];
                } else {
                    for (int i = 0; i < nCols; ++i) staged[i] = (T)0;
                }
                const long long e0 = gs * nCols;
                const int lanes = tile_lanes<T>(mis, e0, nCols);
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = lane; i < lanes; i += 64) tile_store_lane(G.out(), mis, e0, nCols, staged, i);
                G.mark(e0, nCols);
            }
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
        CHECK(pitch_host(in.data() + r.src, r.len, P, hop, phase, host.data()) == r.steps * nCols && host.back() == -3.0, "%s: row %lld", name, i);
        for (long long j = 0; j < r.steps; ++j) {
            brute_step(in.data() + r.src, r.len, phase + j * hop, sampleRate, W, lagMin, lagMax, threshold, what, want.data());
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

int main()
{
    static_assert(pitch_frame_words(kPitchMaxWin, kPitchMaxLag) % 4 == 0 && pitch_curve_words(3) == 4 && pitch_curve_words(1024) == 1026, "the regions' words");
    static_assert(pitch_window_quads(4) == 2 && pitch_window_quads(6) == 3, "the window's pieces");
    CHECK(pitch_lane_lags(3) == 4 && pitch_lane_lags(256) == 4 && pitch_lane_lags(257) == 6 && pitch_lane_lags(368) == 6 && pitch_lane_lags(384) == 6 && pitch_lane_lags(385) == 4 &&
          pitch_lane_lags(1024) == 4 && pitch_lane_lags(267) == 6 && pitch_lane_lags(134) == 4, "the lags a lane keeps");
    const int wins[] = {32, 33, 34, 35, 2048}, lagMaxes[] = {3, 63, 64, 65, 1024};
    int turn = 0;
    for (int W : wins)
        for (int lagMax : lagMaxes)
            for (int low = 0; low < 2; ++low, ++turn) {
                const int lagMin = low ? lagMax - 1 : 2, N = W + lagMax;
                if (lagMin < 2 || lagMin >= lagMax) continue;      // (lagMax 3: 2 is lagMax - 1)
                const bool big = W == 2048 || lagMax == 1024;
                // rows: empty, one sample, shorter than a frame, a frame and a bit; the steps of all come to more than one group of 16
                const long long hop = big ? N + 1 : (turn % 3 == 0 ? 1 : turn % 3 == 1 ? N + 1 : 7), phase = turn % 2 ? 3 : 0;
                std::vector<long long> lengths = {0, 1, N / 2, hop == 1 ? 37 : N + 5 * hop + 1, 4, hop == 1 ? 2 : 12 * hop + 2};
                if (big) lengths = {0, 1, N / 2, 3 * hop + 9, 4, hop + 2};      // (the long frames: a few steps each way)
                const int what = turn % 4 == 0 ? kPitchAllFields : turn % 4 == 1 ? kPitchF0 | kPitchAperiodicity : turn % 4 == 2 ? kPitchCmnd : kPitchPeriod | kPitchLag | kPitchVoiced;
                const double threshold = turn % 5 == 0 ? 0.0 : turn % 5 == 1 ? 1.0 : 0.3;
                const bool padded = turn % 2 == 0;
                const int shift = turn % 3 == 0 ? 0 : turn % 3 == 1 ? 1 : 3;
                if (turn % 2) {
                    model<true, int16_t>(lengths, W, lagMin, lagMax, threshold, hop, phase, what, padded, shift);
                    model<false, float>(lengths, W, lagMin, lagMax, threshold, hop, phase, what, !padded, shift % 2);
                } else {
                    model<false, int16_t>(lengths, W, lagMin, lagMax, threshold, hop, phase, what, padded, shift % 2);
                    model<true, float>(lengths, W, lagMin, lagMax, threshold, hop, phase, what, !padded, shift);
                }
            }
    // hop 1 and hop N + 1 at one small shape, both forms, every field; the usual shape once
    for (int padded = 0; padded < 2; ++padded) {
        model<false, int16_t>({40, 0, 100, 1}, 33, 2, 65, 0.3, 1, 2, kPitchAllFields, padded != 0, 1);
        model<true, float>({40, 0, 300, 1}, 34, 64, 65, 0.3, 34 + 65 + 1, 0, kPitchAllFields, padded != 0, 3);
    }
    model<true, int16_t>({3000, 17, 2200}, 512, 44, 368, 0.3, 256, 0, kPitchF0 | kPitchAperiodicity, true, 0);
    // six lags a lane (lagMax 257 .. 384): every W of the list at the range's ends and inside it
    for (int W : wins)
        for (int lagMax : {257, 379, 384}) {
            const int N = W + lagMax;
            model<false, int16_t>({0, 1, N / 2, 2 * N + 30, 4}, W, 2, lagMax, 0.3, N + 1, 3, kPitchAllFields, W % 2 == 0, 1);
            model<true, float>({N + 7, 3}, W, lagMax - 1, lagMax, 0.3, W < 100 ? 9 : N + 1, 0, kPitchAllFields, W % 2 != 0, 3);
        }
    CHECK(voicedSteps > 50 && unvoicedSteps > 50, "%lld voiced and %lld unvoiced steps", voicedSteps, unvoicedSteps);
    printf("ok %lld\n", checks);
    return 0;
}
