// check_signal.cpp -- the row reader of the signal-reading exports (nvspeechplayer_amd/csrc/klatt_tiles.h: tile_x, tile_inside, tile_sample,
// tile_source, tile_read_lane, signal_plan) against brute force, and the host statements on the two input types.  Every row lives in a
// vector of exactly its length, so a read outside 0 .. len-1 is the sanitizer's to report, whatever the mask would have made of it.
// Built with AddressSanitizer + UBSan by tests/test_signal_host.py; prints "ok <checks>" or the first failure.
#include "../../nvspeechplayer_amd/csrc/klatt_convolve.h"
#include "../../nvspeechplayer_amd/csrc/klatt_spectrum.h"

#include <stdlib.h>
#include <string.h>

using namespace klatt;

static long long checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }

static float value_of(int16_t s) { return (float)s / 32767.0f; }
static float value_of(float s) { return s; }
static void fill(std::vector<int16_t>& x) { for (auto& v : x) v = (int16_t)(rnd() % 65536 - 32768); }
static void fill(std::vector<float>& x) { for (auto& v : x) v = ((float)(rnd() % 20001) - 10000.0f) / 77.0f; }

// ---- a run of the reader: every lane of every lane count, both directions ------------------------------------------------------------------
template <int DIR, typename In> static void check_run(const std::vector<In>& row, long long s0, int count, int lanes)
{
    const long long len = (long long)row.size();
    std::vector<float> xs((size_t)count, -7.0f);      // (exactly `count` values)
    std::vector<int> writes((size_t)count, 0);
    for (int lane = 0; lane < lanes; ++lane) {
        std::vector<float> before = xs;
        tile_read_lane<DIR>(xs.data(), row.data(), len, s0, count, lane, lanes);
        for (int i = 0; i < count; ++i)
            if (i % lanes == lane) ++writes[(size_t)i];
            else CHECK(bits(xs[(size_t)i]) == bits(before[(size_t)i]), "lane %d of %d touched element %d", lane, lanes, i);
    }
    for (int i = 0; i < count; ++i) {
        const long long s = DIR > 0 ? s0 + i : s0 - i;      // brute force: the sample this element stands for
        CHECK(tile_source<DIR>(s0, i) == s, "element %d of a run from %lld", i, s0);
        const float want = s >= 0 && s < len ? value_of(row[(size_t)s]) : 0.0f;
        CHECK(writes[(size_t)i] == 1 && bits(xs[(size_t)i]) == bits(want), "element %d (sample %lld of %lld): %g, not %g", i, s, len, (double)xs[(size_t)i], (double)want);
        CHECK(tile_inside(s, len) == (s >= 0 && s < len), "sample %lld of %lld", s, len);
    }
}

template <typename In> static void check_reader()
{
    for (long long len : {0ll, 1ll, 2ll, 3ll, 7ll, 255ll, 256ll, 257ll, 1023ll, 1025ll}) {
        std::vector<In> row((size_t)len);
        fill(row);
        for (int count : {0, 1, 2, 255, 256, 257, 700}) {
            for (long long s0 : {-300ll, -1ll, 0ll, 1ll, len - 1, len, len + 1, len + 300, len / 2}) {
                for (int lanes : {1, 64, 256}) {
                    check_run<1>(row, s0, count, lanes);
                    check_run<-1>(row, s0, count, lanes);
                }
            }
        }
    }
    // outside the row the value is +0 on its bits, whatever the pointer holds: a null row of no samples is never read
    CHECK(bits(tile_sample((const In*)nullptr, 0, 0)) == 0 && bits(tile_sample((const In*)nullptr, -5, 0)) == 0, "an empty row");
}

// ---- the kernels' runs are the reader's ---------------------------------------------------------------------------------------------------
static void check_kernel_runs()
{
    // the convolution: xr[p] = x[conv_staged_sample(t0, kb, p)] is the run from conv_read_first downwards
    for (long long t0 : {0ll, 1024ll, 5120ll})
        for (int kb : {0, 1024, 4096})
            for (int p : {0, 1, 1023, 1024, 2047})
                CHECK(tile_source<-1>(conv_read_first(t0, kb), p) == conv_staged_sample(t0, kb, p), "t0 %lld kb %d p %d", t0, kb, p);
    // the resampler: input i of a span is sample lo + i
    for (long long lo : {-11ll, 0ll, 77777ll})
        for (int i : {0, 1, 8191}) CHECK(tile_source<1>(lo, i) == lo + i, "lo %lld i %d", lo, i);
}

// ---- the signal's rows ---------------------------------------------------------------------------------------------------------------------
static void check_plan()
{
    std::string why;
    SignalPlan P;
    const long long lens[4] = {5, 0, 9, 3};
    CHECK(signal_plan(P, 1, 4, 9, lens, why) && P.need == 3 * 9 + 3 && P.elSize == 4, "padded: %s", why.c_str());
    for (long long r = 0; r < 4; ++r) CHECK(P.at(r) == r * 9 && P.len(r) == lens[r], "padded row %lld", r);
    const long long offs[5] = {0, 5, 5, 14, 17};
    CHECK(signal_plan(P, 0, 4, 0, offs, why) && P.need == 17 && P.elSize == 2, "packed: %s", why.c_str());
    for (long long r = 0; r < 4; ++r) CHECK(P.at(r) == offs[r] && P.len(r) == lens[r], "packed row %lld", r);
    CHECK(signal_plan(P, 1, 0, 0, nullptr, why) && P.need == 0, "no rows: %s", why.c_str());
    // brute force over small random tables: need is the largest at + len of a row with samples, rows lie inside it and, packed, do not overlap
    for (int it = 0; it < 2000; ++it) {
        const long long n = rnd() % 6, stride = rnd() % 2 ? 0 : 1 + rnd() % 12;
        std::vector<long long> e((size_t)n + 1, 0);
        if (stride) for (long long r = 0; r < n; ++r) e[(size_t)r] = rnd() % (stride + 1);
        else for (long long r = 0; r < n; ++r) e[(size_t)r + 1] = e[(size_t)r] + rnd() % 9;
        CHECK(signal_plan(P, (int)(rnd() % 2), n, stride, e.data(), why), "a valid table: %s", why.c_str());
        long long need = 0;
        for (long long r = 0; r < n; ++r) {
            const long long at = stride ? r * stride : e[(size_t)r], len = stride ? e[(size_t)r] : e[(size_t)r + 1] - e[(size_t)r];
            CHECK(P.at(r) == at && P.len(r) == len, "row %lld", r);
            if (len > 0) need = at + len > need ? at + len : need;      // (an empty row needs no memory, wherever it would start)
        }
        CHECK(P.need == need, "need %lld, not %lld", P.need, need);
    }
    // the refusals, each naming what it refuses
    const long long neg[2] = {4, -1}, above[2] = {4, 10}, late[3] = {1, 2, 3}, down[3] = {0, 5, 4}, huge[1] = {(1ll << 44) + 1}, hugeOff[2] = {0, (1ll << 44) + 1};
    struct Case { int format; long long n, stride; const long long* e; const char* word; } cases[] = {
        {2, 2, 9, lens, "format"}, {-1, 2, 9, lens, "format"}, {1, -1, 9, lens, "nRows"}, {1, 2, -1, lens, "rowStride"}, {1, 2, 9, nullptr, "extent"},
        {1, 2, 9, neg, "extent[1]"}, {1, 2, 9, above, "extent[1]"}, {1, 2, 0, late, "extent[0]"}, {1, 2, 0, down, "extent[2]"},
        {1, 1, 1ll << 45, huge, "extent[0]"}, {1, 1, 0, hugeOff, "extent[1]"}, {1, 1ll << 40, 1ll << 40, nullptr, "extent"}};
    for (const Case& c : cases) {
        why.clear();
        CHECK(!signal_plan(P, c.format, c.n, c.stride, c.e, why) && why.find(c.word) != std::string::npos, "%s: '%s'", c.word, why.c_str());
    }
    // a packed signal of rows within 2^44 samples each whose total leaves 2^60 elements: 2^16 + 1 rows of 2^44 (need * elSize would wrap)
    {
        const long long n = (1ll << 16) + 1;
        std::vector<long long> off((size_t)n + 1);
        for (long long r = 0; r <= n; ++r) off[(size_t)r] = r << 44;
        why.clear();
        CHECK(!signal_plan(P, 1, n, 0, off.data(), why) && why.find("2^60") != std::string::npos && why.find("row 65536") != std::string::npos, "a packed total that wraps: '%s'", why.c_str());
        CHECK(signal_plan(P, 1, n - 1, 0, off.data(), why) && P.need == kSignalMaxElements && (unsigned __int128)P.need * P.elSize < ((unsigned __int128)1 << 63), "2^60 elements is the most: %s", why.c_str());
    }
    // a padded signal whose extent in bytes leaves 62 bits
    std::vector<long long> many(3, 1);
    why.clear();
    CHECK(!signal_plan(P, 1, 3, 1ll << 61, many.data(), why) && why.find("rowStride") != std::string::npos, "a stride that wraps: '%s'", why.c_str());
    // the values a host statement takes
    std::vector<float> x(40, 0.5f);
    x[7] = 65536.0f; x[8] = -65536.0f;
    CHECK(signal_values(x.data(), 40, why), "2^16 is inside the bound: %s", why.c_str());
    const float bad[4] = {65536.0f * (1.0f + 1.0f / 8388608.0f), -1e30f, INFINITY, NAN};
    for (float v : bad) {
        x[13] = v;
        why.clear();
        CHECK(!signal_values(x.data(), 40, why) && why.find("sample 13") != std::string::npos, "%g: '%s'", (double)v, why.c_str());
    }
}

// ---- the statements: int16 and its float32 form give the same bits -------------------------------------------------------------------------
static void check_statements()
{
    std::vector<int16_t> pcm(700);
    fill(pcm);
    pcm[0] = -32768; pcm[1] = 32767; pcm[2] = 0;
    std::vector<float> x(pcm.size());
    for (size_t i = 0; i < pcm.size(); ++i) x[i] = (float)pcm[i] / 32767.0f;
    std::string why;
    // the resampler, three ratios and the identity, both formats
    const int pairs[4][2] = {{22050, 16000}, {16000, 22050}, {32000, 16000}, {16000, 16000}};
    for (auto& pr : pairs) {
        ResPlan P;
        CHECK(res_plan(P, pr[0], pr[1], 6, 0.99, 0, 0.0, why), "%s", why.c_str());
        const long long Lout = res_length((long long)pcm.size(), P.up, P.down);
        std::vector<float> a((size_t)Lout), b((size_t)Lout);
        std::vector<int16_t> qa((size_t)Lout), qb((size_t)Lout);
        CHECK(resample_host(pcm.data(), (long long)pcm.size(), P, 1, a.data()) == Lout && resample_host(x.data(), (long long)x.size(), P, 1, b.data()) == Lout, "lengths");
        resample_host(pcm.data(), (long long)pcm.size(), P, 0, qa.data());
        resample_host(x.data(), (long long)x.size(), P, 0, qb.data());
        for (long long m = 0; m < Lout; ++m) CHECK(bits(a[(size_t)m]) == bits(b[(size_t)m]) && qa[(size_t)m] == qb[(size_t)m], "%d to %d, output %lld", pr[0], pr[1], m);
        if (P.identity) for (long long m = 0; m < Lout; ++m) CHECK(bits(b[(size_t)m]) == bits(x[(size_t)m]) && qb[(size_t)m] == pcm[(size_t)m], "equal rates, output %lld", m);
    }
    // equal rates, format 0, of every int16 value: res_int16(tile_x(s)) is s, the sample itself (what resample_host's identity path rests on)
    {
        std::vector<int16_t> every(65536), back(65536);
        for (int v = 0; v < 65536; ++v) every[(size_t)v] = (int16_t)(v - 32768);
        ResPlan P;
        CHECK(res_plan(P, 22050, 22050, 6, 0.99, 0, 0.0, why) && P.identity, "%s", why.c_str());
        CHECK(resample_host(every.data(), 65536, P, 0, back.data()) == 65536, "length");
        for (int v = 0; v < 65536; ++v) CHECK(back[(size_t)v] == every[(size_t)v] && res_int16(tile_x((int)every[(size_t)v])) == every[(size_t)v], "sample %d", v - 32768);
    }
    // the convolution
    for (int K : {1, 5, 1025}) {
        std::vector<float> h((size_t)K);
        for (int k = 0; k < K; ++k) h[(size_t)k] = ((float)(rnd() % 2001) - 1000.0f) / 1000.0f / (float)(1 + k);
        for (int tail = 0; tail < 2; ++tail) {
            const long long Lout = conv_length((long long)pcm.size(), K, tail);
            std::vector<float> a((size_t)Lout), b((size_t)Lout);
            convolve_host(pcm.data(), (long long)pcm.size(), h.data(), K, tail, 1, a.data());
            convolve_host(x.data(), (long long)x.size(), h.data(), K, tail, 1, b.data());
            for (long long m = 0; m < Lout; ++m) CHECK(bits(a[(size_t)m]) == bits(b[(size_t)m]), "%d taps, output %lld", K, m);
        }
    }
    // the spectrogram
    for (int n : {64, 256}) {
        SpecPlan P;
        CHECK(spec_plan(P, n, nullptr, nullptr, 0, 2, 0.0, 0.0, why), "%s", why.c_str());
        const long long hop = n / 4 + 1, steps = ((long long)pcm.size() - 3 + hop - 1) / hop;
        std::vector<double> a((size_t)(steps * P.nOut)), b(a.size());
        CHECK(spectrogram_host(pcm.data(), (long long)pcm.size(), P, hop, 3, a.data()) == (long long)a.size(), "steps");
        CHECK(spectrogram_host(x.data(), (long long)x.size(), P, hop, 3, b.data()) == (long long)b.size(), "steps");
        CHECK(!memcmp(a.data(), b.data(), a.size() * sizeof(double)), "nFft %d", n);
    }
}

int main()
{
    check_reader<int16_t>();
    check_reader<float>();
    check_kernel_runs();
    check_plan();
    check_statements();
    printf("ok %lld\n", checks);
    return 0;
}
