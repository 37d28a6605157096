// check_spectrum.cpp -- the host statement of the spectrogram (nvspeechplayer_amd/csrc/klatt_spectrum.h: spec_plan, spectrogram_host) against
// a direct binary64 DFT, at the edges of its framing and of its plan.  Built with AddressSanitizer + UBSan by
// tests/test_spectrogram_host.py; prints "ok <checks>" or the first failure.
#include "../../nvspeechplayer_amd/csrc/klatt_spectrum.h"

#include <stdlib.h>

using namespace klatt;

static long long checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// |X_k| of the frame centred on c by the definition's sum, in binary64 over the float32 products xw[i]
static void direct(const std::vector<int16_t>& pcm, const SpecPlan& P, long long c, std::vector<double>& mag, double& norm)
{
    const int N = P.nFft;
    std::vector<double> xw((size_t)N);
    norm = 0.0;
    for (int i = 0; i < N; ++i) {
        const long long t = c - N / 2 + i;
        const int s = t >= 0 && t < (long long)pcm.size() ? pcm[(size_t)t] : 0;
        xw[(size_t)i] = (double)spec_input(s, P.window[(size_t)i]);
        norm += xw[(size_t)i] * xw[(size_t)i];
    }
    norm = sqrt(norm);
    static std::vector<double> cs, sn;      // cos and sin of 2 pi q / N
    if ((int)cs.size() != N) {
        cs.resize((size_t)N); sn.resize((size_t)N);
        for (int q = 0; q < N; ++q) { cs[(size_t)q] = cos(6.283185307179586 * q / N); sn[(size_t)q] = sin(6.283185307179586 * q / N); }
    }
    mag.assign((size_t)N / 2 + 1, 0.0);
    for (int k = 0; k <= N / 2; ++k) {
        double re = 0.0, im = 0.0;
        for (int i = 0; i < N; ++i) {
            const size_t q = (size_t)(((long long)i * k) & (N - 1));
            re += xw[(size_t)i] * cs[q]; im -= xw[(size_t)i] * sn[q];
        }
        mag[(size_t)k] = sqrt(re * re + im * im);
    }
}

static void against_direct(int nFft, long long L, long long hop, long long phase, int kind)
{
    SpecPlan P;
    std::string why;
    CHECK(spec_plan(P, nFft, nullptr, nullptr, 0, 1, 0.0, 0.0, why), "%s", why.c_str());
    std::vector<int16_t> pcm((size_t)L);
    for (long long t = 0; t < L; ++t)
        pcm[(size_t)t] = kind == 0 ? (int16_t)((int)(rng() % 65535u) - 32767) : kind == 1 ? (int16_t)(t & 1 ? 32767 : -32767) : (int16_t)(t % 3 == 0);
    const long long steps = L > phase ? (L - phase + hop - 1) / hop : 0;
    std::vector<double> out((size_t)(steps * P.nOut) + 1, -1.0);
    CHECK(spectrogram_host(pcm.data(), L, P, hop, phase, out.data()) == steps * P.nOut, "nFft %d L %lld", nFft, L);
    CHECK(out.back() == -1.0, "the statement wrote past its output");
    const double u = ldexp(1.0, -24);
    int logN = 0;
    while ((1 << logN) < nFft) ++logN;
    std::vector<double> mag;
    for (long long j = 0; j < steps; j += (steps > 6 ? steps / 6 : 1)) {
        double norm;
        direct(pcm, P, phase + j * hop, mag, norm);
        const double B = (8.0 * logN + 8.0) * u * sqrt((double)nFft) * norm;
        for (int k = 0; k < P.nOut; ++k) {
            const double got = out[(size_t)(j * P.nOut + k)];
            CHECK(fabs(got - mag[(size_t)k]) <= B + 4.0 * u * mag[(size_t)k], "nFft %d step %lld bin %d: %.9g against %.9g (bound %.3g)", nFft, j, k, got, mag[(size_t)k], B);
        }
    }
}

int main()
{
    for (int nFft : {64, 256, 1024, 4096})
        for (int kind = 0; kind < 3; ++kind) {
            against_direct(nFft, nFft + 3, nFft / 4, 0, kind);
            against_direct(nFft, 1, 1, 0, kind);
            against_direct(nFft, nFft / 2 - 1, 7, 5, kind);
            against_direct(nFft, nFft / 2, nFft + 5, 0, kind);
        }
    against_direct(64, 777, 1, 3, 0);
    {   // silence is +0 in every bin, on its bits; a phase at or past the end gives no steps
        SpecPlan P; std::string why;
        CHECK(spec_plan(P, 256, nullptr, nullptr, 0, 2, 0.0, 0.0, why), "%s", why.c_str());
        std::vector<int16_t> pcm(300, 0);
        std::vector<double> out((size_t)(3 * P.nOut), -1.0);
        CHECK(spectrogram_host(pcm.data(), 300, P, 128, 0, out.data()) == 3 * P.nOut, "steps");
        for (double x : out) CHECK(x == 0.0 && !signbit(x), "silence gives %g", x);
        CHECK(spectrogram_host(pcm.data(), 300, P, 128, 300, nullptr) == 0 && spectrogram_host(pcm.data(), 0, P, 1, 0, nullptr) == 0, "no steps");
    }
    {   // a bank: ranges, an empty row, the float32 sum in ascending order, and the logarithm's floor
        const int N = 64, K = N / 2 + 1;
        std::vector<double> bank((size_t)3 * K, 0.0);
        bank[5] = 0.5; bank[9] = 0.25;                  // row 0: columns 5 .. 9
        bank[(size_t)2 * K + K - 1] = 2.0;              // row 2: the last column alone; row 1: empty
        SpecPlan P, Q; std::string why;
        CHECK(spec_plan(P, N, nullptr, bank.data(), 3, 2, 0.0, 0.0, why), "%s", why.c_str());
        CHECK(P.nOut == 3 && P.range[0] == 5 && P.range[1] == 9 && P.range[2] > P.range[3] && P.range[4] == K - 1 && P.range[5] == K - 1, "ranges");
        CHECK(spec_plan(Q, N, nullptr, nullptr, 0, 2, 0.0, 0.0, why), "%s", why.c_str());
        std::vector<int16_t> pcm(100);
        for (auto& s : pcm) s = (int16_t)((int)(rng() % 20001u) - 10000);
        std::vector<double> bands(2 * 3), bins((size_t)2 * K), logs(2 * 3);
        CHECK(spectrogram_host(pcm.data(), 100, P, 50, 0, bands.data()) == 6 && spectrogram_host(pcm.data(), 100, Q, 50, 0, bins.data()) == 2 * K, "counts");
        for (int j = 0; j < 2; ++j) {
            float acc = 0.0f;
            for (int k = 5; k <= 9; ++k) acc = acc + P.weights[(size_t)k] * (float)bins[(size_t)(j * K + k)];
            CHECK(bands[(size_t)j * 3] == (double)acc, "band 0 of step %d", j);
            CHECK(bands[(size_t)j * 3 + 1] == 0.0 && !signbit(bands[(size_t)j * 3 + 1]), "the empty band of step %d", j);
            CHECK(bands[(size_t)j * 3 + 2] == (double)(2.0f * (float)bins[(size_t)(j * K + K - 1)]), "band 2 of step %d", j);
        }
        CHECK(spec_plan(P, N, nullptr, bank.data(), 3, 2, 10.0, 1e-10, why), "%s", why.c_str());
        CHECK(spectrogram_host(pcm.data(), 100, P, 50, 0, logs.data()) == 6, "counts");
        CHECK(fabs(logs[1] - -100.0) < 1e-9 && fabs(logs[0] - 10.0 * log10(bands[0])) < 1e-9, "log: %g, %g", logs[1], logs[0]);
    }
    {   // refusals
        SpecPlan P; std::string why;
        const double nan = NAN, inf = INFINITY;
        std::vector<double> w(64, 1.0), bank(33, 1.0);
        for (int bad : {0, 32, 63, 96, 8192, -64}) CHECK(!spec_plan(P, bad, nullptr, nullptr, 0, 2, 0.0, 0.0, why) && !why.empty(), "nFft %d", bad);
        for (int bad : {0, 3, -1}) CHECK(!spec_plan(P, 64, nullptr, nullptr, 0, bad, 0.0, 0.0, why), "power %d", bad);
        CHECK(!spec_plan(P, 64, nullptr, bank.data(), 0, 2, 0.0, 0.0, why) && !spec_plan(P, 64, nullptr, bank.data(), -1, 2, 0.0, 0.0, why), "bands");
        CHECK(!spec_plan(P, 64, nullptr, nullptr, 0, 2, 10.0, 0.0, why) && !spec_plan(P, 64, nullptr, nullptr, 0, 2, 10.0, -1.0, why), "floor");
        CHECK(!spec_plan(P, 64, nullptr, nullptr, 0, 2, nan, 1.0, why) && !spec_plan(P, 64, nullptr, nullptr, 0, 2, inf, 1.0, why) &&
              !spec_plan(P, 64, nullptr, nullptr, 0, 2, 10.0, nan, why) && !spec_plan(P, 64, nullptr, nullptr, 0, 2, 0.0, inf, why), "non-finite log");
        w[63] = nan; CHECK(!spec_plan(P, 64, w.data(), nullptr, 0, 2, 0.0, 0.0, why), "window");
        w[63] = 1.0; bank[32] = inf; CHECK(!spec_plan(P, 64, w.data(), bank.data(), 1, 2, 0.0, 0.0, why), "bank");
        bank[32] = 1.0; CHECK(spec_plan(P, 64, w.data(), bank.data(), 1, 1, 0.0, -5.0, why), "%s", why.c_str());
    }
    printf("ok %lld\n", checks);
    return 0;
}
