// check_resample.cpp -- the host statement of the resampler (nvspeechplayer_amd/csrc/klatt_resample.h: res_plan, resample_host) against a
// brute-force binary64 loop written from the definition's formulas, at the edges of its lengths and of its plan.  Built with
// AddressSanitizer + UBSan by tests/test_resample_host.py; prints "ok <checks>" or the first failure.
#include "../../nvspeechplayer_amd/csrc/klatt_resample.h"

#include <stdlib.h>

using namespace klatt;

static long long checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// h(t) of the definition in binary64 (I0 by its series with a fixed, generous number of terms)
static double direct_tap(double t, double c, double Wd, int window, double beta)
{
    const double pi = 3.141592653589793;
    if (fabs(t) >= Wd) return 0.0;
    double w;
    if (window == 0) { const double cw = cos(pi * t / (2.0 * Wd)); w = cw * cw; }
    else {
        auto i0 = [](double x) { double term = 1.0, sum = 1.0; for (int k = 1; k < 200; ++k) { term *= (x / 2) * (x / 2) / ((double)k * k); sum += term; } return sum; };
        w = i0(beta * sqrt(1.0 - (t / Wd) * (t / Wd))) / i0(beta);
    }
    const double x = pi * c * t;
    return c * (x == 0.0 ? 1.0 : sin(x) / x) * w;
}

static void against_direct(int sr, int out, int zeros, double rolloff, int window, double beta, long long L, int kind)
{
    ResPlan P;
    std::string why;
    CHECK(res_plan(P, sr, out, zeros, rolloff, window, beta, why), "%d -> %d: %s", sr, out, why.c_str());
    const long long g = res_gcd(sr, out);
    CHECK(P.up == out / g && P.down == sr / g && P.taps == 2 * P.Z && (long long)P.table.size() == (long long)P.up * P.taps, "%d -> %d", sr, out);
    const double c = rolloff * (P.up < P.down ? (double)P.up / P.down : 1.0), Wd = zeros / c;
    CHECK(P.Z == (int)ceil(Wd), "Z %d", P.Z);
    // the table
    for (int p = 0; p < P.up; ++p)
        for (int k = 0; k < P.taps; ++k) {
            const double want = direct_tap((double)(k - P.Z + 1) - (double)p / P.up, c, Wd, window, beta);
            const double got = (double)P.table[(size_t)p * P.taps + k];
            CHECK(fabs(got - want) <= fabs(want) * 1.2e-7 + 1e-13, "h[%d][%d] = %.10g, the formula gives %.10g", p, k, got, want);
        }
    std::vector<int16_t> pcm((size_t)L);
    for (auto& s : pcm) s = kind == 0 ? (int16_t)((int)(rng() % 65535u) - 32767) : kind == 1 ? (int16_t)32767 : (int16_t)(rng() & 1u ? 32767 : -32768);
    const long long Lout = res_length(L, P.up, P.down);
    CHECK(Lout == (L * P.up + P.down - 1) / P.down, "Lout %lld", Lout);
    std::vector<float> y((size_t)Lout + 2, -7.0f);
    std::vector<int16_t> q((size_t)Lout + 2, (int16_t)-7);
    CHECK(resample_host(pcm.data(), L, P, 1, y.data() + 1) == Lout && resample_host(pcm.data(), L, P, 0, q.data() + 1) == Lout, "Lout");
    CHECK(y[0] == -7.0f && y[(size_t)Lout + 1] == -7.0f && q[0] == -7 && q[(size_t)Lout + 1] == -7, "the statement wrote outside its output");
    const double u = ldexp(1.0, -24), gamma = P.taps * u / (1.0 - P.taps * u);
    for (long long m = 0; m < Lout; ++m) {
        const long long n0 = m * P.down / P.up;
        const int p = (int)(m * P.down % P.up);
        double sum = 0.0, mag = 0.0;
        for (int i = -P.Z + 1; i <= P.Z; ++i) {
            const long long n = n0 + i;
            const double x = n >= 0 && n < L ? (double)((float)pcm[(size_t)n] / 32767.0f) : 0.0;
            const double h = (double)P.table[(size_t)p * P.taps + (i + P.Z - 1)];
            sum += x * h; mag += fabs(x * h);
        }
        const float got = y[(size_t)m + 1];
        CHECK(fabs((double)got - sum) <= gamma * mag, "%d -> %d, zeros %d, %lld samples: y[%lld] = %.9g, the double loop gives %.9g (bound %.3g)", sr, out, zeros, L, m, (double)got, sum, gamma * mag);
        const float s = got * 32767.0f;
        const int want = s >= 32767.0f ? 32767 : s <= -32768.0f ? -32768 : (int)nearbyintf(s);
        CHECK(q[(size_t)m + 1] == want, "int16 of y[%lld] = %.9g is %d, not %d", m, (double)got, q[(size_t)m + 1], want);
    }
}

int main()
{
    const int pairs[][2] = {{22050, 16000}, {22050, 24000}, {22050, 44100}, {22050, 11025}, {16000, 22050}, {44100, 48000}, {7, 5}, {5, 7}, {1, 512}, {512, 1}};
    for (const auto& pr : pairs) {
        const long long g = res_gcd(pr[0], pr[1]), down = pr[0] / g;
        const long long lens[] = {0, 1, 2, 3, down, down + 1, 3 * down + 37};
        for (long long L : lens)
            for (int kind = 0; kind < 3; ++kind) {
                if (down > 100 && L > down + 1 && kind == 1) continue;
                against_direct(pr[0], pr[1], pr[0] == 512 ? 1 : 6, pr[0] == 512 ? 1.0 : 0.99, 0, 0.0, L, kind);
                if (L == 3 || L == down + 1) {
                    against_direct(pr[0], pr[1], pr[0] == 512 ? 1 : 2, 1.0, 0, 0.0, L, kind);
                    if (pr[0] != 512) against_direct(pr[0], pr[1], 16, 0.9, 1, 8.6, L, kind);
                }
            }
    }
    against_direct(22050, 16000, 64, 0.99, 1, 8.6, 500, 0);
    // equal rates: the samples themselves
    {
        ResPlan P;
        std::string why;
        CHECK(res_plan(P, 22050, 22050, 6, 0.99, 0, 0.0, why) && P.identity && P.up == 1 && P.down == 1, "%s", why.c_str());
        std::vector<int16_t> pcm = {0, 1, -1, 32767, -32768}, q(5);
        std::vector<float> y(5);
        CHECK(resample_host(pcm.data(), 5, P, 0, q.data()) == 5 && q == pcm, "equal rates, int16");
        CHECK(resample_host(pcm.data(), 5, P, 1, y.data()) == 5, "equal rates, float32");
        for (int i = 0; i < 5; ++i) CHECK(y[(size_t)i] == (float)pcm[(size_t)i] / 32767.0f, "equal rates, sample %d", i);
    }
    // the int16 conversion at its edges
    CHECK(res_int16(1.0f) == 32767 && res_int16(1.59f) == 32767 && res_int16(-1.59f) == -32768 && res_int16(-32768.0f / 32767.0f) == -32768, "clips");
    CHECK(res_int16(0.5f / 32767.0f) == 0 && res_int16(1.5f / 32767.0f) == 2 && res_int16(2.5f / 32767.0f) == 2 && res_int16(-0.5f / 32767.0f) == 0, "ties to even");
    // lengths
    CHECK(res_length(0, 320, 441) == 0 && res_length(1, 320, 441) == 1 && res_length(441, 320, 441) == 320 && res_length(442, 320, 441) == 321, "lengths");
    CHECK(res_length(1ll << 62, 1ll << 30, 1) == 0x7FFFFFFFFFFFFFFFll && res_length(1ll << 40, 3, 2) == 1649267441664ll, "long lengths");
    // the kernel's span: its inputs fit
    for (const auto& pr : pairs) {
        ResPlan P;
        std::string why;
        CHECK(res_plan(P, pr[0], pr[1], pr[0] == 512 ? 1 : 6, pr[0] == 512 ? 1.0 : 0.99, 0, 0.0, why), "%s", why.c_str());
        const int span = res_span(P);
        CHECK(span >= 1 && span <= kResampleTile, "span %d", span);
        for (long long m0 : {0ll, 1ll, 12345ll, (1ll << 40) + 7}) {
            long long nA, nB; int pA, pB;
            res_locate(m0, P.up, P.down, nA, pA);
            res_locate(m0 + span - 1, P.up, P.down, nB, pB);
            CHECK(nB - nA + P.taps <= kResampleIn && pA >= 0 && pA < P.up, "a span of %d outputs from %lld takes %lld inputs", span, m0, nB - nA + P.taps);
        }
        res_transpose(P);
        for (int j = 0; j < P.up; ++j)
            for (int k = 0; k < P.taps; ++k)
                CHECK(P.hT[(size_t)k * P.up + j] == P.table[(size_t)(((long long)j * P.down) % P.up) * P.taps + k], "hT[%d][%d]", k, j);
    }
    // the refusals of the plan
    {
        ResPlan P;
        std::string why;
        const double nan = NAN, inf = INFINITY;
        CHECK(!res_plan(P, 0, 16000, 6, 0.99, 0, 0.0, why) && !res_plan(P, 22050, 0, 6, 0.99, 0, 0.0, why) && !res_plan(P, -1, 16000, 6, 0.99, 0, 0.0, why) && !why.empty(), "rates");
        CHECK(!res_plan(P, 22050, 16000, 0, 0.99, 0, 0.0, why) && !res_plan(P, 22050, 16000, -3, 0.99, 0, 0.0, why), "zeros");
        for (double bad : {0.0, -0.5, 1.0000001, nan, inf}) CHECK(!res_plan(P, 22050, 16000, 6, bad, 0, 0.0, why), "rolloff %g", bad);
        CHECK(!res_plan(P, 22050, 16000, 6, 0.99, 2, 0.0, why) && !res_plan(P, 22050, 16000, 6, 0.99, -1, 0.0, why), "window");
        for (double bad : {-1.0, nan, inf}) CHECK(!res_plan(P, 22050, 16000, 6, 0.99, 1, bad, why), "beta %g", bad);
        CHECK(res_plan(P, 22050, 16000, 6, 0.99, 0, nan, why), "Hann does not look at beta: %s", why.c_str());
        CHECK(!res_plan(P, 22050, 22051, 6, 0.99, 0, 0.0, why), "up 22051");
        CHECK(!res_plan(P, 22050, 16000, 372, 0.99, 0, 0.0, why) && res_plan(P, 22050, 16000, 367, 0.99, 0, 0.0, why) && P.taps == 1022, "taps: %s", why.c_str());
        CHECK(!res_plan(P, 4097, 4096, 500, 1.0, 0, 0.0, why) && !res_plan(P, 2147483647, 1, 1, 1.0, 0, 0.0, why), "table and ratio");
        CHECK(res_plan(P, 4096, 4095, 127, 1.0, 0, 0.0, why) && (long long)P.up * P.taps <= kResampleMaxTable, "%s", why.c_str());
        CHECK(!res_plan(P, 4096, 4095, 128, 1.0, 0, 0.0, why), "up * taps above 2^20");
    }
    printf("ok %lld\n", checks);
    return 0;
}
