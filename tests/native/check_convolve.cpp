// check_convolve.cpp -- the host statement of the convolution export (nvspeechplayer_amd/csrc/klatt_convolve.h: conv_plan, conv_row,
// convolve_host) against an independent binary64 loop, and the kernel's tile / block / skip arithmetic against brute force: a model of
// the kernel written from the index functions alone visits, for every output, exactly its non-skippable terms in ascending tap order,
// stays inside its staged arrays, and arrives at the statement's bits.  Built with AddressSanitizer + UBSan by
// tests/test_convolve_host.py; prints "ok <checks>" or the first failure.
#include "../../nvspeechplayer_amd/csrc/klatt_convolve.h"

#include <stdlib.h>
#include <string.h>

using namespace klatt;

static long long checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static uint32_t rng_state = 2463534242u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static std::vector<int16_t> signal(long long L, int kind)
{
    std::vector<int16_t> pcm((size_t)L);
    for (auto& s : pcm) s = kind == 0 ? (int16_t)((int)(rng() % 65535u) - 32767) : kind == 1 ? (int16_t)(rng() & 1u ? 32767 : -32768) : (int16_t)((rng() % 7u) == 0 ? (int)(rng() % 5u) - 2 : 0);
    return pcm;
}

static std::vector<float> response(int K, int kind)
{
    std::vector<float> h((size_t)K);
    for (int k = 0; k < K; ++k) {
        const float r = (float)((int)(rng() % 2001u) - 1000) / 1000.0f;
        h[(size_t)k] = kind == 0 ? r * expf(-4.0f * (float)k / (float)K) : kind == 1 ? ((rng() % 3u) == 0 ? 0.0f : r) : ldexpf(r, -130);
    }
    return h;
}

// The statement against a double loop written from the definition
static void against_double(long long L, int K, int tail, int sKind, int hKind)
{
    const std::vector<int16_t> pcm = signal(L, sKind);
    const std::vector<float> h = response(K, hKind);
    const long long Lout = conv_length(L, K, tail);
    CHECK(Lout == (tail ? L + K - 1 : L), "Lout %lld", Lout);
    std::vector<float> y((size_t)Lout + 2, -7.0f);
    std::vector<int16_t> q((size_t)Lout + 2, (int16_t)-7);
    CHECK(convolve_host(pcm.data(), L, h.data(), K, tail, 1, y.data() + 1) == Lout && convolve_host(pcm.data(), L, h.data(), K, tail, 0, q.data() + 1) == Lout, "Lout");
    CHECK(y[0] == -7.0f && y[(size_t)Lout + 1] == -7.0f && q[0] == -7 && q[(size_t)Lout + 1] == -7, "the statement wrote outside its output");
    const double u = ldexp(1.0, -24), gamma = K * u / (1.0 - K * u);
    for (long long m = 0; m < Lout; ++m) {
        double sum = 0.0, mag = 0.0;
        for (int k = 0; k < K; ++k) {
            const long long n = m - k;
            const double x = n >= 0 && n < L ? (double)((float)pcm[(size_t)n] / 32767.0f) : 0.0;
            sum += x * (double)h[(size_t)k]; mag += fabs(x * (double)h[(size_t)k]);
        }
        const float got = y[(size_t)m + 1];
        // (products of subnormal responses round in the sum: one half unit of the smallest subnormal per term)
        CHECK(fabs((double)got - sum) <= gamma * mag + K * ldexp(1.0, -150), "L %lld, K %d, tail %d: y[%lld] = %.9g, the double loop gives %.9g (bound %.3g)", L, K, tail, m, (double)got, sum, gamma * mag);
        CHECK(!(got == 0.0f) || bits(got) == 0u, "y[%lld] is -0", m);
        const float s = got * 32767.0f;
        const int want = s >= 32767.0f ? 32767 : s <= -32768.0f ? -32768 : (int)nearbyintf(s);
        CHECK(q[(size_t)m + 1] == want, "int16 of y[%lld] = %.9g is %d, not %d", m, (double)got, q[(size_t)m + 1], want);
    }
}

// The kernel, from its index functions: tiles of a row of `width` elements (the padded form's rowStride, or Lout), every lane of a tile,
// the staged arrays with guards.  terms[o] collects the taps k whose product the lane's output o meets with a sample inside the signal.
static void model(long long L, int K, int tail, long long width, int sKind, int hKind)
{
    const std::vector<int16_t> pcm = signal(L, sKind);
    const std::vector<float> h = response(K, hKind);
    const long long Lout = conv_length(L, K, tail);
    std::vector<float> want((size_t)Lout + 1);
    convolve_host(pcm.data(), L, h.data(), K, tail, 1, want.data());
    const int T = kConvolveTile;
    CHECK(conv_blocks(K) == (K + kConvolveBlock - 1) / kConvolveBlock, "blocks");
    for (long long t0 = 0; t0 < width; t0 += T) {
        const int n = (int)std::min<long long>(T, width - t0);
        const int live = (int)std::max<long long>(0, std::min<long long>(n, Lout - t0));
        std::vector<float> acc((size_t)T, 0.0f);
        std::vector<std::vector<int>> terms((size_t)T);
        bool ended = false;
        for (int b = 0; live > 0 && b < conv_blocks(K); ++b) {
            const int kb = b * kConvolveBlock;
            const int taps = conv_block_taps(K, kb), padded = conv_block_padded(taps);
            CHECK(taps >= 1 && taps <= kConvolveBlock && kb + taps <= K && padded >= taps && padded < taps + 4 && padded % 4 == 0 && padded <= kConvolveBlock, "block %d: %d taps, %d staged", b, taps, padded);
            // brute force: does any live output meet a sample of the signal in this block?
            bool any = false;
            for (int o = 0; o < live && !any; ++o)
                for (int k = kb; k < kb + taps; ++k) { const long long s = t0 + o - k; if (s >= 0 && s < L) { any = true; break; } }
            if (conv_block_last(t0, live, kb)) { ended = true; CHECK(!any, "tile %lld: block %d ends the loop but has terms", t0, b); }
            if (ended) { CHECK(!any && conv_block_skipped(t0, live, L, kb, taps), "tile %lld: block %d after the last one has terms", t0, b); continue; }
            CHECK(conv_block_skipped(t0, live, L, kb, taps) == !any, "tile %lld, block %d: skipped %d, terms %d", t0, b, (int)conv_block_skipped(t0, live, L, kb, taps), (int)any);
            if (!any) continue;
            // the staging: taps and reversed inputs, exact sizes (the sanitizer guards both ends)
            std::vector<float> hs((size_t)padded), xr((size_t)(T + padded));
            std::vector<long long> at((size_t)(T + padded));
            for (int i = 0; i < padded; ++i) hs[(size_t)i] = i < taps ? h[(size_t)(kb + i)] : 0.0f;
            for (int p = 0; p < T + padded; ++p) {
                const long long s = conv_staged_sample(t0, kb, p);
                at[(size_t)p] = s;
                xr[(size_t)p] = res_input(s >= 0 && s < L ? (int)pcm[(size_t)s] : 0);
            }
            for (int lane = 0; lane < 256; ++lane) {
                const int w = conv_window(lane);
                CHECK(w >= 0 && w % 4 == 0 && w + padded + 3 < T + padded, "window %d", w);
                float a[4] = {xr[(size_t)w], xr[(size_t)w + 1], xr[(size_t)w + 2], xr[(size_t)w + 3]};
                float lacc[4] = {acc[(size_t)(4 * lane)], acc[(size_t)(4 * lane + 1)], acc[(size_t)(4 * lane + 2)], acc[(size_t)(4 * lane + 3)]};
                for (int q = 0; q < padded; q += 4) {
                    const size_t nb = (size_t)(w + q + 4);
                    const float bq[4] = {xr.at(nb), xr.at(nb + 1), xr.at(nb + 2), xr.at(nb + 3)};
                    const float v[7] = {a[1], a[2], a[3], bq[0], bq[1], bq[2], bq[3]};
                    const float h4[4] = {hs.at((size_t)q), hs.at((size_t)q + 1), hs.at((size_t)q + 2), hs.at((size_t)q + 3)};
                    conv_step4(lacc, v, h4);
                    for (int t = 0; t < 4; ++t)
                        for (int j = 0; j < 4; ++j) {
                            // v[t + 3 - j] is xr[w + q + 1 + t + 3 - j]: the sample output 4 lane + j meets at tap kb + q + t
                            const long long s = at[(size_t)(w + q + 4 + t - j)];
                            CHECK(s == t0 + 4 * lane + j - (kb + q + t), "lane %d output %d tap %d reads sample %lld", lane, j, kb + q + t, s);
                            if (q + t < taps && s >= 0 && s < L) terms[(size_t)(4 * lane + j)].push_back(kb + q + t);
                        }
                    memcpy(a, bq, sizeof a);
                }
                for (int j = 0; j < 4; ++j) acc[(size_t)(4 * lane + j)] = lacc[j];
            }
        }
        for (int o = 0; o < live; ++o) {
            const long long m = t0 + o;
            // the output's non-skippable terms: taps whose sample lies inside the signal, ascending
            std::vector<int> need;
            for (int k = 0; k < K; ++k) if (m - k >= 0 && m - k < L) need.push_back(k);
            CHECK(terms[(size_t)o] == need, "output %lld (L %lld, K %d): %zu terms visited, %zu needed", m, L, K, terms[(size_t)o].size(), need.size());
            CHECK(bits(conv_finish(acc[(size_t)o])) == bits(want[(size_t)m]), "output %lld (L %lld, K %d, tail %d): the model gives %.9g, the statement %.9g", m, L, K, tail, (double)conv_finish(acc[(size_t)o]), (double)want[(size_t)m]);
        }
    }
}

int main()
{
    const int T = kConvolveTile, B = kConvolveBlock;
    // the statement
    for (int K : {1, 2, 5, B - 1, B, B + 1, 2 * B + 3})
        for (long long L : {0ll, 1ll, 2ll, 3ll, 17ll, 300ll})
            for (int tail = 0; tail < 2; ++tail) {
                if (K > 100 && L > 17 && tail == 0) continue;
                against_double(L, K, tail, (int)((L + K) % 3), K % 2);
            }
    against_double(500, 64, 1, 1, 0);
    against_double(40, 33, 1, 0, 2);      // every product subnormal
    // the kernel's arithmetic
    for (int K : {1, 2, 3, 4, 5, 7, B - 1, B, B + 1, 2 * B + 3})
        for (long long L : {3ll, 4ll, 5ll, (long long)T - 1, (long long)T, (long long)T + 1, 2ll * T + 1}) {
            if (K > 7 && K != B + 1 && L != 3 && L != T + 1) continue;      // (the long responses at every edge are K = B + 1's)
            for (int tail = 0; tail < 2; ++tail) {
                const long long Lout = conv_length(L, K, tail);
                model(L, K, tail, Lout, 0, K % 2);
                if (K <= 5 || L <= 5) model(L, K, tail, Lout + 3, 1, 0);                     // a padded row: the remainder's tiles have no terms
                if (K == B + 1 && L == 3) model(L, K, tail, Lout + 2 * T, 0, 0);
            }
        }
    model(3 * T + 5, 3 * B + 2, 1, conv_length(3 * T + 5, 3 * B + 2, 1), 2, 1);               // sparse signal, zero taps: skips inside a row
    // the conversions the export shares with the resampler
    CHECK(res_int16(1.0f) == 32767 && res_int16(1.59f) == 32767 && res_int16(-1.59f) == -32768, "clips");
    CHECK(res_int16(0.5f / 32767.0f) == 0 && res_int16(1.5f / 32767.0f) == 2 && res_int16(2.5f / 32767.0f) == 2, "ties to even");
    CHECK(bits(conv_finish(-0.0f)) == 0u && bits(conv_finish(0.0f)) == 0u && conv_step(1.0f, 3.0f, 0.5f) == 2.5f, "finish");
    CHECK(conv_step(-1.0f, 1.0f + ldexpf(1.0f, -23), 1.0f - ldexpf(1.0f, -23)) == -ldexpf(1.0f, -46), "conv_step is fused");
    // the plan and its refusals
    {
        ConvPlan P;
        std::string why;
        std::vector<float> ir(70000, 0.25f);
        const long long one[2] = {0, 5}, three[4] = {0, 1, 5, 65541};
        CHECK(conv_plan(P, ir.data(), one, 1, 0, why) && P.nIr == 1 && P.taps.size() == 5 && P.most == 5 && P.start.size() == 2, "%s", why.c_str());
        CHECK(conv_plan(P, ir.data(), three, 3, 1, why) && P.nIr == 3 && P.most == 65536 && P.taps.size() == 65541, "%s", why.c_str());
        const long long rows[4] = {2, 0, 1, 2}, badRow[2] = {0, 3}, negRow[1] = {-1};
        for (int i = 0; i < 4; ++i) CHECK(conv_row(P, rows, i, why) == rows[i], "row %d", i);
        CHECK(conv_row(P, badRow, 1, why) == -1 && conv_row(P, negRow, 0, why) == -1 && conv_row(P, nullptr, 0, why) == -1 && !why.empty(), "irOf");
        CHECK(conv_plan(P, ir.data(), one, 1, 0, why) && conv_row(P, nullptr, 7, why) == 0, "NULL irOf takes the one response");
        CHECK(!conv_plan(P, ir.data(), one, 1, 2, why) && !conv_plan(P, ir.data(), one, 1, -1, why), "tail");
        CHECK(!conv_plan(P, ir.data(), one, 0, 1, why) && !conv_plan(P, ir.data(), one, -3, 1, why), "nIr");
        CHECK(!conv_plan(P, nullptr, one, 1, 1, why) && !conv_plan(P, ir.data(), nullptr, 1, 1, why), "NULL");
        const long long late[2] = {1, 5}, empty[3] = {0, 4, 4}, back[3] = {0, 4, 2}, longer[2] = {0, 65537};
        CHECK(!conv_plan(P, ir.data(), late, 1, 1, why) && !conv_plan(P, ir.data(), empty, 2, 1, why) && !conv_plan(P, ir.data(), back, 2, 1, why), "irStart");
        CHECK(!conv_plan(P, ir.data(), longer, 1, 1, why) && why.find("65537 taps") != std::string::npos, "taps: %s", why.c_str());
        std::vector<float> big((size_t)kConvolveMaxTable + 1, 0.5f);
        std::vector<long long> starts;
        for (long long s = 0; s <= kConvolveMaxTable; s += 65536) starts.push_back(s);
        CHECK(conv_plan(P, big.data(), starts.data(), (long long)starts.size() - 1, 1, why) && (long long)P.taps.size() == kConvolveMaxTable, "%s", why.c_str());
        starts.push_back(kConvolveMaxTable + 1);
        CHECK(!conv_plan(P, big.data(), starts.data(), (long long)starts.size() - 1, 1, why) && why.find("in all") != std::string::npos, "table: %s", why.c_str());
        for (float bad : {NAN, INFINITY, -INFINITY, 4294967808.0f, -8589934592.0f}) {
            ir[3] = bad;
            CHECK(!conv_plan(P, ir.data(), three, 3, 1, why) && why.find("tap 2 of response 1") != std::string::npos, "tap %g: %s", (double)bad, why.c_str());
        }
        ir[3] = -4294967296.0f;
        CHECK(conv_plan(P, ir.data(), three, 3, 1, why), "2^32 is admitted: %s", why.c_str());
    }
    printf("ok %lld\n", checks);
    return 0;
}
