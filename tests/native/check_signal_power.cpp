// check_signal_power.cpp -- the power of a signal's row (nvspeechplayer_amd/csrc/klatt_sigpower.h) against brute force: a model of
// klatt_signal_power and of its row pass written from the shared index functions alone -- the walk over a table that counts blocks, a
// leaf per lane, the load masks, the xor butterfly, the four wave sums, the ascending chain over the partials -- reads every sample of a row
// exactly once and nothing outside it, at every 4-byte misalignment of the row's start inside a 16-byte line, and arrives at the bits of
// the statement (sig_power_host) and of a restatement written here from the definition.  The Lemma is exercised: poison past L changes
// nothing.  The rows are exact-size heap arrays read through plain pointers: the sanitizer guards both ends.
// Built with AddressSanitizer + UBSan by tests/test_signal_mix_host.py; prints "ok <checks>" or the first failure.
#include "../../nvspeechplayer_amd/csrc/klatt_mix.h"

#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace klatt;

static long long checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static uint32_t rng_state = 2463534242u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static uint64_t bits(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }

// Values inside the bound with exponents spread over forty binades, both signs, and the edge values
static float value()
{
    const uint32_t k = rng() % 64u;
    if (k == 0) return -0.0f;
    if (k == 1) return 65536.0f;
    if (k == 2) return -65536.0f;
    if (k == 3) return 0.0f;
    const float m = (float)((int)(rng() % 16777215u) - 8388607) / 8388608.0f;      // 24 significant bits
    return ldexpf(m, (int)(rng() % 41u) - 24);                                      // |v| < 2^16
}

// The definition, written out: the squares of the row padded with +0 to whole blocks, leaves ascending, pairwise halving eight times,
// the blocks ascending from +0.0, over L
static double restated(const float* x, long long L)
{
    const long long nb = (L + 2047) / 2048;
    double Q = 0.0;
    for (long long b = 0; b < nb; ++b) {
        std::vector<double> sq(2048, 0.0);
        for (long long i = 0; i < 2048 && b * 2048 + i < L; ++i) sq[(size_t)i] = (double)x[b * 2048 + i] * (double)x[b * 2048 + i];
        std::vector<double> t(256);
        for (int l = 0; l < 256; ++l) {
            double acc = sq[(size_t)(8 * l)] + sq[(size_t)(8 * l + 1)];
            for (int q = 2; q < 8; ++q) acc = acc + sq[(size_t)(8 * l + q)];
            t[(size_t)l] = acc;
        }
        for (int n = 128; n >= 1; n /= 2) {
            std::vector<double> up((size_t)n);
            for (int i = 0; i < n; ++i) up[(size_t)i] = t[(size_t)(2 * i)] + t[(size_t)(2 * i + 1)];
            t = up;
        }
        Q = Q + t[0];
    }
    return L > 0 ? Q / (double)L : 0.0;
}

// packed_locate (klatt_timeline.h, device only), restated: the last job that starts on or before block g
static void locate(long long g, const std::vector<long long>& start, long long& r, long long& j)
{
    long long lo = 0, hi = (long long)start.size() - 1;
    while (hi - lo > 1) { const long long mid = (lo + hi) >> 1; if (start[(size_t)mid] <= g) lo = mid; else hi = mid; }
    r = lo; j = g - start[(size_t)r];
}

struct Job { const float* row; long long len; std::vector<int>* reads; };

// The kernel and the row pass over the jobs, from the index functions: -> one power per job
static std::vector<double> model(const std::vector<Job>& jobs)
{
    std::vector<long long> blockStart{0};
    for (const Job& job : jobs) blockStart.push_back(blockStart.back() + sig_blocks(job.len));
    const long long nBlocks = blockStart.back(), nJobs = (long long)jobs.size();
    std::vector<double> partials((size_t)nBlocks, -1.0);
    std::vector<int> written((size_t)nBlocks, 0);
    for (long long g = 0; g < nBlocks; ++g) {
        long long r, j;
        locate(g, blockStart, r, j);
        CHECK(r >= 0 && r < nJobs && j >= 0 && j < sig_blocks(jobs[(size_t)r].len), "block %lld is block %lld of job %lld", g, j, r);
        const Job& job = jobs[(size_t)r];
        double t[kSigPowerLeaves];
        for (int lane = 0; lane < kSigPowerLeaves; ++lane) {
            const long long s0 = sig_leaf_start(j, lane);
            const int live = sig_leaf_live(s0, job.len);
            CHECK(live >= 0 && live <= kSigPowerLeaf && (live == 0 || s0 + live <= job.len) && (live == kSigPowerLeaf || s0 + live >= job.len), "leaf at %lld of %lld: %d live", s0, job.len, live);
            double leaf = 0.0;
            if (live > 0) {
                const float* p = job.row + s0;
                float v[kSigPowerLeaf];
                if (sig_leaf_whole(p, live)) {
                    CHECK((reinterpret_cast<uintptr_t>(p) & 15) == 0 && s0 + kSigPowerLeaf <= job.len, "two 16-byte loads at %p, sample %lld of %lld", (const void*)p, s0, job.len);
                    for (int q = 0; q < kSigPowerLeaf; ++q) { v[q] = p[q]; ++(*job.reads)[(size_t)(s0 + q)]; }
                } else {
                    for (int q = 0; q < kSigPowerLeaf; ++q) {
                        v[q] = 0.0f;
                        if (q < live) { CHECK(s0 + q < job.len, "sample %lld of %lld", s0 + q, job.len); v[q] = p[q]; ++(*job.reads)[(size_t)(s0 + q)]; }
                    }
                }
                leaf = sig_leaf(v);
            }
            t[lane] = leaf;
        }
        // the butterfly d = 1 .. 32 within each wavefront of 64 lanes: every lane ends with the same bits
        for (int d = 1; d <= 32; d <<= 1) {
            double next[kSigPowerLeaves];
            for (int lane = 0; lane < kSigPowerLeaves; ++lane) next[lane] = t[lane] + t[(lane & ~63) | ((lane & 63) ^ d)];
            memcpy(t, next, sizeof t);
        }
        for (int lane = 0; lane < kSigPowerLeaves; ++lane) CHECK(bits(t[lane]) == bits(t[lane & ~63]), "lane %d of block %lld", lane, g);
        partials[(size_t)g] = sig_waves(t[0], t[64], t[128], t[192]);
        ++written[(size_t)g];
    }
    for (long long g = 0; g < nBlocks; ++g) CHECK(written[(size_t)g] == 1, "partial %lld written %d times", g, written[(size_t)g]);
    std::vector<double> powers;
    for (long long r = 0; r < nJobs; ++r) {
        const long long b0 = blockStart[(size_t)r], b1 = blockStart[(size_t)r + 1];
        double Q = 0.0;
        for (long long at = b0; at < b1; at += 64)
            for (int k = 0; k < 64; ++k) {
                const double mine = at + k < b1 ? partials[(size_t)(at + k)] : 0.0;      // (the Lemma: a lane without a partial holds +0)
                Q = Q + mine;
            }
        powers.push_back(sig_row_power(Q, jobs[(size_t)r].len));
    }
    return powers;
}

// One row of L samples, `shift` floats past a 16-byte boundary, in an allocation that ends with the row (tail 0) or holds `tail` poisoned
// floats behind it: -> its power by the model, every check made
static double one_row(const std::vector<float>& values, long long L, int shift, int tail)
{
    float* heap = static_cast<float*>(malloc((size_t)(shift + L + tail) * sizeof(float) + 1));      // (malloc aligns to 16 bytes; + 1: no zero-size request)
    CHECK((reinterpret_cast<uintptr_t>(heap) & 15) == 0, "malloc");
    for (int i = 0; i < shift; ++i) heap[i] = NAN;
    float* row = heap + shift;
    if (L) memcpy(row, values.data(), (size_t)L * sizeof(float));
    for (int i = 0; i < tail; ++i) row[L + i] = i % 3 == 0 ? NAN : i % 3 == 1 ? INFINITY : 1e30f;
    std::vector<int> reads((size_t)L, 0);
    const std::vector<double> got = model({Job{row, L, &reads}});
    for (long long s = 0; s < L; ++s) CHECK(reads[(size_t)s] == 1, "sample %lld of %lld (shift %d) is read %d times", s, L, shift, reads[(size_t)s]);
    const double want = sig_power_host(row, L);
    CHECK(bits(got[0]) == bits(want), "L %lld shift %d: the model gives %.17g, the statement %.17g", L, shift, got[0], want);
    CHECK(bits(signal_power(row, 1, L)) == bits(want), "signal_power");
    free(heap);
    return got[0];
}

int main()
{
    std::vector<float> values(40000);
    for (float& v : values) v = value();
    std::vector<long long> lens;
    for (long long L = 0; L <= 4200; ++L) lens.push_back(L);
    for (long long k = 3; k <= 9; ++k) for (long long d = -1; d <= 1; ++d) lens.push_back(2048 * k + d);
    for (long long L : lens) {
        const float* x = values.data() + (L * 7) % 1000;
        const std::vector<float> row(x, x + L);
        const double want = restated(row.data(), L);
        CHECK(want >= 0.0 && (L == 0 ? bits(want) == 0 : true), "P of %lld samples", L);
        for (int shift = 0; shift < 4; ++shift) {
            const double tight = one_row(row, L, shift, 0);
            CHECK(bits(tight) == bits(want), "L %lld shift %d: %.17g, the definition written out gives %.17g", L, shift, tight, want);
            if (L % 64 < 10 || L > 4200) CHECK(bits(one_row(row, L, shift, 77)) == bits(want), "L %lld shift %d: poison past the row changed the power", L, shift);
        }
    }
    // ---- the definition on the plainest cases ----
    {
        const std::vector<float> ones(5000, 1.0f), halves(2048, -0.5f), nothing;
        CHECK(sig_power_host(ones.data(), 5000) == 1.0 && sig_power_host(halves.data(), 2048) == 0.25 && sig_power_host(halves.data(), 1) == 0.25, "constants");
        CHECK(bits(sig_power_host(nothing.data(), 0)) == 0 && bits(sig_row_power(5.0, 0)) == 0, "no samples");
        const std::vector<float> top(4096, 65536.0f);
        CHECK(sig_power_host(top.data(), 4096) == 4294967296.0, "the bound: 2^32");
        const std::vector<float> zeros(3000, -0.0f);
        CHECK(bits(sig_power_host(zeros.data(), 3000)) == 0, "-0 squares to +0");
        CHECK(sig_blocks(0) == 0 && sig_blocks(1) == 1 && sig_blocks(2048) == 1 && sig_blocks(2049) == 2 && sig_blocks(1ll << 44) == 1ll << 33, "blocks");
        // sums that are exact in binary64 come out exact, whatever the shape
        std::vector<float> mixed(2048, 1.0f);
        mixed[0] = 65536.0f;
        CHECK(sig_power_host(mixed.data(), 2048) == (4294967296.0 + 2047.0) / 2048.0, "exact sums");
    }
    // ---- many rows in one walk: empty rows between, a row of several blocks, shared slots of the table ----
    {
        const long long lens2[] = {0, 5, 0, 0, 2048, 2049, 0, 3 * 2048 + 5, 1, 0, 70 * 2048 + 3};
        std::vector<std::vector<float>> rows;
        std::vector<std::vector<int>> reads;
        for (long long L : lens2) { rows.emplace_back((size_t)L); for (float& v : rows.back()) v = value(); reads.emplace_back((size_t)L, 0); }
        std::vector<Job> jobs;
        for (size_t i = 0; i < rows.size(); ++i) jobs.push_back(Job{rows[i].data(), (long long)rows[i].size(), &reads[i]});
        const std::vector<double> got = model(jobs);
        for (size_t i = 0; i < rows.size(); ++i) {
            CHECK(bits(got[i]) == bits(restated(rows[i].data(), (long long)rows[i].size())), "row %zu of the walk", i);
            for (int n : reads[i]) CHECK(n == 1, "row %zu: a sample read %d times", i, n);
        }
    }
    // ---- int16 rows: the pool's definition; the statement of the mix on float32 rows ----
    {
        std::vector<int16_t> pcm(3000);
        for (auto& s : pcm) s = (int16_t)((int)(rng() % 65536u) - 32768);
        CHECK(bits(signal_power(pcm.data(), 0, 3000)) == bits(mix_power(mix_square_sum(pcm.data(), 3000), 3000)) && bits(signal_power(pcm.data(), 0, 0)) == 0, "int16");
        const std::vector<float> x(values.begin(), values.begin() + 700);
        const MixSource self{x.data(), 700, 1, 0.0};
        const MixTermHost term{0, -3, 0, 0.5f};
        std::vector<float> y(700);
        CHECK(mix_host(x.data(), 700, 2.0f, &self, &term, 1, 1, y.data()) == 700, "length");
        for (long long m = 0; m < 700; ++m) {
            const float want = conv_finish(conv_step(2.0f * x[(size_t)m], m + 3 < 700 ? x[(size_t)(m + 3)] : 0.0f, 0.5f));
            uint32_t a, b;
            memcpy(&a, &y[(size_t)m], 4); memcpy(&b, &want, 4);
            CHECK(a == b, "output %lld of a float32 row", m);
        }
    }
    printf("ok %lld\n", checks);
    return 0;
}
