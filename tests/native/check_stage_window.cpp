// check_stage_window.cpp -- a host model of the signal stages that keep a window (csrc/klatt_stage_window.h) in a program of its own, built
// by tests/test_stage_window_host.py with AddressSanitizer + UBSan.  Each model drives the headers' bookkeeping (klatt_stage.h's stage_row_plan,
// stage_frames_emitted, stage_conv_block_last / _skipped, stage_read_lane, stage_sample, stage_history_from_chunk, stage_row_advance) and
// the shared statements (conv_step / conv_finish and the block arithmetic; the spec_* functions) chunk by chunk, as the kernels do, and must
// give, bit for bit, what convolve_host / spectrogram_host give on the concatenation of the chunks.  Every chunk lives in an allocation of
// exactly its size, so a read outside it is an error the sanitizer reports.  Prints "ok <checks>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../nvspeechplayer_amd/csrc/klatt_stage_window.h"

using namespace klatt;

static long long g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static unsigned long long g_rng = 0x9E3779B97F4A7C15ull;
static unsigned long long rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return g_rng;
}

// A chunk: int16 or float32 samples in an allocation of exactly its size, and the same as the statements' float32 input
struct Chunk {
    bool f32 = false, ended = false;
    std::vector<int16_t> s;
    std::vector<float> x;
    long long len() const { return (long long)(f32 ? x.size() : s.size()); }
};
static Chunk make_chunk(long long c, bool ended, std::vector<float>& whole)
{
    Chunk k;
    k.f32 = rnd() & 1; k.ended = ended;
    for (long long i = 0; i < c; ++i) {
        if (k.f32) { k.x.push_back((float)((double)(long long)(rnd() % 2000001) / 1000000.0 - 1.0) * 1.5f); whole.push_back(k.x.back()); }
        else { k.s.push_back((int16_t)(int)(rnd() % 65536 - 32768)); whole.push_back(tile_x((int)k.s.back())); }
    }
    return k;
}

static bool same_bits(const void* a, const void* b, size_t bytes) { return bytes == 0 || memcmp(a, b, bytes) == 0; }

struct RowModel {
    long long N = 0, M = 0;
    std::vector<float> hist;
};

// The next history: the last H of [history | chunk], zeros behind an end
template <typename In>
static void next_history(RowModel& r, const In* chunk, long long c, bool ended)
{
    const int H = (int)r.hist.size();
    std::vector<float> next((size_t)H, 0.0f);
    for (int j = 0; j < H && !ended; ++j) {
        long long at;
        next[(size_t)j] = stage_history_from_chunk(j, H, c, at) ? tile_x(chunk[at]) : r.hist[(size_t)at];
    }
    r.hist = next;
}

// ---- the convolution: the kernel's tiles and tap blocks ------------------------------------------------------------------------------------
template <typename In>
static void conv_push(const StageGeometry& g, const float* h, int K, RowModel& r, const In* chunk, long long c, bool ended, std::vector<float>& out)
{
    long long n;
    const int H = stage_conv_history(K);
    CHECK(stage_keeps_history(g.kind) && stage_row_plan(g, H, r.N, r.M, c, ended, n) && n == c + (ended && g.tail ? K - 1 : 0));
    CHECK((int)r.hist.size() == H);
    std::vector<float> xr, acc;
    for (long long t0 = 0; t0 < n; t0 += kConvolveTile) {
        const int live = (int)std::min<long long>(kConvolveTile, n - t0);
        acc.assign((size_t)live, 0.0f);
        for (int kb = 0; kb < K; kb += kConvolveBlock) {
            if (stage_conv_block_last(r.N, t0, live, kb)) break;
            const int taps = conv_block_taps(K, kb), padded = conv_block_padded(taps);
            if (stage_conv_block_skipped(r.N, r.N + c, t0, live, kb, taps)) continue;
            xr.assign((size_t)(kConvolveTile + padded), -1.0f);
            stage_read_lane<-1>(xr.data(), r.hist.data(), chunk, r.N, H, c, conv_read_first(r.N + t0, kb), kConvolveTile + padded, 0, 1);
            for (int o = 0; o < live; ++o)
                for (int q = 0; q < padded; ++q) {
                    const int p = kConvolveTile - o + q;
                    const long long at = conv_staged_sample(r.N + t0, kb, p);
                    CHECK(at == r.N + t0 + o - kb - q);
                    if (q < taps) {
                        // the lemma: a sample of the stream so far is in the history or in the chunk; one past it is read by an ended row alone
                        long long where;
                        CHECK(stage_where(at, r.N, H, c, where) != 0 || at < 0 || at >= r.N + c);
                        CHECK(at < r.N + c || ended);
                    }
                    acc[(size_t)o] = conv_step(acc[(size_t)o], xr[(size_t)p], q < taps ? h[kb + q] : 0.0f);
                }
        }
        for (int o = 0; o < live; ++o) out.push_back(conv_finish(acc[(size_t)o]));
    }
    next_history(r, chunk, c, ended);
    stage_row_advance(r.N, r.M, c, ended, n);
}

static void conv_stream(const StageGeometry& g, const std::vector<float>& h, RowModel& r, const std::vector<long long>& lens)
{
    const int K = (int)h.size();
    std::vector<float> whole, got;
    for (size_t i = 0; i < lens.size(); ++i) {
        const Chunk k = make_chunk(lens[i], i + 1 == lens.size(), whole);
        if (k.f32) conv_push(g, h.data(), K, r, k.x.data(), k.len(), k.ended, got); else conv_push(g, h.data(), K, r, k.s.data(), k.len(), k.ended, got);
        if (!k.ended) CHECK((long long)got.size() == r.N && r.M == r.N);
    }
    CHECK(r.N == 0 && r.M == 0);
    const long long L = (long long)whole.size();
    std::vector<float> want((size_t)conv_length(L, K, g.tail) + 1);
    const long long Lout = convolve_host(whole.data(), L, h.data(), K, g.tail, 1, want.data());
    CHECK(Lout == (long long)got.size());
    CHECK(same_bits(got.data(), want.data(), (size_t)Lout * sizeof(float)));
    for (float v : r.hist) CHECK(v == 0.0f);
}

static void check_convolve(int K, int tail)
{
    std::vector<float> h((size_t)K);
    for (int k = 0; k < K; ++k) h[(size_t)k] = k % 7 == 3 ? 0.0f : (float)((double)(long long)(rnd() % 2001) / 1000.0 - 1.0);      // (zero taps among them)
    StageGeometry g;
    g.kind = kStageConvolve; g.tail = tail;
    RowModel r;
    r.hist.assign((size_t)stage_conv_history(K), 0.0f);
    const long long k = K, a = k >= 2 ? k - 2 : 0;
    // the edge lengths in both orders, a stream that stays below K - 1 until it ends, an end with an empty last chunk -- on ONE row, which
    // is thereby reused after every end
    conv_stream(g, h, r, {0, 1, a, k - 1, k, 2 * k, 37});
    conv_stream(g, h, r, {2 * k, k, k - 1, a, 1, 0, 3});
    conv_stream(g, h, r, {k > 3 ? (k - 3) / 2 : 0, 0, k > 3 ? (k - 3) / 2 : 0});
    conv_stream(g, h, r, {k, 5, 0});
    conv_stream(g, h, r, {0});
    conv_stream(g, h, r, {3 * k + 1});
    const long long pool[6] = {0, 1, a, k - 1, k, 2 * k};
    for (int s = 0; s < 4; ++s) {
        std::vector<long long> lens;
        for (int i = 0; i < 6; ++i) lens.push_back(pool[rnd() % 6]);
        conv_stream(g, h, r, lens);
    }
}

// ---- the spectrogram: a frame from the virtual row through the shared functions ---------------------------------------------------------------
template <typename In>
static void spec_push(const SpecPlan& P, const StageGeometry& g, RowModel& r, const In* chunk, long long c, bool ended, std::vector<double>& out)
{
    long long n;
    CHECK(stage_keeps_history(g.kind) && stage_row_plan(g, stage_frame_history(g.frames), r.N, r.M, c, ended, n) && n >= 0);
    CHECK(n == stage_frames_emitted(g.frames, r.N + c, ended) - r.M);
    const int H = stage_frame_history(g.frames), M = P.M, K = M + 1, logM = P.logN - 1;
    CHECK(H == P.nFft - 1 && (int)r.hist.size() == H);
    std::vector<SpecCx> z((size_t)M);
    std::vector<float> v((size_t)K);
    for (long long e = 0; e < n; ++e) {
        const long long centre = stage_frame_centre(g.frames, r.M + e), t0 = centre - g.frames.before;
        CHECK(t0 >= r.N - H);                                  // the lemma
        CHECK(centre + g.frames.after < r.N + c || ended);     // a frame past the stream's samples is an ended row's alone
        for (int m = 0; m < M; ++m) {
            const long long ta = t0 + 2 * m, tb = ta + 1;
            long long where;
            CHECK(stage_where(ta, r.N, H, c, where) != 0 || ta < 0 || ta >= r.N + c);
            z[spec_reverse((uint32_t)m, logM)] = SpecCx{spec_windowed(stage_sample(r.hist.data(), chunk, ta, r.N, H, c), P.window[(size_t)(2 * m)]),
                                                       spec_windowed(stage_sample(r.hist.data(), chunk, tb, r.N, H, c), P.window[(size_t)(2 * m + 1)])};
        }
        for (int p = 0; p < logM; ++p)
            for (uint32_t b = 0; b < (uint32_t)M / 2; ++b) {
                uint32_t i0, i1, t;
                spec_butterfly_at(b, p, P.logN, i0, i1, t);
                spec_butterfly(z[i0], z[i1], P.tw[t]);
            }
        for (int k = 0; k < K; ++k)
            v[(size_t)k] = spec_value(spec_unpack(z[(size_t)(k & (M - 1))], z[(size_t)((M - k) & (M - 1))], P.tw[(size_t)k]), P.power);
        for (int b = 0; b < P.nOut; ++b) {
            const float value = P.hasBank ? spec_band(P.weights.data() + (size_t)b * K, v.data(), P.range[(size_t)b * 2], P.range[(size_t)b * 2 + 1]) : v[(size_t)b];
            out.push_back(spec_scale(value, P.logScale, P.floor));
        }
    }
    next_history(r, chunk, c, ended);
    stage_row_advance(r.N, r.M, c, ended, n);
}

static void spec_stream(const SpecPlan& P, const StageGeometry& g, RowModel& r, const std::vector<long long>& lens)
{
    std::vector<float> whole;
    std::vector<double> got;
    for (size_t i = 0; i < lens.size(); ++i) {
        const Chunk k = make_chunk(lens[i], i + 1 == lens.size(), whole);
        if (k.f32) spec_push(P, g, r, k.x.data(), k.len(), k.ended, got); else spec_push(P, g, r, k.s.data(), k.len(), k.ended, got);
        if (!k.ended) CHECK((long long)got.size() == stage_frames_emitted(g.frames, r.N, false) * P.nOut && r.M * P.nOut == (long long)got.size());
    }
    CHECK(r.N == 0 && r.M == 0);
    const long long L = (long long)whole.size(), steps = L > g.frames.phase ? (L - g.frames.phase + g.frames.hop - 1) / g.frames.hop : 0;
    std::vector<double> want((size_t)(steps * P.nOut) + 1);
    const long long n = spectrogram_host(whole.data(), L, P, g.frames.hop, g.frames.phase, want.data());
    CHECK(n == (long long)got.size());
    CHECK(same_bits(got.data(), want.data(), (size_t)n * sizeof(double)));
    for (float v : r.hist) CHECK(v == 0.0f);
}

static void check_spectrogram(int nFft, long long hop, long long phase, int bands, int power, double logScale)
{
    SpecPlan P;
    std::string why;
    std::vector<double> bank;
    if (bands) {      // triangles over the bins, one band without weights
        bank.assign((size_t)bands * (nFft / 2 + 1), 0.0);
        for (int b = 0; b + 1 < bands; ++b)
            for (int k = 0; k <= nFft / 2; ++k) {
                const double centre = (b + 1.0) * (nFft / 2) / bands, d = 1.0 - (k > centre ? k - centre : centre - k) * bands / (double)nFft;
                if (d > 0.0) bank[(size_t)b * (nFft / 2 + 1) + k] = d;
            }
    }
    CHECK(spec_plan(P, nFft, nullptr, bands ? bank.data() : nullptr, bands, power, logScale, 1e-10, why));
    StageGeometry g;
    g.kind = kStageSpectrogram; g.frames = stage_spec_frames(nFft, hop, phase);
    // the counts against brute force
    for (long long N = 0; N <= 3 * nFft + hop; ++N) {
        long long open = 0, ended = 0;
        for (long long j = 0; j <= N; ++j) {
            if (phase + j * hop + nFft / 2 - 1 <= N - 1) ++open;
            if (phase + j * hop < N) ++ended;
        }
        CHECK(stage_frames_emitted(g.frames, N, false) == open && stage_frames_emitted(g.frames, N, true) == ended);
    }
    RowModel r;
    r.hist.assign((size_t)stage_frame_history(g.frames), 0.0f);
    const long long n = nFft, pool[8] = {0, 1, hop - 1, hop, n / 2 - 1, n / 2, n - 1, n};
    spec_stream(P, g, r, {0, 1, hop - 1, hop, n / 2 - 1, n / 2, n - 1, n, 37});
    spec_stream(P, g, r, {n, n - 1, n / 2, n / 2 - 1, hop, hop - 1, 1, 0, 3});
    spec_stream(P, g, r, {1, 0, n / 2 - 5, 0});      // below one frame until it ends
    spec_stream(P, g, r, {n, 5, 0});                 // an end with an empty last chunk
    spec_stream(P, g, r, {0});
    spec_stream(P, g, r, {3 * n + 1});
    for (int s = 0; s < 4; ++s) {
        std::vector<long long> lens;
        for (int i = 0; i < 7; ++i) lens.push_back(pool[rnd() % 8]);
        spec_stream(P, g, r, lens);
    }
}

int main()
{
    for (int tail = 0; tail < 2; ++tail)
        for (int K : {1, 2, 5, 1025}) check_convolve(K, tail);
    check_spectrogram(64, 16, 0, 0, 2, 0.0);
    check_spectrogram(64, 80, 5, 6, 1, 0.0);      // a hop above nFft skips samples
    check_spectrogram(64, 7, 64, 0, 2, 10.0);
    check_spectrogram(128, 1, 3, 5, 2, 0.0);
    check_spectrogram(256, 300, 259, 0, 1, 0.0);
    // the refusals of the plan: a negative chunk, a row that would pass 2^44 samples
    StageGeometry g;
    g.kind = kStageConvolve;
    long long n;
    CHECK(stage_row_plan(g, 2, kResampleMaxLength - 5, 0, 5, false, n) && !stage_row_plan(g, 2, kResampleMaxLength - 5, 0, 6, false, n) &&
          !stage_row_plan(g, 2, 0, 0, -1, false, n));
    printf("ok %lld\n", g_checks);
    return 0;
}
