// check_stage.cpp -- a host model of the signal stages (csrc/klatt_stage.h) in a program of its own, built by tests/test_stage_host.py with
// AddressSanitizer + UBSan.  Each model drives the header's bookkeeping (stage_row_plan, stage_row_advance, stage_sample, stage_where,
// stage_history_from_chunk) and the shared per-sample statements chunk by chunk, as the kernels do, and must give, bit for bit, what
// resample_host / filter_host / code_host give on the concatenation of the chunks.  Every chunk lives in an allocation of exactly its
// size, so a read outside it is an error the sanitizer reports.  Prints "ok <checks>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../nvspeechplayer_amd/csrc/klatt_stage.h"

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

// ---- the resampler ------------------------------------------------------------------------------------------------------------------------
struct ResRowModel {
    long long N = 0, M = 0;
    std::vector<float> hist;
};
template <typename In>
static void res_push(const ResPlan& P, const StageGeometry& g, ResRowModel& r, const In* chunk, long long c, bool ended, std::vector<float>& out)
{
    long long n;
    const int H = stage_history(g.Z);
    CHECK(stage_keeps_history(g.kind) && stage_row_plan(g, H, r.N, r.M, c, ended, n) && n >= 0);
    CHECK((int)r.hist.size() == H);
    if (g.Z == 0) {      // equal rates: the samples themselves
        CHECK(n == c);
        for (long long e = 0; e < n; ++e) out.push_back(tile_x(chunk[e]));
        stage_row_advance(r.N, r.M, c, ended, n);
        return;
    }
    std::vector<float> x((size_t)P.taps);
    for (long long e = 0; e < n; ++e) {
        long long n0; int p;
        res_locate(r.M + e, P.up, P.down, n0, p);
        for (int k = 0; k < P.taps; ++k) {
            const long long at = n0 + k - P.Z + 1;
            long long where;
            const int part = stage_where(at, r.N, H, c, where);
            // the lemma: a sample of the stream so far is in the history or in the chunk; one past it is read by an ended row alone
            CHECK(part != 0 || at < 0 || at >= r.N + c);
            CHECK(at < r.N + c || ended);
            x[(size_t)k] = stage_sample(r.hist.data(), chunk, at, r.N, H, c);
        }
        out.push_back(res_taps(x.data(), P.table.data() + (size_t)p * P.taps, P.taps, 1));
    }
    std::vector<float> next((size_t)H, 0.0f);
    for (int j = 0; j < H && !ended; ++j) {
        long long at;
        next[(size_t)j] = stage_history_from_chunk(j, H, c, at) ? tile_x(chunk[at]) : r.hist[(size_t)at];
    }
    r.hist = next;
    stage_row_advance(r.N, r.M, c, ended, n);
}

static void res_stream(const ResPlan& P, const StageGeometry& g, ResRowModel& r, const std::vector<long long>& lens)
{
    std::vector<float> whole, got;
    for (size_t i = 0; i < lens.size(); ++i) {
        const Chunk k = make_chunk(lens[i], i + 1 == lens.size(), whole);
        const long long before = (long long)got.size();
        if (k.f32) res_push(P, g, r, k.x.data(), k.len(), k.ended, got); else res_push(P, g, r, k.s.data(), k.len(), k.ended, got);
        if (!k.ended) CHECK((long long)got.size() == stage_res_emitted(r.N, g.Z, g.up, g.down, false) && r.M == (long long)got.size());
        CHECK((long long)got.size() >= before);
    }
    CHECK(r.N == 0 && r.M == 0);
    std::vector<float> want((size_t)res_length((long long)whole.size(), P.up, P.down) + 1);
    const long long L = resample_host(whole.data(), (long long)whole.size(), P, 1, want.data());
    CHECK(L == (long long)got.size());
    CHECK(same_bits(got.data(), want.data(), (size_t)L * sizeof(float)));
    for (float h : r.hist) CHECK(h == 0.0f);
}

static void check_resample(int srcRate, int dstRate)
{
    ResPlan P;
    std::string why;
    CHECK(res_plan(P, srcRate, dstRate, 6, 0.99, 0, 0.0, why));
    StageGeometry g;
    g.kind = kStageResample; g.up = P.up; g.down = P.down; g.Z = P.identity ? 0 : P.Z;
    const long long Z = P.Z;
    // the counts against brute force: the m with floor(m down / up) + Z <= N - 1 (open), the statement's length (ended)
    for (long long N = 0; N <= 4 * Z + 3; ++N) {
        long long brute = 0;
        for (long long m = 0; m < (4 * Z + 8) * (long long)P.up; ++m) if (m * P.down / P.up + g.Z <= N - 1) ++brute;
        CHECK(stage_res_emitted(N, g.Z, g.up, g.down, false) == brute);
        CHECK(stage_res_emitted(N, g.Z, g.up, g.down, true) == res_length(N, P.up, P.down));
    }
    ResRowModel r;
    r.hist.assign((size_t)stage_history(g.Z), 0.0f);
    // the edge lengths in both orders, a stream whose total stays below Z until it ends, an end with an empty last chunk -- on ONE row,
    // which is thereby reused after every end
    res_stream(P, g, r, {0, 1, Z - 1, Z, 2 * Z - 2, 2 * Z - 1, 2 * Z, 37});
    res_stream(P, g, r, {2 * Z, 2 * Z - 1, 2 * Z - 2, Z, Z - 1, 1, 0});
    res_stream(P, g, r, {1, 0, Z > 3 ? Z - 3 : 0, 0});
    res_stream(P, g, r, {Z, 5, 0});
    res_stream(P, g, r, {0});
    res_stream(P, g, r, {3 * Z + 1});
    const long long pool[8] = {0, 1, Z - 1, Z, 2 * Z - 2, 2 * Z - 1, 2 * Z, 137};
    for (int t = 0; t < 6; ++t) {
        std::vector<long long> lens;
        for (int i = 0, n = 3 + (int)(rnd() % 8); i < n; ++i) lens.push_back(pool[rnd() % 8]);
        res_stream(P, g, r, lens);
    }
}

// ---- the filter: the kernel's steps, which run on past a row's own count without committing -----------------------------------------------
struct FilterRowModel { float s1[kFilterMaxSections] = {}, s2[kFilterMaxSections] = {}; long long N = 0, M = 0; };
template <typename In>
static void filter_push(const StageGeometry& g, const FilterSection* sec, int K, FilterRowModel& r, const In* chunk, long long c, bool ended, long long groupMost,
                        std::vector<float>& out)
{
    long long n;
    CHECK(!stage_keeps_history(g.kind) && stage_row_plan(g, 0, r.N, r.M, c, ended, n) && n == c + (ended ? g.tail : 0));
    const int bucket = filter_bucket(K);
    FilterSection cs[kFilterMaxSections];
    float s1[kFilterMaxSections], s2[kFilterMaxSections];
    for (int j = 0; j < bucket; ++j) { cs[j] = j < K ? sec[j] : kFilterIdentity; s1[j] = j < K ? r.s1[j] : 0.0f; s2[j] = j < K ? r.s2[j] : 0.0f; }
    const long long steps = (std::max(groupMost, n) + kFilterTile - 1) / kFilterTile * kFilterTile;      // the group's longest row decides
    for (long long t = 0; t < steps; ++t) {
        const bool on = t < n;
        float x = tile_x(tile_inside(t, c) ? chunk[t] : (In)0);
        for (int j = 0; j < bucket; ++j) {
            float a = s1[j], b = s2[j];
            x = filter_section(cs[j], x, a, b);
            if (on) { s1[j] = a; s2[j] = b; }
        }
        if (on) out.push_back(filter_finish(x));
    }
    for (int j = 0; j < K; ++j) { r.s1[j] = ended ? 0.0f : s1[j]; r.s2[j] = ended ? 0.0f : s2[j]; }
    stage_row_advance(r.N, r.M, c, ended, n);
}

static void check_filter(int K, long long tail)
{
    std::vector<FilterSection> sec;
    for (int j = 0; j < K; ++j) {
        const float rad = 0.3f + 0.6f * (float)(rnd() % 1000) / 1000.0f, th = 0.2f + 2.7f * (float)(rnd() % 1000) / 1000.0f;
        sec.push_back(FilterSection{0.4f, 0.1f * (float)(int)(rnd() % 7 - 3), 0.2f, 2.0f * rad * cosf(th), -rad * rad});
    }
    StageGeometry g;
    g.kind = kStageFilter; g.tail = tail;
    FilterRowModel r;
    const long long T = kFilterTile, pool[7] = {0, 1, T - 1, T, T + 1, 2 * T + 3, 5};
    for (int stream = 0; stream < 4; ++stream) {      // one row, reused after every end
        std::vector<float> whole, got;
        const int pushes = stream == 3 ? 1 : 4;
        for (int i = 0; i < pushes; ++i) {
            const bool last = i + 1 == pushes;
            const Chunk k = make_chunk(stream == 2 && last ? 0 : pool[rnd() % 7], last, whole);
            const long long most = pool[rnd() % 7] + (rnd() & 1 ? tail : 0);      // a neighbour's count: longer, shorter or equal
            if (k.f32) filter_push(g, sec.data(), K, r, k.x.data(), k.len(), k.ended, most, got); else filter_push(g, sec.data(), K, r, k.s.data(), k.len(), k.ended, most, got);
        }
        std::vector<float> want(whole.size() + (size_t)tail + 1);
        const long long L = filter_host(whole.data(), (long long)whole.size(), sec.data(), K, tail, 1, want.data());
        CHECK(L == (long long)got.size());
        CHECK(same_bits(got.data(), want.data(), (size_t)L * sizeof(float)));
        for (int j = 0; j < K; ++j) CHECK(r.s1[j] == 0.0f && r.s2[j] == 0.0f);
    }
}

// ---- the codecs ------------------------------------------------------------------------------------------------------------------------------
struct CodeRowModel { int val = 0, idx = 0; long long N = 0, M = 0; };
template <typename In>
static void code_push(const StageGeometry& g, int codec, CodeRowModel& r, const In* chunk, long long c, bool ended, long long groupMost, std::vector<uint8_t>& codes,
                      std::vector<int16_t>& decoded)
{
    long long n;
    CHECK(!stage_keeps_history(g.kind) && stage_row_plan(g, 0, r.N, r.M, c, ended, n) && n == c);
    int val = r.val, idx = r.idx;
    const long long steps = codec == kCodecAdpcm ? (std::max(groupMost, n) + kFilterTile - 1) / kFilterTile * kFilterTile : n;
    for (long long t = 0; t < steps; ++t) {
        const bool on = t < n;
        const int s = codec_sample(tile_inside(t, c) ? chunk[t] : (In)0);
        int code, d;
        if (codec == kCodecUlaw) { code = ulaw_encode(s); d = ulaw_decode(code); }
        else if (codec == kCodecAlaw) { code = alaw_encode(s); d = alaw_decode(code); }
        else {
            int v = val, i = idx;
            code = adpcm_encode(s, kAdpcmTable.step[i], v, i);
            if (on) { val = v; idx = i; }
            d = v;
        }
        if (on) { codes.push_back((uint8_t)code); decoded.push_back(codec_value<false>(d)); }
    }
    r.val = ended ? 0 : val; r.idx = ended ? 0 : idx;
    stage_row_advance(r.N, r.M, c, ended, n);
}

static void check_code(int codec)
{
    StageGeometry g;
    g.kind = kStageCode;
    CodeRowModel r;
    const long long T = kFilterTile, pool[7] = {0, 1, T - 1, T, T + 1, 2 * T + 3, 300};
    for (int stream = 0; stream < 4; ++stream) {
        std::vector<float> whole;
        std::vector<uint8_t> codes;
        std::vector<int16_t> decoded;
        const int pushes = stream == 3 ? 1 : 5;
        for (int i = 0; i < pushes; ++i) {
            const bool last = i + 1 == pushes;
            const Chunk k = make_chunk(stream == 2 && last ? 0 : pool[rnd() % 7], last, whole);
            const long long most = pool[rnd() % 7];
            if (k.f32) code_push(g, codec, r, k.x.data(), k.len(), k.ended, most, codes, decoded); else code_push(g, codec, r, k.s.data(), k.len(), k.ended, most, codes, decoded);
        }
        std::vector<uint8_t> wantCodes(whole.size() + 1);
        std::vector<int16_t> wantDecoded(whole.size() + 1);
        code_host(whole.data(), (long long)whole.size(), codec, 0, wantDecoded.data(), wantCodes.data(), nullptr);
        CHECK(codes.size() == whole.size() && decoded.size() == whole.size());
        CHECK(same_bits(codes.data(), wantCodes.data(), codes.size()));
        CHECK(same_bits(decoded.data(), wantDecoded.data(), decoded.size() * sizeof(int16_t)));
        CHECK(r.val == 0 && r.idx == 0);
    }
}

int main()
{
    const int rates[7][2] = {{22050, 16000}, {22050, 48000}, {22050, 44100}, {22050, 8000}, {22050, 11025}, {48000, 4000}, {16000, 16000}};
    for (const auto& r : rates) check_resample(r[0], r[1]);
    for (int K : {1, 2, 3, 5, 16}) for (long long tail : {0ll, 1ll, (long long)kFilterTile + 3}) check_filter(K, tail);
    for (int codec = 0; codec < kCodecCount; ++codec) check_code(codec);
    // a row may not pass 2^44 samples, and a negative length is no length
    StageGeometry g;
    long long n;
    CHECK(stage_row_plan(g, 0, kResampleMaxLength - 5, 0, 5, false, n) && !stage_row_plan(g, 0, kResampleMaxLength - 5, 0, 6, false, n) && !stage_row_plan(g, 0, 0, 0, -1, false, n));
    printf("ok %lld checks\n", g_checks);
    return 0;
}
