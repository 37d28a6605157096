// check_mix.cpp -- the host statement of the mix export (nvspeechplayer_amd/csrc/klatt_mix.h: mix_bank_plan, mix_check_row, mix_check_term,
// mix_power, mix_gain, mix_host) against loops written from the definition, and the kernel's tile / wrap / skip arithmetic against brute
// force: a model of klatt_mix written from the index functions alone visits, for every output, exactly the terms that read a sample of
// their source, in ascending order and at the element the definition names, stays inside the sources, and arrives at the statement's bits.
// Built with AddressSanitizer + UBSan by tests/test_mix_host.py; prints "ok <checks>" or the first failure.
#include "../../nvspeechplayer_amd/csrc/klatt_mix.h"
#include "../../nvspeechplayer_amd/csrc/klatt_export.h"

#include <stdlib.h>
#include <string.h>

#include <utility>

using namespace klatt;

static long long checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static uint32_t rng_state = 2463534242u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static std::vector<int16_t> signal(long long L, int kind)
{
    std::vector<int16_t> pcm((size_t)L);
    for (auto& s : pcm) s = kind == 0 ? (int16_t)((int)(rng() % 65535u) - 32767) : kind == 1 ? (int16_t)(rng() & 1u ? 32767 : -32768) : (int16_t)0;
    return pcm;
}

static std::vector<float> clip(long long N)
{
    std::vector<float> c((size_t)N);
    for (auto& v : c) v = (float)((int)(rng() % 2001u) - 1000) / 500.0f;
    return c;
}

struct Term { int source; long long offset; int loop; float gain; };

// The kernel, from its index functions: tiles of a row of `width` elements (the padded form's rowStride, or L), every lane of a tile.
// The sources are exact-size heap arrays read through plain pointers: the sanitizer guards both ends.
// shift: the row's samples lie `shift` elements into an allocation of exactly shift + L, as an utterance lies in the pool: the kernel's
// 8-byte speech load must fall back to elements where the address is not aligned, and never read past the row.
static void model(const std::vector<int16_t>& row, float speechGain, const std::vector<MixSource>& sources, const std::vector<Term>& terms, long long width, int shift = 0)
{
    const long long L = (long long)row.size();
    std::vector<int16_t> pool((size_t)(L + shift), (int16_t)12345);
    if (L) memcpy(pool.data() + shift, row.data(), (size_t)L * sizeof(int16_t));
    const int16_t* pcm = pool.data() + shift;
    std::vector<MixTermHost> host;
    for (const Term& t : terms) host.push_back(MixTermHost{t.source, t.offset, t.loop, t.gain});
    std::vector<float> want((size_t)L + 1, -7.0f);
    std::vector<int16_t> want16((size_t)L + 1, (int16_t)-7);
    CHECK(mix_host(pcm, L, speechGain, sources.data(), host.data(), (long long)host.size(), 1, want.data()) == L, "length");
    CHECK(mix_host(pcm, L, speechGain, sources.data(), host.data(), (long long)host.size(), 0, want16.data()) == L, "length");
    CHECK(want[(size_t)L] == -7.0f && want16[(size_t)L] == -7, "the statement wrote past its output");
    const int T = kMixTile;
    const long long tilesPerRow = tile_count(width, T);
    CHECK(tilesPerRow == (width + T - 1) / T, "tiles");
    long long covered = 0;
    for (long long g = 0; g < tilesPerRow; ++g) {
        long long r, j;
        tile_row(g + 5 * tilesPerRow, tilesPerRow, r, j);
        CHECK(r == 5 && j == g, "tile %lld is tile %lld of row %lld", g, j, r);
        const long long t0 = j * T;
        const int n = (int)std::min<long long>(T, width - t0);
        const int live = (int)std::max<long long>(0, std::min<long long>(n, L - t0));
        CHECK(n >= 1 && n <= T && live >= 0 && live <= n, "tile %lld: %d elements, %d live", g, n, live);
        CHECK(tile_n(width, L, t0, T) == n && tile_live(n, L, t0) == live, "tile %lld: the kernel takes %d elements, %d live", g, tile_n(width, L, t0, T), tile_live(n, L, t0));
        covered += live;
        std::vector<float> acc((size_t)T, 0.0f);
        std::vector<std::vector<std::pair<int, long long>>> visited((size_t)T);
        if (live > 0) {
            for (int lane = 0; lane < 256; ++lane) {
                const int o0 = 4 * lane;
                const int16_t* p = pcm + t0 + o0;      // (formed as the kernel forms it; read only where the predicate or the bound allows)
                if (mix_speech_whole(p, o0, live)) {
                    CHECK(o0 + 4 <= live && (reinterpret_cast<uintptr_t>(p) & 7) == 0, "lane %d takes four samples at %p", lane, (const void*)p);
                    for (int q = 0; q < 4; ++q) acc[(size_t)(o0 + q)] = speechGain * res_input((int)p[q]);
                } else {
                    for (int q = 0; q < 4; ++q) if (o0 + q < live) acc[(size_t)(o0 + q)] = speechGain * res_input((int)p[q]);
                }
            }
            for (int jt = 0; jt < (int)terms.size(); ++jt) {
                const Term& t = terms[(size_t)jt];
                const MixSource& s = sources[(size_t)t.source];
                const long long N = s.length;
                // brute force: does any live output of the tile read a sample of the source?
                bool any = false;
                for (int o = 0; o < live && !any; ++o) any = t.loop || (t0 + o - t.offset >= 0 && t0 + o - t.offset < N);
                CHECK(mix_term_skipped(t0, live, t.offset, N, t.loop) == !any, "tile %lld, term %d: skipped %d, reads %d", g, jt, (int)mix_term_skipped(t0, live, t.offset, N, t.loop), (int)any);
                if (!any) continue;
                const int lo = t.loop ? 0 : mix_term_first(t0, t.offset), hi = t.loop ? live : mix_term_last(t0, live, t.offset, N);
                CHECK(lo >= 0 && lo < hi && hi <= live, "tile %lld, term %d: covers %d .. %d of %d", g, jt, lo, hi, live);
                const long long base = t.loop ? mix_loop_start(t.offset, t0, N) : t0 - t.offset;
                CHECK(!t.loop || (base >= 0 && base < N), "start %lld of %lld", base, N);
                for (int lane = 0; lane < 256; ++lane) {
                    const int o0 = 4 * lane;
                    const long long i0 = mix_lane_start(base, o0, N, t.loop);
                    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (mix_lane_whole(o0, lo, hi, i0, N, t.loop)) {
                        CHECK(i0 >= 0 && i0 + 4 <= N && !(t.loop && N < T), "lane %d takes four elements from %lld of %lld", lane, i0, N);
                        for (int q = 0; q < 4; ++q) { v[q] = mix_source_value(s.data, s.isFloat, i0 + q); visited[(size_t)(o0 + q)].push_back({jt, i0 + q}); }
                    } else {
                        for (int q = 0; q < 4; ++q) {
                            const int o = o0 + q;
                            if (o < lo || o >= hi) continue;
                            const long long i = t.loop ? mix_loop_index(base, o, N) : base + o;
                            CHECK(i >= 0 && i < N, "lane %d output %d reads element %lld of %lld", lane, q, i, N);
                            v[q] = mix_source_value(s.data, s.isFloat, i);
                            visited[(size_t)o].push_back({jt, i});
                        }
                    }
                    for (int q = 0; q < 4; ++q) acc[(size_t)(o0 + q)] = conv_step(acc[(size_t)(o0 + q)], v[q], t.gain);
                }
            }
        }
        for (int o = 0; o < live; ++o) {
            const long long m = t0 + o;
            std::vector<std::pair<int, long long>> need;      // the definition, written out
            for (int jt = 0; jt < (int)terms.size(); ++jt) {
                const Term& t = terms[(size_t)jt];
                const long long N = sources[(size_t)t.source].length;
                if (t.loop) need.push_back({jt, (t.offset + m) % N});
                else if (m - t.offset >= 0 && m - t.offset < N) need.push_back({jt, m - t.offset});
            }
            CHECK(visited[(size_t)o] == need, "output %lld of %lld: %zu reads, the definition has %zu", m, L, visited[(size_t)o].size(), need.size());
            const float y = conv_finish(acc[(size_t)o]);
            CHECK(bits(y) == bits(want[(size_t)m]), "output %lld of %lld: the model gives %.9g, the statement %.9g", m, L, (double)y, (double)want[(size_t)m]);
            CHECK(!(y == 0.0f) || bits(y) == 0u, "y[%lld] is -0", m);
            CHECK(res_int16(y) == want16[(size_t)m], "int16 of output %lld", m);
        }
    }
    CHECK(covered == L, "the tiles cover %lld of %lld outputs", covered, L);
}

int main()
{
    const int T = kMixTile;
    // ---- powers and gains ----
    {
        const std::vector<int16_t> full = signal(1000, 1);
        unsigned long long S = 0;
        for (int16_t s : full) S += (unsigned long long)((long long)s * s);
        CHECK(mix_square_sum(full.data(), 1000) == S && S > 1000ull * 32767 * 32767 - 1, "S");
        CHECK(mix_square_sum(full.data(), 0) == 0 && mix_power(0, 0) == 0.0 && mix_power(5, 0) == 0.0, "empty");
        CHECK(mix_power(1073676289ull * 4, 4) == 1.0, "a full-scale square wave has power 1");
        std::vector<int16_t> low((size_t)70000, (int16_t)-32768);      // 70000 * 2^30 is above 2^46: 32-bit sums would have wrapped long before
        CHECK(mix_square_sum(low.data(), 70000) == 70000ull << 30, "64-bit sums");
        CHECK(mix_gain(1.0, 1.0, 1.0) == 1.0f && mix_gain(4.0, 1.0, 1.0) == 2.0f && mix_gain(1.0, 4.0, 1.0) == 0.5f && mix_gain(1.0, 1.0, 100.0) == 0.1f, "gains");
        CHECK(bits(mix_gain(0.0, 1.0, 1.0)) == 0u && bits(mix_gain(1.0, 0.0, 1.0)) == 0u && bits(mix_gain(1.0, 1.0, 0.0)) == 0u, "silence gives +0");
        CHECK(mix_gain(1.0, 1e-30, 1.0) == 4294967296.0f && mix_gain(1.0, 1.0 / 18446744073709551616.0, 1.0) == 4294967296.0f, "the clamp");
        CHECK(mix_gain(1.0, 1.0 / 18446744073709551616.0 * 1.0001, 1.0) < 4294967296.0f, "below the clamp");
        const std::vector<float> c = clip(777);
        double acc = 0.0;
        for (float v : c) acc += (double)v * (double)v;
        CHECK(mix_clip_power(c.data(), 777) == acc / 777.0, "clip power");
        CHECK(mix_ratio(10.0) == 10.0 && mix_ratio(0.0) == 1.0 && mix_ratio(-20.0) == 0.01, "ratio");
    }
    // ---- the statement on the plainest cases ----
    {
        const std::vector<int16_t> pcm = signal(300, 0);
        std::vector<float> y(300);
        std::vector<int16_t> q(300);
        mix_host(pcm.data(), 300, 1.0f, nullptr, nullptr, 0, 1, y.data());
        mix_host(pcm.data(), 300, 1.0f, nullptr, nullptr, 0, 0, q.data());
        for (int m = 0; m < 300; ++m) CHECK(bits(y[(size_t)m]) == bits(conv_finish(res_input(pcm[(size_t)m]))) && q[(size_t)m] == pcm[(size_t)m], "no terms, gain 1: the PCM (%d)", m);
        const MixSource self{pcm.data(), 300, 0, 0.0};
        const MixTermHost twice{0, 0, 0, 1.0f};
        mix_host(pcm.data(), 300, 1.0f, &self, &twice, 1, 1, y.data());
        for (int m = 0; m < 300; ++m) CHECK(y[(size_t)m] == 2.0f * res_input(pcm[(size_t)m]) + 0.0f, "the row's own utterance at gain 1 doubles it (%d)", m);
    }
    // ---- the kernel's arithmetic ----
    const long long lens[] = {3, T - 1, T, T + 1, 2 * T + 1, 5000};
    const long long clipLens[] = {1, 3, T - 1, T, T + 1, 7001};
    std::vector<std::vector<float>> clips;
    for (long long N : clipLens) clips.push_back(clip(N));
    const std::vector<int16_t> other = signal(2 * T + 77, 0), nothing = signal(0, 0);
    for (long long L : lens) {
        const std::vector<int16_t> pcm = signal(L, L == T ? 2 : 0);
        std::vector<MixSource> sources;
        for (const auto& c : clips) sources.push_back(MixSource{c.data(), (long long)c.size(), 1, 0.0});
        const int own = (int)sources.size();
        sources.push_back(MixSource{pcm.data(), L, 0, 0.0});
        const int oth = (int)sources.size();
        sources.push_back(MixSource{other.data(), (long long)other.size(), 0, 0.0});
        const int none = (int)sources.size();
        sources.push_back(MixSource{nothing.data(), 0, 0, 0.0});
        // every clip looped from 0, from N - 1 and from the middle
        for (int k = 0; k < own; ++k) {
            const long long N = sources[(size_t)k].length;
            for (long long offset : {0ll, N - 1, N / 2}) {
                model(pcm, 1.0f, sources, {Term{k, offset, 1, 0.25f}}, L);
                if (L <= T + 1) model(pcm, 0.5f, sources, {Term{k, offset, 1, -0.75f}}, L + 3);      // a padded row
            }
        }
        // once: negative, zero, positive, straddling tiles, beyond the row
        for (long long offset : {-5000ll, -(long long)T, -1ll, 0ll, 1ll, (long long)T - 1, (long long)T, (long long)T + 3, L - 1, L, L + 7, 1ll << 44, -(1ll << 44)}) {
            model(pcm, 1.0f, sources, {Term{5, offset, 0, 0.5f}}, L);
            model(pcm, 1.0f, sources, {Term{oth, offset, 0, 0.5f}}, L);
            model(pcm, 1.0f, sources, {Term{1, offset, 0, 2.0f}}, L + 2 * T);      // a short clip, a padded row with tiles of padding alone
        }
        // no terms; speech gain 0; the row's own utterance; a source of no samples; many terms
        model(pcm, 1.0f, sources, {}, L);
        model(pcm, 0.0f, sources, {Term{3, 17, 1, 1.0f}}, L);
        model(pcm, -0.0f, sources, {}, L);
        model(pcm, 1.0f, sources, {Term{own, 0, 0, 1.0f}, Term{own, L / 2, 1, -0.5f}}, L);
        model(pcm, 1.0f, sources, {Term{none, 0, 0, 1.0f}, Term{none, -3, 0, 1.0f}}, L);
        std::vector<Term> many;
        for (int jt = 0; jt < kMixMaxTerms; ++jt) {
            const int k = jt % (none + 1);
            const long long N = sources[(size_t)k].length;
            const int loop = N > 0 && jt % 3 != 0;
            many.push_back(Term{k, loop ? (long long)(rng() % (uint32_t)N) : (long long)(rng() % 4000u) - 2000, loop, (float)((int)(rng() % 2001u) - 1000) / 1000.0f});
        }
        model(pcm, 0.7f, sources, many, L);
        model(pcm, 0.7f, sources, many, L + 5);
        // the row 1, 2 and 3 samples past an aligned address: the speech goes element by element, to the same bits
        for (int shift = 1; shift < 4; ++shift) model(pcm, 0.5f, sources, {Term{4, 7, 1, 0.25f}, Term{oth, -9, 0, 0.5f}}, L + (shift == 2 ? 3 : 0), shift);
    }
    // ---- the bank and its refusals ----
    {
        MixBank B;
        std::string why;
        std::vector<float> noise(5000, 0.25f);
        const long long three[4] = {0, 1, 5, 5000};
        CHECK(mix_bank_plan(B, noise.data(), three, 3, why) && B.clips() == 3 && B.start.size() == 4 && B.power[0] == 0.0625 && B.power[2] == 0.0625, "%s", why.c_str());
        CHECK(mix_bank_plan(B, nullptr, nullptr, 0, why) && B.clips() == 0, "no clips frees the bank");
        CHECK(!mix_bank_plan(B, noise.data(), three, -1, why) && !mix_bank_plan(B, noise.data(), three, kMixMaxClips + 1, why), "nNoise");
        CHECK(!mix_bank_plan(B, nullptr, three, 3, why) && !mix_bank_plan(B, noise.data(), nullptr, 3, why), "NULL");
        const long long late[2] = {1, 5}, empty[3] = {0, 4, 4}, back[3] = {0, 4, 2}, big[2] = {0, kMixMaxBank + 1};
        CHECK(!mix_bank_plan(B, noise.data(), late, 1, why) && !mix_bank_plan(B, noise.data(), empty, 2, why) && !mix_bank_plan(B, noise.data(), back, 2, why), "noiseStart");
        CHECK(!mix_bank_plan(B, noise.data(), big, 1, why) && why.find("in all") != std::string::npos, "samples: %s", why.c_str());
        for (float bad : {NAN, INFINITY, -INFINITY, 65536.0078125f, -131072.0f}) {
            noise[3] = bad;
            CHECK(!mix_bank_plan(B, noise.data(), three, 3, why) && why.find("sample 2 of clip 1") != std::string::npos, "value %g: %s", (double)bad, why.c_str());
        }
        noise[3] = -65536.0f;
        CHECK(mix_bank_plan(B, noise.data(), three, 3, why), "2^16 is admitted: %s", why.c_str());
    }
    // ---- the refusals of a row and of a term ----
    {
        std::string why;
        const MixTermIn one[1] = {};
        const long long good[4] = {0, 0, 64, 64}, late[2] = {1, 1}, back[3] = {0, 4, 2}, many[2] = {0, 65}, total[3] = {0, kMixMaxCallTerms - 1, kMixMaxCallTerms + 1};
        for (long long i = 0; i < 3; ++i) CHECK(mix_check_row(good, i, one, why), "row %lld: %s", i, why.c_str());
        CHECK(mix_check_row(good, 0, nullptr, why) && !mix_check_row(good, 1, nullptr, why), "terms NULL");
        CHECK(!mix_check_row(nullptr, 0, one, why) && !mix_check_row(late, 0, one, why) && !mix_check_row(back, 1, one, why), "termStart");
        CHECK(!mix_check_row(many, 0, one, why) && why.find("65 terms") != std::string::npos, "%s", why.c_str());
        CHECK(!mix_check_row(total, 1, one, why) && why.find("in all") != std::string::npos, "%s", why.c_str());
        const auto len = [](int kind, long long k) { return kind == 0 ? (k == 0 ? 10ll : 1000ll) : (k == 0 ? 0ll : 500ll); };
        const auto ok = [&](MixTermIn t, long long nClips = 2) { return mix_check_term(t, 7, 3, nClips, 2, len, why); };
        const MixTermIn base{0, 0, 1, 999, 10.0, 1, 0};
        CHECK(ok(base), "%s", why.c_str());
        MixTermIn t = base;
        t.kind = 2; CHECK(!ok(t) && why.find("row 7, term 3") == 0, "%s", why.c_str());
        t = base; t.kind = -1; CHECK(!ok(t), "kind");
        t = base; t.levelKind = 2; CHECK(!ok(t), "levelKind");
        t = base; t.loop = 2; CHECK(!ok(t), "loop");
        t = base; t.loop = -1; CHECK(!ok(t), "loop");
        CHECK(!ok(base, -1) && why.find("no noise bank") != std::string::npos, "%s", why.c_str());
        t = base; t.source = 2; CHECK(!ok(t) && why.find("not in the bank") != std::string::npos, "%s", why.c_str());
        t = base; t.source = -1; CHECK(!ok(t), "clip");
        t = base; t.kind = 1; t.source = 2; t.offset = 0; CHECK(!ok(t) && why.find("not an utterance") != std::string::npos, "%s", why.c_str());
        t = base; t.kind = 1; t.source = 0; t.offset = 0; CHECK(!ok(t) && why.find("length 0") != std::string::npos, "%s", why.c_str());
        t.loop = 0; CHECK(ok(t), "a source of no samples may be placed once: %s", why.c_str());
        t = base; t.offset = 1000; CHECK(!ok(t), "offset N");
        t = base; t.offset = -1; CHECK(!ok(t), "offset -1");
        t = base; t.loop = 0; t.offset = kMixMaxOffset; CHECK(ok(t), "%s", why.c_str());
        t.offset = -kMixMaxOffset; CHECK(ok(t), "%s", why.c_str());
        t.offset = kMixMaxOffset + 1; CHECK(!ok(t), "offset");
        t.offset = -kMixMaxOffset - 1; CHECK(!ok(t), "offset");
        for (double bad : {(double)NAN, (double)INFINITY, -(double)INFINITY, 200.5, -201.0}) { t = base; t.level = bad; CHECK(!ok(t) && why.find("dB") != std::string::npos, "%s", why.c_str()); }
        t = base; t.level = -200.0; CHECK(ok(t), "%s", why.c_str());
        for (double bad : {(double)NAN, (double)INFINITY, 4294967297.0, -1e10}) { t = base; t.levelKind = 1; t.level = bad; CHECK(!ok(t) && why.find("gain") != std::string::npos, "%s", why.c_str()); }
        t = base; t.levelKind = 1; t.level = -4294967296.0; CHECK(ok(t), "%s", why.c_str());
        CHECK(mix_check_speech_gain(4294967296.0f, 0, why) && mix_check_speech_gain(-0.0f, 0, why), "speech gain");
        CHECK(!mix_check_speech_gain(NAN, 4, why) && why.find("row 4") == 0 && !mix_check_speech_gain(INFINITY, 0, why) && !mix_check_speech_gain(-8589934592.0f, 0, why), "speech gain");
    }
    // ---- a staging block with reserved sections: device scratch that carries no contents ----
    {
        const std::vector<long long> rows{1, 2, 3};
        const std::vector<unsigned long long> zeros(5, 0ull);
        StageBlock b;
        const int rowsAt = b.add(rows), slotsAt = b.add(zeros), gainsAt = b.reserve(7 * sizeof(float));
        CHECK(b.offset(rowsAt) == 0 && b.offset(slotsAt) == 32 && b.offset(gainsAt) == 80 && b.bytes() == 112 && b.upload_bytes() == 80, "%zu of %zu bytes cross", b.upload_bytes(), b.bytes());
        std::vector<unsigned char> host(b.bytes(), (unsigned char)0xAB);
        b.copy_to(host.data());
        CHECK(!memcmp(host.data(), rows.data(), 24) && !memcmp(host.data() + 32, zeros.data(), 40), "contents");
        for (size_t i = 80; i < 112; ++i) CHECK(host[i] == 0xAB, "the reserved section was written at %zu", i);
        StageBlock inner;      // a reserved section in front of contents crosses with them
        inner.reserve(20); inner.add(rows);
        CHECK(inner.upload_bytes() == inner.bytes() && inner.bytes() == 64, "%zu", inner.upload_bytes());
        StageBlock none;
        none.reserve(0); none.add(nullptr, 0);
        CHECK(none.upload_bytes() == 0 && none.bytes() == 0, "empty");
        StageBlock plain;      // no reserved section: the whole block, as before
        plain.add(rows); plain.add(zeros);
        CHECK(plain.upload_bytes() == plain.bytes(), "plain");
    }
    printf("ok %lld\n", checks);
    return 0;
}
