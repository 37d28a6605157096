// check_track_plan.cpp -- the host's track planner, shape table and worker pool (nvspeechplayer_amd/csrc/klatt_trackplan.h,
// klatt_hostpool.h) as a stand-alone program.  tests/test_host_logic.py builds it once with AddressSanitizer + UBSan and once with
// ThreadSanitizer; it prints "ok <checks>" and how often each branch below was reached, or the first failure.
//   A  one pass of the planner against a restatement of the reference's frame rules (a transcription of expected() in
//      tests/test_track_planning.py, written without the header's code: maps keyed by the values' bytes), the budget rule included
//   B  planning in parts against one pass, with the frame threshold lowered so that small batches take the parts
//   C  the shape table against a first-occurrence scan
//   D  the pool: run_parts, a part that throws, sections of several callers at once, parallel_ranges
#include "../../nvspeechplayer_amd/csrc/klatt_trackplan.h"

#include <map>
#include <random>
#include <stdexcept>
#include <string>

using namespace klatt;

static long long g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

enum Branch { kBudgetMissKept, kAllOrNothing, kTooLong, kOutOfSilence, kNullAfterNull, kByHash, kMaskCollision, kPartsMerged, kPartsMetByOnePass,
              kPartsMissed, kPartsTooLongFew, kPartsTooLongMany, kGiveUpInPass, kGiveUpAtProbe, kBranches };
static const char* const kBranchNames[kBranches] = {
    "a budget miss kept", "all or nothing", "a fade too long for a track", "a start out of silence", "NULL after NULL", "a frame recognised by its hash",
    "two shapes colliding under a 6-bit mask, found by the host comparison", "parts merged", "parts given up, budget met by the one pass",
    "parts, budget missed", "parts, too-long fades in few", "parts, too-long fades in most", "given up inside the pass", "given up at the look before the parts"};
static long long g_hits[kBranches];

// ---- the tables of tests/test_track_planning.py (frame.h order), not the header's --------------------------------------------------
static const int RES_F[14] = {13, 14, 12, 11, 10, 9, 8, 7, 25, 26, 27, 28, 29, 30};
static const int RES_B[14] = {21, 22, 20, 19, 18, 17, 16, 15, 31, 32, 33, 34, 35, 36};
static const int PAIRS[10][2] = {{23, -1}, {41, 42}, {43, 45}, {24, 44}, {37, 38}, {39, 40}, {1, 2}, {3, 4}, {5, 6}, {44, -1}};
static const int GAINS[17] = {23, 41, 42, 43, 45, 24, 44, 37, 38, 39, 40, 1, 2, 3, 4, 5, 6};
constexpr unsigned long long FIRST = 25;

struct Frame47 { double v[47]; };
struct BatchIn {
    std::vector<long long> start;      // exactly nUtterances + 1 long: an overrun is an ASan report
    std::vector<Frame47> frames;
    std::vector<FrameMeta> meta;
    std::vector<FrameFacts> facts;
    std::vector<unsigned char> eligible;
    long long nU() const { return (long long)start.size() - 1; }
    long long nF() const { return start.back(); }
    FrameSource source() const { return FrameSource{reinterpret_cast<const speechPlayer_frame_t*>(frames.data()), nullptr, nullptr}; }
};
static_assert(sizeof(Frame47) == sizeof(speechPlayer_frame_t), "a frame is 47 doubles");

static HashMask mask_bits(int bits)
{
    HashMask m;
    m.a = bits >= 64 ? ~0ull : (bits == 0 ? 0ull : ((1ull << bits) - 1ull));
    m.b = bits >= 128 ? ~0ull : (bits <= 64 ? 0ull : ((1ull << (bits - 64)) - 1ull));
    return m;
}

// random_frames of tests/test_track_planning.py: few distinct shapes, so that fades repeat across utterances; NULL frames anywhere
static BatchIn random_batch(std::mt19937_64& rng, long long nU, int minFrames, int maxFrames, double pEligible)
{
    std::uniform_real_distribution<double> val(100.0, 5000.0), unit(0.0, 1.0);
    Frame47 shapes[6];
    for (auto& s : shapes) for (double& x : s.v) x = val(rng);
    shapes[1] = shapes[0]; shapes[1].v[9] += 1.0;           // differs from shape 0 in one formant only
    shapes[2].v[13] = 0.0; shapes[3] = shapes[2]; shapes[3].v[13] = -0.0;      // equal by value, different bits
    shapes[4] = shapes[0]; shapes[4].v[44] += 0.25;         // ... in the gain only
    shapes[5] = shapes[0]; shapes[5].v[5] *= 0.5;           // ... in a source parameter only
    static const uint32_t kFades[5] = {0, 1, 2, 50, 300};
    BatchIn b;
    b.start.assign(1, 0);
    for (long long u = 0; u < nU; ++u) {
        const int n = minFrames + (int)(rng() % (unsigned)(maxFrames - minFrames + 1));
        for (int i = 0; i < n; ++i) {
            b.frames.push_back(shapes[rng() % 6]);
            FrameMeta m;
            m.minSamples = 0; m.userIndex = -1;
            m.fadeSamples = std::max(kFades[rng() % 5], 1u);
            m.flags = unit(rng) < 0.25 ? FRAME_NULL : 0u;
            b.meta.push_back(m);
        }
        b.start.push_back(b.start.back() + n);
        b.eligible.push_back(unit(rng) < pEligible ? 1 : 0);
    }
    b.start.shrink_to_fit();
    b.facts.resize(b.frames.size());
    for (size_t k = 0; k < b.frames.size(); ++k) b.facts[k] = frame_facts(b.frames[k].v, 1e300, 1e300);
    return b;
}

// ---- the restatement ---------------------------------------------------------------------------------------------------------------
static uint32_t moved(const double* o, const double* n)
{
    uint32_t m = 0;
    for (int r = 0; r < 14; ++r)
        if (o[RES_F[r]] != n[RES_F[r]] || o[RES_B[r]] != n[RES_B[r]]) m |= 1u << r;
    for (int e = 0; e < 10; ++e)
        if (o[PAIRS[e][0]] != n[PAIRS[e][0]] || (PAIRS[e][1] >= 0 && o[PAIRS[e][1]] != n[PAIRS[e][1]])) m |= 1u << (14 + e);
    return m;
}
static void append_shape(std::string& s, const double* p)
{
    for (int r = 0; r < 14; ++r) { s.append(reinterpret_cast<const char*>(&p[RES_F[r]]), 8); s.append(reinterpret_cast<const char*>(&p[RES_B[r]]), 8); }
    for (int g : GAINS) s.append(reinterpret_cast<const char*>(&p[g]), 8);
}
static unsigned popcount(uint32_t m) { unsigned n = 0; for (; m; m &= m - 1) ++n; return n; }

struct Expected {
    std::vector<uint32_t> mask, rep, kinds;
    std::vector<unsigned long long> off;
    std::vector<std::string> key;           // per frame: its fade, by the bytes of both ends and the length
    std::vector<unsigned char> tracked;
    unsigned long long entries = 0;
    long long nTracks = 0, eligible = 0, missedSize = 0, missedBudget = 0;
    bool collision = false;                 // two frames with one (masked) hash and different values among the frames walked
    long long outOfSilence = 0, nullAfterNull = 0, byHash = 0;
};
// The plan of one pass over the whole batch: utterances in order, a fade's track placed where the tracks end when the fade is first
// met; an utterance with a fade of 2^27 entries or more, or whose new tracks pass the budget, takes its tracks back and stays out;
// once more than a tenth of the eligible are out, nothing is tracked.
static Expected restate(const BatchIn& b, unsigned long long budget, HashMask hm)
{
    Expected x;
    const long long nU = b.nU(), nF = b.nF();
    x.mask.assign((size_t)nF, 0); x.rep.assign((size_t)nF, 0xFFFFFFFFu); x.off.assign((size_t)nF, 0); x.key.resize((size_t)nF);
    x.tracked.assign((size_t)nU, 0); x.kinds.assign((size_t)nU, 0);
    for (long long u = 0; u < nU; ++u) x.eligible += b.eligible[u] ? 1 : 0;
    std::map<std::string, unsigned long long> placed;
    std::map<std::pair<unsigned long long, unsigned long long>, long long> firstSeen;
    long long missed = 0;
    for (long long u = 0; u < nU && missed * 10 <= x.eligible; ++u) {
        if (!b.eligible[u]) continue;
        double prev[47] = {0};
        bool prevNull = true, fits = true;
        std::vector<std::string> added;
        const unsigned long long before = x.entries;
        const long long tracksBefore = x.nTracks;
        uint32_t kinds = 0;
        for (long long k = b.start[u]; k < b.start[u + 1]; ++k) {
            double o[47], n[47];
            const unsigned long long F = b.meta[k].fadeSamples;
            if (b.meta[k].flags & FRAME_NULL) {
                memcpy(o, prev, sizeof o); memcpy(n, prev, sizeof n);
                n[44] = 0.0;
                if (k > b.start[u] && prevNull) ++x.nullAfterNull;
                prevNull = true;
            } else {
                memcpy(n, b.frames[k].v, sizeof n);
                memcpy(o, prevNull ? n : prev, sizeof o);
                if (prevNull) { o[44] = 0.0; ++x.outOfSilence; }
                prevNull = false;
                const std::pair<unsigned long long, unsigned long long> h{b.facts[k].h0 & hm.a, b.facts[k].h1 & hm.b};
                auto it = firstSeen.find(h);
                if (it == firstSeen.end()) firstSeen.emplace(h, k);
                else {
                    x.rep[k] = (uint32_t)it->second; ++x.byHash;
                    if (memcmp(&b.frames[k].v[1], &b.frames[it->second].v[1], 45 * sizeof(double))) x.collision = true;
                }
            }
            const uint32_t m = moved(o, n);
            if (k > b.start[u]) kinds |= moved(prev, o);      // what the fade's first sample re-sets to other values than the last fade ended on
            kinds |= m;
            memcpy(prev, n, sizeof prev);
            std::string key;
            append_shape(key, o); append_shape(key, n);
            key.append(reinterpret_cast<const char*>(&F), 8);
            auto p = placed.find(key);
            if (p == placed.end()) {
                const unsigned long long size = FIRST + (F - 1) * (popcount(m) + (m & 1u));
                if (size >= (1ull << 27)) { ++x.missedSize; fits = false; break; }
                if (x.entries + size > budget) { ++x.missedBudget; fits = false; break; }
                p = placed.emplace(key, x.entries).first;
                added.push_back(key);
                x.entries += size;
                ++x.nTracks;
            }
            x.off[k] = p->second; x.mask[k] = m; x.key[k] = key;
        }
        x.kinds[u] = kinds;
        if (fits) x.tracked[u] = 1;
        else {
            for (const std::string& key : added) placed.erase(key);
            x.entries = before; x.nTracks = tracksBefore;
            ++missed;
        }
    }
    if (missed * 10 > x.eligible) { x.tracked.assign((size_t)nU, 0); x.entries = 0; x.nTracks = 0; }
    return x;
}

// what plan_tracks_view does with a plan's rep: every frame recognised by its hash against the frame that stood for it
static bool host_comparison_finds_a_collision(const BatchIn& b, const TrackPlan& p)
{
    for (long long k = 0; k < b.nF() && !p.rep.empty(); ++k) {
        const uint32_t r = p.rep[(size_t)k];
        if (r == 0xFFFFFFFFu || (long long)r == k) continue;
        if (!shape_values_equal(b.frames[k].v, b.frames[r].v)) return true;
    }
    return false;
}

// the tracks tile [0, entries) in the order of the jobs, kTrackFirst + (F - 1) * slots entries each; every tracked frame names one
static void check_tiling(const BatchIn& b, const TrackPlan& p)
{
    unsigned long long at = 0;
    std::map<unsigned long long, const TrackJob*> byOff;
    for (const TrackJob& j : p.jobs) {
        CHECK(j.off == at);
        at += (unsigned long long)kTrackFirst + (unsigned long long)(j.fadeSamples - 1u) * (popcount(j.mask) + (j.mask & 1u));
        byOff[j.off] = &j;
    }
    CHECK(at == p.entries);
    for (long long u = 0; u < b.nU(); ++u) {
        if (!p.tracked[(size_t)u]) continue;
        for (long long k = b.start[u]; k < b.start[u + 1]; ++k) {
            const TrackRef& r = p.ref[(size_t)k];
            auto it = byOff.find(r.off);
            CHECK(it != byOff.end() && it->second->mask == r.mask && it->second->fadeSamples == b.meta[k].fadeSamples);
            CHECK(r.nSlots == popcount(r.mask) + (r.mask & 1u));
        }
    }
}

static void check_against_restatement(const BatchIn& b, const TrackPlan& p, const Expected& x)
{
    CHECK(p.eligible == x.eligible && p.missedSize == x.missedSize && p.missedBudget == x.missedBudget);
    CHECK(p.entries == x.entries && (long long)p.jobs.size() == x.nTracks);
    CHECK((long long)p.ref.size() == b.nF() && (long long)p.rep.size() == b.nF() && (long long)p.tracked.size() == b.nU());
    std::map<std::string, unsigned long long> byKey;
    std::map<unsigned long long, std::string> byOff;
    for (long long u = 0; u < b.nU(); ++u) {
        CHECK(p.tracked[(size_t)u] == x.tracked[(size_t)u]);
        if (!p.tracked[(size_t)u]) continue;      // (the refs and kinds of an utterance that stays out mean nothing: the views clear them)
        CHECK(p.kinds[(size_t)u] == x.kinds[(size_t)u]);
        for (long long k = b.start[u]; k < b.start[u + 1]; ++k) {
            CHECK(p.ref[(size_t)k].mask == x.mask[(size_t)k] && p.ref[(size_t)k].off == x.off[(size_t)k]);
            // equal fades share a track, unequal ones do not
            CHECK(byKey.emplace(x.key[(size_t)k], p.ref[(size_t)k].off).first->second == p.ref[(size_t)k].off);
            CHECK(byOff.emplace(p.ref[(size_t)k].off, x.key[(size_t)k]).first->second == x.key[(size_t)k]);
        }
    }
    CHECK((long long)byKey.size() == (long long)p.jobs.size());
    for (long long k = 0; k < b.nF(); ++k) CHECK(p.rep[(size_t)k] == x.rep[(size_t)k]);
    check_tiling(b, p);
}

// ---- A -----------------------------------------------------------------------------------------------------------------------------
static void one_pass_against_the_restatement(std::mt19937_64& rng)
{
    const unsigned long long ample = track_budget_entries(16384);
    CHECK(ample == (1ull << 28) - (1ull << 21) - 64 && track_budget_entries(-5) == 0 && track_budget_entries(1) == 65536);
    for (int round = 0; round < 2000; ++round) {
        BatchIn b = random_batch(rng, (long long)(rng() % 41), 0, 6, 0.7);
        if (round % 8 == 0)      // a fade of 2^23 samples: too long for a track once it moves 16 kinds or more
            for (int i = 0; i < 2 && b.nF() > 0; ++i) b.meta[(size_t)(rng() % (unsigned long long)b.nF())].fadeSamples = 1u << 23;
        TrackPlan p;
        const FrameSource src = b.source();
        auto run = [&](unsigned long long budget, HashMask hm) {
            plan_tracks(b.nU(), b.start.data(), src, b.facts.data(), b.meta.data(), b.eligible.data(), budget, hm, p, 1u);
        };
        run(ample, HashMask());
        const Expected whole = restate(b, ample, HashMask());
        CHECK(!whole.collision);
        check_against_restatement(b, p, whole);
        g_hits[kOutOfSilence] += whole.outOfSilence; g_hits[kNullAfterNull] += whole.nullAfterNull; g_hits[kByHash] += whole.byHash;
        const unsigned long long need = whole.entries;
        for (unsigned long long budget : {0ull, need > 0 ? need - 1 : 0ull, need + 1}) {
            run(budget, HashMask());
            const Expected x = restate(b, budget, HashMask());
            check_against_restatement(b, p, x);
            long long in = 0;
            for (unsigned char t : x.tracked) in += t;
            if (x.missedSize > 0) ++g_hits[kTooLong];
            if (x.missedBudget > 0 && in > 0) { CHECK(x.missedBudget * 10 <= x.eligible); ++g_hits[kBudgetMissKept]; }
            if ((x.missedBudget + x.missedSize) * 10 > x.eligible) { CHECK(in == 0 && p.entries == 0 && p.jobs.empty()); ++g_hits[kAllOrNothing]; }
        }
        // six bits of the hash: different shapes may collide.  The planner then takes one for the other -- and the comparison of every
        // recognised frame with the frame that stood for it (plan_tracks_view on the host, klatt_verify_shared on the device) must say so.
        // (Batches without the long fades: every frame of an eligible utterance is walked whatever the planner takes its shape to be.)
        if (round % 8 != 0) {
            const HashMask six = mask_bits(6);
            run(ample, six);
            const Expected x = restate(b, ample, six);
            for (long long k = 0; k < b.nF(); ++k) CHECK(p.rep[(size_t)k] == x.rep[(size_t)k]);
            CHECK(host_comparison_finds_a_collision(b, p) == x.collision);
            if (x.collision) ++g_hits[kMaskCollision];
            else check_against_restatement(b, p, x);
        }
    }
}

// ---- B -----------------------------------------------------------------------------------------------------------------------------
static const double* shape_row(const TrackPlan& p, uint32_t id) { return &p.shapes[(size_t)id * kShapeStride]; }
// Parts and one pass make the same tracks in the same places.  Shape ids may differ (a gated shape gets its number when somebody first
// asks for it), so a track is compared by its fade's values and length; rep may differ too -- a part recognises a frame by the first
// frame of that hash in the PART -- so it is held to what the verification needs: an earlier frame, itself a first one, with the same hash.
static void compare_plans(const BatchIn& b, const TrackPlan& one, const TrackPlan& many)
{
    CHECK(one.entries == many.entries && one.jobs.size() == many.jobs.size() && one.eligible == many.eligible);
    CHECK(one.tracked == many.tracked);
    bool any = false;
    for (unsigned char t : one.tracked) any = any || t;
    // (once nothing is tracked the one pass has stopped counting: the parts' counters say more)
    if (any) CHECK(one.missedSize == many.missedSize && one.missedBudget == many.missedBudget);
    for (size_t i = 0; i < one.jobs.size(); ++i) {
        const TrackJob &x = one.jobs[i], &y = many.jobs[i];
        CHECK(x.off == y.off && x.fadeSamples == y.fadeSamples && x.mask == y.mask);
        CHECK(!memcmp(shape_row(one, x.fromShape), shape_row(many, y.fromShape), kShapeValues * sizeof(double)));
        CHECK(!memcmp(shape_row(one, x.toShape), shape_row(many, y.toShape), kShapeValues * sizeof(double)));
    }
    for (long long u = 0; u < b.nU(); ++u) {
        if (!one.tracked[(size_t)u]) continue;
        CHECK(one.kinds[(size_t)u] == many.kinds[(size_t)u]);
        for (long long k = b.start[u]; k < b.start[u + 1]; ++k) {
            const TrackRef &x = one.ref[(size_t)k], &y = many.ref[(size_t)k];
            CHECK(x.off == y.off && x.mask == y.mask && x.nSlots == y.nSlots);
            if (many.rep.empty()) continue;
            const uint32_t r = many.rep[(size_t)k];
            if (r == 0xFFFFFFFFu) continue;
            CHECK((long long)r < k && many.rep[r] == 0xFFFFFFFFu && one.rep[(size_t)k] != 0xFFFFFFFFu && one.rep[(size_t)k] <= r);
            CHECK(b.facts[r].h0 == b.facts[(size_t)k].h0 && b.facts[r].h1 == b.facts[(size_t)k].h1);
        }
    }
    if (any) check_tiling(b, many);
}

static void parts_against_one_pass(std::mt19937_64& rng)
{
    const unsigned long long ample = track_budget_entries(16384);
    struct Case { long long nU; unsigned threads; };
    const Case cases[] = {{130, 2}, {520, 5}, {520, 8}, {611, 5}, {700, 8}, {700, 5}};
    for (const Case& c : cases) {
        BatchIn b = random_batch(rng, c.nU, 1, 6, 0.9);
        const FrameSource src = b.source();
        auto both = [&](unsigned long long budget, TrackPlan& one, TrackPlan& many) {
            plan_tracks(b.nU(), b.start.data(), src, b.facts.data(), b.meta.data(), b.eligible.data(), budget, HashMask(), one, 1u, 0);
            plan_tracks(b.nU(), b.start.data(), src, b.facts.data(), b.meta.data(), b.eligible.data(), budget, HashMask(), many, c.threads, 0);
            compare_plans(b, one, many);
        };
        TrackPlan one, many;
        both(ample, one, many);
        check_against_restatement(b, one, restate(b, ample, HashMask()));
        // (a budget of eight times what all the parts could make together: no part gives up, the merge is the plan)
        CHECK(one.entries > 0 && one.entries * c.threads * 8 < ample);
        ++g_hits[kPartsMerged];
        const unsigned long long need = one.entries;
        both(need * 2, one, many);      // the parts pass a quarter of it and give up; the one pass meets it
        CHECK(one.entries == need && one.missedBudget == 0);
        ++g_hits[kPartsMetByOnePass];
        for (unsigned long long budget : {need - 1, need / 3, 0ull}) {
            both(budget, one, many);
            CHECK(one.missedBudget > 0);
            ++g_hits[kPartsMissed];
        }
        for (double share : {0.05, 0.9}) {
            BatchIn saved = b;
            std::uniform_real_distribution<double> unit(0.0, 1.0);
            // On the second frame (the first only moves the gain: from silence), and only where that fade moves 16 kinds or more.  A fade
            // of 2^23 samples that moves FEW kinds fits a track -- of 8 to 120 million entries --, and a few hundred utterances with
            // such tracks among the first of them are given up at the look before the parts while one pass keeps them: the look-outs
            // are estimates made for large batches, and that difference is not what this comparison is about.
            const Expected moves = restate(b, ample, HashMask());
            for (long long u = 0; u < b.nU(); ++u) {
                if (b.start[u + 1] - b.start[u] < 2 || unit(rng) >= share) continue;
                const uint32_t m = moves.mask[(size_t)b.start[u] + 1];
                if (popcount(m) + (m & 1u) >= 16) b.meta[(size_t)b.start[u] + 1].fadeSamples = 1u << 23;
            }
            both(ample, one, many);
            CHECK(many.missedSize > 0);
            bool any = false;
            for (unsigned char t : one.tracked) any = any || t;
            if (share < 0.1) { CHECK(any); ++g_hits[kPartsTooLongFew]; }
            else { CHECK(!any && one.entries == 0 && many.jobs.empty()); ++g_hits[kPartsTooLongMany]; }
            b = saved;
        }
    }
    // 8192 utterances of two frames, every shape different: the tracks double with the utterances and end far beyond the budget.
    // One pass gives up at its second look-out (after 1/16 of the batch), the parts at the look before they start.
    BatchIn b;
    std::uniform_real_distribution<double> val(100.0, 5000.0);
    b.start.assign(1, 0);
    for (long long u = 0; u < 8192; ++u) {
        for (int i = 0; i < 2; ++i) {
            Frame47 f;
            for (double& x : f.v) x = val(rng);
            b.frames.push_back(f);
            b.meta.push_back(FrameMeta{0u, 300u, -1, 0u});
        }
        b.start.push_back(b.start.back() + 2);
    }
    b.eligible.assign(8192, 1);
    b.facts.resize(b.frames.size());
    for (size_t k = 0; k < b.frames.size(); ++k) b.facts[k] = frame_facts(b.frames[k].v, 1e300, 1e300);
    const FrameSource src = b.source();
    const unsigned long long budget = 20000000;      // entries; the batch needs some 66 million
    TrackPlan one, many;
    plan_tracks(8192, b.start.data(), src, b.facts.data(), b.meta.data(), b.eligible.data(), budget, HashMask(), one, 1u, 0);
    CHECK(one.entries == 0 && one.jobs.empty() && one.missedBudget == 8192 && (long long)one.rep.size() == b.nF());
    // (it stopped at utterance 512: no later frame was looked at)
    for (long long k = 2 * 512; k < b.nF(); ++k) CHECK(one.ref[(size_t)k].nSlots == 0);
    CHECK(one.ref[2 * 511].nSlots != 0);
    ++g_hits[kGiveUpInPass];
    plan_tracks(8192, b.start.data(), src, b.facts.data(), b.meta.data(), b.eligible.data(), budget, HashMask(), many, 8u, 0);
    CHECK(many.entries == 0 && many.jobs.empty() && many.missedBudget == 8192 && many.eligible == 8192 && many.rep.empty());
    for (long long k = 0; k < b.nF(); ++k) CHECK(many.ref[(size_t)k].nSlots == 0);      // (nothing was merged: given up before the parts)
    ++g_hits[kGiveUpAtProbe];
    compare_plans(b, one, many);
}

// ---- C -----------------------------------------------------------------------------------------------------------------------------
static void shape_table_against_a_scan(std::mt19937_64& rng)
{
    for (int round = 0; round < 60; ++round) {
        const BatchIn b = random_batch(rng, (long long)(rng() % 120), 0, 6, 0.7);
        for (int bits : {128, 6, 0}) {
            const HashMask hm = mask_bits(bits);
            std::map<std::pair<unsigned long long, unsigned long long>, uint32_t> rowOfKey;
            std::vector<long long> first;
            std::vector<long long> want((size_t)b.nF(), -1);
            for (long long u = 0; u < b.nU(); ++u) {
                if (!b.eligible[(size_t)u]) continue;
                for (long long k = b.start[u]; k < b.start[u + 1]; ++k) {
                    if (b.meta[(size_t)k].flags & FRAME_NULL) continue;
                    auto it = rowOfKey.emplace(std::make_pair(b.facts[(size_t)k].h0 & hm.a, b.facts[(size_t)k].h1 & hm.b), (uint32_t)first.size());
                    if (it.second) first.push_back(k);
                    want[(size_t)k] = it.first->second;
                }
            }
            if (bits == 0) CHECK(first.size() <= 1);
            for (unsigned threads : {1u, 3u, 8u}) {
                RawVector<uint32_t> rowOf;
                std::vector<long long> rep(3, 77);
                shape_table_rows(b.nU(), b.start.data(), b.meta.data(), b.facts.data(), b.eligible.data(), hm, rowOf, rep, threads, 16);
                CHECK(rep == first && (long long)rowOf.size() == b.nF());
                for (long long k = 0; k < b.nF(); ++k)
                    if (want[(size_t)k] >= 0) CHECK((long long)rowOf[(size_t)k] == want[(size_t)k]);
            }
        }
    }
}

// ---- D -----------------------------------------------------------------------------------------------------------------------------
static void the_pool()
{
    for (unsigned n : {0u, 1u, 2u, 33u}) {
        std::vector<std::atomic<int>> ran(n);
        for (auto& r : ran) r.store(0);
        run_parts(n, [&](unsigned t) { ran[t].fetch_add(1); });
        for (auto& r : ran) CHECK(r.load() == 1);
    }
    // a part that throws: the caller sees the exception, and only after every other part has run; the pool works afterwards
    for (unsigned thrower : {0u, 3u, 7u}) {
        std::atomic<int> others{0};
        bool caught = false;
        try {
            run_parts(8u, [&](unsigned t) {
                if (t == thrower) throw std::runtime_error("a part gave up");
                std::this_thread::sleep_for(std::chrono::milliseconds(2));
                others.fetch_add(1);
            });
        } catch (const std::runtime_error& e) {
            caught = true;
            // (without workers the parts run one after the other on the caller, and a throw ends the section)
            CHECK((others.load() == 7 || WorkerPool::get().workers() == 0) && std::string(e.what()) == "a part gave up");
        }
        CHECK(caught);
        std::atomic<int> sum{0};
        run_parts(5u, [&](unsigned t) { sum.fetch_add((int)t + 1); });
        CHECK(sum.load() == 15);
    }
    // sections of four callers at once share the workers
    std::vector<long long> totals(4, 0);
    std::vector<std::thread> callers;
    for (int c = 0; c < 4; ++c)
        callers.emplace_back([&totals, c] {
            for (int s = 0; s < 50; ++s) {
                std::vector<long long> part(7, 0);
                run_parts(7u, [&](unsigned t) { part[t] = (long long)(t + 1) * (c + 1) + s; });
                for (long long v : part) totals[(size_t)c] += v;
            }
        });
    for (std::thread& t : callers) t.join();
    for (int c = 0; c < 4; ++c) CHECK(totals[(size_t)c] == 50ll * 28 * (c + 1) + 7ll * (49 * 50 / 2));
    // parallel_ranges covers [0, n) exactly once
    const long long grain = 1000;
    for (long long n : {0ll, 1ll, grain - 1, grain, 2 * grain + 1, 1000000ll}) {
        std::vector<unsigned char> seen((size_t)n, 0);
        std::atomic<long long> covered{0};
        std::atomic<bool> outside{false};
        parallel_ranges(n, grain, [&](long long a, long long e) {
            if (!(0 <= a && a <= e && e <= n)) { outside.store(true); return; }      // (no CHECK on a worker thread: its counter is the main thread's)
            for (long long i = a; i < e; ++i) ++seen[(size_t)i];
            covered.fetch_add(e - a);
        });
        CHECK(!outside.load() && covered.load() == n);
        for (unsigned char s : seen) if (s != 1) CHECK(s == 1);
    }
}

int main()
{
    std::mt19937_64 rng(20240611);
    one_pass_against_the_restatement(rng);
    parts_against_one_pass(rng);
    shape_table_against_a_scan(rng);
    the_pool();
    printf("ok %lld checks, %u pool workers\n", g_checks, WorkerPool::get().workers());
    bool all = true;
    for (int i = 0; i < kBranches; ++i) {
        printf("  %s: %lld\n", kBranchNames[i], g_hits[i]);
        all = all && g_hits[i] > 0;
    }
    if (!all) { printf("FAILED: a branch was never reached\n"); return 1; }
    return 0;
}
