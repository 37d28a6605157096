// check_dead_terms2.cpp -- the second word of "present" facts of a frame (nvspeechplayer_amd/csrc/klatt_plan.h: shape_present2, present2_of --
// parallel resonators 2..6 and the nasal pair), each side of every rule on hand-written frames, their OR over a frame list
// (klatt_batchplan.h, classify_list with a present2 word) and that no step of the routing (reroute_lonely_quiet, mark_tracked, route_direct,
// restore_rerouted, pack_lanes) touches them or is touched by them; dead2_wave_counts on a width-4 order for every value of the built mask.
// Built with AddressSanitizer + UBSan by tests/test_dead_terms2_host.py; prints "ok <checks>" and how often each branch below was
// reached, or the first failure.
#include "../../nvspeechplayer_amd/csrc/klatt_batchplan.h"
#include "../../nvspeechplayer_amd/csrc/klatt_plan.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

using namespace klatt;

static long long g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

enum Branch { kAllDead, kAmplitudeSet, kAmplitudeNegZero, kBandwidthLow, kBandwidthHigh, kFrequencyFar, kGainFar, kNotANumber, kNasalCoupled, kNasalNegZero,
              kNasalUnstable, kNasalSourceFar, kNasalAspirationFar, kOffenderInTheMiddle, kNullFrameIgnored, kRerouted, kRestored, kTrackedKeeps, kDirectKeeps, kPackingSame,
              kPlanCounts, kEveryMask, kBranches };
static const char* const kBranchNames[kBranches] = {
    "every term dead", "pa_k non-zero", "pa_k = -0.0 is dead", "pb_k below 1", "pb_k above 1e6", "pf_k beyond 1e6", "a gain beyond 1e30", "a NaN keeps the term",
    "caNP non-zero", "caNP = -0.0 is dead", "N0 / NP outside their bounds", "the source beyond 1e30", "aspirationAmplitude beyond 1e30", "one offending frame in the middle of a list",
    "a NULL frame adds nothing", "a re-routed quiet list keeps its word", "a restored list keeps its word", "a tracked list keeps its word",
    "a direct list keeps its word", "the word does not change the packing", "the plan's wavefront counts", "every value of the built mask"};
static long long g_hits[kBranches];
#define HIT(b) (++g_hits[b])

constexpr double kMaxF = 1e300, kMaxBw = 1e300;      // (the direct stages' bounds: not what this program is about)

struct Frame { double p[kNumParams]; };

// a speech-like frame in which parallel 2..6 and the nasal pair are dead (and parallel 1, turbulence and aspiration present)
static Frame dead_frame()
{
    Frame f;
    for (double& v : f.p) v = 0.0;
    f.p[0] = 120.0; f.p[46] = 110.0;
    f.p[3] = 0.2; f.p[4] = 0.5; f.p[5] = 1.0; f.p[6] = 0.2;
    const double cf[8] = {700, 1200, 2600, 3300, 3750, 4900, 450, 270}, cb[8] = {90, 100, 150, 250, 200, 1000, 100, 100};
    for (int i = 0; i < 8; ++i) { f.p[7 + i] = cf[i]; f.p[15 + i] = cb[i]; }
    f.p[24] = 0.3;
    const double pf[6] = {720, 1250, 2500, 3400, 3800, 4800}, pb[6] = {80, 110, 160, 240, 210, 900}, pa[6] = {0.5, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < 6; ++i) { f.p[25 + i] = pf[i]; f.p[31 + i] = pb[i]; f.p[37 + i] = pa[i]; }
    f.p[43] = 0.3; f.p[44] = 1.0; f.p[45] = 0.6;
    return f;
}
static uint32_t present2(const Frame& f) { return frame_facts(f.p, kMaxF, kMaxBw).present2; }
static Frame with(int param, double v) { Frame f = dead_frame(); f.p[param] = v; return f; }
static uint32_t par_bit(int k) { return 1u << (k - 2); }

static void the_rules_frame_by_frame()
{
    CHECK(present2(dead_frame()) == 0u); HIT(kAllDead);
    static_assert(UTT2_PARALLEL2 == 1u && UTT2_PARALLEL6 == 16u && UTT2_NASAL == 32u && kUtt2Present == 63u, "the word's bits");
    static_assert(kUttPresent == 0x70u, "the first word's present bits stay where they were");
    const double denormal = 4.9406564584124654e-324;
    for (int k = 2; k <= 6; ++k) {
        const int pf = 24 + k, pb = 30 + k, pa = 36 + k;
        const uint32_t bit = par_bit(k);
        // pa_k: zero of either sign is dead, anything else -- a NaN too -- is present
        CHECK(present2(with(pa, 0.0)) == 0u);
        CHECK(present2(with(pa, -0.0)) == 0u); HIT(kAmplitudeNegZero);
        for (const double v : {1e-300, -1e-300, denormal, 0.5, (double)NAN, (double)INFINITY}) { CHECK(present2(with(pa, v)) == bit); HIT(kAmplitudeSet); if (v != v) HIT(kNotANumber); }
        // pb_k in [1, 1e6]
        CHECK(present2(with(pb, 1.0)) == 0u && present2(with(pb, 1e6)) == 0u);
        for (const double v : {0.999, 0.0, -80.0}) { CHECK(present2(with(pb, v)) == bit); HIT(kBandwidthLow); }
        for (const double v : {1.0000001e6, 1e300, (double)INFINITY}) { CHECK(present2(with(pb, v)) == bit); HIT(kBandwidthHigh); }
        CHECK(present2(with(pb, NAN)) == bit); HIT(kNotANumber);
        // |pf_k| <= 1e6
        CHECK(present2(with(pf, 1e6)) == 0u && present2(with(pf, -1e6)) == 0u && present2(with(pf, 0.0)) == 0u);
        for (const double v : {1.0000001e6, -1.0000001e6, (double)INFINITY, (double)NAN}) { CHECK(present2(with(pf, v)) == bit); HIT(kFrequencyFar); }
    }
    // |fricationAmplitude| (24) and |preFormantGain| (44) <= 1e30: the input of every parallel resonator (44 also bounds the nasal pair's)
    for (const int g : {24, 44}) {
        CHECK(present2(with(g, 1e30)) == 0u && present2(with(g, -1e30)) == 0u && present2(with(g, 0.0)) == 0u);
        const uint32_t want = 31u | (g == 44 ? UTT2_NASAL : 0u);
        for (const double v : {1.0000001e30, -1.0000001e30, (double)INFINITY, (double)NAN}) { CHECK(present2(with(g, v)) == want); HIT(kGainFar); }
    }
    // parallel 1 and the bypass are not this word's business
    for (const int q : {25, 31, 37, 43}) CHECK(present2(with(q, 12345.0)) == 0u);
    // the nasal pair: FACT_NASAL's rule, carried over.  caNP (23) zero of either sign, cbN0 (21) and cbNP (22) in [1 or 0, 1e6], |cfN0|, |cfNP| (13, 14) <= 1e6,
    // |voiceAmplitude| (5), |preFormantGain| (44) and the pitches <= 1e30
    CHECK(present2(with(23, -0.0)) == 0u); HIT(kNasalNegZero);
    for (const double v : {1e-300, -1e-300, 0.5, (double)NAN}) { CHECK(present2(with(23, v)) == UTT2_NASAL); HIT(kNasalCoupled); }
    CHECK(present2(with(21, 1.0)) == 0u && present2(with(21, 1e6)) == 0u && present2(with(22, 0.0)) == 0u);
    for (const double v : {0.999, 0.0, -5.0, 1.0000001e6, (double)NAN}) { CHECK(present2(with(21, v)) == UTT2_NASAL); HIT(kNasalUnstable); }
    for (const double v : {-1e-3, 1.0000001e6, (double)NAN}) { CHECK(present2(with(22, v)) == UTT2_NASAL); HIT(kNasalUnstable); }
    for (const int q : {13, 14}) for (const double v : {1.0000001e6, -1.0000001e6}) { CHECK(present2(with(q, v)) == UTT2_NASAL); HIT(kNasalUnstable); }
    for (const int q : {0, 46, 5}) for (const double v : {1.0000001e30, -1.0000001e30, (double)INFINITY}) { CHECK(present2(with(q, v)) == UTT2_NASAL); HIT(kNasalSourceFar); }
    // |aspirationAmplitude| (6) <= 1e30: the second word's own bound (a noisy list's source has the aspiration in it), which FACT_NASAL does not know
    CHECK(present2(with(6, 1e30)) == 0u && present2(with(6, -1e30)) == 0u && present2(with(6, 0.0)) == 0u && present2(with(6, -0.0)) == 0u);
    for (const double v : {1.0000001e30, -1.0000001e30, 1e307, -1e307, (double)INFINITY, (double)NAN}) {
        CHECK(present2(with(6, v)) == UTT2_NASAL); HIT(kNasalAspirationFar);
        if (v == v && fact_finite(v)) CHECK(!(frame_facts(with(6, v).p, kMaxF, kMaxBw).flags & FACT_NASAL));      // (the first word's fact is what it was)
    }
    CHECK(shape_present2(with(6, 1e307).p) == UTT2_NASAL && shape_present2(dead_frame().p) == 0u && shape_present2(with(23, 0.5).p) == 0u);      // (caNP: by FACT_NASAL)
    // otherwise the bit says what FACT_NASAL says, whatever else the frame holds
    for (const int q : {3, 6, 23, 24, 37, 38}) for (const double v : {0.0, 0.5}) {
        const FrameFacts ff = frame_facts(with(q, v).p, kMaxF, kMaxBw);
        CHECK(((ff.flags & FACT_NASAL) != 0u) == ((ff.present2 & UTT2_NASAL) != 0u));
    }
    // present2_of by hand, and nothing outside the word's six bits
    CHECK(present2_of(FACT_NASAL | FACT_NOISE, 5u) == (5u | UTT2_NASAL) && present2_of(FACT_NOISE | FACT_PARALLEL1, 31u) == 31u);
    // ... and the first word is what it was
    CHECK(frame_facts(dead_frame().p, kMaxF, kMaxBw).flags == (shape_flags(dead_frame().p, kMaxF, kMaxBw) | pitch_flags(120.0, 110.0)));
}

struct Meta { uint32_t minSamples, fadeSamples, flags; };
struct Facts { uint32_t flags, present2; };

static uint32_t classify(const std::vector<Frame>& frames, const std::vector<bool>& isNull, uint32_t* flagsOut = nullptr)
{
    std::vector<Meta> meta;
    std::vector<Facts> facts;
    for (size_t k = 0; k < frames.size(); ++k) {
        meta.push_back(Meta{600u, 100u, isNull[k] ? FRAME_NULL : 0u});
        const FrameFacts ff = frame_facts(frames[k].p, kMaxF, kMaxBw);      // (a NULL frame's values are whatever the caller left there: here the worst)
        facts.push_back(Facts{ff.flags, ff.present2});
    }
    uint32_t flags = 0, p2 = 0xFFFFFFFFu, flags5 = 0;
    unsigned char shape = 0, shape5 = 0;
    classify_list(meta.data(), facts.data(), (long long)frames.size(), flags, shape, p2);
    classify_list(meta.data(), facts.data(), (long long)frames.size(), flags5, shape5);
    CHECK(flags == flags5 && shape == shape5);      // the first word does not know of the second
    if (flagsOut) *flagsOut = flags;
    return p2;
}

static void the_list_level_or()
{
    const Frame d = dead_frame();
    CHECK(classify({d, d, d, d, d}, {false, false, false, false, false}) == 0u);
    CHECK(classify({}, {}) == 0u);
    const struct { int param; double v; uint32_t bits; } offenders[] = {
        {39, 1e-300, UTT2_PARALLEL3}, {35, 0.999, UTT2_PARALLEL5}, {41, 0.25, UTT2_PARALLEL5}, {42, -1e-300, UTT2_PARALLEL6}, {26, 2e6, UTT2_PARALLEL2},
        {40, NAN, UTT2_PARALLEL4}, {23, 0.4, UTT2_NASAL}, {21, 0.999, UTT2_NASAL}, {6, 1e307, UTT2_NASAL}, {24, 2e30, 31u}};
    for (const auto& o : offenders) {
        const Frame bad = with(o.param, o.v);
        for (size_t at = 0; at < 5; ++at) {
            std::vector<Frame> frames(5, d);
            frames[at] = bad;
            std::vector<bool> nulls(5, false);
            CHECK(classify(frames, nulls) == o.bits);
            if (at == 2) HIT(kOffenderInTheMiddle);
            nulls[at] = true;      // the same frame as a NULL frame holds the previous values: it adds nothing
            CHECK(classify(frames, nulls) == 0u); HIT(kNullFrameIgnored);
        }
    }
    // -0.0 everywhere is as dead as +0.0; every bit from a frame of its own
    { Frame z = d; for (int q : {23, 38, 39, 40, 41, 42}) z.p[q] = -0.0; CHECK(classify({z, d, z}, {false, false, false}) == 0u); }
    CHECK(classify({with(38, 0.1), with(39, 0.1), d, with(40, 0.1), with(41, 0.1), with(42, 0.1), with(23, 0.1)}, std::vector<bool>(7, false)) == kUtt2Present);
    // a QUIET list (no noise gain) keeps the nasal fact in the second word whatever becomes of UTT_NO_NASAL, and a noisy one has it at all
    {
        Frame q = d; q.p[3] = q.p[6] = q.p[24] = 0.0;
        uint32_t fl = 0;
        CHECK(classify({q, q}, {false, false}, &fl) == 0u && fl == (UTT_NO_NASAL | UTT_PARALLEL1));
        Frame qn = q; qn.p[23] = 0.3;
        CHECK(classify({q, qn}, {false, false}, &fl) == UTT2_NASAL && !(fl & (UTT_NO_NASAL | UTT_NEEDS_NOISE)));
        CHECK(classify({d, d}, {false, false}, &fl) == 0u && (fl & UTT_NEEDS_NOISE) && !(fl & UTT_NO_NASAL));      // noisy: classify_list's first word drops the fact
    }
}

// ListTable.present2 is what every utterance of the list is handed: no step of the routing touches the word, and it changes no step
static void through_the_routing()
{
    ListTable lists;
    // 0: noisy, gets tracks; 1: noisy, gets tracks; 2: noisy, direct; 3: quiet and lonely, re-routed and tracked; 4: quiet and lonely, re-routed, gets nothing:
    // restored; 5..: quiet lists of one timing
    const uint32_t in[5] = {UTT_NEEDS_NOISE | UTT_PARALLEL1, UTT_NEEDS_NOISE, UTT_NEEDS_NOISE | UTT_TURBULENCE, UTT_NO_NASAL | UTT_PARALLEL1, UTT_PARALLEL1 | UTT_ASPIRATION};
    const uint32_t word[5] = {UTT2_NASAL | UTT2_PARALLEL5, 0u, kUtt2Present, UTT2_PARALLEL2 | UTT2_PARALLEL6, UTT2_NASAL};
    for (int l = 0; l < 5; ++l) { lists.flags.push_back(in[l]); lists.present2.push_back(word[l]); lists.lens.push_back(1000u + (uint32_t)l); lists.timing.push_back(100ull + (unsigned long long)l); lists.shape.push_back(3); lists.weight.push_back(1u); }
    for (int l = 0; l < 40; ++l) { lists.flags.push_back(UTT_NO_NASAL); lists.present2.push_back(0u); lists.lens.push_back(5000u); lists.timing.push_back(7ull); lists.shape.push_back(3); lists.weight.push_back(1u); }
    ListTable bare = lists;      // the same lists with an empty second word: every step must decide the same
    std::fill(bare.present2.begin(), bare.present2.end(), 0u);
    const std::vector<uint32_t> before = lists.present2;
    RouteOptions o;
    o.nFrames = 1000;
    const Rerouted rerouted = reroute_lonely_quiet(lists, o), reroutedBare = reroute_lonely_quiet(bare, o);
    CHECK(rerouted == reroutedBare && rerouted.size() == 2 && lists.flags == bare.flags);
    CHECK(!(lists.flags[3] & UTT_NO_NASAL) && lists.present2 == before); HIT(kRerouted);      // the first word lost the nasal fact; the second has it (dead: bit clear)
    std::vector<unsigned char> eligible = eligible_lists(lists, o);
    CHECK(eligible == eligible_lists(bare, o));
    eligible[4] = 0;
    std::vector<unsigned char> tracked(lists.flags.size(), 0);
    std::vector<uint32_t> kinds(lists.flags.size(), 0);
    tracked[0] = tracked[1] = tracked[3] = 1; kinds[0] = 0xABCDEFu; kinds[1] = 0x1u; kinds[3] = 0xFFFFFFu;
    mark_tracked(lists, tracked.data(), kinds.data()); mark_tracked(bare, tracked.data(), kinds.data());
    CHECK(lists.flags == bare.flags && lists.present2 == before && (lists.flags[3] & UTT_TRACKED)); HIT(kTrackedKeeps);
    o.direct = 2;
    CHECK(route_direct(lists, eligible.data(), o) == route_direct(bare, eligible.data(), o));
    CHECK(lists.flags == bare.flags && (lists.flags[2] & UTT_DIRECT) && lists.present2 == before); HIT(kDirectKeeps);
    restore_rerouted(lists, rerouted); restore_rerouted(bare, reroutedBare);
    CHECK(lists.flags == bare.flags && lists.flags[4] == in[4] && lists.present2 == before); HIT(kRestored);
    // the packing reads the first word alone: the same order, and the word of the utterance in every slot is its list's
    std::vector<uint32_t> lens(lists.flags.size(), 1000u);
    std::vector<unsigned long long> timing(lists.flags.size(), 1ull);
    const LanePacking a = pack_lanes((long long)lists.flags.size(), [&](uint32_t u) { return lists.flags[u]; }, lens.data(), timing.data(), true);
    const LanePacking c = pack_lanes((long long)bare.flags.size(), [&](uint32_t u) { return bare.flags[u]; }, lens.data(), timing.data(), true);
    CHECK(a.order == c.order && a.nQuiet == c.nQuiet && a.nTracked == c.nTracked && a.nDirectSlots == c.nDirectSlots && lists.present2 == before); HIT(kPackingSame);
    // the tracked group's one wavefront holds lists 0, 1, 3 (sparse: replicas): what the plan says of it
    long long n[kDead2Counts];
    dead2_wave_counts(a.order.data(), a.nQuietSlots, a.nTracked, [&](uint32_t u) { return lists.flags[u]; }, [&](uint32_t u) { return lists.present2[u]; }, 120, n);
    CHECK(n[0] == 0 && n[1] == 0 && n[2] == 0 && n[3] == 0);      // nasal in list 0, parallel 5 in 0, parallel 1 in 0 and 3
}

// dead2_wave_counts: what the plan says the stages will decide, wavefront by wavefront (width 4 here), for every value of the built mask
static void the_plan_counts_wavefronts()
{
    const uint32_t T = UTT_TURBULENCE, P1 = UTT_PARALLEL1, N = kNoUtt;
    const uint32_t P2 = UTT2_PARALLEL2, P4 = UTT2_PARALLEL4, P5 = UTT2_PARALLEL5, P6 = UTT2_PARALLEL6, NA = UTT2_NASAL;
    // utterance:             0    1    2    3    4    5        6             7
    const uint32_t flags[8] = {0u, 0u, T, P1, 0u, 0u, 0u, T | P1 | UTT_ASPIRATION};
    const uint32_t word[8] = {0u, NA, 0u, 0u, P5, P6, P2 | P4, kUtt2Present};
    auto flagsOf = [&](uint32_t u) { return flags[u]; };
    auto wordOf = [&](uint32_t u) { return word[u]; };
    // two quiet slots in front (everything present: not counted), then
    //   A all dead | B nasal in a replica lane | C turbulence alone | D parallel 1 alone | E parallel 5 | F parallel 6 | G parallel 2 and 4 | H empty | I one dead lane, the group ends
    const uint32_t order[] = {7, 7, /*A*/ 0, 0, 0, 0, /*B*/ 0, 1, 0, 1, /*C*/ 2, 0, 0, N, /*D*/ 0, 3, N, N, /*E*/ 4, 0, 0, 0, /*F*/ 0, 5, 0, 0, /*G*/ 6, 0, N, N, /*H*/ N, N, N, N, /*I*/ 0, N};
    const long long nSlots = (long long)(sizeof order / sizeof order[0]) - 2;
    //                    A  B  C  D  E  F  G  I
    const int nasal[8] = {1, 0, 0, 1, 1, 1, 1, 1};      // [0]: needs turbulence dead too
    const int no5[8]   = {1, 1, 1, 1, 0, 1, 1, 1};
    const int no56[8]  = {1, 1, 1, 1, 0, 0, 1, 1};
    const int none[8]  = {1, 1, 1, 0, 1, 1, 0, 1};      // [3]: needs parallel 1 dead too
    long long c[kDead2Counts];
    for (int built = 0; built < 128; ++built) {
        dead2_wave_counts(order, 2, nSlots, flagsOf, wordOf, built, c, 4);
        long long want[kDead2Counts] = {0, 0, 0, 0};
        for (int w = 0; w < 8; ++w) {
            const int fin = ((built & 32) && no56[w]) ? 2 : (((built & 16) && no5[w]) ? 1 : 0);
            want[0] += (built & 8) ? nasal[w] : 0;
            want[1] += fin >= 1; want[2] += fin >= 2;
            want[3] += (built & 64) ? none[w] : 0;
        }
        for (int k = 0; k < kDead2Counts; ++k) CHECK(c[k] == want[k]);
        HIT(kEveryMask);
        // the first word's counts do not depend on the new bits of the mask
        long long c3[3], c3b[3];
        dead_wave_counts(order, 2, nSlots, flagsOf, built, c3, 4);
        dead_wave_counts(order, 2, nSlots, flagsOf, built & 7, c3b, 4);
        CHECK(c3[0] == c3b[0] && c3[1] == c3b[1] && c3[2] == c3b[2]);
    }
    dead2_wave_counts(order, 2, nSlots, flagsOf, wordOf, 120, c, 4);
    CHECK(c[0] == 6 && c[1] == 7 && c[2] == 6 && c[3] == 6); HIT(kPlanCounts);      // written out: nasal A D E F G I; no 5: all but E; no 5, 6: but E, F; none: but D, G
    dead2_wave_counts(order, 2, nSlots, flagsOf, wordOf, 32, c, 4);      // without the body for parallel 5 alone, F keeps the general one
    CHECK(c[0] == 0 && c[1] == 6 && c[2] == 6 && c[3] == 0);
    dead2_wave_counts(order, 2, 0, flagsOf, wordOf, 127, c, 4);
    CHECK(c[0] == 0 && c[1] == 0 && c[2] == 0 && c[3] == 0);
}

int main()
{
    the_rules_frame_by_frame();
    the_list_level_or();
    through_the_routing();
    the_plan_counts_wavefronts();
    printf("ok %lld checks\n", g_checks);
    bool all = true;
    for (int i = 0; i < kBranches; ++i) {
        printf("  %s: %lld\n", kBranchNames[i], g_hits[i]);
        all = all && g_hits[i] > 0;
    }
    if (!all) { printf("FAILED: a branch was never reached\n"); return 1; }
    return 0;
}
