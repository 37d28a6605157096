// check_dead_terms.cpp -- the three "present" facts of a frame (nvspeechplayer_amd/csrc/klatt_plan.h, shape_flags: turbulence, aspiration,
// parallel resonator 1), each side of every rule on hand-written frames, their OR over a frame list and their way into UttDesc.flags
// through the routing (klatt_batchplan.h: classify_list, reroute_lonely_quiet, mark_tracked, route_direct, restore_rerouted).
// Built with AddressSanitizer + UBSan by tests/test_dead_terms_host.py; prints "ok <checks>" and how often each branch below was
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

enum Branch { kAllDead, kTurbulenceSet, kAspirationSet, kAmplitudeSet, kBandwidthLow, kBandwidthHigh, kFrequencyFar, kGainFar, kNotANumber,
              kOffenderInTheMiddle, kNullFrameIgnored, kRerouted, kRestored, kTrackedKeeps, kDirectKeeps, kPlanCounts, kBranches };
static const char* const kBranchNames[kBranches] = {
    "every term dead", "turbulence present", "aspiration present", "pa1 non-zero", "pb1 below 1", "pb1 above 1e6", "pf1 beyond 1e6",
    "a gain beyond 1e30", "a NaN keeps the term", "one offending frame in the middle of a list", "a NULL frame adds nothing",
    "a re-routed quiet list keeps its bits", "a restored list keeps its bits", "a tracked list keeps its bits", "a direct list keeps its bits", "the plan's wavefront counts"};
static long long g_hits[kBranches];
#define HIT(b) (++g_hits[b])

constexpr double kMaxF = 1e300, kMaxBw = 1e300;      // (the direct stages' bounds: not what this program is about)
constexpr uint32_t kPresent = FACT_TURBULENCE | FACT_ASPIRATION | FACT_PARALLEL1;

struct Frame { double p[kNumParams]; };

// a speech-like frame in which all three terms are dead
static Frame dead_frame()
{
    Frame f;
    for (double& v : f.p) v = 0.0;
    f.p[0] = 120.0; f.p[46] = 110.0;
    f.p[4] = 0.5; f.p[5] = 1.0;
    const double cf[8] = {700, 1200, 2600, 3300, 3750, 4900, 450, 270}, cb[8] = {90, 100, 150, 250, 200, 1000, 100, 100};
    for (int i = 0; i < 8; ++i) { f.p[7 + i] = cf[i]; f.p[15 + i] = cb[i]; }
    f.p[24] = 0.3;
    const double pf[6] = {720, 1250, 2500, 3400, 3800, 4800}, pb[6] = {80, 110, 160, 240, 210, 900}, pa[6] = {0.0, 0.45, 0.4, 0.35, 0.3, 0.25};
    for (int i = 0; i < 6; ++i) { f.p[25 + i] = pf[i]; f.p[31 + i] = pb[i]; f.p[37 + i] = pa[i]; }
    f.p[43] = 0.3; f.p[44] = 1.0; f.p[45] = 0.6;
    return f;
}
static uint32_t present(const Frame& f) { return shape_flags(f.p, kMaxF, kMaxBw) & kPresent; }
static Frame with(int param, double v) { Frame f = dead_frame(); f.p[param] = v; return f; }

static void the_rules_frame_by_frame()
{
    CHECK(present(dead_frame()) == 0u); HIT(kAllDead);
    // frame_facts carries what shape_flags says (the device classification and the record form go through the same two functions)
    { const Frame f = with(3, 0.25); CHECK((frame_facts(f.p, kMaxF, kMaxBw).flags & kPresent) == FACT_TURBULENCE); }
    CHECK((frame_facts(dead_frame().p, kMaxF, kMaxBw).flags & kPresent) == 0u);
    // parameters 3 and 6: bit-for-bit +0.0 or present
    const double denormal = 4.9406564584124654e-324;
    for (const double v : {-0.0, denormal, -denormal, 1e-300, 0.2, (double)NAN, (double)INFINITY}) {
        CHECK(present(with(3, v)) == FACT_TURBULENCE); HIT(kTurbulenceSet);
        CHECK(present(with(6, v)) == FACT_ASPIRATION); HIT(kAspirationSet);
        if (v != v) HIT(kNotANumber);
    }
    CHECK(present(with(3, 0.0)) == 0u && present(with(6, 0.0)) == 0u);
    { Frame f = with(3, 0.1); f.p[6] = -0.0; CHECK(present(f) == (FACT_TURBULENCE | FACT_ASPIRATION)); }
    // pa1 (parameter 37): zero of either sign is dead, anything else -- a NaN too -- is present
    CHECK(present(with(37, 0.0)) == 0u && present(with(37, -0.0)) == 0u);
    for (const double v : {1e-300, -1e-300, denormal, 0.5, (double)NAN}) { CHECK(present(with(37, v)) == FACT_PARALLEL1); HIT(kAmplitudeSet); }
    // pb1 (parameter 31) in [1, 1e6]
    CHECK(present(with(31, 1.0)) == 0u && present(with(31, 1e6)) == 0u);
    for (const double v : {0.999, 0.0, -80.0}) { CHECK(present(with(31, v)) == FACT_PARALLEL1); HIT(kBandwidthLow); }
    for (const double v : {1.0000001e6, 1e300, (double)INFINITY}) { CHECK(present(with(31, v)) == FACT_PARALLEL1); HIT(kBandwidthHigh); }
    CHECK(present(with(31, NAN)) == FACT_PARALLEL1); HIT(kNotANumber);
    // |pf1| (parameter 25) <= 1e6
    CHECK(present(with(25, 1e6)) == 0u && present(with(25, -1e6)) == 0u && present(with(25, 0.0)) == 0u);
    for (const double v : {1.0000001e6, -1.0000001e6, (double)INFINITY, (double)NAN}) { CHECK(present(with(25, v)) == FACT_PARALLEL1); HIT(kFrequencyFar); }
    // |fricationAmplitude| (24) and |preFormantGain| (44) <= 1e30
    for (const int g : {24, 44}) {
        CHECK(present(with(g, 1e30)) == 0u && present(with(g, -1e30)) == 0u && present(with(g, 0.0)) == 0u);
        for (const double v : {1.0000001e30, -1.0000001e30, (double)INFINITY, (double)NAN}) { CHECK(present(with(g, v)) == FACT_PARALLEL1); HIT(kGainFar); }
    }
    // the other parallel resonators and amplitudes are not this rule's business
    for (const int q : {26, 32, 38, 42, 43}) CHECK(present(with(q, 12345.0)) == 0u);
    // ... and the older facts are what they were
    CHECK((shape_flags(dead_frame().p, kMaxF, kMaxBw) & ~kPresent) == (FACT_NOISE | 0u));      // frication 0.3: noisy; caNP 0 with stable N0 / NP: nasal-free
    CHECK((shape_flags(with(23, 0.5).p, kMaxF, kMaxBw) & ~kPresent) == (FACT_NOISE | FACT_NASAL));
}

struct Meta { uint32_t minSamples, fadeSamples, flags; };
struct Facts { uint32_t flags; };

static uint32_t classify(const std::vector<Frame>& frames, const std::vector<bool>& isNull)
{
    std::vector<Meta> meta;
    std::vector<Facts> facts;
    for (size_t k = 0; k < frames.size(); ++k) {
        meta.push_back(Meta{600u, 100u, isNull[k] ? FRAME_NULL : 0u});
        // (a NULL frame's values are whatever the caller left there: here the worst)
        facts.push_back(Facts{frame_facts(frames[k].p, kMaxF, kMaxBw).flags});
    }
    uint32_t flags = 0;
    unsigned char shape = 0;
    classify_list(meta.data(), facts.data(), (long long)frames.size(), flags, shape);
    return flags;
}

static void the_list_level_or()
{
    const Frame d = dead_frame();
    CHECK((classify({d, d, d, d, d}, {false, false, false, false, false}) & kUttPresent) == 0u);
    CHECK((classify({}, {}) & kUttPresent) == 0u);
    const struct { int param; double v; uint32_t bit; } offenders[] = {
        {3, 1e-300, UTT_TURBULENCE}, {6, -0.0, UTT_ASPIRATION}, {37, 1e-300, UTT_PARALLEL1}, {31, 0.999, UTT_PARALLEL1}, {25, 2e6, UTT_PARALLEL1}, {44, 2e30, UTT_PARALLEL1}};
    for (const auto& o : offenders) {
        const Frame bad = with(o.param, o.v);
        for (size_t at = 0; at < 5; ++at) {
            std::vector<Frame> frames(5, d);
            frames[at] = bad;
            std::vector<bool> nulls(5, false);
            const uint32_t fl = classify(frames, nulls);
            CHECK((fl & kUttPresent) == o.bit && (fl & UTT_NEEDS_NOISE));
            if (at == 2) HIT(kOffenderInTheMiddle);
            // the same frame as a NULL frame holds the previous values: it adds nothing
            nulls[at] = true;
            CHECK((classify(frames, nulls) & kUttPresent) == 0u); HIT(kNullFrameIgnored);
        }
    }
    // all three from three different frames
    CHECK((classify({with(3, 0.1), d, with(6, 0.1), with(37, 0.1)}, {false, false, false, false}) & kUttPresent) == kUttPresent);
    // the bits and the entry kinds do not overlap, and the routing's own bits are where they were
    static_assert((kUttPresent & (UTT_NEEDS_NOISE | UTT_NO_NASAL | UTT_TRACKED | UTT_DIRECT)) == 0u && kUttPresent == 0x70u && (kUttPresent >> kUttKindShift) == 0u, "bits 4..6");
}

// lists.flags is what every utterance of the list carries as UttDesc.flags: the bits survive every step of the routing
static void through_the_routing()
{
    ListTable lists;
    // 0: noisy, parallel 1 present, gets tracks; 1: noisy, all dead, gets tracks; 2: noisy, turbulence, direct; 3: quiet and lonely, pa1 set, re-routed and
    // tracked; 4: quiet and lonely, re-routed, gets nothing: restored; 5..: quiet lists of one timing
    const uint32_t in[5] = {UTT_NEEDS_NOISE | UTT_PARALLEL1, UTT_NEEDS_NOISE, UTT_NEEDS_NOISE | UTT_TURBULENCE, UTT_NO_NASAL | UTT_PARALLEL1, UTT_PARALLEL1 | UTT_ASPIRATION};
    for (int l = 0; l < 5; ++l) { lists.flags.push_back(in[l]); lists.lens.push_back(1000u + (uint32_t)l); lists.timing.push_back(100ull + (unsigned long long)l); lists.shape.push_back(3); lists.weight.push_back(1u); }
    for (int l = 0; l < 40; ++l) { lists.flags.push_back(UTT_NO_NASAL); lists.lens.push_back(5000u); lists.timing.push_back(7ull); lists.shape.push_back(3); lists.weight.push_back(1u); }
    RouteOptions o;
    o.nFrames = 1000;
    const Rerouted rerouted = reroute_lonely_quiet(lists, o);
    CHECK(rerouted.size() == 2 && rerouted[0].first == 3 && rerouted[1].first == 4);
    CHECK(lists.flags[3] == (UTT_NEEDS_NOISE | UTT_PARALLEL1) && lists.flags[4] == (UTT_NEEDS_NOISE | UTT_PARALLEL1 | UTT_ASPIRATION)); HIT(kRerouted);
    std::vector<unsigned char> eligible = eligible_lists(lists, o);
    CHECK(eligible[0] == 3 && eligible[3] == 3 && eligible[5] == 0);
    eligible[4] = 0;      // (as a list with a non-finite parameter would be: neither tracks nor direct stages)
    std::vector<unsigned char> tracked(lists.flags.size(), 0);
    std::vector<uint32_t> kinds(lists.flags.size(), 0);
    tracked[0] = tracked[1] = tracked[3] = 1; kinds[0] = 0xABCDEFu; kinds[1] = 0x1u; kinds[3] = 0xFFFFFFu;
    mark_tracked(lists, tracked.data(), kinds.data());
    CHECK(lists.flags[0] == (UTT_NEEDS_NOISE | UTT_PARALLEL1 | UTT_TRACKED | (0xABCDEFu << kUttKindShift)));
    CHECK(lists.flags[1] == (UTT_NEEDS_NOISE | UTT_TRACKED | (0x1u << kUttKindShift)));
    CHECK(lists.flags[3] == (UTT_NEEDS_NOISE | UTT_PARALLEL1 | UTT_TRACKED | (0xFFFFFFu << kUttKindShift))); HIT(kTrackedKeeps);
    o.direct = 2;
    route_direct(lists, eligible.data(), o);
    CHECK(lists.flags[2] == (UTT_NEEDS_NOISE | UTT_TURBULENCE | UTT_DIRECT)); HIT(kDirectKeeps);
    restore_rerouted(lists, rerouted);
    CHECK(lists.flags[4] == in[4] && (lists.flags[3] & UTT_TRACKED)); HIT(kRestored);
    // and the packing reads the groups from the same words: the bits change no utterance's group
    std::vector<uint32_t> lens(lists.flags.size(), 1000u);
    std::vector<unsigned long long> timing(lists.flags.size(), 1ull);
    const LanePacking with_bits = pack_lanes((long long)lists.flags.size(), [&](uint32_t u) { return lists.flags[u]; }, lens.data(), timing.data(), true);
    const LanePacking without = pack_lanes((long long)lists.flags.size(), [&](uint32_t u) { return lists.flags[u] & ~kUttPresent; }, lens.data(), timing.data(), true);
    CHECK(with_bits.order == without.order && with_bits.nQuiet == without.nQuiet && with_bits.nTracked == without.nTracked && with_bits.nDirectSlots == without.nDirectSlots);
}

// dead_wave_counts: what the plan says the stages will decide, wavefront by wavefront (width 4 here)
static void the_plan_counts_wavefronts()
{
    const uint32_t T = UTT_TURBULENCE, A = UTT_ASPIRATION, P = UTT_PARALLEL1, N = kNoUtt;
    const uint32_t flags[8] = {0u, P, T, A, T | A | P, A | P, UTT_NEEDS_NOISE | UTT_TRACKED | (0xFFFFFFu << kUttKindShift), T | P};
    auto flagsOf = [&](uint32_t u) { return flags[u]; };
    // two quiet slots in front, then: all dead | dead + a replica | one lane with parallel 1 | aspiration only | empty | turbulence in a sparse wavefront
    const uint32_t order[] = {7, 7, /**/ 0, 6, 0, 6, /**/ 0, 0, 0, N, /**/ 0, 1, 6, 0, /**/ 3, 0, 3, N, /**/ N, N, N, N, /**/ 2, N};
    long long c[3];
    dead_wave_counts(order, 2, 22, flagsOf, 7, c, 4);
    CHECK(c[0] == 4 && c[1] == 4 && c[2] == 3); HIT(kPlanCounts);
    dead_wave_counts(order, 2, 22, flagsOf, 3, c, 4);      // without the body that drops the generator: such a wavefront still drops turbulence
    CHECK(c[0] == 4 && c[1] == 4 && c[2] == 0);
    dead_wave_counts(order, 2, 22, flagsOf, 5, c, 4);      // without the turbulence-only body: aspiration present keeps the general one
    CHECK(c[0] == 4 && c[1] == 3 && c[2] == 3);
    dead_wave_counts(order, 2, 22, flagsOf, 0, c, 4);
    CHECK(c[0] == 0 && c[1] == 0 && c[2] == 0);
    dead_wave_counts(order, 2, 0, flagsOf, 7, c, 4);
    CHECK(c[0] == 0 && c[1] == 0 && c[2] == 0);
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
