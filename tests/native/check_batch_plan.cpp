// check_batch_plan.cpp -- the set call's host planning (nvspeechplayer_amd/csrc/klatt_batchplan.h: per-list length, timing and class,
// the routing, lane packing) against the rules as its comments state them, restated by brute force, and against small cases whose
// expected order is written out.  Built with AddressSanitizer + UBSan by tests/test_host_logic.py; prints "ok <checks>" or the first failure.
#include "../../nvspeechplayer_amd/csrc/klatt_batchplan.h"

#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <random>

using namespace klatt;

static long long g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

// the branches of the packing and the routing that the inputs must reach: one hit zero times fails the run
enum Branch { kLongRunEndsWavefront, kQuarterEndsWavefront, kAllGroups, kOnlyDirect, kTrackedDirectUnsorted, kSparseGroup, kHalfFullGroup,
              kOneQuietTiming, kRerouted, kRestored, kTracksDropped, kDirectAligned, kBranches };
static const char* const kBranchNames[kBranches] = {
    "a run of a wavefront or more follows a partly filled wavefront", "a run filled a quarter or more of its last wavefront", "every group at once",
    "only the direct group", "tracked plus direct without sort", "a sparse group", "a group of half a wavefront or more, less than one",
    "all quiet, one timing", "a lonely quiet list re-routed", "a re-routed list back with the quiet ones", "tracks dropped for the direct stages",
    "direct candidates aligned"};
static long long g_hits[kBranches];

constexpr uint32_t N = kNoUtt;
enum Group { kNoNasal, kQuiet, kTracked, kDirect, kUntracked, kGroups };
static const uint32_t kGroupFlags[kGroups] = {UTT_NO_NASAL, 0u, UTT_NEEDS_NOISE | UTT_TRACKED | (5u << kUttKindShift), UTT_NEEDS_NOISE | UTT_DIRECT, UTT_NEEDS_NOISE};
static Group group_of(uint32_t flags)
{
    if (!(flags & UTT_NEEDS_NOISE)) return (flags & UTT_NO_NASAL) ? kNoNasal : kQuiet;
    return (flags & UTT_TRACKED) ? kTracked : (flags & UTT_DIRECT) ? kDirect : kUntracked;
}

struct Utts { std::vector<uint32_t> flags, lens; std::vector<unsigned long long> timing; };

static LanePacking pack(const Utts& u, bool sorted, int width)
{
    return pack_lanes((long long)u.flags.size(), [&](uint32_t x) { return u.flags[x]; }, u.lens.data(), u.timing.data(), sorted, width);
}

// the eight rules of the packing, by brute force over the finished order
static void check_packing(const Utts& u, bool sorted, int W)
{
    const LanePacking p = pack(u, sorted, W);
    const long long nU = (long long)u.flags.size(), nSlots = (long long)p.order.size();
    long long count[kGroups] = {0, 0, 0, 0, 0};
    for (uint32_t f : u.flags) ++count[group_of(f)];
    CHECK(p.nNoNasal == count[kNoNasal] && p.nQuiet == count[kNoNasal] + count[kQuiet] && p.nTrackedUtt == count[kTracked]);
    // the slot counts add up: the five groups' slots, in this order, are the whole order
    const long long start[kGroups + 1] = {0, p.nNoNasalSlots, p.nQuietSlots, p.nQuietSlots + p.nTracked, p.nQuietSlots + p.nTracked + p.nDirectSlots, nSlots};
    for (int g = 0; g < kGroups; ++g) CHECK(start[g] <= start[g + 1] && (start[g] < start[g + 1]) == (count[g] > 0));
    // each noisy group starts on a wavefront boundary (the noisy wavefronts count from the end of the quiet groups) and the last ends on one
    // (except without the sort and without a direct group: there the untracked utterances follow the tracked ones at once, and a
    // sparse last wavefront that holds both repeats both)
    const bool merged = !sorted && count[kDirect] == 0 && count[kTracked] > 0 && count[kUntracked] > 0;
    for (int g = kTracked; g < kGroups; ++g) CHECK(count[g] == 0 || (merged && g == kUntracked) || (start[g] - start[kTracked]) % W == 0);
    CHECK((nSlots - start[kTracked]) % W == 0);
    std::vector<std::vector<long long>> slotsOf((size_t)nU);
    for (int g = 0; g < kGroups; ++g) {
        const long long base = g < kTracked ? start[g] : start[kTracked];      // where the group's wavefronts count from
        uint32_t prev = N;      // the utterance before, among those met for the first time
        std::map<std::pair<unsigned long long, uint32_t>, long long> runSize;      // (timing, length) -> utterances of the group
        for (long long x = 0; x < nU; ++x) if (group_of(u.flags[(size_t)x]) == g) ++runSize[{u.timing[(size_t)x], u.lens[(size_t)x]}];
        for (long long s = start[g]; s < start[g + 1]; ++s) {
            const uint32_t x = p.order[(size_t)s];
            if (x == N) { CHECK(g >= kTracked); continue; }      // empty slots only in the noisy groups
            CHECK((long long)x < nU);
            const bool first = slotsOf[x].empty();
            CHECK(group_of(u.flags[x]) == g || (merged && !first && g == kUntracked && group_of(u.flags[x]) == kTracked));      // the groups in their order
            // a replica names an utterance that is live in the same wavefront
            if (!first) CHECK((slotsOf[x][0] - base) / W == (s - base) / W && slotsOf[x][0] >= start[merged && g == kUntracked ? kTracked : g]);
            slotsOf[x].push_back(s);
            if (!first || !sorted) continue;
            if (prev != N) {
                // lengths never increase, equal lengths are ordered by timing
                CHECK(u.lens[prev] > u.lens[x] || (u.lens[prev] == u.lens[x] && u.timing[prev] <= u.timing[x]));
                const bool sameRun = u.lens[prev] == u.lens[x] && u.timing[prev] == u.timing[x];
                const long long w0 = base + (s - base) / W * W;
                if (!sameRun && (g == kTracked || g == kUntracked) && slotsOf[prev][0] >= w0) {
                    // two runs in one wavefront: the earlier one filled less than a quarter of it, this one is shorter than a wavefront
                    long long lanesOfPrev = 0;
                    for (long long t = w0; t < s; ++t) {
                        const uint32_t y = p.order[(size_t)t];
                        lanesOfPrev += y != N && u.lens[y] == u.lens[prev] && u.timing[y] == u.timing[prev];
                    }
                    CHECK(lanesOfPrev < W / 4 && (runSize[{u.timing[x], u.lens[x]}]) < W);
                }
                if (!sameRun && (g == kTracked || g == kUntracked) && slotsOf[prev][0] < w0 && (s - base) % W == 0 && (slotsOf[prev][0] - base) % W != W - 1) {
                    // ... and where a run does end its wavefront early, the rule gives the reason
                    long long lanesOfPrev = 0;
                    const long long wp = base + (slotsOf[prev][0] - base) / W * W;
                    for (long long t = wp; t <= slotsOf[prev][0]; ++t) {
                        const uint32_t y = p.order[(size_t)t];
                        lanesOfPrev += y != N && u.lens[y] == u.lens[prev] && u.timing[y] == u.timing[prev];
                    }
                    const bool longRun = runSize[{u.timing[x], u.lens[x]}] >= W;
                    CHECK(lanesOfPrev >= W / 4 || longRun);
                    ++g_hits[lanesOfPrev >= W / 4 ? kQuarterEndsWavefront : kLongRunEndsWavefront];
                }
            }
            prev = x;
        }
    }
    for (long long x = 0; x < nU; ++x) CHECK(!slotsOf[(size_t)x].empty());      // every utterance occupies at least one slot
    // an empty slot never sits in a wavefront with fewer than half its lanes live; a quiet group's last wavefront is never sparse
    for (long long w = start[kTracked]; w < nSlots; w += W) {
        long long live = 0, empty = 0;
        for (long long s = w; s < w + W; ++s) { CHECK(s < nSlots); (p.order[(size_t)s] == N ? empty : live) += 1; }
        CHECK(empty == 0 || live >= W / 2);
    }
    for (int g = 0; g < kTracked; ++g) CHECK((start[g + 1] - start[g]) % W == 0 || (start[g + 1] - start[g]) % W >= W / 2);
    // which branches this batch reached
    bool all = true;
    for (int g = 0; g < kGroups; ++g) {
        all = all && count[g] > 0;
        if (count[g] % W > 0 && count[g] % W < W / 2) ++g_hits[kSparseGroup];
        if (count[g] >= W / 2 && count[g] < W) ++g_hits[kHalfFullGroup];
    }
    if (all) ++g_hits[kAllGroups];
    if (count[kDirect] == nU && nU > 0) ++g_hits[kOnlyDirect];
    if (!sorted && count[kTracked] > 0 && count[kDirect] > 0) ++g_hits[kTrackedDirectUnsorted];
}

static void check_literal(const std::vector<uint32_t>& groups, const std::vector<uint32_t>& lens, const std::vector<unsigned long long>& timing, bool sorted,
                          const std::vector<uint32_t>& order, long long nNoNasalSlots, long long nQuietSlots, long long nTracked, long long nDirectSlots)
{
    Utts u;
    for (uint32_t g : groups) u.flags.push_back(kGroupFlags[g]);
    u.lens = lens; u.timing = timing;
    const LanePacking p = pack(u, sorted, 8);
    CHECK(p.order == order);
    CHECK(p.nNoNasalSlots == nNoNasalSlots && p.nQuietSlots == nQuietSlots && p.nTracked == nTracked && p.nDirectSlots == nDirectSlots);
    check_packing(u, sorted, 8);
}

// Width 8: a quarter of a wavefront is 2 lanes, a sparse one has fewer than 4 live.
static void check_literals()
{
    const uint32_t Q = kQuiet, NN = kNoNasal, T = kTracked, D = kDirect, U = kUntracked;
    // all different: packed densely, the sparse wavefront repeats its utterances
    check_literal({U, U, U}, {30, 20, 10}, {1, 2, 3}, true, {0, 1, 2, 0, 1, 2, 0, 1}, 0, 0, 0, 0);
    // a run of 3 filled a quarter of its wavefront: the next run starts its own
    check_literal({U, U, U, U, U, U, U, U}, {50, 50, 50, 40, 40, 40, 40, 40}, {7, 7, 7, 9, 9, 9, 9, 9}, true,
                  {0, 1, 2, 0, 1, 2, 0, 1, 3, 4, 5, 6, 7, N, N, N}, 0, 0, 0, 0);
    // a run of 1 filled less than a quarter, but a run of a whole wavefront follows; the untracked utterance starts its own wavefront
    check_literal({T, T, T, T, T, T, T, T, T, U}, {90, 50, 50, 50, 50, 50, 50, 50, 50, 10}, {1, 2, 2, 2, 2, 2, 2, 2, 2, 3}, true,
                  {0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 9, 9, 9, 9, 9}, 0, 0, 16, 0);
    // a run of 1, then a run of 3: both in one wavefront, which is half full and keeps its empty lanes
    check_literal({U, U, U, U}, {90, 50, 50, 50}, {1, 2, 2, 2}, true, {0, 1, 2, 3, N, N, N, N}, 0, 0, 0, 0);
    // every group at once, each of one utterance
    check_literal({Q, NN, T, D, U}, {10, 10, 10, 10, 10}, {1, 1, 1, 1, 1}, true,
                  {1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4}, 8, 16, 8, 8);
    // tracked plus direct without sort: the order of the call within a group, the last wavefront's dead lanes go to the direct group
    check_literal({D, T, T, Q}, {10, 20, 30, 40}, {1, 2, 3, 4}, false, {3, 3, 3, 3, 3, 3, 3, 3, 1, 2, 1, 2, 1, 2, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0}, 0, 8, 8, 8);
    // ... with untracked utterances behind them, and no tracked ones
    check_literal({U, D, U}, {10, 20, 30}, {1, 2, 3}, false, {1, 1, 1, 1, 1, 1, 1, 1, 0, 2, 0, 2, 0, 2, 0, 2}, 0, 0, 0, 8);
    // only the direct group: longest first
    check_literal({D, D, D}, {10, 30, 20}, {1, 2, 3}, true, {1, 2, 0, 1, 2, 0, 1, 2}, 0, 0, 0, 8);
    // equal lengths by timing, in the order of the call where that is equal too; five of eight lanes are not sparse
    check_literal({Q, Q, Q, Q, Q}, {10, 10, 10, 10, 10}, {5, 3, 9, 3, 1}, true, {4, 1, 3, 0, 2}, 0, 5, 0, 0);
    // nothing at all
    check_literal({}, {}, {}, true, {}, 0, 0, 0, 0);
}

struct Meta { uint32_t minSamples, fadeSamples; int32_t userIndex; uint32_t flags; };
struct Facts { uint32_t flags; };

static void check_lists()
{
    const Meta m[4] = {{100, 10, -1, 0}, {5, 10, -1, 0}, {0, 1, -1, FRAME_NULL}, {0xFFFFFFFFu, 0xFFFFFFFFu, -1, 0}};
    uint32_t len = 7;
    CHECK(list_length(m, 0, len) && len == 0);
    CHECK(list_length(m, 3, len) && len == 101 + 12 + 3);      // max(min, fade + 1) + 1 each
    CHECK(!list_length(m, 4, len) && len == 0);                // 2^32 + 1 more samples: too long
    CHECK(list_timing(m, 3) == list_timing(m, 3) && list_timing(m, 2) != list_timing(m, 3) && list_timing(m, 0) != list_timing(m, 1));
    Meta other[3] = {m[0], m[1], m[2]};
    other[1].userIndex = 9;      // an index mark is no part of the timing; a silence, a duration and a fade are
    CHECK(list_timing(other, 3) == list_timing(m, 3));
    other[2].flags = 0;
    CHECK(list_timing(other, 3) != list_timing(m, 3));
    other[2].flags = FRAME_NULL; other[0].fadeSamples = 11;
    CHECK(list_timing(other, 3) != list_timing(m, 3));
    // the five kinds of list; the facts of a NULL frame do not count
    const struct { uint32_t facts, flags; int shape; } kinds[5] = {
        {0, UTT_NO_NASAL, 3}, {FACT_NASAL, 0, 3}, {FACT_NOISE, UTT_NEEDS_NOISE, 3}, {FACT_NOISE | FACT_UNBOUNDED, UTT_NEEDS_NOISE, 1}, {FACT_NONFINITE | FACT_NASAL, UTT_NEEDS_NOISE, 0}};
    for (const auto& k : kinds) {
        const Facts f[3] = {{k.facts & FACT_NASAL}, {k.facts}, {FACT_NOISE | FACT_NONFINITE | FACT_NASAL | FACT_UNBOUNDED}};
        uint32_t flags = 99; unsigned char shape = 99;
        classify_list(m, f, 3, flags, shape);
        CHECK(flags == k.flags && shape == k.shape);
    }
}

// The routing, with a random subset of the eligible lists standing for plan_tracks' answer, against the rules restated with
// quadratic counts: how many utterances share a list's (timing, length), and what share of a set sits in runs of kRunMin or more.
static void check_routing(ListTable lists, const RouteOptions& o, std::mt19937& rng, bool bigTracks)
{
    const long long nL = lists.size();
    const ListTable before = lists;
    auto mates = [&](const ListTable& t, long long l, auto pred) {      // utterances of the lists `pred` selects that share l's run
        long long n = 0;
        for (long long j = 0; j < nL; ++j) if (pred(j) && t.timing[(size_t)j] == t.timing[(size_t)l] && t.lens[(size_t)j] == t.lens[(size_t)l]) n += t.weight[(size_t)j];
        return n;
    };
    auto share = [&](const ListTable& t, auto pred, long long& total, long long& inRuns) {
        total = inRuns = 0;
        for (long long l = 0; l < nL; ++l) if (pred(l)) { total += t.weight[(size_t)l]; if (mates(t, l, pred) >= kRunMin) inRuns += t.weight[(size_t)l]; }
    };
    auto quiet = [&](long long l) { return !(before.flags[(size_t)l] & UTT_NEEDS_NOISE); };
    const Rerouted rerouted = reroute_lonely_quiet(lists, o);
    bool oneRun = true;
    for (long long l = 0, first = -1; l < nL; ++l)
        if (quiet(l)) { if (first < 0) first = l; oneRun = oneRun && before.timing[(size_t)l] == before.timing[(size_t)first] && before.lens[(size_t)l] == before.lens[(size_t)first]; }
    size_t r = 0;
    for (long long l = 0; l < nL; ++l) {
        const bool lonely = o.plans() && o.layout == -1 && quiet(l) && !oneRun && mates(before, l, quiet) < kRunMin;
        if (lonely) {
            CHECK(r < rerouted.size() && rerouted[r].first == l && rerouted[r].second == before.flags[(size_t)l]);
            CHECK(lists.flags[(size_t)l] == UTT_NEEDS_NOISE);
            ++r;
        } else
            CHECK(lists.flags[(size_t)l] == before.flags[(size_t)l]);
    }
    CHECK(r == rerouted.size());
    if (r) ++g_hits[kRerouted];
    if (o.plans() && o.layout == -1 && oneRun && std::count_if(before.flags.begin(), before.flags.end(), [](uint32_t f) { return !(f & UTT_NEEDS_NOISE); }) == nL && nL > 0)
        ++g_hits[kOneQuietTiming];
    const std::vector<unsigned char> eligible = eligible_lists(lists, o);
    CHECK(eligible.size() == (o.plans() ? (size_t)nL : 0));
    for (size_t l = 0; l < eligible.size(); ++l)
        CHECK(eligible[l] == ((lists.flags[l] & UTT_NEEDS_NOISE) && lists.weight[l] ? lists.shape[l] : 0));
    if (o.want_tracks() && o.nFrames > 0) {
        std::vector<unsigned char> tracked((size_t)nL, 0);
        std::vector<uint32_t> kinds((size_t)nL, 0);
        const unsigned keep = rng() % 4;      // none, some, most, all of the eligible lists
        for (long long l = 0; l < nL; ++l) { tracked[(size_t)l] = eligible[(size_t)l] && (rng() % 3 < keep); kinds[(size_t)l] = rng() & 0xFFFFFFu; }
        const unsigned long long bytes = bigTracks ? (128ull << 20) + 16 : (128ull << 20);
        long long total, inRuns, direct = 0;
        share(lists, [&](long long l) { return tracked[(size_t)l] != 0; }, total, inRuns);
        for (long long l = 0; l < nL; ++l) if (tracked[(size_t)l] && (eligible[(size_t)l] & 2)) direct += lists.weight[(size_t)l];
        const bool drop = o.want_direct() && o.direct == 1 && o.fast && bigTracks && o.sortByLength && inRuns * 2 <= total && direct == total &&
                          (total + kLanes - 1) / kLanes > o.cus;
        CHECK(tracks_pay(lists, eligible.data(), tracked.data(), bytes, o) == !drop);
        if (drop) ++g_hits[kTracksDropped];
        else {
            const ListTable unmarked = lists;
            mark_tracked(lists, tracked.data(), kinds.data());
            for (long long l = 0; l < nL; ++l)
                CHECK(lists.flags[(size_t)l] == (unmarked.flags[(size_t)l] | (tracked[(size_t)l] ? UTT_TRACKED | (kinds[(size_t)l] << kUttKindShift) : 0u)));
        }
    }
    if (o.want_direct()) {
        const ListTable undirected = lists;
        auto candidate = [&](long long l) { return (eligible[(size_t)l] & 2) && !(undirected.flags[(size_t)l] & UTT_TRACKED); };
        long long total, inRuns;
        share(undirected, candidate, total, inRuns);
        const bool aligned = o.sortByLength && inRuns * 2 > total;
        CHECK(route_direct(lists, eligible.data(), o) == aligned);
        if (aligned) ++g_hits[kDirectAligned];
        const bool take = o.direct == 2 || !aligned || o.fast;
        for (long long l = 0; l < nL; ++l) CHECK(lists.flags[(size_t)l] == (undirected.flags[(size_t)l] | (take && candidate(l) ? UTT_DIRECT : 0u)));
    }
    const ListTable routed = lists;
    restore_rerouted(lists, rerouted);
    r = 0;
    for (long long l = 0; l < nL; ++l) {
        const bool back = r < rerouted.size() && rerouted[r].first == l && !(routed.flags[(size_t)l] & (UTT_TRACKED | UTT_DIRECT));
        if (r < rerouted.size() && rerouted[r].first == l) ++r;
        CHECK(lists.flags[(size_t)l] == (back ? before.flags[(size_t)l] : routed.flags[(size_t)l]));
        if (back) ++g_hits[kRestored];
    }
}

// a batch of `n` utterances (or lists): groups from `mix` (bit g: group g takes part), few lengths and timings so that runs form
static Utts random_utts(std::mt19937& rng, long long n, unsigned mix, int nLens, int nTimings, int runLength)
{
    Utts u;
    std::vector<uint32_t> groups;
    for (uint32_t g = 0; g < kGroups; ++g) if (mix >> g & 1) groups.push_back(g);
    while ((long long)u.flags.size() < n) {
        const uint32_t g = groups[rng() % groups.size()], len = 100 + rng() % (unsigned)nLens;
        const unsigned long long t = rng() % (unsigned)nTimings;
        for (long long k = 1 + rng() % (unsigned)runLength; k > 0 && (long long)u.flags.size() < n; --k) {
            u.flags.push_back(kGroupFlags[g]); u.lens.push_back(len); u.timing.push_back(t);
        }
    }
    // (the order of the call is no order at all)
    for (size_t i = u.flags.size(); i > 1; --i) {
        const size_t j = rng() % i;
        std::swap(u.flags[i - 1], u.flags[j]); std::swap(u.lens[i - 1], u.lens[j]); std::swap(u.timing[i - 1], u.timing[j]);
    }
    return u;
}

int main()
{
    std::mt19937 rng(20240607u);
    check_lists();
    check_literals();
    // structured: every non-empty set of groups, each group of every size around the thresholds of a wavefront of 8
    for (unsigned mix = 1; mix < 1u << kGroups; ++mix)
        for (int sorted = 0; sorted < 2; ++sorted)
            for (long long n : {1, 3, 4, 7, 8, 9, 17, 40})
                check_packing(random_utts(rng, n, mix, 3, 2, n > 9 ? 12 : 2), sorted != 0, 8);
    // random: 0 to 400 utterances, wavefronts of 4, 8 and 64 lanes
    long long cases = 0;
    for (int i = 0; i < 3000; ++i, ++cases) {
        const int W = i % 3 == 0 ? 4 : i % 3 == 1 ? 8 : 64;
        const unsigned mix = i % 5 == 0 ? 1u << (rng() % kGroups) : 1 + rng() % 31;
        const Utts u = random_utts(rng, rng() % 401, mix, 1 + (int)(rng() % 6), 1 + (int)(rng() % 4), 1 + (int)(rng() % (i % 2 ? 3 : 150)));
        check_packing(u, rng() % 4 != 0, W);
    }
    // the routing: lists of every class, some unspoken, some spoken many times
    for (int i = 0; i < 3000; ++i, ++cases) {
        ListTable lists;
        const long long nL = rng() % 120;
        const bool allQuiet = i % 10 == 0, heavy = i % 3 == 0;
        const bool distinct = i % 7 == 0;      // every list a timing of its own, all within the range of klatt_math.h: what the direct stages are for
        const int nLens = 1 + (int)(rng() % 3), nTimings = i % 20 == 0 ? 1 : 1 + (int)(rng() % 5);
        for (long long l = 0; l < nL; ++l) {
            static const uint32_t flags[5] = {UTT_NO_NASAL, 0u, UTT_NEEDS_NOISE, UTT_NEEDS_NOISE, UTT_NEEDS_NOISE};
            static const unsigned char shape[5] = {3, 3, 3, 1, 0};
            const unsigned k = allQuiet ? rng() % 2 : distinct ? rng() % 3 : rng() % 5;
            lists.flags.push_back(flags[k]); lists.shape.push_back(shape[k]);
            lists.lens.push_back(i % 20 == 0 ? 100u : 100u + rng() % (unsigned)nLens); lists.timing.push_back(distinct ? rng() : rng() % (unsigned)nTimings);
            lists.weight.push_back(rng() % 8 == 0 ? 0u : heavy && !distinct ? 1u + rng() % 600 : 1u + rng() % 3);
        }
        RouteOptions o;
        o.tracks = (int)(rng() % 3); o.direct = (int)(rng() % 3); o.layout = (int)(rng() % 3) - 1;
        o.fast = rng() % 2; o.sortByLength = rng() % 4 != 0; o.noTracks = rng() % 8 == 0;
        if (distinct) { o.tracks = o.direct = 1; o.layout = -1; o.fast = true; }      // (where dropping the tracks is in question at all)
        o.cus = i % 2 ? 1 : 256;
        o.nFrames = rng() % 16 == 0 ? 0 : 1000;
        check_routing(lists, o, rng, rng() % 2);
    }
    for (int b = 0; b < kBranches; ++b)
        if (g_hits[b] == 0) { printf("FAILED: no input reached the branch \"%s\"\n", kBranchNames[b]); return 1; }
    printf("ok %lld checks, %lld random cases; branches reached:", g_checks, cases);
    for (int b = 0; b < kBranches; ++b) printf(" %lld", g_hits[b]);
    printf("\n");
    return 0;
}
