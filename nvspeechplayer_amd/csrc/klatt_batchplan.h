// klatt_batchplan.h -- the host-only planning of a set call (klatt_engine.hip, batch_set): what a frame list is (its length, its
// timing, its class), which kernels its utterances go to (the routing), and which wavefront lane each utterance gets (pack_lanes).
//
// Plain C++17 over arrays and vectors: no HIP, no Batch.  These decisions fix the speed of every later launch -- whether BASELINE
// configs[2] runs in 8.4 or in 31 ms -- and hold the measured thresholds (kRunMin, a quarter of a wavefront, half of one, 128 MB of
// tracks, half of the candidates in runs).  tests/native/check_batch_plan.cpp restates the rules by brute force.
//
// The order of a set call: list_length, list_timing and classify_list per list (the engine runs them on its threads), then
//   reroute_lonely_quiet -> eligible_lists -> [plan_tracks, klatt_trackplan.h] -> tracks_pay / mark_tracked -> route_direct -> restore_rerouted
// and, with the flags of every utterance final, pack_lanes.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <unordered_map>
#include <utility>
#include <vector>

#include "klatt_consts.h"

namespace klatt {

// ---- per list, from its frames' meta words (Meta: minSamples, fadeSamples, flags) and facts (Facts: flags) --------------------------

// Its length in samples from the durations alone (closed form, reference src/frame.cpp:41-80).  false: 2^32 - 1 samples or more.
template <class Meta>
inline bool list_length(const Meta* meta, long long n, uint32_t& length)
{
    unsigned long long len = 0;
    for (long long k = 0; k < n; ++k) {
        const unsigned long long m = meta[k].minSamples, f = meta[k].fadeSamples;
        len += std::max(m, f + 1) + 1;   // samples one request spans
    }
    length = len >= 0xFFFFFFFFull ? 0u : (uint32_t)len;
    return len < 0xFFFFFFFFull;
}

// A list's TIMING: a hash of its sequence of frame durations, fades and silences -- the same text at the same speed, whatever
// the pitch, the voice or the noise seed.  Lanes with one timing dequeue and fade on the same samples (pack_lanes).
template <class Meta>
inline unsigned long long list_timing(const Meta* meta, long long n)
{
    unsigned long long h = 0x9E3779B97F4A7C15ull ^ (unsigned long long)n;
    for (long long k = 0; k < n; ++k) {
        h ^= ((unsigned long long)meta[k].minSamples << 32) ^ meta[k].fadeSamples ^ ((unsigned long long)(meta[k].flags & FRAME_NULL) << 63);
        h *= 0xFF51AFD7ED558CCDull; h ^= h >> 29;
    }
    return h;
}

// Whether the list needs its noise sources, whether it may skip the nasal pair (`flags`: UTT_*), and -- for the tracks and the direct
// stages -- whether all its parameters are finite (bit 0 of `shape`) and within the range of klatt_math.h (bit 1).  NULL frames carry
// no parameters of their own.
template <class Meta, class Facts>
inline void classify_list(const Meta* meta, const Facts* facts, long long n, uint32_t& flags, unsigned char& shape)
{
    uint32_t fl = 0;
    for (long long k = 0; k < n; ++k)
        if (!(meta[k].flags & FRAME_NULL)) fl |= facts[k].flags;
    const bool finite = !(fl & FACT_NONFINITE), needsNoise = (fl & FACT_NOISE) || !finite;
    flags = (needsNoise ? UTT_NEEDS_NOISE : (!(fl & FACT_NASAL) ? UTT_NO_NASAL : 0u)) | (fl & kUttPresent);      // (FACT_* and UTT_* of the present terms are the same bits)
    shape = finite ? (!(fl & FACT_UNBOUNDED) ? 3 : 1) : 0;
}
// ... and the list's second word of present terms (UTT2_*; Facts: flags, present2): whatever the routing makes of the list -- a noisy
// one, or a quiet one sent to the flat stages, loses UTT_NO_NASAL -- this word keeps what the frames said.
template <class Meta, class Facts>
inline void classify_list(const Meta* meta, const Facts* facts, long long n, uint32_t& flags, unsigned char& shape, uint32_t& present2)
{
    classify_list(meta, facts, n, flags, shape);
    uint32_t p2 = 0;
    for (long long k = 0; k < n; ++k)
        if (!(meta[k].flags & FRAME_NULL)) p2 |= facts[k].present2;
    present2 = p2 & kUtt2Present;
}

// ---- the routing: which kernels a list's utterances go to --------------------------------------------------------------------------

struct ListTable {      // per frame list
    std::vector<uint32_t> lens;                  // list_length
    std::vector<unsigned long long> timing;      // list_timing
    std::vector<uint32_t> flags;                 // classify_list, then the routing: UTT_*, what every utterance of the list carries
    std::vector<unsigned char> shape;            // classify_list
    std::vector<uint32_t> weight;                // how many utterances speak it
    std::vector<uint32_t> present2;              // classify_list: UTT2_*, the second word of present terms; no step of the routing touches it
    long long size() const { return (long long)flags.size(); }
    // utterances with one (timing, length) are a RUN: their lanes fade together
    unsigned long long run_key(long long l) const { return timing[(size_t)l] ^ ((unsigned long long)lens[(size_t)l] * 0x9E3779B97F4A7C15ull); }
};

struct RouteOptions {       // the batch's options (speechPlayer_batch_setOption) and what the routing needs to know of the call
    int tracks = 1, direct = 1, layout = -1;
    bool fast = false;               // MODE_FAST
    bool sortByLength = true;
    bool noTracks = false;           // the second attempt of a batch whose shared shapes failed their verification
    int cus = 256;                   // compute units of the device
    long long nFrames = 0;
    bool want_tracks() const { return tracks && !noTracks; }
    bool want_direct() const { return direct && layout != 0 && nFrames > 0 && nFrames < 0xFFFFFFFFll; }
    bool plans() const { return (want_tracks() || want_direct()) && nFrames > 0; }
};

constexpr long long kRunMin = 32;       // a run of this many utterances or more fills wavefronts with lanes that fade together

// Of the lists `pred` selects: the utterances per run, how many there are in all and how many of them sit in runs of kRunMin or more.
struct RunShare {
    long long total = 0, inRuns = 0;
    std::unordered_map<unsigned long long, long long> runOf;
};
template <class Pred>
inline RunShare run_share(const ListTable& lists, Pred pred)
{
    RunShare s;
    for (long long l = 0; l < lists.size(); ++l)
        if (pred(l)) { s.total += lists.weight[(size_t)l]; s.runOf[lists.run_key(l)] += lists.weight[(size_t)l]; }
    for (const auto& kv : s.runOf) if (kv.second >= kRunMin) s.inRuns += kv.second;
    return s;
}

// A quiet utterance whose timing too few others share cannot fill a wavefront of the quiet kernels with lanes that fade together:
// its wavefront would run every chunk sample by sample, evaluating exp / cos for whichever lane is fading (a few workgroups that
// take longer than the whole flat launch: 24 ms for the 8192 quiet utterances of a batch with 65 536 different timings).  Such an
// utterance goes with the noisy ones instead -- same PCM (its noise gains are zero: the sources add exactly 0), flat stages.
// Returns (list, its flags as a quiet one): back to the quiet kernels if it gets no tracks (restore_rerouted).
using Rerouted = std::vector<std::pair<long long, uint32_t>>;
inline Rerouted reroute_lonely_quiet(ListTable& lists, const RouteOptions& o)
{
    Rerouted rerouted;
    if (!o.plans() || o.layout != -1) return rerouted;      // (an explicit layout is taken at its word)
    auto quiet = [&](long long l) { return !(lists.flags[(size_t)l] & UTT_NEEDS_NOISE); };
    const RunShare runs = run_share(lists, quiet);
    // (quiet utterances that ALL share one timing fade together however few they are: a single sentence, a handful of copies)
    if (runs.runOf.size() <= 1) return rerouted;
    for (long long l = 0; l < lists.size(); ++l)
        if (quiet(l) && runs.runOf.at(lists.run_key(l)) < kRunMin) {
            rerouted.emplace_back(l, lists.flags[(size_t)l]);
            lists.flags[(size_t)l] = (lists.flags[(size_t)l] | UTT_NEEDS_NOISE) & ~UTT_NO_NASAL;
        }
    return rerouted;
}

// Tracks (klatt_tracks.h) are for the noisy lists whose parameters are all finite, the direct stages (klatt_direct.h) for those
// among them that get none: a list's `shape` where it may have either, 0 elsewhere.  Empty when the batch plans neither.
// A NaN anywhere ("hold" targets, reference src/utils.h:21) or an infinite parameter keeps an utterance with the untracked kernel.
// Finite parameters whose COEFFICIENTS overflow (a huge bandwidth or frequency) are tracked all the same: klatt_tracks evaluates
// the same expressions as the kernels' own coefficient code, so the track holds the same inf / NaN the kernel would have computed.
inline std::vector<unsigned char> eligible_lists(const ListTable& lists, const RouteOptions& o)
{
    std::vector<unsigned char> eligible;
    if (!o.plans()) return eligible;
    eligible.assign((size_t)lists.size(), 0);
    for (long long l = 0; l < lists.size(); ++l)
        if ((lists.flags[(size_t)l] & UTT_NEEDS_NOISE) && lists.weight[(size_t)l]) eligible[(size_t)l] = lists.shape[(size_t)l];
    return eligible;
}

// MODE_FAST, lanes that fade at unrelated times, tracks far beyond the caches (every fading lane streams through a track of its
// own: the jittered batch's 445 MB): the lean direct stages, whose pole recurrences compute what the tracks would deliver, are
// faster than the flat stages waiting for rows -- 18.4 against 21.8 ms (bench.py, jittered_durations) -- so such a batch is
// not tracked.  (MODE_EXACT keeps its tracks: the polynomials cost more than the rows' latency, 22 ms against ~35.)
// `tracked`: the lists plan_tracks gave tracks, `trackBytes` what those take.  false: drop them.
inline bool tracks_pay(const ListTable& lists, const unsigned char* eligible, const unsigned char* tracked, unsigned long long trackBytes, const RouteOptions& o)
{
    if (!(o.want_direct() && o.direct == 1 && o.fast && trackBytes > (128ull << 20))) return true;
    long long direct = 0;      // ... of the tracked utterances, those the direct stages could take
    const RunShare runs = run_share(lists, [&](long long l) { return tracked[l] != 0; });
    for (long long l = 0; l < lists.size(); ++l)
        if (tracked[l] && (eligible[l] & 2)) direct += lists.weight[(size_t)l];
    const long long groups = (runs.total + kLanes - 1) / kLanes;
    return !(o.sortByLength && runs.inRuns * 2 <= runs.total && direct == runs.total && groups > o.cus);
}

inline void mark_tracked(ListTable& lists, const unsigned char* tracked, const uint32_t* kinds)
{
    for (long long l = 0; l < lists.size(); ++l)
        if (tracked[l]) lists.flags[(size_t)l] |= UTT_TRACKED | (kinds[l] << kUttKindShift);
}

// The direct stages are for lanes that fade at unrelated times.  A group whose wavefronts hold equally timed utterances (the
// BASELINE recipes without their tracks, a batch of few sentences in many voices) runs whole chunks on the uniform paths of the
// stages with the frame state machine, two workgroups per CU, and is faster there (cfg2 without tracks 13.9 against 19.1 ms,
// DESIGN.md section 4.7): "direct" = 1 decides by the share of the candidates that sit in runs of kRunMin or more equally long,
// equally timed utterances; 2 takes the direct stages whatever the timing.  Marks the lists taken UTT_DIRECT; returns whether the
// candidates are ALIGNED (Batch::directAligned).  For a batch with want_direct().
inline bool route_direct(ListTable& lists, const unsigned char* eligible, const RouteOptions& o)
{
    auto candidate = [&](long long l) { return (eligible[l] & 2) && !(lists.flags[(size_t)l] & UTT_TRACKED); };
    const RunShare runs = run_share(lists, candidate);
    // (without the sort by length and timing nothing is side by side; in MODE_FAST the direct stages advance coefficients by
    // recurrences and win on the aligned batches whose fades move everything too -- "distinct" 19.2 -> 15.9 ms -- while a batch
    // of few moving kinds loses 8 % there: cfg2 without its tracks 12.7 -> 13.7)
    const bool aligned = o.sortByLength && runs.inRuns * 2 > runs.total;
    const bool take = o.direct == 1 ? (!aligned || o.fast) : true;
    if (take)
        for (long long l = 0; l < lists.size(); ++l)
            if (candidate(l)) lists.flags[(size_t)l] |= UTT_DIRECT;
    return aligned;
}

// (a re-routed quiet list that got neither tracks nor the direct stages goes back to the quiet kernels)
inline void restore_rerouted(ListTable& lists, const Rerouted& rerouted)
{
    for (const auto& r : rerouted)
        if (!(lists.flags[(size_t)r.first] & (UTT_TRACKED | UTT_DIRECT))) lists.flags[(size_t)r.first] = r.second;
}

// ---- lane packing: which slot of `order` (wavefront slot / width, lane slot % width) runs which utterance -----------------------------

constexpr uint32_t kNoUtt = 0xFFFFFFFFu;      // an order slot without an utterance: the lane stays empty

struct LanePacking {
    std::vector<uint32_t> order;      // the groups in launch order: quiet without nasal pair, quiet, tracked, direct, untracked
    long long nNoNasal = 0, nQuiet = 0;                // utterances of the first group; of the first two
    long long nNoNasalSlots = 0, nQuietSlots = 0;      // ... and their slots: with the replicas that complete a sparse last wavefront
    long long nTrackedUtt = 0, nTracked = 0;           // utterances of the tracked group; its slots (utterances, padding, replicas)
    long long nDirectSlots = 0;                        // slots of the direct group
};

// lanes from slot n to the next wavefront boundary (0 on one)
inline size_t lanes_to_boundary(size_t n, int width) { return ((size_t)width - n % (size_t)width) % (size_t)width; }

// The noisy groups (64 utterances per wavefront): a wavefront that holds two timings runs every chunk on the general
// path -- ~2.6 times the time of a pure one for the whole length of its utterances, and it is the last to finish.  So a
// run of equally timed utterances that filled at least a quarter of its last wavefront, or that is followed by a run
// of 64 or more, ends its wavefront there: the remaining lanes stay empty (kNoUtt).  Batches of
// utterances that are all different (runs of 1) are packed densely.
inline void pad_runs(const uint32_t* first, const uint32_t* last, const uint32_t* lens, const unsigned long long* timing, int width, std::vector<uint32_t>& out)
{
    const size_t W = (size_t)width;
    size_t lanesOfRun = 0;     // lanes the current run occupies in the wavefront being filled
    for (const uint32_t* it = first; it != last;) {
        const uint32_t* runEnd = it;
        while (runEnd != last && timing[*runEnd] == timing[*it] && lens[*runEnd] == lens[*it]) ++runEnd;
        const size_t runSize = (size_t)(runEnd - it), fill = out.size() % W;
        if (fill != 0 && (lanesOfRun >= W / 4 || runSize >= W)) out.insert(out.end(), W - fill, kNoUtt);
        out.insert(out.end(), it, runEnd);
        const size_t tail = out.size() % W;
        lanesOfRun = tail == 0 ? 0 : std::min(runSize, tail);
        it = runEnd;
    }
}

// A wavefront with FEW live lanes takes up to 1.7 times as long as a full one for the same instructions (measured:
// streams_synthesize, tools/lone_probe2.py: 1 .. 8 live lanes 4.3 / 6.1 / 7.4 ms from launch to launch, 16 or more a steady 4.13).  Its
// empty slots are given its own utterances again: those lanes compute the same samples and store the same bytes to the same places.
// (What a batch of a handful of sentences -- or the tail of a large one -- costs in latency; nothing for full wavefronts.)
// SPARSE: fewer than half the lanes live (16 of 64 still wavered a little: 4.32 against 4.15 ms).
//
// A quiet group [begin, end) is packed densely: only its LAST wavefront can be sparse (one vowel alone: 46 ns per sample against 31).
// Returns the slots inserted at `end`.
inline long long fill_tail(std::vector<uint32_t>& order, long long begin, long long end, int width)
{
    const long long n = end - begin, tail = n % width;
    if (n == 0 || tail == 0 || tail >= width / 2) return 0;
    const long long ext = width - tail;
    std::vector<uint32_t> rep((size_t)ext);
    for (long long j = 0; j < ext; ++j) rep[(size_t)j] = order[(size_t)(end - tail + j % tail)];
    order.insert(order.begin() + end, rep.begin(), rep.end());
    return ext;
}

// The noisy groups, whole wavefronts from slot `begin`: the empty lanes of every sparse wavefront repeat its live ones in turn.
inline void fill_sparse_wavefronts(std::vector<uint32_t>& order, long long begin, int width)
{
    const int sparse = width / 2;
    std::vector<uint32_t> live((size_t)sparse);
    for (long long w = begin; w + width <= (long long)order.size(); w += width) {
        int nLive = 0;
        for (int i = 0; i < width && nLive < sparse; ++i)
            if (order[(size_t)(w + i)] != kNoUtt) live[(size_t)nLive++] = order[(size_t)(w + i)];
        if (nLive == 0 || nLive >= sparse) continue;
        int next = 0;
        for (int i = 0; i < width; ++i)
            if (order[(size_t)(w + i)] == kNoUtt) { order[(size_t)(w + i)] = live[(size_t)next]; next = (next + 1) % nLive; }
    }
}

// Lane packing: similar lengths share a wavefront (longest first), so lanes finish together -- within each of the five groups,
// which are launched as separate kernels.  flagsOf(u): utterance u's UTT_* flags; lens, timing: per utterance (its list's).
// `width`: lanes per wavefront (the engine's is kLanes; a test may read a narrower one at a glance).
template <class FlagsOf>
inline LanePacking pack_lanes(long long nUtt, FlagsOf flagsOf, const uint32_t* lens, const unsigned long long* timing, bool sortByLength, int width = kLanes)
{
    LanePacking p;
    std::vector<uint32_t>& order = p.order;
    order.resize((size_t)nUtt);
    std::iota(order.begin(), order.end(), 0u);
    auto quietEnd = std::stable_partition(order.begin(), order.end(), [&](uint32_t x) { return !(flagsOf(x) & UTT_NEEDS_NOISE); });
    p.nQuiet = quietEnd - order.begin();
    auto noNasalEnd = std::stable_partition(order.begin(), quietEnd, [&](uint32_t x) { return (flagsOf(x) & UTT_NO_NASAL) != 0; });
    p.nNoNasal = noNasalEnd - order.begin();
    auto trackedEnd = std::stable_partition(quietEnd, order.end(), [&](uint32_t x) { return (flagsOf(x) & UTT_TRACKED) != 0; });
    p.nTrackedUtt = trackedEnd - quietEnd;
    p.nTracked = p.nTrackedUtt;
    auto directEnd = std::stable_partition(trackedEnd, order.end(), [&](uint32_t x) { return (flagsOf(x) & UTT_DIRECT) != 0; });
    p.nDirectSlots = directEnd - trackedEnd;
    const bool untrackedFollow = directEnd != order.end();
    if (sortByLength) {
        // Within a group: longest first, and utterances with the same TIMING side by side.  Lanes with one timing dequeue and fade
        // on the same samples, so their wavefront runs whole chunks on the uniform paths.
        auto before = [&](uint32_t x, uint32_t y) { return lens[x] != lens[y] ? lens[x] > lens[y] : timing[x] < timing[y]; };
        std::stable_sort(order.begin(), noNasalEnd, before);
        std::stable_sort(noNasalEnd, quietEnd, before);
        std::stable_sort(quietEnd, trackedEnd, before);
        std::stable_sort(trackedEnd, directEnd, before);
        std::stable_sort(directEnd, order.end(), before);
        const uint32_t* const o = order.data();
        const size_t q = (size_t)p.nQuiet, t = q + (size_t)p.nTrackedUtt, d = t + (size_t)p.nDirectSlots;
        std::vector<uint32_t> tracked, direct(o + t, o + d), untracked;
        pad_runs(o + q, o + t, lens, timing, width, tracked);
        if (!tracked.empty() && t != order.size()) tracked.insert(tracked.end(), lanes_to_boundary(tracked.size(), width), kNoUtt);   // the next group starts its own wavefront
        // (the direct stages do not care whether their lanes fade together: packed densely, longest first)
        if (!direct.empty() && untrackedFollow) direct.insert(direct.end(), lanes_to_boundary(direct.size(), width), kNoUtt);
        pad_runs(o + d, o + order.size(), lens, timing, width, untracked);
        p.nTracked = (long long)tracked.size();
        p.nDirectSlots = (long long)direct.size();
        order.resize(q);
        order.insert(order.end(), tracked.begin(), tracked.end());
        order.insert(order.end(), direct.begin(), direct.end());
        order.insert(order.end(), untracked.begin(), untracked.end());
    } else if (p.nDirectSlots > 0 && (untrackedFollow || p.nTrackedUtt > 0)) {
        // unsorted: the groups still start on wavefront boundaries (each is a launch of its own)
        const size_t padT = p.nTrackedUtt > 0 ? lanes_to_boundary((size_t)p.nTrackedUtt, width) : 0;
        order.insert(order.begin() + p.nQuiet + p.nTrackedUtt, padT, kNoUtt);
        p.nTracked = p.nTrackedUtt + (long long)padT;
        if (untrackedFollow) {
            const size_t padD = lanes_to_boundary((size_t)p.nDirectSlots, width);
            order.insert(order.begin() + p.nQuiet + p.nTracked + p.nDirectSlots, padD, kNoUtt);
            p.nDirectSlots += (long long)padD;
        }
    }
    p.nNoNasalSlots = p.nNoNasal + fill_tail(order, 0, p.nNoNasal, width);
    p.nQuietSlots = p.nQuiet + (p.nNoNasalSlots - p.nNoNasal);
    p.nQuietSlots += fill_tail(order, p.nNoNasalSlots, p.nQuietSlots, width);
    const long long noisy = (long long)order.size() - p.nQuietSlots;
    if (noisy % width != 0) {
        // the last wavefront's dead lanes become slots of the group that ends there
        const long long ext = width - noisy % width;
        const long long untracked = noisy - p.nTracked - p.nDirectSlots;
        if (untracked <= 0) { if (p.nDirectSlots > 0) p.nDirectSlots += ext; else p.nTracked += ext; }
        order.insert(order.end(), (size_t)ext, kNoUtt);
    }
    fill_sparse_wavefronts(order, p.nQuietSlots, width);
    return p;
}

// What the flat stages will decide (klatt_systolic.h), from the plan: of the tracked group's wavefronts -- order[first, first + n) in
// wavefronts of `width` slots -- how many run without parallel 1 [0], without turbulence [1], without the aspiration generator [2]: a term
// goes when no utterance of the wavefront (replica lanes name one, empty slots none) has it present.  `built`: the bodies the kernel
// was compiled with (KLATT_DEAD_TERMS: 1 without parallel 1, 2 without turbulence, 4 without turbulence and the generator).
template <class FlagsOf>
inline void dead_wave_counts(const uint32_t* order, long long first, long long n, FlagsOf flagsOf, int built, long long counts[3], int width = kLanes)
{
    counts[0] = counts[1] = counts[2] = 0;
    for (long long w = first; w < first + n; w += width) {
        uint32_t present = 0;
        bool any = false;
        for (long long s = w; s < std::min(w + width, first + n); ++s)
            if (order[s] != kNoUtt) { present |= flagsOf(order[s]); any = true; }
        if (!any) continue;
        const bool noTurb = !(present & UTT_TURBULENCE), noAsp = noTurb && !(present & UTT_ASPIRATION);
        const int body = ((built & 4) && noAsp) ? 2 : (((built & 2) && noTurb) ? 1 : 0);
        counts[0] += ((built & 1) && !(present & UTT_PARALLEL1)) ? 1 : 0;
        counts[1] += body >= 1 ? 1 : 0;
        counts[2] += body >= 2 ? 1 : 0;
    }
}

// The same for the second word of present terms (present2Of(u): utterance u's UTT2_* bits), the bodies behind KLATT_DEAD_TERMS bits 8 .. 64:
// wavefronts whose source stage runs without turbulence and the nasal pair [0] (bit 8; the stage needs turbulence dead too, flagsOf),
// whose final stage runs without parallel 5 [1] (bit 16 or 32) and without parallel 5 and 6 [2] (bit 32), whose parallel stage runs
// without parallel 1..4 [3] (bit 64; parallel 1 by flagsOf).
template <class FlagsOf, class Present2Of>
inline void dead2_wave_counts(const uint32_t* order, long long first, long long n, FlagsOf flagsOf, Present2Of present2Of, int built, long long counts[kDead2Counts],
                              int width = kLanes)
{
    for (int k = 0; k < kDead2Counts; ++k) counts[k] = 0;
    for (long long w = first; w < first + n; w += width) {
        uint32_t present = 0, present2 = 0;
        bool any = false;
        for (long long s = w; s < std::min(w + width, first + n); ++s)
            if (order[s] != kNoUtt) { present |= flagsOf(order[s]); present2 |= present2Of(order[s]); any = true; }
        if (!any) continue;
        const bool no5 = !(present2 & UTT2_PARALLEL5), no56 = no5 && !(present2 & UTT2_PARALLEL6);
        const int fin = ((built & 32) && no56) ? 2 : (((built & 16) && no5) ? 1 : 0);
        counts[0] += ((built & 8) && !(present & UTT_TURBULENCE) && !(present2 & UTT2_NASAL)) ? 1 : 0;
        counts[1] += fin >= 1 ? 1 : 0;
        counts[2] += fin >= 2 ? 1 : 0;
        counts[3] += ((built & 64) && !(present & UTT_PARALLEL1) && !(present2 & kUtt2Parallel234)) ? 1 : 0;
    }
}

}  // namespace klatt
