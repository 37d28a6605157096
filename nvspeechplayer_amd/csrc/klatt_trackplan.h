// klatt_trackplan.h -- planning the tracks of a batch (host only; klatt_tracks.h, klatt_layout.h for the track layout), and the two
// smaller walks over a batch's frames beside it: the shape table of frames that stay in device memory, the end points of the direct
// stages' fades.  Plain C++17: no HIP, no Batch, no global -- the budget (in entries), the hash mask and the thread count are
// arguments.  tests/native/check_track_plan.cpp holds it to a restatement under AddressSanitizer, UBSan and ThreadSanitizer.
// Per frame of an eligible utterance: which entry kinds its fade moves and where the fade's track will be.  The state walked
// here is the part of the frame state machine that decides a fade's end points (reference src/frame.cpp:55-72, restated by
// stage_event): silence keeps the last request's values with the gain gated off, the first frame after silence starts from its
// own values with the gain gated off, any other frame fades from the previous request's values.  A SHAPE is the vector of
// the 39 parameter values a track depends on (klatt_layout.h); fades with bitwise equal shapes at both ends and the same
// length share one track.
// Tracks pay when (nearly) the whole noisy group has them: a batch whose fades share nothing may need more memory than the
// budget, and splitting such a batch into a tracked and an untracked launch measured slower than either kernel alone
// (tools/track_probe.py +distinct).  So once more than a tenth of the eligible utterances did not fit, nothing is tracked.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <unordered_map>
#include <vector>

#include "../../include/speechPlayer_batch.h"
#include "klatt_consts.h"
#include "klatt_hostpool.h"
#include "klatt_layout.h"
#include "klatt_plan.h"

namespace klatt {

constexpr size_t kTrackPad = 64;   // slack past the last track
// The budget of a batch's tracks in 16-byte entries (the flat stages address the tracks with 32-bit byte offsets: below 4 GB, 2^28 entries).
inline unsigned long long track_budget_entries(long long budgetMB)
{
    return std::min((unsigned long long)std::max(budgetMB, 0ll) * (1ull << 20) / 16u, (1ull << 28) - (1ull << 21) - kTrackPad);
}

// hash of a shape's 45 values: four independent multiply-xor chains (one chain of 45 dependent steps was half the planning's time)
inline unsigned long long hash_shape(const double* v)
{
    unsigned long long h[4] = {0x9E3779B97F4A7C15ull, 0xC2B2AE3D27D4EB4Full, 0x165667B19E3779F9ull, 0x27D4EB2F165667C5ull};
    int i = 0;
    for (; i + 4 <= kShapeValues; i += 4)
        for (int j = 0; j < 4; ++j) { unsigned long long w; memcpy(&w, &v[i + j], 8); h[j] = (h[j] ^ w) * 0xFF51AFD7ED558CCDull; h[j] ^= h[j] >> 29; }
    for (; i < kShapeValues; ++i) { unsigned long long w; memcpy(&w, &v[i], 8); h[0] = (h[0] ^ w) * 0xFF51AFD7ED558CCDull; h[0] ^= h[0] >> 29; }
    unsigned long long x = h[0] ^ (h[1] * 0x9E3779B97F4A7C15ull) ^ (h[2] << 21 | h[2] >> 43) ^ (h[3] * 0xC2B2AE3D27D4EB4Full);
    x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 32;
    return x;
}

// The bits of a frame's 128-bit shape hash (FrameFacts) that the planner and the shape table look at: all of them, unless a test
// asked for fewer (speechPlayer_setGlobalOption "plan_hash_bits").  Passed by value: what a call read once holds for all its threads.
struct HashMask { unsigned long long a = ~0ull, b = ~0ull; };
struct Key128 {
    unsigned long long a, b;
    bool operator==(const Key128& o) const { return a == o.a && b == o.b; }
    static Key128 of(const FrameFacts& f, HashMask m = HashMask()) { return Key128{f.h0 & m.a, f.h1 & m.b}; }
};
// (`a` is an avalanched word, and all there is of a key masked to 64 bits or fewer)
struct Key128Hash { size_t operator()(const Key128& k) const { return (size_t)k.a; } };
// A fade by its end points' shape ids and its length.
struct FadeKey { uint32_t from, to, len; bool operator==(const FadeKey& o) const { return from == o.from && to == o.to && len == o.len; } };
struct FadeKeyHash { size_t operator()(const FadeKey& k) const { unsigned long long h = ((unsigned long long)k.from << 32 | k.to) * 0x9E3779B97F4A7C15ull; h ^= h >> 29; h += k.len; h *= 0xFF51AFD7ED558CCDull; return (size_t)(h ^ (h >> 32)); } };

// where a frame's parameter values are on the host: in the caller's frames, or -- records -- in the row of the shape table a record names
// (the planner reads parameters 1..45 only: a record's own pitches are not among them), or -- frames that stay in device memory
// (speechPlayer_batch_setUtterancesDevice) -- in the row rowOf[k] of a table that holds ONE frame per distinct (masked) shape hash,
// downloaded for the planner: equal hashes stand for equal values, as the planner assumes anyway, and klatt_verify_shared checks it
struct FrameSource {
    const speechPlayer_frame_t* frames;
    const speechPlayer_frameRecord_t* records;
    const speechPlayer_frame_t* shapes;
    const uint32_t* rowOf = nullptr;
    const double* values(long long k) const
    {
        if (rowOf) return reinterpret_cast<const double*>(shapes + rowOf[k]);
        return reinterpret_cast<const double*>(records ? shapes + records[k].shape : frames + k);
    }
};
struct TrackPlan {
    std::vector<TrackRef> ref;              // [nFrames]
    std::vector<uint32_t> rep;              // [nFrames] the frame whose shape values stand for this frame's (the first one seen with its hash); 0xFFFFFFFF: itself / none
    std::vector<TrackJob> jobs;             // one per distinct track
    std::vector<double> shapes;             // [nShapes][kShapeStride]
    std::vector<unsigned char> tracked;     // [nUtterances]
    std::vector<uint32_t> kinds;            // [nUtterances] the entry kinds whose values change after the first sample of the utterance's first fade (UttDesc.flags)
    unsigned long long entries = 0;
    long long eligible = 0, missedSize = 0, missedBudget = 0;   // utterances that may be tracked; that a fade of 2^27 entries or the budget kept out
    // the plan of a batch of which nothing is tracked (yet): every array at its size
    void reset(long long nUtterances, long long nFrames, bool withRep)
    {
        ref.assign((size_t)nFrames, TrackRef{0, 0, 0});
        rep.assign(withRep ? (size_t)nFrames : 0, 0xFFFFFFFFu);
        tracked.assign((size_t)nUtterances, 0);
        kinds.assign((size_t)nUtterances, 0);
        jobs.clear(); shapes.clear(); entries = 0;
        eligible = 0; missedSize = 0; missedBudget = 0;
    }
};
// One pass over utterances [0, nUtterances) of the arrays given (frameStart may start anywhere: ref is indexed from frameStart[0]).
// `budget`: in entries (track_budget_entries).
// `whole`: this is the whole batch -- apply the all-or-nothing rule; a part of it (plan_tracks below) leaves that to the merge,
// and gives up (missedBudget != 0) as soon as the parts' tracks together (`sum`) pass a quarter of the budget: that batch is
// planned in one pass (its fades are shared by few utterances, if at all: the parts would each make most of the tracks again, or
// fill the budget with 400 MB of shapes and map nodes only for the one pass to find that nothing fits -- 0.4 s for 65 536
// utterances with nothing in common, which is what such a batch costs without the parts).
// `facts`: klatt_plan.h's 128-bit hash of every frame's shape values (indexed like `frames`): a frame seen before is recognised by
// it (under `mask`), without gathering, hashing or comparing its 45 values again.
inline void plan_tracks_pass(long long nUtterances, const long long* frameStart, const FrameSource& frames, const FrameFacts* facts, const FrameMeta* meta,
                             const unsigned char* eligible, unsigned long long budget, HashMask mask, bool whole, std::atomic<unsigned long long>* sum,
                             TrackPlan& out)
{
    const long long frame0 = frameStart[0], nF = frameStart[nUtterances] - frame0;
    const bool wantRep = frameStart[nUtterances] < 0xFFFFFFFFll;
    out.reset(nUtterances, nF, wantRep);
    // the entry kinds whose values differ between two shapes (the comparisons stage_event makes on the device)
    auto diff_kinds = [](const double* a, const double* c) -> uint32_t {
        uint32_t m = 0;
        for (int r = 0; r < kNumRes; ++r)
            if (!(c[2 * r] == a[2 * r]) || !(c[2 * r + 1] == a[2 * r + 1])) m |= 1u << r;
        for (int e = kNumRes; e < kTrackEntries; ++e) {
            const int x = entry_value(e, 0), y = entry_value(e, 1);
            if (!(c[x] == a[x]) || (y >= 0 && !(c[y] == a[y]))) m |= 1u << e;
        }
        return m;
    };
    struct Shape { double v[kShapeValues]; bool operator==(const Shape& o) const { return !memcmp(v, o.v, sizeof v); } };
    struct ShapeHash { size_t operator()(const Shape& k) const { return (size_t)hash_shape(k.v); } };
    std::unordered_map<Shape, uint32_t, ShapeHash> shapes;          // values -> id (row of out.shapes)
    std::unordered_map<FadeKey, TrackRef, FadeKeyHash> fades;       // (from, to, length) -> the fade's track
    auto shape_id = [&](const Shape& sh) -> uint32_t {
        auto it = shapes.find(sh);
        if (it != shapes.end()) return it->second;
        const uint32_t id = (uint32_t)shapes.size();
        shapes.emplace(sh, id);
        out.shapes.resize((size_t)(id + 1) * kShapeStride, 0.0);
        memcpy(&out.shapes[(size_t)id * kShapeStride], sh.v, sizeof sh.v);
        return id;
    };
    Shape zero; memset(&zero, 0, sizeof zero);
    shape_id(zero);
    // frames seen before, by their hash: the id of their shape and (once somebody needed it) of the same values with the gain gated off
    struct FrameIds { uint32_t plain, gated; long long first; };
    std::unordered_map<Key128, FrameIds, Key128Hash> seen;
    std::vector<uint32_t> gatedOf;          // shape id -> the id of its values with the gain gated off (0xFFFFFFFF: not asked for yet)
    auto gated_id = [&](uint32_t id) -> uint32_t {
        if (gatedOf.size() <= id) gatedOf.resize((size_t)id + 64, 0xFFFFFFFFu);
        if (gatedOf[id] == 0xFFFFFFFFu) {
            Shape g;
            memcpy(g.v, &out.shapes[(size_t)id * kShapeStride], sizeof g.v);
            g.v[kShapePreGain] = 0.0;
            gatedOf[id] = shape_id(g);
        }
        return gatedOf[id];
    };
    std::vector<FadeKey> added;
    long long nEligible = 0, nMissed = 0;
    for (long long u = 0; u < nUtterances; ++u) nEligible += eligible[u] ? 1 : 0;
    out.eligible = nEligible;
    // Give up early on a batch whose fades are (nearly) all different: its tracks grow in proportion to the utterances walked and
    // would pass the budget long before the end -- walking on until they do, hashing 45 values per frame and filling the maps,
    // was 0.6 s for 65 536 such utterances (30 launches' worth) for nothing.  Two look-outs, after 1/32 and 1/16 of the
    // utterances: tracks that doubled in between (no sharing yet: a batch that shares its fades saturates early) and that at this
    // rate end beyond the budget.
    const long long look1 = nUtterances / 32, look2 = nUtterances / 16;
    unsigned long long entriesAt1 = 0;
    for (long long u = 0; u < nUtterances && (!whole || nMissed * 10 <= nEligible); ++u) {
        if (whole && look1 >= 256) {
            if (u == look1) entriesAt1 = out.entries;
            if (u == look2 && out.entries - entriesAt1 >= entriesAt1 - entriesAt1 / 8 &&
                (long double)out.entries * ((long double)nUtterances / (long double)look2) > (long double)budget) {
                nMissed = nEligible + 1;      // the all-or-nothing rule below: nothing is tracked
                out.missedBudget = nEligible;
                break;
            }
        }
        if (!eligible[u]) continue;
        if (sum && sum->load(std::memory_order_relaxed) > budget / 4) { ++out.missedBudget; return; }
        added.clear();
        const unsigned long long before = out.entries;
        const size_t jobsBefore = out.jobs.size();
        bool fits = true, prevNull = true;
        uint32_t prevId = 0;       // the previous request's values (a fresh handle: all zero = shape 0)
        uint32_t kinds = 0;
        for (long long k = frameStart[u]; k < frameStart[u + 1] && fits; ++k) {
            uint32_t fromId = prevId, toId;
            const uint32_t lastTo = prevId;
            if (meta[k].flags & FRAME_NULL) {
                toId = gated_id(prevId);                       // silence: the old values, the gain gated off (:59-63)
                prevNull = true;
            } else {
                // (records: the key is the shape's number, exact -- never masked)
                const Key128 fk = Key128::of(facts[k], frames.records ? HashMask() : mask);
                auto it = seen.find(fk);
                if (it == seen.end()) {
                    Shape to;
                    const double* p = frames.values(k);
                    for (int i = 0; i < kShapeValues; ++i) to.v[i] = p[shape_param(i)];
                    it = seen.emplace(fk, FrameIds{shape_id(to), 0xFFFFFFFFu, k}).first;
                } else if (wantRep) {
                    out.rep[k - frame0] = (uint32_t)it->second.first;      // taken on trust here; compared where the frames are (klatt_verify_shared)
                }
                toId = it->second.plain;
                if (prevNull) {                                // out of silence: the new values, from gain 0 (:64-67)
                    if (it->second.gated == 0xFFFFFFFFu) it->second.gated = gated_id(toId);
                    fromId = it->second.gated;
                }
                prevNull = false;
            }
            prevId = toId;
            const FadeKey key{fromId, toId, meta[k].fadeSamples};
            auto f = fades.find(key);
            if (f == fades.end()) {
                // a new fade: what moves in it (the comparisons stage_event makes on the device), its size, its place
                const uint32_t moves = diff_kinds(&out.shapes[(size_t)fromId * kShapeStride], &out.shapes[(size_t)toId * kShapeStride]);
                const uint32_t nSlots = track_slots(moves);
                const unsigned long long n = (unsigned long long)kTrackFirst + (unsigned long long)(meta[k].fadeSamples - 1u) * nSlots;
                if (n >= (1ull << 27)) { fits = false; ++out.missedSize; break; }
                if (out.entries + n > budget) { fits = false; ++out.missedBudget; break; }
                if (sum && sum->fetch_add(n, std::memory_order_relaxed) + n > budget / 4) { ++out.missedBudget; return; }
                f = fades.emplace(key, TrackRef{out.entries, moves, nSlots}).first;
                added.push_back(key);
                out.jobs.push_back(TrackJob{out.entries, key.from, key.to, meta[k].fadeSamples, moves});
                out.entries += n;
            }
            out.ref[k - frame0] = f->second;
            // what changes after the utterance's first fade sample: what a fade moves, and what a later fade's first sample re-sets
            // to other values than the previous fade ended on (the frame after a silence starts from ITS values, gain gated off)
            kinds |= f->second.mask;
            if (k > frameStart[u] && fromId != lastTo)
                kinds |= diff_kinds(&out.shapes[(size_t)lastTo * kShapeStride], &out.shapes[(size_t)fromId * kShapeStride]);
        }
        out.kinds[u] = kinds;
        if (fits) out.tracked[u] = 1;
        else {
            for (const FadeKey& key : added) fades.erase(key);
            out.jobs.resize(jobsBefore);
            out.entries = before;
            ++nMissed;
        }
    }
    if (whole && nMissed * 10 > nEligible) {
        out.tracked.assign((size_t)nUtterances, 0);
        out.jobs.clear();
        out.entries = 0;
    }
}

// The plan of a batch.  Large batches are planned in parts, one host thread each (the walk is a hash of 45 values and two map
// look-ups per frame: 0.2 s for BASELINE configs[2] on one thread), and the parts' shapes and fades merged: equal fades of
// different parts end up with one track.  If the merged tracks fit the budget that is the plan; if not -- or if the parts gave
// up (plan_tracks_pass) -- the batch is planned again in one pass, whose order decides which utterances stay in.
// `nThreads`, `minFrames`: who takes the parts -- batches of minFrames frames or more on two threads or more (a test passes smaller ones).
inline void plan_tracks(long long nUtterances, const long long* frameStart, const FrameSource& frames, const FrameFacts* facts, const FrameMeta* meta,
                        const unsigned char* eligible, unsigned long long budget, HashMask mask, TrackPlan& out,
                        unsigned nThreads = host_threads(), long long minFrames = 200000)
{
    const long long nF = frameStart[nUtterances];
    static const bool trace = getenv("SPEECHPLAYER_PLAN_TRACE") != nullptr;      // where the planning's time goes, on stderr
    const auto tStart = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (trace) fprintf(stderr, "[speechPlayer/plan] %s: %.1f ms since the start\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tStart).count());
    };
    auto one_pass = [&] { plan_tracks_pass(nUtterances, frameStart, frames, facts, meta, eligible, budget, mask, true, nullptr, out); };
    if (nThreads < 2 || nF < minFrames || nUtterances < (long long)nThreads * 64) { one_pass(); return; }
    // A look at the first 128th of the batch before the threads start (the look-outs of plan_tracks_pass, whole = true): a batch
    // whose fades are all different is given up after a few milliseconds instead of after the parts have filled a quarter of the budget.
    {
        TrackPlan probe;
        // (never past the batch: the threaded path is entered with as few as 2 x 64 utterances -- ADVICE r3)
        const long long nProbe = std::min<long long>(nUtterances, std::max<long long>(nUtterances / 128, 256));
        plan_tracks_pass(nProbe, frameStart, frames, facts, meta, eligible, budget, mask, false, nullptr, probe);
        TrackPlan half;
        plan_tracks_pass(nProbe / 2, frameStart, frames, facts, meta, eligible, budget, mask, false, nullptr, half);
        if (trace) fprintf(stderr, "[speechPlayer/plan] look: %llu entries after %lld utterances, %llu after %lld; budget %llu\n", half.entries, nProbe / 2, probe.entries, nProbe, budget);
        const long double scale = (long double)nUtterances / (long double)nProbe;
        // (tracks that double with the utterances and at that rate end more than a ninth beyond the budget: then more than a tenth of
        // the utterances would not fit, and the rule is all or nothing)
        if (half.entries > 0 && probe.missedBudget == 0 && probe.entries - half.entries >= half.entries - half.entries / 8 &&
            (long double)probe.entries * scale * 0.9L > (long double)budget) {
            out.reset(nUtterances, nF, false);
            for (long long u = 0; u < nUtterances; ++u) out.eligible += eligible[u] ? 1 : 0;
            out.missedBudget = out.eligible;
            lap("given up after the look at the first utterances");
            return;
        }
    }
    lap("looked at the first utterances");
    // parts of about equal frame counts
    std::vector<long long> cut(nThreads + 1, nUtterances);
    cut[0] = 0;
    for (unsigned t = 1; t < nThreads; ++t)
        cut[t] = std::lower_bound(frameStart, frameStart + nUtterances, nF * (long long)t / nThreads) - frameStart;
    std::vector<TrackPlan> part(nThreads);
    std::atomic<unsigned long long> sum{0};
    run_parts(nThreads, [&](unsigned t) {
        plan_tracks_pass(cut[t + 1] - cut[t], frameStart + cut[t], frames, facts, meta, eligible + cut[t], budget, mask, false, &sum, part[t]);
    });
    lap("parts planned");
    // merge: shapes by value, fades by (from, to, length)
    struct ShapeKey { const double* v; bool operator==(const ShapeKey& o) const { return !memcmp(v, o.v, kShapeValues * sizeof(double)); } };
    struct ShapeKeyHash { size_t operator()(const ShapeKey& k) const { return (size_t)hash_shape(k.v); } };
    long long eligibleAll = 0, missedSize = 0, missedBudget = 0;
    size_t nShapesUpper = 0;
    for (const TrackPlan& p : part) { eligibleAll += p.eligible; missedSize += p.missedSize; missedBudget += p.missedBudget; nShapesUpper += p.shapes.size() / kShapeStride; }
    if (missedBudget > 0) { part.clear(); one_pass(); return; }
    std::vector<double> mergedShapes;
    mergedShapes.reserve(nShapesUpper * kShapeStride);     // no reallocation below: the keys point into it
    std::vector<TrackJob> mergedJobs;
    unsigned long long mergedEntries = 0;
    std::unordered_map<ShapeKey, uint32_t, ShapeKeyHash> shapes;
    std::unordered_map<FadeKey, unsigned long long, FadeKeyHash> fades;
    std::vector<std::unordered_map<unsigned long long, unsigned long long>> offOf(nThreads);   // part, its track's first entry -> the merged track's
    for (unsigned t = 0; t < nThreads; ++t) {
        const TrackPlan& p = part[t];
        std::vector<uint32_t> gid(p.shapes.size() / kShapeStride);
        for (size_t i = 0; i < gid.size(); ++i) {
            const ShapeKey key{&p.shapes[i * kShapeStride]};
            auto it = shapes.find(key);
            if (it == shapes.end()) {
                const uint32_t id = (uint32_t)(mergedShapes.size() / kShapeStride);
                mergedShapes.insert(mergedShapes.end(), key.v, key.v + kShapeStride);
                it = shapes.emplace(ShapeKey{&mergedShapes[(size_t)id * kShapeStride]}, id).first;
            }
            gid[i] = it->second;
        }
        for (const TrackJob& j : p.jobs) {
            const FadeKey key{gid[j.fromShape], gid[j.toShape], j.fadeSamples};
            auto it = fades.find(key);
            if (it == fades.end()) {
                it = fades.emplace(key, mergedEntries).first;
                mergedJobs.push_back(TrackJob{mergedEntries, key.from, key.to, j.fadeSamples, j.mask});
                mergedEntries += (unsigned long long)kTrackFirst + (unsigned long long)(j.fadeSamples - 1u) * track_slots(j.mask);
            }
            offOf[t].emplace(j.off, it->second);
        }
    }
    if (mergedEntries > budget) { one_pass(); return; }
    out.reset(nUtterances, nF, nF < 0xFFFFFFFFll);
    out.shapes.swap(mergedShapes);
    out.eligible = eligibleAll; out.missedSize = missedSize;
    if (missedSize * 10 > eligibleAll) return;   // all or nothing
    out.jobs.swap(mergedJobs);
    out.entries = mergedEntries;
    run_parts(nThreads, [&](unsigned t) {
        const TrackPlan& p = part[t];
        const long long f0 = frameStart[cut[t]];
        for (long long u = cut[t]; u < cut[t + 1]; ++u) {
            if (!p.tracked[u - cut[t]]) continue;
            out.tracked[u] = 1;
            out.kinds[u] = p.kinds[u - cut[t]];
            for (long long k = frameStart[u]; k < frameStart[u + 1]; ++k) {
                TrackRef r = p.ref[k - f0];
                r.off = offOf[t].find(r.off)->second;
                out.ref[k] = r;
                if (!out.rep.empty() && !p.rep.empty()) out.rep[k] = p.rep[k - f0];
            }
        }
    });
    lap("merged");
}

// Frames in device memory (speechPlayer_batch_setUtterancesDevice) and the track planner, which reads the values of a frame whose
// (masked) shape hash it has not seen yet (FrameSource::values): one frame per distinct hash among the frames it may read -- the
// non-silent frames of the lists that may be tracked --, the first in frame order, stands for all frames of that hash; rowOf[k] names
// frame k's row, rep[row] that first frame (rowOf is written for those frames only).  The engine gathers the rows on the device and
// downloads them.  Host threads over parts of the lists (one per `framesPerPart` frames, `nThreads` at most), each with a map of its
// own; the maps are merged in frame order.
inline void shape_table_rows(long long nL, const long long* listStart, const FrameMeta* meta, const FrameFacts* facts, const unsigned char* eligible,
                             HashMask mask, RawVector<uint32_t>& rowOf, std::vector<long long>& rep,
                             unsigned nThreads = host_threads(), long long framesPerPart = 65536)
{
    struct Part { std::unordered_map<Key128, uint32_t, Key128Hash> id; std::vector<long long> first; std::vector<Key128> keys; };
    const long long nF = listStart[nL];
    rowOf.resize((size_t)nF);
    const unsigned nT = (unsigned)std::max<long long>(1, std::min<long long>(nThreads, nF / framesPerPart + 1));
    std::vector<long long> cut(nT + 1, nL);
    cut[0] = 0;
    for (unsigned t = 1; t < nT; ++t) cut[t] = std::lower_bound(listStart, listStart + nL, nF * (long long)t / nT) - listStart;
    std::vector<Part> part(nT);
    auto each_frame = [&](unsigned t, auto fn) {
        for (long long l = cut[t]; l < cut[t + 1]; ++l)
            if (eligible[l])
                for (long long k = listStart[l]; k < listStart[l + 1]; ++k)
                    if (!(meta[k].flags & FRAME_NULL)) fn(k);
    };
    run_parts(nT, [&](unsigned t) {
        Part& p = part[t];
        each_frame(t, [&](long long k) {
            const Key128 key = Key128::of(facts[k], mask);
            auto it = p.id.find(key);
            if (it == p.id.end()) { it = p.id.emplace(key, (uint32_t)p.first.size()).first; p.first.push_back(k); p.keys.push_back(key); }
            rowOf[k] = it->second;
        });
    });
    std::unordered_map<Key128, uint32_t, Key128Hash> global;
    std::vector<std::vector<uint32_t>> remap(nT);
    rep.clear();
    for (unsigned t = 0; t < nT; ++t) {
        const Part& p = part[t];
        remap[t].resize(p.first.size());
        for (size_t i = 0; i < p.first.size(); ++i) {
            auto it = global.find(p.keys[i]);
            if (it == global.end()) { it = global.emplace(p.keys[i], (uint32_t)rep.size()).first; rep.push_back(p.first[i]); }
            remap[t][i] = it->second;
        }
    }
    run_parts(nT, [&](unsigned t) { each_frame(t, [&](long long k) { rowOf[k] = remap[t][rowOf[k]]; }); });
}

// The end points of the fades of one utterance's frames [k0, k1), appended to `out` (reference src/frame.cpp:55-72: a NULL request
// -- silence -- keeps the previous request's values with the gain gated off; the first frame after silence starts from its own
// values with the gain gated off; any other frame fades from the previous request's values).  klatt_seeds reads the values
// themselves on the device.  Host-only view for the tests: speechPlayer_planDirect.
template <class V>
void walk_fade_ends(long long k0, long long k1, const FrameMeta* meta, V& out)
{
    uint32_t prevReal = kNoFrame;
    bool prevNull = true;
    for (long long k = k0; k < k1; ++k) {
        DirectJob j;
        j.frame = (uint32_t)k;
        if (meta[k].flags & FRAME_NULL) {
            j.from = prevReal; j.to = prevReal;
            j.flags = (prevNull ? 1u : 0u) | 2u;
            prevNull = true;
        } else {
            j.to = (uint32_t)k;
            j.from = prevNull ? (uint32_t)k : prevReal;
            j.flags = prevNull ? 1u : 0u;
            prevReal = (uint32_t)k;
            prevNull = false;
        }
        out.push_back(j);
    }
}

}  // namespace klatt
