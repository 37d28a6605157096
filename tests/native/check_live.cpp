// check_live.cpp -- the host half of the live handles (nvspeechplayer_amd/csrc/klatt_live.h) as a stand-alone program.
// tests/test_host_logic.py builds it once with AddressSanitizer + UBSan and once with ThreadSanitizer; it prints "ok <checks>" and how
// often each branch below was reached, or the first failure.
//   1  a handle's frame queue against a model: a plain deque of (span, id) and a consumer that takes the next frame when the samples of
//      the current one are used up, driven by random queue / purge / pull calls the way the engine's pull loop drives it
//   2  the log's indices over an array of 8 entries
//   3  the plan of a pull, as a written-out table; the control block's offsets and its fill
//   4  the options: every name's clamps, the environment's defaults, setters beside snapshots
#include "../../nvspeechplayer_amd/csrc/klatt_live.h"

#include <stdio.h>
#include <deque>
#include <random>
#include <thread>

using namespace klatt;

static long long g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

enum Branch { kOnePiece, kSeveralPieces, kRefillEmptied, kRefillLeftSome, kCompacted, kPurgeBothSides, kBranches };
static const char* const kBranchNames[kBranches] = {"a pull in one piece", "a pull in several pieces", "refill emptied the host queue", "refill left some",
                                                    "the host queue compacted", "a purge with frames on both sides"};
static long long g_hits[kBranches];

// ---- 1 -----------------------------------------------------------------------------------------------------------------------------
// the model's own span: samples from a frame's dequeue to the next one's (reference src/frame.cpp:54-75), capped to 32 bits
static unsigned long long model_span(uint32_t minSamples, uint32_t fadeSamples)
{
    unsigned long long v = minSamples;
    if (v < (unsigned long long)fadeSamples + 1) v = (unsigned long long)fadeSamples + 1;
    v += 1;
    return v > 0xFFFFFFFFull ? 0xFFFFFFFFull : v;
}

struct Item { unsigned long long span; long long id; };

struct Handle {
    FrameQueue q;
    std::deque<Item> model;              // every queued frame the consumer has not taken, in queue order
    unsigned long long left = 0;         // the consumer: samples left in the frame it took last
    long long ringId[kRing];             // what each ring position holds: the id of an untaken frame, or -1
    long long nextId = 0;                // ids count up in queue order
    long long nextToRing = 0;            // the id that reaches the ring next
    bool purged = false;                 // the model's side of purgePending
    Handle() { for (long long& r : ringId) r = -1; }

    size_t host_waiting() const { return q.overflow.size() - q.overHead; }
    void to_ring(long long id, uint32_t pos)
    {
        CHECK(pos < kRing && ringId[pos] == -1);         // never a position that holds an untaken frame
        CHECK(id == nextToRing);                         // frames reach the ring in queue order
        ringId[pos] = id;
        nextToRing = id + 1;
    }
    void queue(uint32_t minSamples, uint32_t fadeSamples)
    {
        FrameMeta m{minSamples, fadeSamples, -1, 0u};
        const long long id = nextId++;
        model.push_back(Item{model_span(minSamples, fadeSamples), id});
        if (q.takes_now()) to_ring(id, q.claim(m));
        else {
            double p[kNumParams] = {0.0};
            p[0] = (double)id;
            q.push_host(p, m);
        }
    }
    void purge()
    {
        if (q.ringCount > 0 && host_waiting() > 0) ++g_hits[kPurgeBothSides];
        for (uint32_t k = 0; k < q.ringCount; ++k) ringId[(q.ringHead + k) & (kRing - 1)] = -1;
        q.purge();
        CHECK(q.ringCount == 0 && q.overflow.empty() && q.overHead == 0 && q.purgePending);
        model.clear();                                   // nothing queued before a purge is ever taken: the consumer checks ids
        nextToRing = nextId;
        purged = true;
    }
    // the kernel, for `piece` samples over the ring as it is: returns the frames it took
    uint32_t consume(unsigned int piece)
    {
        CHECK(q.purgePending == purged);
        if (purged) { left = 0; purged = false; }         // the state half of a purge: the next sample dequeues
        uint32_t taken = 0;
        unsigned int produced = 0;
        while (produced < piece) {
            if (left == 0) {
                if (taken == q.ringCount) { CHECK(model.empty() && host_waiting() == 0); break; }     // ran dry: a short count
                // the ring's last frame is dequeued only when nothing waits on the host to follow it
                if (taken + 1 == q.ringCount) CHECK(host_waiting() == 0);
                const uint32_t pos = (q.ringHead + taken) & (kRing - 1);
                CHECK(!model.empty() && ringId[pos] == model.front().id && q.span[pos] == model.front().span);
                left = model.front().span;
                model.pop_front();
                ringId[pos] = -1;
                ++taken;
            }
            const unsigned long long step = std::min<unsigned long long>(left, piece - produced);
            left -= step;
            produced += (unsigned int)step;
        }
        return taken;
    }
    // the engine's pull loop: refill, how far, launch, apply -- piece by piece
    void pull(unsigned int count)
    {
        unsigned int at = 0, pieces = 0;
        while (at < count) {
            const size_t before = host_waiting(), headBefore = q.overHead;
            const int rc = q.refill([&](const PendingFrame& f, uint32_t pos) { to_ring((long long)f.p[0], pos); return 0; });
            CHECK(rc == 0);
            if (before > 0) {
                ++g_hits[host_waiting() == 0 ? kRefillEmptied : kRefillLeftSome];
                if (host_waiting() > 0 && q.overHead == 0 && headBefore + (before - host_waiting()) > 0) ++g_hits[kCompacted];
                CHECK(host_waiting() == 0 || q.ringCount == kRing);
            }
            const unsigned int piece = q.reach(count - at);
            // at least one sample while anything is asked for: a frame's span is at least 2, and a ring with frames waiting behind it
            // is full, so the spans of all its frames but the last come to 510 or more
            CHECK(piece >= 1 && piece <= count - at);
            const uint32_t k = consume(piece);
            CHECK(k <= q.ringCount);
            q.took(k);
            at += piece;
            ++pieces;
        }
        CHECK(at == count);                              // the pieces sum to the pull
        ++g_hits[pieces == 1 ? kOnePiece : kSeveralPieces];
    }
    // the frames not taken yet, ring first, then the host queue
    std::vector<long long> waiting_ids() const
    {
        std::vector<long long> ids;
        for (uint32_t k = 0; k < q.ringCount; ++k) ids.push_back(ringId[(q.ringHead + k) & (kRing - 1)]);
        for (size_t j = q.overHead; j < q.overflow.size(); ++j) ids.push_back((long long)q.overflow[j].p[0]);
        return ids;
    }
};

static void queue_against_the_model(std::mt19937_64& rng)
{
    auto below = [&](unsigned long long n) { return (unsigned long long)(rng() % n); };
    std::vector<Handle> handles(4);
    auto burst = [&](Handle& h, unsigned frames) {
        for (unsigned f = 0; f < frames; ++f) {
            if (below(3000) == 0) { h.queue(0xFFFFFFFFu, (uint32_t)below(2) * 0xFFFFFFFFu); continue; }      // a span capped at 2^32 - 1
            const uint32_t minS = (uint32_t)below(60), fade = (uint32_t)below(minS + 1);      // spans 2 .. 60
            h.queue(minS, fade);
        }
    };
    for (int op = 0; op < 6000; ++op) {
        Handle& h = handles[below(handles.size())];
        const unsigned what = (unsigned)below(100);
        if (what < 42) burst(h, (unsigned)(below(2) ? below(901) : below(21)));
        else if (what < 50) { h.purge(); burst(h, 1 + (unsigned)(below(2) ? below(900) : below(20))); }
        else {
            // a pull of a + b samples leaves the frames not taken (ring and host queue together: where the line between the two runs
            // depends on when the last refill was) and the consumer where pulls of a and then b leave them
            const unsigned int count = 1 + (unsigned int)below(20000), a = (unsigned int)below(count + 1);
            Handle twice = h;
            h.pull(count);
            if (a) twice.pull(a);
            if (count - a) twice.pull(count - a);
            CHECK(twice.left == h.left && twice.model.size() == h.model.size() && twice.q.purgePending == h.q.purgePending);
            CHECK(twice.waiting_ids() == h.waiting_ids());
            std::vector<long long> ids = h.waiting_ids();
            CHECK(ids.size() == h.model.size());
            for (size_t j = 0; j < ids.size(); ++j) if (ids[j] != h.model[j].id) CHECK(ids[j] == h.model[j].id);
        }
    }
}

// ---- 2 -----------------------------------------------------------------------------------------------------------------------------
static void the_log_indices()
{
    struct Entry { double value; uint32_t target; };      // (the engine's entry holds a frame; the indices know its target only)
    Entry storage[8];
    memset(storage, 0, sizeof storage);
    LogIndex<Entry> log;
    log.entries = storage; log.cap = 8;
    LogMine a, b;
    // full at 8 and not before
    for (int i = 0; i < 8; ++i) {
        Entry* e = log.append(i % 2 ? b : a);
        CHECK(e == &storage[i]);
        e->target = 100u + (uint32_t)i;
    }
    CHECK(log.append(a) == nullptr && log.append(b) == nullptr && log.waiting() == 8 && a.idx.size() == 4 && b.idx.size() == 4);
    // un-target marks exactly that handle's waiting entries
    log.untarget(a);
    for (int i = 0; i < 8; ++i) CHECK(storage[i].target == (i % 2 ? 100u + (uint32_t)i : kNoTarget));
    CHECK(a.idx.empty() && b.idx.size() == 4);
    // ... and none after a send
    const uint32_t epoch = log.epoch;
    log.mark_sent();
    CHECK(log.waiting() == 0 && log.epoch != epoch && log.tail == 8 && log.sent == 8 && log.append(b) == nullptr);
    log.untarget(b);
    for (int i = 0; i < 8; ++i) CHECK(storage[i].target == (i % 2 ? 100u + (uint32_t)i : kNoTarget));
    CHECK(b.idx.empty());
    // after sent and arrived it starts over at 0
    log.arrived();
    CHECK(log.tail == 0 && log.sent == 0);
    CHECK(log.append(a) == &storage[0] && log.append(b) == &storage[1] && log.append(a) == &storage[2]);
    CHECK(a.idx.size() == 2 && a.idx[0] == 0 && a.idx[1] == 2 && b.idx.size() == 1 && b.idx[0] == 1);
    // a handle's index list is dropped when the epoch moves
    log.mark_sent();
    CHECK(log.append(a) == &storage[3] && a.idx.size() == 1 && a.idx[0] == 3 && log.waiting() == 1);
    // something still waits: nothing starts over, and the log is full at 8 again
    log.arrived();
    CHECK(log.tail == 4 && log.sent == 3);
    for (int i = 4; i < 8; ++i) CHECK(log.append(b) == &storage[i]);
    CHECK(log.append(b) == nullptr && b.idx.size() == 4 && b.idx[0] == 4);
    storage[3].target = 7u; storage[4].target = 9u;
    log.untarget(a);
    CHECK(storage[3].target == kNoTarget && storage[4].target != kNoTarget);
}

// ---- 3 -----------------------------------------------------------------------------------------------------------------------------
static LiveSettings settings(int layout, int replicate, int alone, int cus)
{
    LiveSettings s{};
    s.layout = layout; s.replicate = replicate; s.alone = alone; s.cus = cus;
    return s;
}

static void the_pull_plan()
{
    // layout 0: the lane kernel, an entry per handle, no replicas -- whatever the other options say
    for (int n : {1, 5, 64, 65})
        for (int replicate : {0, 1}) {
            const PullPlan p = pull_plan(n, settings(0, replicate, 1536, 0), 256);
            CHECK(p.launch == LiveLaunch::Lane && p.nCtl == n && !p.replicate && !p.fillSparse && p.rep == 1 && p.nResults == n && p.groups == (n + 63) / 64);
        }
    // up to live_alone handles: a workgroup of 64 replicas each
    for (int n : {1, 2, 1536}) {
        const PullPlan p = pull_plan(n, settings(1, 1, 1536, 0), 256);
        CHECK(p.launch == LiveLaunch::Lone && p.replicate && !p.fillSparse && p.rep == 64 && p.nCtl == 64 * n && p.groups == n && p.nResults == 64 * n);
    }
    {
        const PullPlan p = pull_plan(1537, settings(1, 1, 1536, 0), 256);
        CHECK(p.launch == LiveLaunch::StreamOnePerCu && !p.replicate && !p.fillSparse && p.rep == 1 && p.nCtl == 1537 && p.groups == 25 && p.nResults == 1537);
    }
    // live_alone 1: only a handle pulled alone
    {
        const PullPlan p = pull_plan(1, settings(1, 1, 1, 0), 256);
        CHECK(p.launch == LiveLaunch::Lone && p.replicate && p.nCtl == 64 && p.groups == 1 && p.nResults == 64);
    }
    for (int n : {2, 5, 31}) {       // fewer than half a wavefront: the empty lanes are filled
        const PullPlan p = pull_plan(n, settings(1, 1, 1, 0), 256);
        CHECK(p.launch == LiveLaunch::StreamOnePerCu && !p.replicate && p.fillSparse && p.rep == 1 && p.nCtl == 64 && p.groups == 1 && p.nResults == n);
    }
    for (int n : {32, 64}) {
        const PullPlan p = pull_plan(n, settings(1, 1, 1, 0), 256);
        CHECK(p.launch == LiveLaunch::StreamOnePerCu && !p.replicate && !p.fillSparse && p.nCtl == n && p.groups == 1 && p.nResults == n);
    }
    // live_alone 7: the boundary between the two policies
    {
        const PullPlan p7 = pull_plan(7, settings(1, 1, 7, 0), 256), p8 = pull_plan(8, settings(1, 1, 7, 0), 256);
        CHECK(p7.launch == LiveLaunch::Lone && p7.replicate && p7.nCtl == 448 && p7.groups == 7 && p7.nResults == 448);
        CHECK(p8.launch == LiveLaunch::StreamOnePerCu && !p8.replicate && p8.fillSparse && p8.nCtl == 64 && p8.groups == 1 && p8.nResults == 8);
    }
    // live_alone below 1 counts as 1 (a snapshot never holds one; the plan does not rely on that)
    CHECK(pull_plan(1, settings(1, 1, 0, 0), 256).launch == LiveLaunch::Lone && pull_plan(2, settings(1, 1, 0, 0), 256).fillSparse);
    // live_replicate 0: no replicas, no fill
    for (int n : {1, 2, 31, 64, 1536, 1537}) {
        const PullPlan p = pull_plan(n, settings(1, 0, 1536, 0), 256);
        CHECK(p.launch == LiveLaunch::StreamOnePerCu && !p.replicate && !p.fillSparse && p.rep == 1 && p.nCtl == n && p.nResults == n && p.groups == (n + 63) / 64);
    }
    // one workgroup per CU while they all fit: the device's 256 CUs ...
    CHECK(pull_plan(16384, settings(1, 1, 1536, 0), 256).launch == LiveLaunch::StreamOnePerCu && pull_plan(16384, settings(1, 1, 1536, 0), 256).groups == 256);
    CHECK(pull_plan(16385, settings(1, 1, 1536, 0), 256).launch == LiveLaunch::StreamTwoPerCu && pull_plan(16385, settings(1, 1, 1536, 0), 256).groups == 257);
    CHECK(pull_plan(16384, settings(1, 1, 1536, 0), 64).launch == LiveLaunch::StreamTwoPerCu);      // (another device)
    // ... or "live_cus" forced to 1 (with live_alone 1, so that 64 handles share a wavefront), which the device's count does not change
    CHECK(pull_plan(64, settings(1, 1, 1, 1), 256).launch == LiveLaunch::StreamOnePerCu);
    CHECK(pull_plan(65, settings(1, 1, 1, 1), 256).launch == LiveLaunch::StreamTwoPerCu && pull_plan(65, settings(1, 1, 1, 1), 256).groups == 2);
    CHECK(pull_plan(65, settings(1, 1, 1, 2), 1).launch == LiveLaunch::StreamOnePerCu);
}

static void the_control_block()
{
    static_assert(sizeof(UttDesc) == 32 && sizeof(double*) == 8 && sizeof(UttResult) == 16, "the control block's entries");
    for (size_t nCtl : {(size_t)1, (size_t)64, (size_t)448, (size_t)1537}) {
        const CtlBlock b{nCtl};
        CHECK(b.state_offset() == 32 * nCtl && b.control_offset() == 40 * nCtl && b.bytes() == 44 * nCtl);
        unsigned char* base = reinterpret_cast<unsigned char*>((uintptr_t)4096);      // (an address only: nothing is read)
        const CtlBlock::View v = b.at(base);
        CHECK(reinterpret_cast<unsigned char*>(v.utt) == base && reinterpret_cast<unsigned char*>(v.state) == base + 32 * nCtl &&
              reinterpret_cast<unsigned char*>(v.control) == base + 40 * nCtl);
    }
    double states[8];
    auto entry = [&](int i) {
        CtlEntry e;
        e.utt = UttDesc{1000ll + i, 32ll * i, (uint32_t)(10 + i), (uint32_t)(20 + i), UTT_NEEDS_NOISE, 77u};
        e.state = &states[i];
        e.control = (i & 1) ? 1u : 0u;
        return e;
    };
    auto same = [](const CtlBlock::View& v, size_t j, const CtlEntry& e, uint32_t control) {
        return memcmp(&v.utt[j], &e.utt, sizeof(UttDesc)) == 0 && v.state[j] == e.state && v.control[j] == control;
    };
    // the blocks are allocated to their exact size: a write beyond is an AddressSanitizer report
    {   // replicas: entry 64 i into 64 i + 1 .. 64 i + 63, control bit 1 set in all of them
        const int n = 3;
        const PullPlan p = pull_plan(n, settings(1, 1, 1536, 0), 256);
        const CtlBlock b{(size_t)p.nCtl};
        std::vector<double> mem(b.bytes() / 8);
        CHECK(mem.size() * 8 == b.bytes());
        const CtlBlock::View v = b.at(reinterpret_cast<unsigned char*>(mem.data()));
        fill_ctl(v, p, n, entry);
        for (int i = 0; i < n; ++i)
            for (size_t j = 64 * (size_t)i; j < 64 * (size_t)(i + 1); ++j) CHECK(same(v, j, entry(i), entry(i).control | 2u));
    }
    {   // the sparse fill: entry i holds what entry i % n holds
        const int n = 5;
        const PullPlan p = pull_plan(n, settings(1, 1, 1, 0), 256);
        const CtlBlock b{(size_t)p.nCtl};
        std::vector<double> mem(b.bytes() / 8);
        const CtlBlock::View v = b.at(reinterpret_cast<unsigned char*>(mem.data()));
        fill_ctl(v, p, n, entry);
        for (size_t j = 0; j < 64; ++j) CHECK(same(v, j, entry((int)(j % n)), entry((int)(j % n)).control));
    }
    {   // neither: an entry per handle
        const int n = 7;
        const PullPlan p = pull_plan(n, settings(0, 1, 1536, 0), 256);
        const CtlBlock b{(size_t)p.nCtl};
        std::vector<uint32_t> mem(b.bytes() / 4 + 1);      // 44 * 7 bytes, 8-aligned by the allocator
        const CtlBlock::View v = b.at(reinterpret_cast<unsigned char*>(mem.data()));
        fill_ctl(v, p, n, entry);
        for (size_t j = 0; j < (size_t)n; ++j) CHECK(same(v, j, entry((int)j), entry((int)j).control));
    }
}

// ---- 4 -----------------------------------------------------------------------------------------------------------------------------
static bool producible(const LiveSettings& s)
{
    return (s.layout == 0 || s.layout == 1) && s.cus >= 0 && (s.replicate == 0 || s.replicate == 1) && (s.mode == 0 || s.mode == 1) &&
           s.alone >= 1 && s.alone <= 65536 && (s.trim == 0 || s.trim == 1);
}

static void the_options()
{
    LiveOptions o;
    LiveSettings d = o.snapshot();
    CHECK(d.layout == 1 && d.cus == 0 && d.replicate == 1 && d.mode == 0 && d.alone == 1536 && d.trim == 0);
    // every name stores and clamps as its comment says
    CHECK(o.set("live_layout", 0) == 0 && o.snapshot().layout == 0);
    CHECK(o.set("live_layout", 5) == 0 && o.snapshot().layout == 1);
    CHECK(o.set("live_layout", -3) == 0 && o.snapshot().layout == 1);
    CHECK(o.set("live_cus", 7) == 0 && o.snapshot().cus == 7);
    CHECK(o.set("live_cus", -5) == 0 && o.snapshot().cus == 0);
    CHECK(o.set("live_replicate", 0) == 0 && o.snapshot().replicate == 0);
    CHECK(o.set("live_replicate", 9) == 0 && o.snapshot().replicate == 1);
    CHECK(o.set("live_mode", 1) == 0 && o.snapshot().mode == 1);
    CHECK(o.set("live_mode", 2) == -1 && o.snapshot().mode == 1);        // refused: the value stays
    CHECK(o.set("live_mode", -1) == -1 && o.snapshot().mode == 1);
    CHECK(o.set("live_mode", 0) == 0 && o.snapshot().mode == 0);
    CHECK(o.set("live_alone", 7) == 0 && o.snapshot().alone == 7);
    CHECK(o.set("live_alone", 0) == 0 && o.snapshot().alone == 1);
    CHECK(o.set("live_alone", -9) == 0 && o.snapshot().alone == 1);
    CHECK(o.set("live_alone", 65536) == 0 && o.snapshot().alone == 65536);
    CHECK(o.set("live_alone", 65537) == 0 && o.snapshot().alone == 65536);
    CHECK(o.set("live_trim", 3) == 0 && o.snapshot().trim == 1);
    CHECK(o.set("live_trim", 0) == 0 && o.snapshot().trim == 0);
    // not a live option: nothing changes
    const LiveSettings before = o.snapshot();
    CHECK(o.set("no_such_option", 1) == 1 && o.set(nullptr, 1) == 1 && o.set("plan_hash_bits", 6) == 1 && o.set("live_", 1) == 1);
    const LiveSettings after = o.snapshot();
    CHECK(memcmp(&before, &after, sizeof before) == 0);
    // the environment's defaults go through the same clamps; a refused value leaves the default
    setenv("SPEECHPLAYER_LIVE_ALONE", "70000", 1); setenv("SPEECHPLAYER_LIVE_MODE", "2", 1);
    setenv("SPEECHPLAYER_LIVE_LAYOUT", "0", 1); setenv("SPEECHPLAYER_LIVE_REPLICATE", "5", 1);
    const LiveSettings e = LiveOptions().snapshot();
    CHECK(e.alone == 65536 && e.mode == 0 && e.layout == 0 && e.replicate == 1 && e.cus == 0 && e.trim == 0);
    setenv("SPEECHPLAYER_LIVE_MODE", "1", 1); setenv("SPEECHPLAYER_LIVE_ALONE", "-4", 1);
    const LiveSettings f = LiveOptions().snapshot();
    CHECK(f.mode == 1 && f.alone == 1);
    for (const char* name : {"SPEECHPLAYER_LIVE_ALONE", "SPEECHPLAYER_LIVE_MODE", "SPEECHPLAYER_LIVE_LAYOUT", "SPEECHPLAYER_LIVE_REPLICATE"}) unsetenv(name);

    // four threads set options in a loop, two take 10^5 snapshots each: every snapshot holds values the setter can produce
    // (no CHECK on another thread: its counter is the main thread's)
    std::atomic<bool> stop{false}, bad{false};
    std::atomic<long long> sets{0};
    std::vector<std::thread> threads;
    static const char* const kNames[] = {"live_layout", "live_cus", "live_replicate", "live_mode", "live_alone", "live_trim", "no_such_option"};
    static const int kValues[] = {0, 1, -1, 2, 7, 1536, 65536, 70000, -2147483647 - 1, 2147483647};
    for (unsigned t = 0; t < 4; ++t)
        threads.emplace_back([&, t] {
            for (unsigned k = t; !stop.load(std::memory_order_relaxed); ++k) {
                (void)o.set(kNames[k % 7], kValues[(k / 7 + t) % 10]);
                sets.fetch_add(1, std::memory_order_relaxed);
            }
        });
    for (int t = 0; t < 2; ++t)
        threads.emplace_back([&] {
            for (int k = 0; k < 100000; ++k)
                if (!producible(o.snapshot())) bad.store(true);
        });
    threads[4].join(); threads[5].join();
    stop.store(true);
    for (int t = 0; t < 4; ++t) threads[(size_t)t].join();
    CHECK(!bad.load() && sets.load() > 0 && producible(o.snapshot()));
}

int main()
{
    std::mt19937_64 rng(20241020);
    queue_against_the_model(rng);
    the_log_indices();
    the_pull_plan();
    the_control_block();
    the_options();
    printf("ok %lld checks\n", g_checks);
    bool all = true;
    for (int i = 0; i < kBranches; ++i) {
        printf("  %s: %lld\n", kBranchNames[i], g_hits[i]);
        all = all && g_hits[i] > 0;
    }
    if (!all) { printf("FAILED: a branch was never reached\n"); return 1; }
    return 0;
}
