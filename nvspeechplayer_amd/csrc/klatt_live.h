// klatt_live.h -- the host half of the live handles (the streams behind the reference's five entry points, klatt_engine.hip) that
// touches no device: the process-wide live options, a handle's frame queue (its ring on the device and what waits on the host), the
// indices of the pinned log, and the plan of one pull with its control block.  Plain C++17: no HIP include;
// tests/native/check_live.cpp holds it to account under AddressSanitizer + UBSan and ThreadSanitizer.  The arena, the log's memory and
// its way to the device, every launch and every copy stay in the engine.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <vector>

#include "klatt_consts.h"
#include "klatt_layout.h"

namespace klatt {

constexpr uint32_t kRing = 256;                  // frames of a handle on the device; further ones wait on the host (FrameQueue::overflow)
constexpr uint32_t kNoTarget = 0xFFFFFFFFu;

struct PendingFrame {
    double p[kNumParams];
    FrameMeta meta;
};

inline uint32_t frame_span(const FrameMeta& m)      // samples from this frame's dequeue to the next one's, the closed form of speechPlayer_batch_setUtterances
{
    const unsigned long long v = std::max<unsigned long long>(m.minSamples, (unsigned long long)m.fadeSamples + 1) + 1;
    return (uint32_t)std::min<unsigned long long>(v, 0xFFFFFFFFull);
}

// ---- (a) the live options ------------------------------------------------------------------------------------------------------
// Process-wide, set by name (speechPlayer_setGlobalOption, from any thread) and read as ONE snapshot: a pull takes it on entry and
// finishes under it, whatever is set meanwhile.  The environment's defaults (SPEECHPLAYER_LIVE_*) go through the same setter.
struct LiveSettings {
    int layout;              // which kernel advances live handles: 1 = the stage-parallel kernel's STREAM instantiation (four wavefronts per
                             // 64 handles; default), 0 = the lane kernel's (one wavefront per 64 handles).  Same saved state, same PCM
    int cus;                 // above 0: this many workgroups of live handles count as one per CU; 0: the pulled device's CU count
    int replicate;           // a lone handle fills its wavefront (pull_plan)
    int mode;                // arithmetic mode of handles created from now on: 0 MODE_EXACT, 1 MODE_FAST
    int alone;               // pulls of up to this many handles: a wavefront per handle (pull_plan)
    int trim;                // release a device's arena when its last handle is terminated
};
class LiveOptions {
public:
    LiveOptions()
    {
        static const char* const kEnv[][2] = {{"SPEECHPLAYER_LIVE_LAYOUT", "live_layout"}, {"SPEECHPLAYER_LIVE_REPLICATE", "live_replicate"},
                                              {"SPEECHPLAYER_LIVE_MODE", "live_mode"}, {"SPEECHPLAYER_LIVE_ALONE", "live_alone"}};
        for (const auto& e : kEnv)
            if (const char* v = getenv(e[0])) (void)set(e[1], atoi(v));      // (a refused value leaves the default)
    }
    // 0: stored; -1: a value the option does not take; 1: not a live option
    int set(const char* name, int value)
    {
        if (!name) return 1;
        if (!strcmp(name, "live_layout")) return put(layout_, value ? 1 : 0);
        // "live_cus": how many workgroups of live handles count as one per CU (0: the device's CU count).  Beyond it a pull of live handles
        // takes the two-workgroups-per-CU instantiation of the stream kernel -- on a 256-CU device from 16 385 handles on; a small value
        // lets a test (or a small device) reach that kernel with a few hundred handles.
        if (!strcmp(name, "live_cus")) return put(cus_, value < 0 ? 0 : value);
        // "live_replicate": 1 (default) a handle pulled alone is advanced in all 64 lanes of its wavefront (pull_plan); 0: in one lane
        if (!strcmp(name, "live_replicate")) return put(replicate_, value ? 1 : 0);
        // "live_mode": the arithmetic mode of handles created from now on -- 0 (default) MODE_EXACT, 1 MODE_FAST (fused multiply-adds in the filters)
        if (!strcmp(name, "live_mode")) return value == 0 || value == 1 ? put(mode_, value) : -1;
        // "live_alone": pulls of up to this many handles give every handle a wavefront of its own (default 1536; 1: only a handle pulled alone)
        if (!strcmp(name, "live_alone")) return put(alone_, value < 1 ? 1 : (value > 65536 ? 65536 : value));
        // "live_trim": 1 = a device's arena of live handles (~100 KB of HBM per slot, grown by doubling) is released when the last handle on
        // that device is terminated -- and now, on devices where none lives (the engine's sweep); 0 (default): it stays for the next handles.
        if (!strcmp(name, "live_trim")) return put(trim_, value ? 1 : 0);
        return 1;
    }
    LiveSettings snapshot() const
    {
        return LiveSettings{get(layout_), get(cus_), get(replicate_), get(mode_), get(alone_), get(trim_)};
    }
private:
    static int put(std::atomic<int>& f, int v) { f.store(v, std::memory_order_relaxed); return 0; }
    static int get(const std::atomic<int>& f) { return f.load(std::memory_order_relaxed); }
    std::atomic<int> layout_{1}, cus_{0}, replicate_{1}, mode_{0}, alone_{1536}, trim_{0};
};

// ---- (b) a handle's frame queue ------------------------------------------------------------------------------------------------
// The ring of kRing frames the handle owns on the device, as the host accounts for it, and the frames queued beyond it, which wait on
// the host until a pull refills the ring.  The owner's mutex is held around every call.
struct FrameQueue {
    uint32_t ringHead = 0;               // ring position of the oldest frame the kernel has not taken
    uint32_t ringCount = 0;              // frames in the ring from there on (travelled, or waiting in the log)
    uint32_t span[kRing];                // frame_span of each ring position; read only while frames wait in `overflow`
    std::vector<PendingFrame> overflow;  // queued beyond the ring: overflow[overHead ..], in order
    size_t overHead = 0;
    bool purgePending = false;

    // A queued frame goes into the ring while the ring has room and nothing waits on the host, else into the host queue, from where the
    // next pulls refill the ring.
    bool takes_now() const { return overHead == overflow.size() && ringCount < kRing; }
    // the next ring position, for a frame (ringCount < kRing: takes_now, or refill's own look)
    uint32_t claim(const FrameMeta& meta)
    {
        const uint32_t pos = (ringHead + ringCount) & (kRing - 1);
        span[pos] = frame_span(meta);
        ringCount++;
        return pos;
    }
    void unclaim() { ringCount--; }      // the frame of the last claim could not be sent after all
    // (copied: the caller may reuse its frame, reference src/frame.cpp:97)
    void push_host(const double* p, const FrameMeta& meta)
    {
        PendingFrame f;
        memset(&f, 0, sizeof f);
        f.meta = meta;
        if (p) memcpy(f.p, p, sizeof f.p);
        overflow.push_back(f);
    }
    // forget what the ring holds (close; the ring half of a purge)
    void drop()
    {
        ringHead = (ringHead + ringCount) & (kRing - 1);
        ringCount = 0;
    }
    // A purge request (reference src/frame.cpp:103-112): what the handle queued is forgotten, in the ring and on the host; the state
    // half of the purge runs in the kernel before the next sample.
    void purge()
    {
        drop();
        overflow.clear(); overHead = 0;
        purgePending = true;
    }
    // The ring takes what waited on the host, in order: give(frame, ring position) sends each on its way and returns non-zero if it
    // cannot (the frame then stays where it was, and refill returns -1).
    template <class Give>
    int refill(Give&& give)
    {
        if (overHead == overflow.size()) return 0;
        while (ringCount < kRing && overHead < overflow.size()) {
            const PendingFrame& f = overflow[overHead];
            if (give(f, claim(f.meta))) { unclaim(); return -1; }
            overHead++;
        }
        if (overHead == overflow.size()) { overflow.clear(); overHead = 0; }
        else if (overHead >= 64 && overHead * 2 >= overflow.size()) { overflow.erase(overflow.begin(), overflow.begin() + (long)overHead); overHead = 0; }
        return 0;
    }
    // How far of `want` samples may the next launch go?  While frames wait on the host, the ring's last frame may be dequeued only
    // when its successor is there to follow it: up to the spans of all the ring's frames but the last.
    unsigned int reach(unsigned int want) const
    {
        if (overHead == overflow.size()) return want;
        unsigned long long safe = 0;
        for (uint32_t k = 0; k + 1 < ringCount && safe < want; ++k) safe += span[(ringHead + k) & (kRing - 1)];
        return (unsigned int)std::min<unsigned long long>(want, safe);
    }
    // the kernel took k of the ring's frames (k <= ringCount), and ran the purge if one was pending
    void took(uint32_t k)
    {
        purgePending = false;
        ringHead = (ringHead + k) & (kRing - 1);
        ringCount -= k;
    }
};

// ---- (c) the log's indices -----------------------------------------------------------------------------------------------------
// A queued frame is written once, into a log that travels to the device in one copy.  These are its indices, over storage that the
// owner allocates: entries [sent, tail) have not travelled.  Sending, waiting and the lock around all of it are the owner's, and so
// is the entry's layout, of which only `target` is known here (the engine's LogEntry, which its scatter kernel reads).
struct LogMine {                         // one handle's entries in the part of the log that has not travelled
    uint32_t epoch = 0;                  // idx is valid for this epoch of the log only
    std::vector<uint32_t> idx;
};
template <class Entry>
struct LogIndex {
    using Mine = LogMine;
    Entry* entries = nullptr;
    size_t cap = 0;
    size_t tail = 0, sent = 0;
    uint32_t epoch = 1;                  // moves with every send
    size_t waiting() const { return tail - sent; }
    // the next entry, for the handle to fill; nullptr: the log is full (the owner sends it, waits, calls arrived())
    Entry* append(Mine& m)
    {
        if (tail == cap) return nullptr;
        if (m.epoch != epoch) { m.idx.clear(); m.epoch = epoch; }
        m.idx.push_back((uint32_t)tail);
        return &entries[tail++];
    }
    void mark_sent() { sent = tail; epoch++; }      // [sent, tail) is on its way: every Mine is stale from here on
    void arrived() { if (sent == tail) sent = tail = 0; }      // everything sent has arrived: an empty log starts over
    // the handle's waiting entries go nowhere (purge, close)
    void untarget(Mine& m)
    {
        if (m.epoch == epoch)
            for (uint32_t i : m.idx) entries[i].target = kNoTarget;
        m.idx.clear();
    }
};

// ---- (d) the plan of one pull ---------------------------------------------------------------------------------------------------
enum class LiveLaunch {
    Lane,                    // the lane kernel's STREAM instantiation
    Lone,                    // the stage-parallel kernel's LONE instantiation: 64 replicas of one handle per workgroup
    StreamOnePerCu,          // the stage-parallel kernel, one workgroup per CU (16-sample hand-overs)
    StreamTwoPerCu,          // two per CU (8-sample hand-overs), as for batches
};
struct PullPlan {
    bool replicate, fillSparse;
    int rep;                 // control entries (lanes) per handle
    int nCtl;                // control entries of the launch
    long long groups;        // its workgroups
    int nResults;            // results that come back
    LiveLaunch launch;
};
// A LONE handle -- the reference's own use (one stream pulled 8192 samples at a time, nvdaAddon/synthDrivers/nvSpeechPlayer/__init__.py:62-81)
// -- is advanced in ALL 64 lanes of its wavefront: every lane is given the same control entry (same state block, same ring, same PCM
// row) and computes the same samples; they store the same values to the same places.  A wavefront with one active lane runs the same
// instructions but, measured, takes 1.0 / 1.4 / 1.7 times as long from launch to launch (4.3 / 6.1 / 7.4 ms for one cfg2 utterance
// against a steady 4.13 ms with 16 or more lanes active: tools/lone_probe2.py); with all lanes active a pull costs what 64 handles cost:
// thirty 8192-sample pulls of one handle 3.05 -> 2.04 ms of kernel time on average (tools/single_stream_ab.sh).  The launch then takes
// the kernel's LONE instantiation, whose fade chunks are computed side by side across the identical lanes (klatt_systolic.h,
// stage_loop: 2.04 -> 1.84 ms); control bit 1 marks the entries.
// The same goes for a pull of SEVERAL handles, up to "live_alone" of them (default 1536: six rounds of 256 workgroups; the two policies meet near 1850 unrelated handles): a workgroup per handle, 64 replicas each.  Handles
// that share a wavefront pay for one another -- with unrelated handles every chunk has some lane at an event or in a fade and runs sample
// by sample: 11.7 ms per 8192-sample pull however few they are -- while a handle alone in its wavefront costs 1.3-1.7 ms and 256 of them
// run side by side, one per CU (the LONE instantiation's LDS allows one workgroup per CU): n handles take ceil(n / CUs) rounds of that.
// (A FEW handles pulled together -- fewer than half a wavefront -- get their empty lanes filled with replicas of themselves too, on the
// ordinary kernel: the same effect, and the same remedy as for the sparse wavefronts of a batch.)
// deviceCus: the pulled device's CU count, which "live_cus" above 0 overrides.
inline PullPlan pull_plan(int n, const LiveSettings& o, int deviceCus)
{
    PullPlan p;
    p.replicate = n >= 1 && n <= std::max(1, o.alone) && o.layout != 0 && o.replicate;
    p.rep = p.replicate ? kLanes : 1;
    p.fillSparse = !p.replicate && n > 1 && n < kLanes / 2 && o.layout != 0 && o.replicate;
    p.nCtl = p.replicate ? n * kLanes : (p.fillSparse ? kLanes : n);
    p.groups = (p.nCtl + kLanes - 1) / kLanes;
    p.nResults = p.replicate ? p.nCtl : n;
    // one workgroup per CU while they all fit, else two per CU
    p.launch = o.layout == 0 ? LiveLaunch::Lane
               : p.replicate ? LiveLaunch::Lone
                             : (p.groups <= (o.cus > 0 ? o.cus : deviceCus) ? LiveLaunch::StreamOnePerCu : LiveLaunch::StreamTwoPerCu);
    return p;
}

// The control block of a launch, one copy: UttDesc[nCtl] | state pointer[nCtl] | control[nCtl].  at(base) is the block at its host
// address and at its device address alike.
struct CtlBlock {
    size_t nCtl;
    struct View { UttDesc* utt; double** state; uint32_t* control; };
    size_t state_offset() const { return nCtl * sizeof(UttDesc); }
    size_t control_offset() const { return nCtl * (sizeof(UttDesc) + sizeof(double*)); }
    size_t bytes() const { return nCtl * (sizeof(UttDesc) + sizeof(double*) + sizeof(uint32_t)); }
    View at(unsigned char* base) const
    {
        return View{reinterpret_cast<UttDesc*>(base), reinterpret_cast<double**>(base + state_offset()), reinterpret_cast<uint32_t*>(base + control_offset())};
    }
};
struct CtlEntry { UttDesc utt; double* state; uint32_t control; };      // what to do for one handle of the call
// entry(i) for each of the n handles into the block, at i * rep; then the replicas -- control bit 1: every lane of the wavefront
// advances THIS handle -- or the lanes a few handles leave empty.
template <class Entry>
void fill_ctl(const CtlBlock::View& v, const PullPlan& p, int n, Entry&& entry)
{
    for (int i = 0; i < n; ++i) {
        const CtlEntry e = entry(i);
        const size_t j = (size_t)i * p.rep;
        v.utt[j] = e.utt; v.state[j] = e.state; v.control[j] = e.control;
    }
    if (p.replicate) {
        for (int i = 0; i < n; ++i) {
            const size_t j0 = (size_t)i * kLanes;
            v.control[j0] |= 2u;
            for (size_t j = j0 + 1; j < j0 + kLanes; ++j) { v.utt[j] = v.utt[j0]; v.state[j] = v.state[j0]; v.control[j] = v.control[j0]; }
        }
    } else if (p.fillSparse) {
        for (int i = n; i < p.nCtl; ++i) { v.utt[i] = v.utt[i % n]; v.state[i] = v.state[i % n]; v.control[i] = v.control[i % n]; }
    }
}

}  // namespace klatt
