// klatt_hostpool.h -- the host's worker threads, which every parallel section of a set call runs on (klatt_engine.hip, the track
// planner of klatt_trackplan.h), and the vector those sections fill.  Plain C++17: no HIP; tests/native/check_track_plan.cpp runs the
// pool under ThreadSanitizer and AddressSanitizer.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>

namespace klatt {

// The host's worker threads.  Until round 5 every parallel section started and joined its own std::threads: eight sections of a
// setUtterances call are ~56 thread starts, 2-4 ms of a 22 ms call on the GPU box.  Now a pool that lives as long as the process:
// workers sleep on a condition variable, a section queues its parts and its caller works on queued parts (its own or anybody's) until
// its own are done -- so sections of several callers (the setter threads of a pipeline, the device threads of a node) share the workers
// without waiting for each other, and a section whose parts all queue behind others still finishes on its caller's thread.
// Parts never start sections of their own.  The pool is never destroyed (its threads sleep at process exit).
class WorkerPool {
public:
    struct Section { std::atomic<unsigned> left{0}; };
    static WorkerPool& get() { static WorkerPool* p = new WorkerPool(); return *p; }
    void submit(Section* sec, std::function<void()> fn)
    {
        { std::lock_guard<std::mutex> lg(mu_); queue_.emplace_back(sec, std::move(fn)); }
        cv_.notify_one();
    }
    // run queued parts until `sec` has none left
    void help_until_done(Section* sec)
    {
        std::unique_lock<std::mutex> lk(mu_);
        while (sec->left.load(std::memory_order_acquire) != 0) {
            if (!queue_.empty()) run_front(lk);
            else done_.wait_for(lk, std::chrono::microseconds(200));
        }
    }
    unsigned workers() const { return nWorkers_; }
private:
    WorkerPool()
    {
        // as many workers as the process may really use: CPU affinity, capped by the cgroup quota (the GPU box shows 256 hardware threads
        // and grants 16 CPUs) and by 32
        unsigned n = std::max(1u, std::thread::hardware_concurrency());
        if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char q[64] = {0}; long long period = 0;
            if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) n = std::min<unsigned>(n, (unsigned)std::max<long long>(1, atoll(q) / period));
            fclose(f);
        }
        n = std::min(n, 32u);
        for (unsigned i = 0; i + 1 < n; ++i) {
            try { std::thread([this] { loop(); }).detach(); ++nWorkers_; } catch (const std::system_error&) { break; }
        }
    }
    void loop()
    {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [this] { return !queue_.empty(); });
            run_front(lk);
        }
    }
    // the queue's first part, run without the lock
    void run_front(std::unique_lock<std::mutex>& lk)
    {
        auto job = std::move(queue_.front());
        queue_.pop_front();
        lk.unlock();
        job.second();
        job.first->left.fetch_sub(1, std::memory_order_acq_rel);
        done_.notify_all();
        lk.lock();
    }
    std::mutex mu_;
    std::condition_variable cv_, done_;
    std::deque<std::pair<Section*, std::function<void()>>> queue_;
    unsigned nWorkers_ = 0;
};

// fn(0) .. fn(n - 1) side by side: n - 1 of them offered to the pool, the last one on the caller's thread, which then helps until all are done.
template <class F>
void run_parts(unsigned n, F fn)
{
    if (n <= 1) { if (n) fn(0u); return; }
    WorkerPool& pool = WorkerPool::get();
    if (pool.workers() == 0) { for (unsigned t = 0; t < n; ++t) fn(t); return; }
    // A part that throws (std::bad_alloc in a planner's maps) must neither unwind this frame while queued parts still point at it nor
    // leave the section's count standing: every part runs under a guard that keeps the first exception, the caller helps until all
    // parts are done, and only then is the exception thrown on -- on the caller's thread.
    WorkerPool::Section sec;
    std::mutex emu;
    std::exception_ptr first;
    auto guarded = [&](unsigned t) {
        try { fn(t); } catch (...) { std::lock_guard<std::mutex> g(emu); if (!first) first = std::current_exception(); }
    };
    sec.left.store(n - 1, std::memory_order_release);
    for (unsigned t = 0; t + 1 < n; ++t) pool.submit(&sec, [&guarded, t] { guarded(t); });
    guarded(n - 1);
    pool.help_until_done(&sec);
    if (first) std::rethrow_exception(first);
}

// Host threads of setUtterances (the planner's setting: SPEECHPLAYER_PLAN_THREADS, else up to 8), and a loop over [0, n) cut into
// one contiguous range per thread (small loops stay on the caller's thread).
inline unsigned host_threads()
{
    unsigned n = std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
    if (const char* e = getenv("SPEECHPLAYER_PLAN_THREADS")) n = (unsigned)std::max(1, atoi(e));
    return n;
}
template <class F>
void parallel_ranges(long long n, long long grain, F fn)
{
    const unsigned t = (unsigned)std::min<long long>(host_threads(), std::max<long long>(1, n / std::max<long long>(grain, 1)));
    if (t < 2) { fn(0ll, n); return; }
    run_parts(t, [&](unsigned k) { fn(n * (long long)k / t, n * (long long)(k + 1) / t); });
}

// A vector whose resize() does not value-initialise (trivial element types only): the per-frame work arrays of setUtterances are
// written in full, in parallel, right after they are sized -- a zero-fill by the calling thread first costs ~1 ms per 6 MB.
template <class T>
struct NoInitAlloc : std::allocator<T> {
    template <class U> struct rebind { using other = NoInitAlloc<U>; };
    NoInitAlloc() = default;
    template <class U> NoInitAlloc(const NoInitAlloc<U>&) {}
    template <class U> void construct(U* p) { ::new (static_cast<void*>(p)) U; }
    template <class U, class... A> void construct(U* p, A&&... a) { ::new (static_cast<void*>(p)) U(std::forward<A>(a)...); }
};
template <class T> using RawVector = std::vector<T, NoInitAlloc<T>>;

}  // namespace klatt
