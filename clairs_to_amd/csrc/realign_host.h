// Host-side plumbing of the batched realigner's driver (realign_batch.hip), none of it about alignment: the memory of one call (bump
// arenas on the device and page-locked on the host), objects the library keeps between calls (Kept), worker threads
// that outlive a call, a thread that frees behind the caller's back, and the stage clock of CTO_REALIGN_TRACE.
#pragma once
#include <pthread.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>
#include "common.h"
#include "hip_buffers.h"

namespace cto {
namespace realign_host {

// ------------------------------------------------------------------------------------------------------------------------
// An object the library keeps between calls, one per type and process.  It belongs to the device of the first call that asks for it;
// one call at a time holds it.  A call that finds it held, or that runs on another device, gets an object of its own that goes when
// the lease does.  (The kept one is never destroyed: at exit the runtime it would call into may be gone before it.)
template <class T>
class Kept {
    std::mutex m;
    bool busy = false;
    int device = -1;
    T obj;
    static Kept& instance() { static Kept* k = new Kept(); return *k; }
public:
    class Lease {
        Kept* from = nullptr;              // null: `p` is this lease's own
        T* p = nullptr;
    public:
        Lease() {
            int dev = -1;
            (void)hipGetDevice(&dev);
            Kept& k = instance();
            {
                std::lock_guard<std::mutex> g(k.m);
                if (!k.busy && (k.device < 0 || k.device == dev)) { k.busy = true; k.device = dev; from = &k; p = &k.obj; }
            }
            if (!from) p = new T();
        }
        ~Lease() {
            if (from) { std::lock_guard<std::mutex> g(from->m); from->busy = false; }
            else delete p;
        }
        Lease(const Lease&) = delete;
        Lease& operator=(const Lease&) = delete;
        bool kept() const { return from != nullptr; }
        T* operator->() const { return p; }
        T& operator*() const { return *p; }
    };
};

// ------------------------------------------------------------------------------------------------------------------------
// Memory of one call: a bump allocator over blocks that double (256-byte granules).  A call makes ~25 small device allocations; as
// hipMalloc / hipFree pairs they cost it ~3 ms (hipFree waits for the device each time).  The same for page-locked host memory: what a
// call copies up and down (operand bytes, descriptors, results) is built in and landed on pinned blocks, so that hipMemcpyAsync is a
// DMA and not a staged copy through the runtime's bounce buffers.
struct DeviceMem {
    static constexpr size_t kFirstBlock = size_t(32) << 20;
    static hipError_t allocate(void** p, size_t n) { return hipMalloc(p, n); }
    static void release(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
    static constexpr size_t kFirstBlock = size_t(16) << 20;
    static hipError_t allocate(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
    static void release(void* p) { (void)hipHostFree(p); }
};
template <class Mem>
struct Arena {
    struct Block { char* p; size_t cap, used; };
    std::vector<Block> blocks;
    size_t asked = 0;                  // bytes taken since the last reset
    Arena() = default;
    Arena(const Arena&) = delete;
    Arena& operator=(const Arena&) = delete;
    ~Arena() { free_all(); }
    void* take(size_t bytes) {         // null: no more memory of this kind
        bytes = (std::max<size_t>(bytes, 1) + 255) & ~size_t(255);
        asked += bytes;
        if (!blocks.empty() && blocks.back().used + bytes <= blocks.back().cap) {
            void* r = blocks.back().p + blocks.back().used;
            blocks.back().used += bytes;
            return r;
        }
        const size_t cap = std::max<size_t>(bytes, std::max<size_t>(Mem::kFirstBlock, blocks.empty() ? 0 : 2 * blocks.back().cap));
        void* p = nullptr;
        if (Mem::allocate(&p, cap) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        blocks.push_back(Block{static_cast<char*>(p), cap, bytes});
        return p;
    }
    bool owns(const void* q) const {
        for (const Block& b : blocks) if (q >= b.p && q < b.p + b.cap) return true;
        return false;
    }
    void free_all() { for (Block& b : blocks) Mem::release(b.p); blocks.clear(); asked = 0; }
    // end of a call: one block large enough for what this call took, so that the next one of its size allocates nothing
    void reset() {
        if (blocks.size() > 1) {
            const size_t want = asked + asked / 4;
            free_all();
            void* p = nullptr;
            if (Mem::allocate(&p, want) == hipSuccess) blocks.push_back(Block{static_cast<char*>(p), want, 0});
            else (void)hipGetLastError();
        } else if (!blocks.empty()) {
            blocks.back().used = 0;
        }
        asked = 0;
    }
};
struct Arenas { Arena<DeviceMem> device; Arena<PinnedMem> host; };

// the arenas of the call this thread is in (ArenaLease); null outside one
inline thread_local Arena<DeviceMem>* t_arena = nullptr;
inline thread_local Arena<PinnedMem>* t_harena = nullptr;

// A device call's first local: the kept arenas (reset when they go back) or a pair of its own, current on this thread while it lives.
// Declared before anything that allocates from them or runs work on them, so that it goes last.
struct ArenaLease {
    Kept<Arenas>::Lease arenas;
    Arena<DeviceMem>* prev = t_arena;
    Arena<PinnedMem>* hprev = t_harena;
    ArenaLease() { t_arena = &arenas->device; t_harena = &arenas->host; }
    ~ArenaLease() {
        t_arena = prev; t_harena = hprev;
        if (arenas.kept()) { arenas->device.reset(); arenas->host.reset(); }
    }
};

// std::vector over the call's pinned arena (plain heap outside a call or when the arena cannot grow)
template <class T>
struct PinnedAlloc {
    typedef T value_type;
    PinnedAlloc() = default;
    template <class U> PinnedAlloc(const PinnedAlloc<U>&) {}
    T* allocate(size_t n) {
        if (t_harena) { void* p = t_harena->take(n * sizeof(T)); if (p) return static_cast<T*>(p); }
        return static_cast<T*>(::operator new(n * sizeof(T)));
    }
    void deallocate(T* p, size_t) { if (!(t_harena && t_harena->owns(p))) ::operator delete(p); }
    template <class U> bool operator==(const PinnedAlloc<U>&) const { return true; }
    template <class U> bool operator!=(const PinnedAlloc<U>&) const { return false; }
};
template <class T> using pinned_vector = std::vector<T, PinnedAlloc<T>>;

// n elements of the call's device arena (a hipMalloc of its own outside a call)
template <class T>
struct ArenaBuf {
    T* p = nullptr;
    bool owned = true;                 // false: the call's arena owns the bytes
    ArenaBuf() = default;
    ArenaBuf(const ArenaBuf&) = delete;
    ArenaBuf& operator=(const ArenaBuf&) = delete;
    ~ArenaBuf() { if (p && owned) (void)hipFree(p); }
    int alloc(size_t n) {
        if (t_arena) {
            p = static_cast<T*>(t_arena->take(std::max<size_t>(n, 1) * sizeof(T)));
            owned = false;
            CTO_REQUIRE(p != nullptr, CTO_EHIP, "cto_realign_windows: out of device memory");
            return CTO_OK;
        }
        CTO_HIP(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T)));
        return CTO_OK;
    }
    template <class A>
    int put(const std::vector<T, A>& v, hipStream_t s) {
        int rc = alloc(v.size());
        if (rc != CTO_OK) return rc;
        if (!v.empty()) CTO_HIP(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
        return CTO_OK;
    }
    void swap(ArenaBuf& o) { std::swap(p, o.p); std::swap(owned, o.owned); }
};

// ------------------------------------------------------------------------------------------------------------------------
// Side streams kept between calls: creating and destroying four streams and their events cost a call ~1 ms.
struct StreamSet {
    static constexpr int kMax = 5;
    hipStream_t sx[kMax] = {};
    Event join[kMax];                  // join[i]: what a call records on sx[i] for its own stream to wait for
    int n = 0;
    StreamSet() = default;
    StreamSet(const StreamSet&) = delete;
    StreamSet& operator=(const StreamSet&) = delete;
    ~StreamSet() { for (int i = 0; i < n; ++i) (void)hipStreamDestroy(sx[i]); }
    // stream i (made on first use)
    int get(int i, hipStream_t* out) {
        if (i >= kMax) return CTO_EINVAL;
        while (n <= i) {
            // at the device's highest priority: the runtime keeps a pool of hardware queues PER PRIORITY and hands a new stream the least used
            // queue of its pool - beside a process's ordinary streams (torch's, the pipeline's) two of these could land on one queue and their
            // classes would run one after the other (bench.py's process: 7.2 ms for the stage the stand-alone tool runs in 5.6); a pool of their own
            // gives the four of them a queue each
            int lo = 0, hi = 0;
            if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { (void)hipGetLastError(); lo = hi = 0; }
            if (join[n].e == nullptr && join[n].create(hipEventDisableTiming) != CTO_OK) return CTO_EHIP;
            if (hipStreamCreateWithPriority(&sx[n], hipStreamNonBlocking, hi) != hipSuccess) return CTO_EHIP;
            ++n;
        }
        *out = sx[i];
        return CTO_OK;
    }
};
// The side streams of one stage.  Declared AFTER the events and device buffers that the work on them refers to: whichever way the
// stage is left, the streams are drained here first, and only then do those go (and the kept set back to the library).
struct SideStreams {
    Kept<StreamSet>::Lease set;
    ~SideStreams() { for (int i = 0; i < set->n; ++i) (void)hipStreamSynchronize(set->sx[i]); }
    int get(int i, hipStream_t* out) { return set->get(i, out); }
    hipEvent_t join(int i) const { return set->join[i]; }
};

// ------------------------------------------------------------------------------------------------------------------------
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Worker threads that outlive a call.  A call runs a dozen parallel loops over its windows (packing, collecting pairs, filing results,
// planning and composing tracebacks) of a millisecond or less each; as std::threads created and joined per loop, sixteen at a time, the
// creation alone was a third of a millisecond per loop.  The pool is made once (grown on demand, never destroyed: its threads sleep on a
// condition variable and end with the process); one call at a time uses it, a concurrent one falls back to threads of its own.
class WorkerPool {
    std::mutex m;
    std::condition_variable cv_start, cv_done;
    std::vector<std::thread> th;
    const std::function<void()>* job = nullptr;
    unsigned long long gen = 0;
    int want = 0, pending = 0;
    void worker(int id) {
        unsigned long long seen = 0;
        for (;;) {
            const std::function<void()>* mine = nullptr;
            {
                std::unique_lock<std::mutex> lk(m);
                cv_start.wait(lk, [&] { return gen != seen; });
                seen = gen;
                if (id < want) mine = job;
            }
            if (!mine) continue;
            (*mine)();
            std::lock_guard<std::mutex> lk(m);
            if (--pending == 0) cv_done.notify_all();
        }
    }
public:
    std::mutex use;                                    // held by the call that runs loops on the pool
    bool run(int helpers, const std::function<void()>& f) {
        try {
            std::lock_guard<std::mutex> lk(m);
            while (int(th.size()) < helpers) { th.emplace_back(&WorkerPool::worker, this, int(th.size())); th.back().detach(); }
        } catch (...) {
            return false;                              // no more threads to be had
        }
        {
            std::lock_guard<std::mutex> lk(m);
            job = &f; want = helpers; pending = helpers; ++gen;
        }
        cv_start.notify_all();
        f();
        std::unique_lock<std::mutex> lk(m);
        cv_done.wait(lk, [&] { return pending == 0; });
        job = nullptr;
        return true;
    }
    // (a child of fork() has none of the parent's threads: it starts with a pool of its own; the parent's object is left as it is)
    static WorkerPool*& slot() { static WorkerPool* p = nullptr; return p; }
    static WorkerPool& get() {
        static std::once_flag once;
        std::call_once(once, [] { (void)pthread_atfork(nullptr, nullptr, [] { slot() = new WorkerPool(); }); slot() = new WorkerPool(); });
        return *slot();
    }
};

template <class F>
void parallel_for(size_t n, int threads, F&& f) {
    // an exception on a worker (std::bad_alloc in a window's vectors) must not reach std::terminate: the first one is kept, every
    // worker stops taking items, and the caller rethrows it after the join - where the C boundary's CTO_CATCH turns it into an error code
    std::atomic<size_t> next{0};
    std::atomic<bool> failed{false};
    std::exception_ptr first;
    std::mutex first_lock;
    const std::function<void()> work = [&]() {
        try {
            for (size_t i = next++; i < n && !failed.load(std::memory_order_relaxed); i = next++) f(i);
        } catch (...) {
            std::lock_guard<std::mutex> g(first_lock);
            if (!first) first = std::current_exception();
            failed.store(true);
        }
    };
    const int nt = int(std::min<size_t>(size_t(std::max(1, threads)), n));
    bool done = false;
    if (nt > 1) {
        WorkerPool& pool = WorkerPool::get();
        std::unique_lock<std::mutex> mine(pool.use, std::try_to_lock);
        if (mine.owns_lock()) done = pool.run(nt - 1, work);
    }
    if (!done) {
        std::vector<std::thread> own;
        try {
            for (int t = 1; t < nt; ++t) own.emplace_back(work);
        } catch (...) {                               // no more threads to be had: the ones that started and this one do the work
        }
        work();
        for (std::thread& t : own) t.join();
    }
    if (first) std::rethrow_exception(first);
}

// A thread that destroys what a call is done with behind the caller's back; the next call (or the library's unloading) waits for it.
struct Reaper {
    std::mutex m;
    std::thread t;
    void wait() { if (t.joinable()) t.join(); }
    ~Reaper() { wait(); }
};
inline Reaper g_reaper;
template <class T>
void reap(T&& what) {
    std::lock_guard<std::mutex> lock(g_reaper.m);
    g_reaper.wait();
    auto* gone = new T(std::move(what));
    g_reaper.t = std::thread([gone]() { delete gone; });
}

// CTO_REALIGN_TRACE=1: the classes of the Smith-Waterman stage and the wall time of every stage of a call, on stderr
inline bool trace_on() { static const bool on = std::getenv("CTO_REALIGN_TRACE") != nullptr; return on; }
struct StageClock {
    double t = now_ms();
    void lap(const char* what) { if (trace_on()) { const double n = now_ms(); std::fprintf(stderr, "[realign] %-28s %8.3f ms\n", what, n - t); t = n; } }
};

}  // namespace realign_host
}  // namespace cto
