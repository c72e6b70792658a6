// Host-side plumbing of the device front end (pipeline.hip, pileup.hip, tokenise.hip): buffers that only grow, on the device and
// page-locked on the host, waits for the device that sleep instead of spinning, and events and streams that go with their scope.
#pragma once
#include <unistd.h>
#include <cstring>
#include <mutex>
#include "common.h"

namespace cto {

// what a buffer grows to when `n` bytes do not fit: room for a quarter more, so that slowly growing chunks reallocate rarely
inline size_t grown_capacity(size_t n) { return n + n / 4 + 4096; }
inline size_t align16(size_t n) { return (n + 15) & ~size_t(15); }

struct DevBuf {                          // a device allocation that only grows (its bytes do not survive growth)
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t n) {
        if (n <= cap) return CTO_OK;
        if (p) CTO_HIP(hipFree(p));
        p = nullptr;
        cap = 0;
        const size_t want = grown_capacity(n);
        CTO_HIP(hipMalloc(&p, want));
        cap = want;
        return CTO_OK;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
    ~DevBuf() { if (p) (void)hipFree(p); }
};

struct PinBuf {                          // page-locked host memory that only grows
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t n) { return grow_keeping(n, 0); }
    int grow_keeping(size_t n, size_t keep) {              // ensure(n) that carries the first `keep` bytes over
        if (n <= cap) return CTO_OK;
        void* q = nullptr;
        const size_t want = grown_capacity(n);
        CTO_HIP(hipHostMalloc(&q, want, hipHostMallocDefault));
        if (p) {
            if (keep) memcpy(q, p, keep);
            CTO_HIP(hipHostFree(p));
        }
        p = q;
        cap = want;
        return CTO_OK;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
    ~PinBuf() { if (p) (void)hipHostFree(p); }
};

// Waits for an event without occupying a core: hipEventSynchronize / hipStreamSynchronize poll the completion signal from the calling
// thread (measured: every chunk waiting for the device inflate cost a second of CPU), and the producer and writer threads that wait
// share the host with the threads that tokenise and inflate.
inline hipError_t wait_event(hipEvent_t ev) {
    for (int spins = 0;; ++spins) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        if (spins >= 4) usleep(spins < 64 ? 50 : 200);
    }
}

// the same for everything queued on `s` so far
inline hipError_t record_and_wait(hipEvent_t ev, hipStream_t s) {
    const hipError_t e = hipEventRecord(ev, s);
    return e != hipSuccess ? e : wait_event(ev);
}

// An event that goes with its scope
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    int create(unsigned flags = hipEventDefault) { CTO_HIP(hipEventCreateWithFlags(&e, flags)); return CTO_OK; }
    operator hipEvent_t() const { return e; }
};

// A context that lives as long as the process (buffers kept from call to call).  Never destroyed: at process exit the HIP runtime
// may already be gone when static destructors run, and ~DevBuf / ~PinBuf / ~Event would call into it.
template <class T> T& process_wide() { static T* p = new T(); return *p; }

// The device side of an entry point that runs one batch at a time on a stream of its own and keeps its buffers from call to call
// (process_wide: the stream stays a raw handle, nothing ever waits for it at exit).  Derive a type per entry point.
struct BatchCtx {
    std::mutex mu;
    hipStream_t stream = nullptr;
    Event ev0, ev1, done;                // around the kernels; behind the copy back
    PinBuf h_in, h_out;
    DevBuf d_in, d_out;
    int open(size_t bytes_in, size_t bytes_out) {       // under mu: stream and events on first use, room for this batch
        int rc;
        if (!stream) {
            if ((rc = ev0.create()) || (rc = ev1.create()) || (rc = done.create())) return rc;
            CTO_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        }
        if ((rc = h_in.ensure(bytes_in)) || (rc = d_in.ensure(bytes_in)) || (rc = h_out.ensure(bytes_out))) return rc;
        return d_out.ensure(bytes_out);
    }
};

// A stream that goes with its scope: what is queued on it is waited for, then it is destroyed.  Whoever queues on it from another
// thread must be joined before that - declare the stream BEFORE what joins the threads.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    int create(unsigned flags = hipStreamNonBlocking) { CTO_HIP(hipStreamCreateWithFlags(&s, flags)); return CTO_OK; }
    int create_on_cus(const uint32_t* mask, uint32_t words) { CTO_HIP(hipExtStreamCreateWithCUMask(&s, words, mask)); return CTO_OK; }
    operator hipStream_t() const { return s; }
};

}  // namespace cto
