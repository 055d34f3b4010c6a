// solver_host.hpp — the host runtime shared by every device solver (ba_solve.hip, sim3.hip, essential_graph.hip, the RANSACs, the
// mapping and loop-closing entry points) and the entropy gate (select.hip): grow-only staging buffers, a stream per device, and the
// layout of a one-copy upload.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "common.hpp"

namespace sivo {

// Grow-only buffer of pinned host (Pinned) or device memory: a request that does not fit frees it and allocates twice the request, at
// least the owner's minimum (a pinned allocation costs ~0.2 ms: never per call).  The contents do not survive a growth.
template <bool Pinned>
class GrowBuf {
 public:
    explicit GrowBuf(size_t min_bytes) : min_(min_bytes) {}
    ~GrowBuf() { release(); }
    GrowBuf(const GrowBuf &) = delete;
    GrowBuf &operator=(const GrowBuf &) = delete;
    char *reserve(size_t bytes) {
        if (bytes > cap_) {
            if (p_) SIVO_HIP(Pinned ? hipHostFree(p_) : hipFree(p_));
            p_ = nullptr; cap_ = 0;
            const size_t cap = std::max(2 * bytes, min_);
            SIVO_HIP(Pinned ? hipHostMalloc((void **)&p_, cap, hipHostMallocDefault) : hipMalloc((void **)&p_, cap));
            cap_ = cap;
        }
        return p_;
    }
    void release() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr; cap_ = 0;
    }

 private:
    char *p_ = nullptr;
    size_t cap_ = 0, min_;
};
using PinnedBuf = GrowBuf<true>;
using DeviceBuf = GrowBuf<false>;

// A solver's state on the calling thread's current device: a non-blocking stream of its own (the null stream is also PyTorch's default
// stream: a solve must not queue behind whatever the host application runs there) and the grow-only buffers of its calls.  bind()
// rebuilds all of it when the current device changed since the last call; nothing is allocated in a call once the buffers fit.
struct SolverCtx {
    hipStream_t stream = nullptr;
    PinnedBuf in, out;
    DeviceBuf dev;
    SolverCtx(bool high_priority, size_t in_min, size_t out_min, size_t dev_min)
        : in(in_min), out(out_min), dev(dev_min), high_(high_priority) {}
    ~SolverCtx() { release(); }
    bool bind() {                              // true: rebuilt (what an owner keeps beside it belongs to another device now)
        int d = 0;
        SIVO_HIP(hipGetDevice(&d));
        if (d == device_) return false;
        release();
        int lo = 0, hi = 0;
        if (high_) SIVO_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
        SIVO_HIP(high_ ? hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, hi) : hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        device_ = d;
        return true;
    }

 private:
    void release() {
        in.release(); out.release(); dev.release();
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr; device_ = -1;
    }
    bool high_;
    int device_ = -1;
};

// A device buffer of a one-shot entry point that takes host arrays, freed when the call returns: up() allocates it (at least one byte)
// and copies `src` into it when there is one.
struct CallBuf {
    void *p = nullptr;
    ~CallBuf() { (void)hipFree(p); }
    void up(const void *src, size_t bytes) {
        SIVO_HIP(hipMalloc(&p, bytes ? bytes : 1));
        if (src) SIVO_HIP(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    }
};

// Regions packed into one device buffer at 256-byte offsets: first those with a host source, then those that start at zero, then those
// the device writes before anything reads them (results).  Each region names the pointer that receives its device address; place()
// fills them all and stages the sources into a host buffer at the same offsets, send() uploads the sourced part in one copy and
// zeroes the zero part in one memset.
class Layout {
 public:
    // src == nullptr: the caller writes the content at host(p) between place() and send()
    template <class T> void copy(T *&p, const void *src, size_t bytes) { add(&p, set<T>, src, bytes, 0); }
    template <class T> void zero(T *&p, size_t bytes) { add(&p, set<T>, nullptr, bytes, 1); }
    template <class T> void take(T *&p, size_t bytes) { add(&p, set<T>, nullptr, bytes, 2); }
    size_t staged() const { return end_[0]; }                       // the host buffer place() needs (without results)
    size_t results() const { return end_[2]; }                      // the results part (from the first take() region on)
    size_t bytes() const { return end_[0] + end_[1] + end_[2]; }
    void place(char *dev, char *host) {
        dev_ = dev; host_ = host;
        for (int i = 0; i < n_; ++i) {
            const Region &r = r_[i];
            const size_t off = r.off + (r.kind > 0 ? end_[0] : 0) + (r.kind > 1 ? end_[1] : 0);
            r.set(r.slot, dev + off);
            if (r.src && r.bytes) std::memcpy(host + off, r.src, r.bytes);
        }
    }
    void send(hipStream_t stream) const {
        SIVO_HIP(hipMemcpyAsync(dev_, host_, end_[0], hipMemcpyHostToDevice, stream));
        if (end_[1]) SIVO_HIP(hipMemsetAsync(dev_ + end_[0], 0, end_[1], stream));
    }
    template <class T> T *host(const T *p) const { return (T *)(host_ + ((const char *)p - dev_)); }

 private:
    template <class T> static void set(void *slot, char *at) { *static_cast<T **>(slot) = (T *)at; }
    struct Region { void *slot; void (*set)(void *, char *); const void *src; size_t bytes, off; int kind; };
    void add(void *slot, void (*s)(void *, char *), const void *src, size_t bytes, int kind) {
        if (n_ == kMax) throw std::logic_error("Layout: too many regions");
        r_[n_++] = Region{slot, s, src, bytes, end_[kind], kind};
        end_[kind] += (std::max<size_t>(bytes, 8) + 255) / 256 * 256;
    }
    static constexpr int kMax = 64;
    Region r_[kMax];
    int n_ = 0;
    size_t end_[3] = {0, 0, 0};
    char *dev_ = nullptr, *host_ = nullptr;
};

}  // namespace sivo
