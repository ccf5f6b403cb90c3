// rh_host.h -- host-side owners of what a context holds on the device (roger_hip.hip, rh_sas.hip): each releases what it holds in
// its destructor, so a context is torn down by `delete ctx` and a member that was never allocated costs nothing; and the rules of a
// ring of rows that the observers of both contexts share (at the end).  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

// One hipMalloc allocation, move-only.  Converts to the pointer it holds, so it is passed to HIP calls and kernels like one.
template <class T>
class DevBuf {
    T *p_ = nullptr;

public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            (void)release();
            p_ = o.p_;
            o.p_ = nullptr;
        }
        return *this;
    }
    ~DevBuf() { (void)release(); }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    T *operator->() const { return p_; }
    // where the pointer itself is kept: the source of a copy of the POINTER to the device, valid as long as the owner
    T *const *addr() const { return &p_; }
    hipError_t release() {
        const hipError_t e = p_ ? hipFree(p_) : hipSuccess;
        p_ = nullptr;
        return e;
    }
    // (re)allocate to `bytes`: what was held is freed first, its contents are not kept
    hipError_t alloc(size_t bytes) {
        const hipError_t e = release();
        return e != hipSuccess ? e : hipMalloc((void **)&p_, bytes);
    }
    // ... only if nothing is held yet (buffers whose size follows from the context's shape)
    hipError_t alloc_once(size_t bytes) { return p_ ? hipSuccess : hipMalloc((void **)&p_, bytes); }
};

// One zero-filled object in pinned host memory that the device writes directly (hipHostMallocMapped).
template <class T>
class PinnedBlock {
    T *p_ = nullptr;

public:
    PinnedBlock() = default;
    PinnedBlock(const PinnedBlock &) = delete;
    PinnedBlock &operator=(const PinnedBlock &) = delete;
    ~PinnedBlock() {
        if (p_) (void)hipHostFree(p_);
    }
    T *get() const { return p_; }
    T *operator->() const { return p_; }
    hipError_t alloc() {
        const hipError_t e = hipHostMalloc((void **)&p_, sizeof(T), hipHostMallocMapped);
        if (e == hipSuccess) *p_ = T{};
        return e;
    }
};

// The stream a context enqueues on: its own (create) until the caller hands one over (adopt); converts to hipStream_t.
class Stream {
    hipStream_t s_ = nullptr;
    bool own_ = false;

public:
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() {
        if (own_ && s_) (void)hipStreamDestroy(s_);
    }
    operator hipStream_t() const { return s_; }
    hipError_t create() {
        const hipError_t e = hipStreamCreate(&s_);
        own_ = e == hipSuccess;
        return e;
    }
    // the work enqueued so far is waited for, an own stream is destroyed
    hipError_t adopt(hipStream_t other) {
        hipError_t e = hipStreamSynchronize(s_);
        if (e == hipSuccess && own_) e = hipStreamDestroy(s_);
        if (e != hipSuccess) return e;
        s_ = other;
        own_ = false;
        return hipSuccess;
    }
};

// Pairs (start, stop) of timing events, one per timed launch; the pool is reused after restart() and only ever grows.
struct EventPool {
    std::vector<hipEvent_t> ev;
    size_t used = 0;

    EventPool() = default;
    EventPool(const EventPool &) = delete;
    EventPool &operator=(const EventPool &) = delete;
    ~EventPool() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    void restart() { used = 0; }
    size_t launches() const { return used / 2; }
    // the next pair, created on demand; taken() once the launch they belong to is enqueued
    hipError_t next_pair(hipEvent_t *ev0, hipEvent_t *ev1) {
        while (ev.size() < used + 2) {
            hipEvent_t e;
            const hipError_t rc = hipEventCreate(&e);
            if (rc != hipSuccess) return rc;
            ev.push_back(e);
        }
        *ev0 = ev[used];
        *ev1 = ev[used + 1];
        return hipSuccess;
    }
    void taken() { used += 2; }
    hipError_t elapsed_ms(size_t launch, float *ms) const { return hipEventElapsedTime(ms, ev[2 * launch], ev[2 * launch + 1]); }
    // the sum over all timed launches (the caller has synchronised the stream)
    hipError_t total_ms(double *sum) const {
        *sum = 0;
        for (size_t k = 0; k < launches(); ++k) {
            float ms = 0;
            const hipError_t rc = elapsed_ms(k, &ms);
            if (rc != hipSuccess) return rc;
            *sum += ms;
        }
        return hipSuccess;
    }
};

// ---- a ring of rows: row r of `total` recorded ones lives in slot r mod cap, the last cap of them are resident.  Neither context type
// appears here, so both libraries' observers share these; each reports a refusal through its own fail / sfail.
// The refusal of a capacity that a configure call was given, behind `prefix` ("<function>: "), or an empty string.  max_rows: 0 where
// the caller bounds the ring's bytes itself.
static inline std::string ring_capacity_refusal(const std::string &prefix, int64_t capacity, int64_t max_rows) {
    if (capacity < 1) return prefix + "capacity = " + std::to_string(capacity) + " (at least one row)";
    if (max_rows && capacity > max_rows) return prefix + "capacity = " + std::to_string(capacity) + " rows is beyond any device";
    return std::string();
}
// The refusal of a read of rows [first_row, first_row + n_rows) by the function `who`, or an empty string: the rows are recorded and
// still resident, or there are none.
static inline std::string ring_range_refusal(const char *who, int64_t first_row, int64_t n_rows, int64_t total, int64_t cap) {
    if (first_row < 0 || n_rows < 0 || first_row > total || n_rows > total - first_row)
        return std::string(who) + ": rows " + std::to_string(first_row) + " ... " + std::to_string(first_row + n_rows - 1) +
               " have not been recorded (" + std::to_string(total) + " rows so far)";
    if (n_rows && first_row < total - cap)
        return std::string(who) + ": rows " + std::to_string(first_row) + " ... " + std::to_string(total - cap - 1) +
               " have been overwritten (the ring holds the last " + std::to_string(cap) + " of " + std::to_string(total) + " rows)";
    return std::string();
}
// The at most two pieces of an accepted range -- it may straddle the ring's wrap: piece(done, slot, m) for m rows from slot `slot` on,
// `done` rows into the range; the first piece that returns non-zero ends the walk with that value.
template <class F>
static inline int ring_pieces(int64_t first_row, int64_t n_rows, int64_t cap, F &&piece) {
    for (int64_t done = 0; done < n_rows;) {
        const int64_t slot = (first_row + done) % cap;
        const int64_t m = std::min<int64_t>(n_rows - done, cap - slot);
        if (const int rc = piece(done, slot, m)) return rc;
        done += m;
    }
    return 0;
}
