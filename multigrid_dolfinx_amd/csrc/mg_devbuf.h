// Who owns device memory (host code only).  Three move-only types:
//   DevBuf<T>  a buffer that remembers its element count and the handle it is accounted to: allocation adds its bytes to
//              the handle's ledger (mg_memory_bytes), release takes exactly those bytes off again
//   DVector    a level vector [pad | lower halo | owned rows | upper halo]: a DevBuf plus two pointers into it
//   DevTemp    set-up scratch that frees itself and is NOT counted
// The includer provides the HIP runtime declarations (hipMalloc, hipFree, hipMemsetAsync, hipGetErrorString), HIP_TRY
// with fail(), and defines tracked_bytes() once mg_context is complete; tests/host/ does so with a counting stand-in.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>

struct mg_context;

namespace {

int64_t& tracked_bytes(mg_context* c);      // c->bytes

template <class T>
class DevBuf {
    T* p_ = nullptr;
    size_t n_ = 0;
    mg_context* c_ = nullptr;               // (the context is heap-allocated and never moves)

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)), c_(std::exchange(o.c_, nullptr)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); c_ = std::exchange(o.c_, nullptr);
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    // read sites and kernel argument structs take the buffer as the plain pointer it was
    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t count() const { return n_; }

    // `count` elements (0 counts as 1) in place of whatever the buffer held; uninitialised
    int alloc(mg_context* c, size_t count) {
        reset();
        if (count == 0) count = 1;
        T* p = nullptr;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)));
        adopt(c, p, count);
        return 0;
    }
    // memory that was allocated elsewhere (a DevTemp's) becomes this buffer's, and counted
    void adopt(mg_context* c, T* p, size_t count) {
        reset();
        p_ = p; n_ = count; c_ = c;
        tracked_bytes(c_) += (int64_t)(n_ * sizeof(T));
    }
    void reset() {
        if (!p_) return;
        (void)hipFree(p_);
        tracked_bytes(c_) -= (int64_t)(n_ * sizeof(T));
        p_ = nullptr; n_ = 0; c_ = nullptr;
    }
};

// A device vector in local lexicographic storage: [pad | lower halo | owned rows | upper halo],
// padded so that the first owned row is 32-byte aligned (the tile kernels load R rows per lane).
struct DVector {
    DevBuf<double> raw;
    double* base = nullptr;     // start of [lower halo | owned | upper halo]
    double* rows = nullptr;     // first owned row = base + lead

    DVector() = default;
    DVector(DVector&& o) noexcept : raw(std::move(o.raw)), base(std::exchange(o.base, nullptr)), rows(std::exchange(o.rows, nullptr)) {}
    DVector& operator=(DVector&& o) noexcept {
        if (this != &o) {
            raw = std::move(o.raw);
            base = std::exchange(o.base, nullptr); rows = std::exchange(o.rows, nullptr);
        }
        return *this;
    }

    // `total` zero-filled doubles with base = raw + front and rows = base + lead; a vector that exists stays as it is
    int alloc(mg_context* c, size_t total, size_t front, size_t lead, hipStream_t stream) {
        if (raw) return 0;
        MG_TRY(raw.alloc(c, total));
        base = raw + front;
        rows = base + lead;
        HIP_TRY(hipMemsetAsync(raw, 0, total * sizeof(double), stream));
        return 0;
    }
};

// Temporary device buffer that frees itself (set-up paths have many early exits).  Not counted in the ledger.
struct DevTemp {
    void* p = nullptr;
    DevTemp() = default;
    DevTemp(const DevTemp&) = delete;
    DevTemp& operator=(const DevTemp&) = delete;
    DevTemp(DevTemp&& o) noexcept : p(std::exchange(o.p, nullptr)) {}
    DevTemp& operator=(DevTemp&& o) noexcept {
        if (this != &o) { reset(); p = std::exchange(o.p, nullptr); }
        return *this;
    }
    ~DevTemp() { reset(); }
    int alloc(size_t bytes) {
        reset();
        HIP_TRY(hipMalloc(&p, std::max<size_t>(1, bytes)));
        return 0;
    }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
    // the memory leaves the guard: its next owner (DevBuf::adopt) frees it
    template <class T>
    T* release() { return static_cast<T*>(std::exchange(p, nullptr)); }
};

}  // namespace
