// The owners of device memory (csrc/mg_devbuf.h) against a counting stand-in for the four HIP calls they use, built with
// -fsanitize=address,undefined by tests/test_devbuf_host.py: no GPU, no Python.  The stand-in allocates with malloc, so a
// leak, a double free, a free of memory it never handed out and a write past a buffer's end all end the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;
typedef void* hipStream_t;

static std::map<void*, size_t> g_live;      // what the stand-in has handed out
static long g_mallocs = 0, g_frees = 0, g_fail_in = -1;     // g_fail_in: the hipMalloc that many calls from now fails

static hipError_t hipMalloc(void** p, size_t bytes) {
    if (g_fail_in == 0) { g_fail_in = -1; *p = nullptr; return hipErrorOutOfMemory; }
    if (g_fail_in > 0) --g_fail_in;
    *p = std::malloc(bytes);
    g_live[*p] = bytes;
    ++g_mallocs;
    return hipSuccess;
}
static hipError_t hipFree(void* p) {
    if (!p) return hipSuccess;
    if (!g_live.erase(p)) { std::fprintf(stderr, "hipFree of memory that is not live\n"); std::abort(); }
    std::free(p);
    ++g_frees;
    return hipSuccess;
}
static hipError_t hipMemsetAsync(void* p, int value, size_t bytes, hipStream_t) {
    std::memset(p, value, bytes);
    return hipSuccess;
}
static const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "success" : "out of memory"; }

static std::string g_err;
static int fail(const std::string& msg) { g_err = msg; return 1; }
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
#define MG_TRY(expr) do { int r_ = (expr); if (r_ != 0) return r_; } while (0)

struct mg_context { int64_t bytes = 0; };

#include "../../multigrid_dolfinx_amd/csrc/mg_devbuf.h"

namespace {
int64_t& tracked_bytes(mg_context* c) { return c->bytes; }
}

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

static size_t live_bytes() {
    size_t n = 0;
    for (auto& kv : g_live) n += kv.second;
    return n;
}

// what a level is to these types: buffers, vectors and plain state with default member initialisers
struct Slot {
    DevBuf<double> vals;
    DevBuf<int> cols;
    DVector v, v2;
    std::vector<int> splits;
    int mc_ok = -1;
    bool set = false;
};

static int fill(mg_context* c, Slot& s, size_t n) {
    MG_TRY(s.vals.alloc(c, 3 * n));
    MG_TRY(s.cols.alloc(c, 3 * n));
    MG_TRY(s.v.alloc(c, n + 40, 16, 8, nullptr));
    MG_TRY(s.v2.alloc(c, n + 40, 16, 8, nullptr));
    s.splits.assign(2, (int)n);
    s.mc_ok = 1;
    s.set = true;
    return 0;
}

static int build_two(mg_context* c, DevBuf<double>& out_a, DevBuf<int>& out_b) {       // locals, published on success
    DevBuf<double> a;
    DevBuf<int> b;
    MG_TRY(a.alloc(c, 100));
    MG_TRY(b.alloc(c, 50));
    out_a = std::move(a); out_b = std::move(b);
    return 0;
}

static int run() {
    mg_context ctx;
    mg_context* c = &ctx;
    {   // alloc, re-alloc, count 0 taken as 1, reset
        DevBuf<double> b;
        CHECK(!b && b.count() == 0);
        CHECK(b.alloc(c, 10) == 0 && b && b.count() == 10 && ctx.bytes == 80);
        b[9] = 1.0;
        CHECK(b.alloc(c, 0) == 0 && b.count() == 1 && ctx.bytes == 8);         // what it held is freed first
        CHECK(g_live.size() == 1);
        b.reset();
        CHECK(!b && ctx.bytes == 0 && g_live.empty());
        b.reset();                                                             // twice is once
        CHECK(b.alloc(c, 4) == 0);
    }                                                                          // the destructor frees
    CHECK(ctx.bytes == 0 && g_live.empty());
    {   // move and swap leave the ledger alone
        DevBuf<int> a, b;
        CHECK(a.alloc(c, 5) == 0 && b.alloc(c, 7) == 0 && ctx.bytes == 48);
        int* const pa = a; int* const pb = b;
        std::swap(a, b);
        CHECK(a == pb && b == pa && a.count() == 7 && b.count() == 5 && ctx.bytes == 48);
        DevBuf<int> m(std::move(a));
        CHECK(!a && a.count() == 0 && m == pb && ctx.bytes == 48);
        b = std::move(m);                                                      // what b held (5 ints) goes
        CHECK(!m && b == pb && ctx.bytes == 28 && g_live.size() == 1);
        DevBuf<int>& self = b;
        b = std::move(self);
        CHECK(b == pb && ctx.bytes == 28);
    }
    CHECK(ctx.bytes == 0 && g_live.empty());
    {   // adopt: a temporary's memory becomes a counted buffer; temporaries are never counted
        DevTemp t;
        CHECK(t.alloc(64 * sizeof(double)) == 0 && ctx.bytes == 0);
        t.as<double>()[63] = 2.0;
        DevBuf<double> kappa;
        CHECK(kappa.alloc(c, 3) == 0);
        kappa.adopt(c, t.release<double>(), 64);
        CHECK(!t.p && kappa.count() == 64 && kappa[63] == 2.0 && ctx.bytes == 512 && g_live.size() == 1);
        DevTemp table;
        CHECK(table.alloc(8 * sizeof(int)) == 0 && ctx.bytes == 512 && g_live.size() == 2);
        DevTemp u, w;
        CHECK(u.alloc(0) == 0 && w.alloc(16) == 0);                            // (0 bytes taken as 1)
        void* const pw = w.p;
        u = std::move(w);                                                      // what u held goes
        CHECK(u.p == pw && !w.p && g_live.size() == 3);
        CHECK(u.alloc(32) == 0 && g_live.size() == 3);                         // so does it when u allocates again
    }
    CHECK(ctx.bytes == 0 && g_live.empty());
    {   // vectors: zero fill, the two pointers, swap keeps raw meaningful, an existing vector stays
        DVector v, v2;
        CHECK(v.alloc(c, 100, 16, 8, nullptr) == 0 && v2.alloc(c, 100, 16, 8, nullptr) == 0 && ctx.bytes == 1600);
        CHECK(v.base == v.raw + 16 && v.rows == v.base + 8);
        for (int i = 0; i < 100; ++i) CHECK(v.raw[i] == 0.0);
        double* const r = v.raw; double* const r2 = v2.raw;
        v.rows[0] = 3.0;
        CHECK(v.alloc(c, 500, 0, 0, nullptr) == 0 && v.raw == r && v.rows[0] == 3.0 && ctx.bytes == 1600);
        std::swap(v, v2);
        CHECK(v.raw == r2 && v2.raw == r && v2.rows == r + 24 && v2.rows[0] == 3.0 && v.base == r2 + 16 && ctx.bytes == 1600);
        v = DVector{};                                                         // vec_free
        CHECK(!v.raw && !v.base && !v.rows && ctx.bytes == 800);
        DVector moved(std::move(v2));
        CHECK(!v2.raw && !v2.base && !v2.rows && moved.raw == r && moved.rows == r + 24);
    }
    CHECK(ctx.bytes == 0 && g_live.empty());
    {   // an allocation that fails: the buffer is empty, the ledger unmoved, what was built before it is given back
        DevBuf<double> a;
        DevBuf<int> b;
        g_fail_in = 1;                                                         // the second hipMalloc of build_two
        CHECK(build_two(c, a, b) == 1 && !g_err.empty());
        CHECK(!a && !b && ctx.bytes == 0 && g_live.empty());
        CHECK(build_two(c, a, b) == 0 && a.count() == 100 && b.count() == 50 && ctx.bytes == 1000);
        g_fail_in = 0;
        CHECK(a.alloc(c, 10) == 1 && !a && a.count() == 0 && ctx.bytes == 200);    // (what it held went first)
        DVector v;
        g_fail_in = 0;
        CHECK(v.alloc(c, 10, 0, 0, nullptr) == 1 && !v.raw && !v.base && !v.rows && ctx.bytes == 200);
    }
    CHECK(ctx.bytes == 0 && g_live.empty());
    {   // levels in a vector that is resized: growth moves them (no copy, no double free), shrinking destroys the tail,
        // `= Slot{}` is a fresh slot
        std::vector<Slot> L(2);
        CHECK(fill(c, L[0], 10) == 0 && fill(c, L[1], 20) == 0);
        const int64_t two = ctx.bytes;
        CHECK(two == (int64_t)((30 + 100) * 8 + 30 * 4 + (60 + 120) * 8 + 60 * 4) && live_bytes() == (size_t)two);
        double* const v0 = L[0].v.raw;
        L.resize(L.capacity() + 5);                                            // reallocates
        CHECK(ctx.bytes == two && L[0].v.raw == v0 && L[0].v.rows == v0 + 24 && L[1].splits[0] == 20 && !L[4].set);
        CHECK(fill(c, L[5], 30) == 0);
        std::swap(L[0].v, L[0].v2);
        L.resize(1);
        CHECK(ctx.bytes == (int64_t)((30 + 100) * 8 + 30 * 4) && L[0].v2.raw == v0);
        L[0] = Slot{};
        CHECK(ctx.bytes == 0 && g_live.empty() && !L[0].set && L[0].mc_ok == -1 && L[0].splits.empty() && !L[0].v2.raw);
        CHECK(fill(c, L[0], 7) == 0);
    }                                                                          // the vector's destructor frees the rest
    CHECK(ctx.bytes == 0 && g_live.empty());
    CHECK(g_mallocs == g_frees && g_mallocs > 30);
    return 0;
}

int main() {
    const int rc = run();
    if (rc == 0) std::printf("devbuf_check: ok, %ld allocations, all freed, ledger at zero\n", g_mallocs);
    return rc;
}
