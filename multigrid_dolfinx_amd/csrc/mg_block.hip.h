// Block linear algebra of a Rayleigh-Ritz step (mg_eigs, mg_block_gram, mg_block_combine): streaming kernels over whole
// level vectors.  Every vector is a row pointer of one level, 16-byte aligned like the fcg_* operands, so the bodies move
// double2 and thread 0 takes an odd last row.  No atomics: every block writes its own partial sums, fcg_fold sums them in
// a fixed order.
#pragma once

#include "mg_kernels.hip.h"

namespace mgk {

constexpr int BG_MAX = 4;           // vectors per side of one block_gram tile
constexpr int BC_MAX_IN = 24;       // inputs / outputs of one block_combine launch
constexpr int BC_MAX_OUT = 8;

struct GramArgs {
    const double* a[BG_MAX];
    const double* b[BG_MAX];
    const double* d;                // nodal weight (WEIGHTED), row-based
    double* out;                    // gridDim.x groups of NA * NB partial sums, pair (i, j) at i * NB + j
    int64_t n;
};

// Partial sums of a_i . (d * b_j) for the NA x NB pairs of one tile: one pass reads NA + NB (+ 1) vectors, 8 (NA + NB (+ 1))
// bytes per row.  Each accumulator is ONE fma chain over the thread's rows in ascending order (x then y of a double2, the
// odd last row at thread 0), the product d * b_j rounded once before it: the sum of pair (i, j) does not depend on the tile
// it was computed in as long as the grid is the level's (gram_grid), so a 1 x 1 and a 4 x 4 launch give a pair the same bits.
template <int NA, int NB, bool WEIGHTED>
__global__ __launch_bounds__(BLOCK) void block_gram(GramArgs g) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    double acc[NA][NB];
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = 0.0;
    for (int64_t t = tid; t < (g.n >> 1); t += stride) {
        double2 a[NA], b[NB];
#pragma unroll
        for (int i = 0; i < NA; ++i) a[i] = reinterpret_cast<const double2*>(g.a[i])[t];
#pragma unroll
        for (int j = 0; j < NB; ++j) b[j] = reinterpret_cast<const double2*>(g.b[j])[t];
        if (WEIGHTED) {
            const double2 d = reinterpret_cast<const double2*>(g.d)[t];
#pragma unroll
            for (int j = 0; j < NB; ++j) { b[j].x = d.x * b[j].x; b[j].y = d.y * b[j].y; }
        }
#pragma unroll
        for (int i = 0; i < NA; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                acc[i][j] = fma(a[i].x, b[j].x, acc[i][j]);
                acc[i][j] = fma(a[i].y, b[j].y, acc[i][j]);
            }
    }
    if (tid == 0 && (g.n & 1)) {
        const int64_t t = g.n - 1;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const double bj = WEIGHTED ? g.d[t] * g.b[j][t] : g.b[j][t];
#pragma unroll
            for (int i = 0; i < NA; ++i) acc[i][j] = fma(g.a[i][t], bj, acc[i][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const double s = block_sum(acc[i][j]);
            if (threadIdx.x == 0) g.out[(int64_t)blockIdx.x * (NA * NB) + i * NB + j] = s;
        }
}

struct CombineArgs {
    const double* s[BC_MAX_IN];
    double* out[BC_MAX_OUT];
    double c[BC_MAX_IN * BC_MAX_OUT];   // c[i * NO + o], in the kernel arguments (1.5 KiB at most)
    int64_t n;
};

// out_o[t] = sum_i c[i][o] s_i[t], i ascending: the first product, then one fma per further input.  A thread reads its rows
// of ALL inputs before it writes any output, and rows are independent, so an output may BE one of the inputs (the pointers
// carry no __restrict__).  8 (NS + NO) bytes per row.
template <int NS, int NO>
__global__ __launch_bounds__(BLOCK) void block_combine(CombineArgs g) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = tid; t < (g.n >> 1); t += stride) {
        double2 v[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) v[i] = reinterpret_cast<const double2*>(g.s[i])[t];
        double2 r[NO];
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            r[o].x = g.c[o] * v[0].x; r[o].y = g.c[o] * v[0].y;
#pragma unroll
            for (int i = 1; i < NS; ++i) {
                r[o].x = fma(g.c[i * NO + o], v[i].x, r[o].x);
                r[o].y = fma(g.c[i * NO + o], v[i].y, r[o].y);
            }
        }
#pragma unroll
        for (int o = 0; o < NO; ++o) reinterpret_cast<double2*>(g.out[o])[t] = r[o];
    }
    if (tid == 0 && (g.n & 1)) {
        const int64_t t = g.n - 1;
        double v[NS], r[NO];
#pragma unroll
        for (int i = 0; i < NS; ++i) v[i] = g.s[i][t];
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            r[o] = g.c[o] * v[0];
#pragma unroll
            for (int i = 1; i < NS; ++i) r[o] = fma(g.c[i * NO + o], v[i], r[o]);
        }
#pragma unroll
        for (int o = 0; o < NO; ++o) g.out[o][t] = r[o];
    }
}

// ---- the vector kernels of mg_eigs --------------------------------------------------------------------------------------
// The lumped mass m = R(rho) is +0.0 on the Dirichlet nodes of the level's face set and > 0 on every free node, so m > 0
// is the free-node test of all of them.

// m (reaction_diag: every node has its value) -> +0.0 on the nodes outside the free box; lexicographic nodes, x fastest
__global__ void eigs_mass_mask(double* __restrict__ m, FreeBox box, int nx, int ny, int64_t n) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(t % nx), j = (int)((t / nx) % ny), k = (int)(t / ((int64_t)nx * ny));
        if (!free_node(box, i, j, k)) m[t] = 0.0;
    }
}

__global__ void eigs_fill(double* __restrict__ x, int64_t n, double value) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) x[t] = value;
}

// Set-up check of a density field: as sigma_check, for entries that are not finite doubles > 0.
__global__ void rho_check(const double* __restrict__ rho, int64_t n, unsigned long long* first) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        const double x = rho[q];
        if (!(x > 0.0 && x <= 1.7976931348623157e308)) atomicMin(first, (unsigned long long)q);
    }
}

// the start block of a cold call: x[t] = cheb_hash(row + offset) on free rows, +0.0 on Dirichlet rows
__global__ void eigs_start(double* __restrict__ x, const double* __restrict__ m, int64_t n, uint64_t offset) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
        x[t] = m[t] > 0.0 ? cheb_hash((uint64_t)t + offset) : 0.0;
}

// x = +0.0 on Dirichlet rows (a warm start, the cycle's result, the Ritz vectors on their way out)
__global__ void eigs_mask(double* __restrict__ x, const double* __restrict__ m, int64_t n) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
        if (!(m[t] > 0.0)) x[t] = 0.0;
}

struct EigsResidArgs {
    const double* kx; const double* x; const double* m;
    double* r;
    double* out;        // partial sums: r . r at 2 block, (m x) . (m x) at 2 block + 1
    double lambda;
    int64_t n;
};

// r = K x - lambda (m * x) on free rows, +0.0 on Dirichlet rows, with the partial sums of both norms of the stopping test in
// the same pass: 24 B read and 8 B written per row.
__device__ __forceinline__ double eigs_resid_row(double kx, double x, double m, double lambda, double& rr, double& mm) {
    const double mx = m * x;
    const double r = m > 0.0 ? fma(-lambda, mx, kx) : 0.0;
    rr = fma(r, r, rr);
    mm = fma(mx, mx, mm);
    return r;
}

__global__ __launch_bounds__(BLOCK) void eigs_residual(EigsResidArgs a) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    double rr = 0.0, mm = 0.0;
    for (int64_t t = tid; t < (a.n >> 1); t += stride) {
        const double2 kx = reinterpret_cast<const double2*>(a.kx)[t], x = reinterpret_cast<const double2*>(a.x)[t],
                      m = reinterpret_cast<const double2*>(a.m)[t];
        double2 r;
        r.x = eigs_resid_row(kx.x, x.x, m.x, a.lambda, rr, mm);
        r.y = eigs_resid_row(kx.y, x.y, m.y, a.lambda, rr, mm);
        reinterpret_cast<double2*>(a.r)[t] = r;
    }
    if (tid == 0 && (a.n & 1)) {
        const int64_t t = a.n - 1;
        a.r[t] = eigs_resid_row(a.kx[t], a.x[t], a.m[t], a.lambda, rr, mm);
    }
    const double s1 = block_sum(rr);
    const double s2 = block_sum(mm);
    if (threadIdx.x == 0) { a.out[2 * blockIdx.x] = s1; a.out[2 * blockIdx.x + 1] = s2; }
}

}  // namespace mgk
