// Insulated bodies (mg_set_diffusion_insulated): the projections of a solve whose operator has the constants as its null
// space, and the pin of the coarsest level's factorisation.
//
// A mean removal is two plain streams over n rows (16-byte aligned: a level's row pointer, vec_front):
//   ns_partial   part[b] = sum over block b's rows of w_i x_i (w null: of x_i)                            8 or 16 B/row
//   fcg_fold     one block: the partial sums in a fixed order -> one total
//   ns_subtract  x_i -= m u_i (u null: x_i -= m), m = inv_denom * total                                  16 or 24 B/row
// so with the right w, u and inv_denom one pair is each of
//   Q   x = x - 1 (w.x) / s       (w = the lumped mass, u null, inv_denom = 1 / s)
//   Q^T b = b - w (1.b) / s       (w null, u = the lumped mass, inv_denom = 1 / s)
//   the Euclidean one, x - 1 (1.x) / n  (w, u null, inv_denom = 1 / n).
// Block b takes the rows [NS_TILE b, NS_TILE (b + 1)), so the grid and every order of summation depend on n alone: the same
// bits on every run and on every device.  No atomics.
#pragma once
#include "mg_kernels.hip.h"

namespace mgk {

constexpr int NS_TILE = 8 * BLOCK;          // rows per workgroup: four double2 per thread

__host__ __device__ __forceinline__ int64_t ns_blocks(int64_t n) { return n > 0 ? (n + NS_TILE - 1) / NS_TILE : 1; }

__global__ __launch_bounds__(BLOCK) void ns_partial(const double* __restrict__ x, const double* __restrict__ w, int64_t n,
                                                    double* __restrict__ part) {
    const int64_t lo = (int64_t)blockIdx.x * NS_TILE, hi = lo + NS_TILE < n ? lo + NS_TILE : n;
    const int64_t pairs = (hi - lo) >> 1;       // (lo is even: the tile is)
    const double2* X = reinterpret_cast<const double2*>(x + lo);
    const double2* W = reinterpret_cast<const double2*>(w ? w + lo : nullptr);
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < pairs; i += BLOCK) {
        const double2 xv = X[i];
        if (w) {
            const double2 wv = W[i];
            acc = fma(wv.x, xv.x, acc); acc = fma(wv.y, xv.y, acc);
        } else {
            acc += xv.x; acc += xv.y;
        }
    }
    if (threadIdx.x == 0 && ((hi - lo) & 1)) acc = w ? fma(w[hi - 1], x[hi - 1], acc) : acc + x[hi - 1];
    const double s = block_sum(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(BLOCK) void ns_subtract(double* __restrict__ x, const double* __restrict__ u, int64_t n,
                                                     const double* __restrict__ total, double inv_denom,
                                                     double* __restrict__ mean_out) {
    const double m = *total * inv_denom;
    if (mean_out && blockIdx.x == 0 && threadIdx.x == 0) *mean_out = m;
    const int64_t lo = (int64_t)blockIdx.x * NS_TILE, hi = lo + NS_TILE < n ? lo + NS_TILE : n;
    const int64_t pairs = (hi - lo) >> 1;
    double2* X = reinterpret_cast<double2*>(x + lo);
    const double2* U = reinterpret_cast<const double2*>(u ? u + lo : nullptr);
    for (int64_t i = threadIdx.x; i < pairs; i += BLOCK) {
        double2 xv = X[i];
        if (u) {
            const double2 uv = U[i];
            xv.x = fma(-m, uv.x, xv.x); xv.y = fma(-m, uv.y, xv.y);
        } else {
            xv.x -= m; xv.y -= m;
        }
        X[i] = xv;
    }
    if (threadIdx.x == 0 && ((hi - lo) & 1)) x[hi - 1] = u ? fma(-m, u[hi - 1], x[hi - 1]) : x[hi - 1] - m;
}

// The coarsest level's first diagonal block with node 0 pinned: identity row, column dropped.  What is left is the
// operator on the other nodes, which is regular, so Gauss-Jordan meets no rounding-size pivot.
__global__ void ns_pin_dense(double* __restrict__ A, int p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p) return;
    A[(size_t)i * p] = i == 0 ? 1.0 : 0.0;
    if (i) A[i] = 0.0;
}

// ... and, inverted, with the pinned node's entry dropped: row and column 0 of the inverse are zero, so the node's value is
// 0 whatever its right-hand side holds, and no coupling of the next block reaches it
__global__ void ns_unpin_inverse(double* __restrict__ T) {
    if (blockIdx.x == 0 && threadIdx.x == 0) T[0] = 0.0;
}

}  // namespace mgk
