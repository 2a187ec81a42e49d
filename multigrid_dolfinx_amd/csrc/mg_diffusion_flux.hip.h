// Cell gradients and fluxes of a nodal field for gfx950: the mean of grad x_h over the six Kuhn simplices of every cell of a
// 3-D level, weighted by a cell field (mg_diffusion_cell_gradient: q = -F(kappa, u) is the cell average of -kappa grad u_h),
// its transpose in x (mg_diffusion_cell_gradient_t) and its contraction with a 3-component cell field
// (mg_diffusion_cell_gradient_dot).  From the grid alone: no matrix and no kappa of the level is read, and no mask is applied --
// x is the field itself, Dirichlet values included.
//
// Cells in kappa's order (ck * N + cj) * N + ci, nodes lexicographic, a 3-component cell field with component d in {x, y, z} at
// d * N^3 + cell.  h = 1 / N, s = N / 6.0 computed once on the host.  With U[dz][dy][dx] = x at the corners of cell c:
//   G_d(x)_c = acc_d * s, one accumulator per axis over the cell's four edges of that axis in dk_cell's edge order
//              (mg_diffusion_adj.hip.h) with its weights n = 2, 1, 1, 2:
//                acc_x = 2.0 * (U001 - U000);  acc_x = acc_x + (U011 - U010);  + (U101 - U100);  + 2.0 * (U111 - U110)
//              (the x edges at (dz, dy) = (0,0), (0,1), (1,0), (1,1)); the y edges at (dz, dx) and the z edges at (dy, dx) alike.
//   F(w, x)   -> 3 N^3:    F_{d,c} = w_c * G_d(x)_c; with w null F = G to the bit, no product.
//   C(p, x)   -> N^3:      out_c = ((p_{x,c} * G_x) + p_{y,c} * G_y) + p_{z,c} * G_z.
//   F^T(w, p) -> (N+1)^3:  out_i = acc * s.  acc starts at +0.0 and takes the cells around node i in ascending (oz, oy, ox), the
//              cell being (k + oz, j + oy, i + ox) with each offset -1 then 0; cells outside the grid are skipped.  Inside a cell the
//              products q_d = w_c * p_{d,c} (q_d = p_{d,c} with w null) are formed first, then x, y, z in this order:
//              acc = acc + t or acc = acc - t with t = 2.0 * q_d where the node's two other local coordinates in the cell are
//              equal, else q_d; + where the node is the upper end of its edge of that axis in the cell (offset -1 along it).
// <p, F(w, x)> = <x, F^T(w, p)> = <w, C(p, x)> up to rounding, and the three close under differentiation (torch_diffusion.py).
// The bits are DEFINED by cg_cell_f, cg_cell_c and cg_node_t below, shared by whatever kernel form computes them; poisson.diffusion_cell_gradient,
// _t and _dot restate them add for add.  Built with -ffp-contract=off: no product is fused into an add.
//
// One thread per cell (F, C: eight corner loads through the caches) or per node (F^T: up to eight cells, three or four loads
// each), DK_BLOCK threads, blockIdx.y = the plane.  Byte models per cell: F 8 (x) + 8 (w) + 24 written, C 24 + 8 + 8, F^T 24 + 8 + 8.
// Plane-march forms of F and C on the skeleton of diffusion_dkappa_march (one staged vector, w and p read per cell from global
// memory) were written, measured and deleted: at 257^3 they were 7 % (F) and 15 % (C) SLOWER than these kernels, at 1025^3 18 %
// and 4 % faster -- short of the 10 % at both sizes that kept diffusion_dkappa_march ("Cell gradients and fluxes").
// With one vector instead of two the caches already serve the eight corner loads.
#pragma once
#include "mg_diffusion_adj.hip.h"

namespace mgk {

struct CgArgs {
    const double* w;        // F, F^T: the cell weight ([N][N][N] cells) or null; C: unused
    const double* p;        // C, F^T: the 3-component cell field (3 N^3); F: unused
    const double* x;        // F, C: the nodal field ([nz][ny][nx], x fastest); F^T: unused
    double* out;            // F: 3 N^3, C: N^3, F^T: nodes
    int nx, ny, nz, N;
    int64_t P;              // nx * ny
    int64_t C3;             // N^3
    double s;               // N / 6.0
};

__device__ __forceinline__ void cg_grad(const double (&U)[2][2][2], double s, double (&G)[3]) {
    double a = 2.0 * (U[0][0][1] - U[0][0][0]);
    a = a + (U[0][1][1] - U[0][1][0]);
    a = a + (U[1][0][1] - U[1][0][0]);
    a = a + 2.0 * (U[1][1][1] - U[1][1][0]);
    G[0] = a * s;
    a = 2.0 * (U[0][1][0] - U[0][0][0]);
    a = a + (U[0][1][1] - U[0][0][1]);
    a = a + (U[1][1][0] - U[1][0][0]);
    a = a + 2.0 * (U[1][1][1] - U[1][0][1]);
    G[1] = a * s;
    a = 2.0 * (U[1][0][0] - U[0][0][0]);
    a = a + (U[1][0][1] - U[0][0][1]);
    a = a + (U[1][1][0] - U[0][1][0]);
    a = a + 2.0 * (U[1][1][1] - U[0][1][1]);
    G[2] = a * s;
}

// F of one cell: `w` null leaves G untouched
__device__ __forceinline__ void cg_cell_f(const double (&U)[2][2][2], double s, const double* w, int64_t cell, double (&F)[3]) {
    cg_grad(U, s, F);
    if (w) {
        const double wc = w[cell];
        F[0] = wc * F[0];
        F[1] = wc * F[1];
        F[2] = wc * F[2];
    }
}

// C of one cell
__device__ __forceinline__ double cg_cell_c(const double (&U)[2][2][2], double s, const double* p, int64_t C3, int64_t cell) {
    double G[3];
    cg_grad(U, s, G);
    return ((p[cell] * G[0]) + p[C3 + cell] * G[1]) + p[2 * C3 + cell] * G[2];
}

// F^T of node (i, j, k)
__device__ __forceinline__ double cg_node_t(const CgArgs& a, int i, int j, int k) {
    double acc = 0.0;
#pragma unroll
    for (int oz = -1; oz <= 0; ++oz)
#pragma unroll
        for (int oy = -1; oy <= 0; ++oy)
#pragma unroll
            for (int ox = -1; ox <= 0; ++ox) {
                const int ci = i + ox, cj = j + oy, ck = k + oz;
                if (ci < 0 || ci >= a.N || cj < 0 || cj >= a.N || ck < 0 || ck >= a.N) continue;
                const int64_t cell = ((int64_t)ck * a.N + cj) * a.N + ci;
                double q[3] = {a.p[cell], a.p[a.C3 + cell], a.p[2 * a.C3 + cell]};
                if (a.w) {
                    const double wc = a.w[cell];
                    q[0] = wc * q[0];
                    q[1] = wc * q[1];
                    q[2] = wc * q[2];
                }
                // the node's local coordinates in the cell are (-oz, -oy, -ox): upper end along an axis where the offset is -1
                const double tx = oy == oz ? 2.0 * q[0] : q[0];
                acc = ox < 0 ? acc + tx : acc - tx;
                const double ty = ox == oz ? 2.0 * q[1] : q[1];
                acc = oy < 0 ? acc + ty : acc - ty;
                const double tz = ox == oy ? 2.0 * q[2] : q[2];
                acc = oz < 0 ? acc + tz : acc - tz;
            }
    return acc * a.s;
}

// KIND of the cell kernels
constexpr int CG_F = 0, CG_C = 1;

// blockIdx.x: DK_BLOCK cells of a cell plane (x fastest), blockIdx.y: the cell plane
template <int KIND>
__global__ __launch_bounds__(DK_BLOCK) void cell_grad_cells(CgArgs a) {
    const int64_t t = (int64_t)blockIdx.x * DK_BLOCK + threadIdx.x;
    if (t >= (int64_t)a.N * a.N) return;
    const int ci = (int)(t % a.N), cj = (int)(t / a.N), ck = blockIdx.y;
    double U[2][2][2];
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx)
                U[dz][dy][dx] = a.x[(int64_t)(ck + dz) * a.P + (int64_t)(cj + dy) * a.nx + (ci + dx)];
    const int64_t cell = (int64_t)ck * a.N * a.N + t;
    if constexpr (KIND == CG_F) {
        double F[3];
        cg_cell_f(U, a.s, a.w, cell, F);
        a.out[cell] = F[0];
        a.out[a.C3 + cell] = F[1];
        a.out[2 * a.C3 + cell] = F[2];
    } else {
        a.out[cell] = cg_cell_c(U, a.s, a.p, a.C3, cell);
    }
}

// blockIdx.x: DK_BLOCK nodes of a node plane, blockIdx.y: the plane
__global__ __launch_bounds__(DK_BLOCK) void cell_grad_t(CgArgs a) {
    const int64_t t = (int64_t)blockIdx.x * DK_BLOCK + threadIdx.x;
    if (t >= a.P) return;
    const int i = (int)(t % a.nx), j = (int)(t / a.nx), k = blockIdx.y;
    a.out[(int64_t)k * a.P + t] = cg_node_t(a, i, j, k);
}

}  // namespace mgk
