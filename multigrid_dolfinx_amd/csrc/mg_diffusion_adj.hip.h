// Sensitivity of the diffusion operator to kappa for gfx950: out[c] = d(a^T A(kappa) b) / d kappa_c for every cell c of a
// 3-D level, from the grid alone (mg_diffusion_dkappa).
//
// A(kappa) of gen_diffusion (mg_kernels.hip.h) is linear in kappa: the axis edge e = (i, j) carries
// w_e = (sum_c n_{c,e} kappa_c) h / 6 over the four cells around it, a_ij = a_ji = -w_e and the diagonal is the sum of the
// row's w_e.  Boundary rows are identity rows and interior rows have no boundary column, so with the boundary entries of
// a and b taken as 0 (a~, b~)
//     a~^T A b~ = sum_e w_e (a~_i - a~_j) (b~_i - b~_j),        d / d kappa_c = (h / 6) sum_{12 edges of c} n_{c,e} (...)(...)
// with n_{c,e} = 2 where the cell's two other local coordinates at the edge are equal, else 1 -- gen_diffusion's weights.
// Neither kappa nor a matrix is read: the kernel works on stored and on matrix-free levels alike.
//
// The result is DEFINED by dk_cell below, which poisson.diffusion_dkappa restates add for add (same bits):
//   * A[dz][dy][dx], B[dz][dy][dx]: a~, b~ at the cell's corner (ci + dx, cj + dy, ck + dz);
//   * an edge's term is (A_upper - A_lower) * (B_upper - B_lower), upper = the end with the larger coordinate, times 2.0
//     where n = 2 (exact);
//   * one accumulator takes the twelve terms in this order: the x edges at (dz, dy) = (0,0), (0,1), (1,0), (1,1)
//     (n = 2, 1, 1, 2), the y edges at (dz, dx) in the same order, the z edges at (dy, dx) in the same order;
//   * out = acc * (h / 6.0), the scale computed once on the host as (1.0 / N) / 6.0.
// Built with -ffp-contract=off like everything else: no product is fused into an add.
//
// One thread per cell; a cell needs its eight corners of a and of b, read through the caches (sixteen loads, each node
// shared by up to eight cells of neighbouring threads and planes).  Model: 8 + 8 B per node read, 8 B per cell written.
// Nodes on the boundary are not loaded at all: the mask is the zero.
//
// mg_diffusion_dkappa_ex takes the mask per vector (a_all, b_all): out[c] = d / d w_c (M_A a)^T A^(w) (M_B b) with A^ the
// natural P1 matrix of a cell field on all nodes (no boundary condition) and M the mask of the interior nodes or the
// identity.  The mask acts where a node is loaded and nowhere else: dk_cell and its adds are the same, and (interior,
// interior) is mg_diffusion_dkappa to the bit.  An unmasked vector is read at every corner: all of them are on the grid.
//
// With a face set (mg_set_diffusion_faces) the interior nodes are the free nodes of the set, nodes on no-flux faces
// included: both kernels take the box of the free nodes (FreeBox) where they had 1 <= index <= n - 2, and nothing else
// changes.  The default set gives that box.
#pragma once
#include "mg_kernels.hip.h"

namespace mgk {

constexpr int DK_BLOCK = 256;

struct DkArgs {
    const double* a;        // [nz][ny][nx] nodes, x fastest (lexicographic); may be the same pointer as b
    const double* b;
    double* out;            // [N][N][N] cells, x fastest
    int nx, ny, nz, N;      // nodes per axis (N + 1 each), cells per axis
    int64_t P;              // nx * ny
    double scale;           // h / 6.0
    int a_all, b_all;       // 0: the entries of the vector outside `box` count as 0 (not loaded); 1: every node is read
    FreeBox box;            // the free nodes of the handle's face set (the default set: the interior nodes)
};

// one pointer passed twice is loaded once -- where both vectors are masked alike, or the one mask would serve the other
__device__ __forceinline__ bool dk_same(const DkArgs& p) { return p.a == p.b && p.a_all == p.b_all; }

__device__ __forceinline__ double dk_cell(const double (&A)[2][2][2], const double (&B)[2][2][2], double scale) {
    double s = 2.0 * ((A[0][0][1] - A[0][0][0]) * (B[0][0][1] - B[0][0][0]));
    s = s + (A[0][1][1] - A[0][1][0]) * (B[0][1][1] - B[0][1][0]);
    s = s + (A[1][0][1] - A[1][0][0]) * (B[1][0][1] - B[1][0][0]);
    s = s + 2.0 * ((A[1][1][1] - A[1][1][0]) * (B[1][1][1] - B[1][1][0]));
    s = s + 2.0 * ((A[0][1][0] - A[0][0][0]) * (B[0][1][0] - B[0][0][0]));
    s = s + (A[0][1][1] - A[0][0][1]) * (B[0][1][1] - B[0][0][1]);
    s = s + (A[1][1][0] - A[1][0][0]) * (B[1][1][0] - B[1][0][0]);
    s = s + 2.0 * ((A[1][1][1] - A[1][0][1]) * (B[1][1][1] - B[1][0][1]));
    s = s + 2.0 * ((A[1][0][0] - A[0][0][0]) * (B[1][0][0] - B[0][0][0]));
    s = s + (A[1][0][1] - A[0][0][1]) * (B[1][0][1] - B[0][0][1]);
    s = s + (A[1][1][0] - A[0][1][0]) * (B[1][1][0] - B[0][1][0]);
    s = s + 2.0 * ((A[1][1][1] - A[0][1][1]) * (B[1][1][1] - B[0][1][1]));
    return s * scale;
}

// blockIdx.x: DK_BLOCK cells of a cell plane (x fastest), blockIdx.y: the cell plane
__global__ __launch_bounds__(DK_BLOCK) void diffusion_dkappa_gather(DkArgs p) {
    const int64_t t = (int64_t)blockIdx.x * DK_BLOCK + threadIdx.x;
    if (t >= (int64_t)p.N * p.N) return;
    const int ci = (int)(t % p.N), cj = (int)(t / p.N), ck = blockIdx.y;
    const bool same = dk_same(p);
    double A[2][2][2], B[2][2][2];
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int i = ci + dx, j = cj + dy, k = ck + dz;
                const bool inner = free_node(p.box, i, j, k);
                const int64_t r = (int64_t)k * p.P + (int64_t)j * p.nx + i;
                A[dz][dy][dx] = inner || p.a_all ? p.a[r] : 0.0;
                B[dz][dy][dx] = inner || p.b_all ? (same ? A[dz][dy][dx] : p.b[r]) : 0.0;
            }
    p.out[(int64_t)ck * p.N * p.N + t] = dk_cell(A, B, p.scale);
}

// ---- sensitivities of the lumped reaction term R(sigma) (mg_kernels.hip.h, reaction_diag) --------------------------------
// R is diagonal and linear in sigma.  T_sigma(w, x)_i = R(w)_i x_i on free nodes and +0.0 on Dirichlet nodes
// (diffusion_apply_dsigma), and its adjoint D_sigma(a, b)_c = scale * sum_i t_{c,i} a~_i b~_i over the eight corners of cell c
// (diffusion_dsigma), a~ and b~ taking Dirichlet nodes as 0:  a . T_sigma(w, x) = w . D_sigma(a, x).  Neither reads sigma or a
// matrix.  The bits are DEFINED here and restated by poisson.diffusion_dsigma / diffusion_apply_dsigma:
//   * D: one accumulator starts with 6.0 * (A * B) of corner (0,0,0) and takes t * (A * B) of the other corners in ascending
//     (dz, dy, dx), t = 6.0 at (1,1,1) and 2.0 elsewhere; out = acc * scale with scale = h^3 / 24.0 from the host.  The mask
//     acts where a node is loaded, as in diffusion_dkappa_gather.
//   * T: react_node's sum (mg_kernels.hip.h), then one product with x.  No fma: -ffp-contract=off.
// Streaming kernels: D reads 8 + 8 B per node through the caches and writes 8 B per cell, T reads 8 B per cell and per node
// and writes 8 B per node.
struct DsArgs {
    const double* a;        // D: a, T: the direction dsigma ([N][N][N] cells)
    const double* b;        // D: b (may be a), T: x
    double* out;            // D: cells, T: nodes
    int nx, ny, nz, N;
    int64_t P;
    double scale;           // D: h^3 / 24.0, T: h^3
    FreeBox box;
};

__global__ __launch_bounds__(DK_BLOCK) void diffusion_dsigma(DsArgs p) {
    const int64_t t = (int64_t)blockIdx.x * DK_BLOCK + threadIdx.x;
    if (t >= (int64_t)p.N * p.N) return;
    const int ci = (int)(t % p.N), cj = (int)(t / p.N), ck = blockIdx.y;
    const bool same = p.a == p.b;
    double s = 0.0;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int i = ci + dx, j = cj + dy, k = ck + dz;
                const bool inner = free_node(p.box, i, j, k);
                const int64_t r = (int64_t)k * p.P + (int64_t)j * p.nx + i;
                const double A = inner ? p.a[r] : 0.0;
                const double B = inner ? (same ? A : p.b[r]) : 0.0;
                const double term = (dx == dy && dy == dz ? 6.0 : 2.0) * (A * B);
                s = dz + dy + dx == 0 ? term : s + term;
            }
    p.out[(int64_t)ck * p.N * p.N + t] = s * p.scale;
}

// blockIdx.x: DK_BLOCK nodes of a node plane, blockIdx.y: the plane
__global__ __launch_bounds__(DK_BLOCK) void diffusion_apply_dsigma(DsArgs p) {
    const int64_t t = (int64_t)blockIdx.x * DK_BLOCK + threadIdx.x;
    if (t >= p.P) return;
    const int i = (int)(t % p.nx), j = (int)(t / p.nx), k = blockIdx.y;
    const int64_t r = (int64_t)k * p.P + t;
    p.out[r] = free_node(p.box, i, j, k) ? react_node(p.a, p.N, i, j, k, p.scale) * p.b[r] : 0.0;
}

// ---- sensitivities of the lumped Robin term B(alpha) (mg_kernels.hip.h, robin_diag), per face F ------------------------
// B is diagonal and linear in alpha.  T_alpha,F(w, x)_i = b_F(w)_i x_i on the free nodes of F and +0.0 on every other node
// of the level (diffusion_apply_drobin), and its adjoint D_alpha,F(a, b)_q = scale * sum_i t_{q,i} a~_i b~_i over the four
// corners of face-cell q (diffusion_drobin), a~ and b~ taking Dirichlet nodes as 0.  The bits are DEFINED here and restated
// by poisson.diffusion_drobin / diffusion_apply_drobin:
//   * D: one accumulator starts with 2.0 * (A * B) of corner (0,0) and takes t * (A * B) of the others in ascending
//     (db, da), t = 2.0 at (1,1) and 1.0 elsewhere; out = acc * scale with scale = h^2 / 6.0 from the host.
//   * T: robin_face_node's sum, then one product with x.  No fma: -ffp-contract=off.
// D reads 8 + 8 B per face node and writes 8 B per face-cell; T writes all n_global nodes (8 B each) and reads x and the
// field on the face only.
struct DrArgs {
    const double* a;        // D: a, T: the direction dalpha ([N][N] face-cells)
    const double* b;        // D: b (may be a), T: x
    double* out;            // D: face-cells, T: nodes
    int nx, nz, N;
    int axis, at;           // the face: normal to `axis`, at node index `at` (0 or N) along it
    int64_t P;
    double scale;           // D: h^2 / 6.0, T: h^2
    FreeBox box;
};

__global__ __launch_bounds__(DK_BLOCK) void diffusion_drobin(DrArgs p) {
    const int64_t t = (int64_t)blockIdx.x * DK_BLOCK + threadIdx.x;
    if (t >= (int64_t)p.N * p.N) return;
    const int ca = (int)(t % p.N), cb = (int)(t / p.N);
    const bool same = p.a == p.b;
    double s = 0.0;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int da = 0; da < 2; ++da) {
            const int pa = ca + da, pb = cb + db;
            const int i = p.axis == 0 ? p.at : pa, j = p.axis == 0 ? pa : (p.axis == 1 ? p.at : pb), k = p.axis == 2 ? p.at : pb;
            const bool inner = free_node(p.box, i, j, k);
            const int64_t r = (int64_t)k * p.P + (int64_t)j * p.nx + i;
            const double A = inner ? p.a[r] : 0.0;
            const double B = inner ? (same ? A : p.b[r]) : 0.0;
            const double term = (da == db ? 2.0 : 1.0) * (A * B);
            s = db + da == 0 ? term : s + term;
        }
    p.out[t] = s * p.scale;
}

// blockIdx.x: DK_BLOCK nodes of a node plane, blockIdx.y: the plane
__global__ __launch_bounds__(DK_BLOCK) void diffusion_apply_drobin(DrArgs p) {
    const int64_t t = (int64_t)blockIdx.x * DK_BLOCK + threadIdx.x;
    if (t >= p.P) return;
    const int i = (int)(t % p.nx), j = (int)(t / p.nx), k = blockIdx.y;
    const int64_t r = (int64_t)k * p.P + t;
    const int c = p.axis == 0 ? i : (p.axis == 1 ? j : k);
    double o = 0.0;
    if (c == p.at && free_node(p.box, i, j, k)) {
        int pa, pb;
        face_plane(p.axis, i, j, k, pa, pb);
        o = robin_face_node(p.a, p.N, pa, pb, p.scale) * p.b[r];
    }
    p.out[r] = o;
}

// The plane march, in the shape of diffusion_mf (mg_diffusion_mf.hip.h): a tile of MF_TX x MF_TY cells goes up through the cell
// planes of a z segment.  The masked images of a and b (tile + one line of nodes in x and y) of node planes k and k + 1 are
// in LDS, two slots per vector: step k reads plane k + 1 (the corners of plane k stay in registers from the step before),
// writes plane k + 2 over plane k from registers whose loads were issued a step earlier, and issues the loads of plane k + 3
// before its arithmetic; one barrier per step.  A wave reads 64 consecutive doubles of an image line: no bank conflicts.
constexpr int DK_W = MF_TX + 1, DK_S = DK_W * (MF_TY + 1);

struct DkMarchArgs {
    DkArgs d;
    int ntx, nty, nseg, seglen;     // tiles of cells, segments of cell planes
    unsigned nitems, ch;
};

__global__ __launch_bounds__(MF_NT) void diffusion_dkappa_march(DkMarchArgs m) {
    __shared__ double sA[2][DK_S];
    __shared__ double sB[2][DK_S];
    const DkArgs& p = m.d;
    const int tid = threadIdx.x;
    const int lx = tid & 63, ly = tid >> 6;
    unsigned id;
    {
        const unsigned b = blockIdx.x, xcd = b & 7u, j = b >> 3, ch = m.ch;
        id = ((j / ch) * 8u + xcd) * ch + (j % ch);
    }
    if (id >= m.nitems) return;
    const unsigned ntile = (unsigned)(m.ntx * m.nty);
    const int seg = (int)(id / ntile);
    const unsigned t = id % ntile;
    const int tix = (int)(t / (unsigned)m.nty), tiy = (int)(t % (unsigned)m.nty);
    const int z0 = seg * m.seglen, z1 = min(p.N, z0 + m.seglen);       // cell planes [z0, z1)
    const int tx0 = tix * MF_TX, ty0 = tiy * MF_TY;
    const int ci = tx0 + lx, cj = ty0 + ly;
    const bool on_grid = ci < p.N && cj < p.N;
    const bool same = dk_same(p);

    // the elements of an image this thread fills: e = tid and tid + MF_NT; -1: outside the grid (0); ni: a free node of
    // its plane (a masked vector reads no other)
    int64_t no[2];
    int ne[2];
    bool ni[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int e = tid + q * MF_NT;
        ne[q] = e < DK_S ? e : -1;
        const int i = tx0 + e % DK_W, j = ty0 + e / DK_W;
        no[q] = (e < DK_S && i <= p.nx - 1 && j <= p.ny - 1) ? (int64_t)j * p.nx + i : -1;
        ni[q] = i >= p.box.lo[0] && i <= p.box.hi[0] && j >= p.box.lo[1] && j <= p.box.hi[1];
    }
    auto load = [&](int plane, double (&va)[2], double (&vb)[2]) {
        const bool on = plane >= 0 && plane <= p.nz - 1, ok = plane >= p.box.lo[2] && plane <= p.box.hi[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const bool in = on && no[q] >= 0, inner = ok && ni[q];
            va[q] = in && (inner || p.a_all) ? p.a[(int64_t)plane * p.P + no[q]] : 0.0;
            vb[q] = in && (inner || p.b_all) ? (same ? va[q] : p.b[(int64_t)plane * p.P + no[q]]) : 0.0;
        }
    };
    auto park = [&](int plane, const double (&va)[2], const double (&vb)[2]) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (ne[q] >= 0) {
                sA[plane & 1][ne[q]] = va[q];
                sB[plane & 1][ne[q]] = vb[q];
            }
    };
    const int c0 = ly * DK_W + lx;      // corner (ci, cj) of this cell in an image
    auto corners = [&](int plane, double (&A)[2][2], double (&B)[2][2]) {
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                A[dy][dx] = sA[plane & 1][c0 + dy * DK_W + dx];
                B[dy][dx] = sB[plane & 1][c0 + dy * DK_W + dx];
            }
    };

    // ---- warm-up: planes z0 and z0 + 1 in place, the corners of plane z0 in registers, plane z0 + 2 on its way ----
    double ra[2], rb[2], A[2][2][2], B[2][2][2];
    load(z0, ra, rb); park(z0, ra, rb);
    load(z0 + 1, ra, rb); park(z0 + 1, ra, rb);
    load(z0 + 2, ra, rb);
    __syncthreads();
    corners(z0, A[0], B[0]);
    __syncthreads();                    // (step z0 writes plane z0 + 2 over plane z0)

    const int64_t CP = (int64_t)p.N * p.N;
    for (int k = z0; k < z1; ++k) {
        park(k + 2, ra, rb);
        if (k + 3 <= z1) load(k + 3, ra, rb);
        corners(k + 1, A[1], B[1]);
        if (on_grid) p.out[(int64_t)k * CP + (int64_t)cj * p.N + ci] = dk_cell(A, B, p.scale);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                A[0][dy][dx] = A[1][dy][dx];
                B[0][dy][dx] = B[1][dy][dx];
            }
        __syncthreads();
    }
}

}  // namespace mgk
