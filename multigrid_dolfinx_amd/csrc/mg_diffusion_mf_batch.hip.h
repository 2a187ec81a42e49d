// The matrix-free diffusion march (mg_diffusion_mf.hip.h) over NV vectors at once: one operator, several right-hand sides.
//
// The one-vector march is bound by the rebuild of the row -- eight kappa reads from LDS, six edge sums, the diagonal sum and
// seven mf_div6 per node -- and its LDS traffic, not by HBM ("Matrix-free diffusion levels").  That rebuild does
// not depend on the vector.  Here a row is rebuilt ONCE per node, its seven entries stay in registers, and they are applied
// to NV vectors:
//   * the same tile (MF_TX x MF_TY), the same MfPlan of the level (tiles, segments, ch, workgroup order), the same rotation of
//     the images through 4 (x) and 3 (kappa) slots, one barrier per step;
//   * one set of x images per vector, ONE kappa image, one read of the nodal diagonal term (REACT) per row;
//   * the fma chain (z-, y-, x-, diag, x+, y+, z+), the epilogue and the x0 * acc partial sum once per vector, expression for
//     expression as in mf_march; DOT writes one partial sum per workgroup and vector, reduced in mf_march's order.
// So every output double and every partial sum of every vector has the bits the one-vector kernel gives for that vector
// alone (tests/test_diffusion_batch.py).  Modes: Jacobi, residual, SpMV (with or without DOT); default faces or the box of a
// face set (FACES); with or without the nodal diagonal term (REACT).  No TANGENT, no Chebyshev step: those run per vector.
//
// LDS: NV * 4 * MF_XS * 8 B of x images + 3 * MF_KS * 8 B of kappa + the partial sums: 56 / 77 / 99 KB at NV = 2 / 3 / 4 of
// the 160 KiB of a CU, so 2 / 2 / 1 workgroups share a CU instead of the 4 the plan's "4 x CUs slots" assumes.  The plan must
// stay the level's for the partial sums to match; what that costs is measured ("Batched solves").
#pragma once
#include "mg_diffusion_mf.hip.h"

namespace mgk {

constexpr int MF_BATCH_MAX = 4;     // the largest NV instantiated

template <int NV>
struct MfBatchArgs {
    MfArgs a;               // x, f, out, partials unused: the geometry, the plan, kappa, h, omega
    FreeBox box;            // FACES: the free nodes of the level's face set
    const double* r;        // REACT: the nodal diagonal term, row-based
    const double* x[NV];    // row-based, one per vector
    const double* f[NV];
    double* out[NV];        // != x of any vector
    double* partials[NV];   // DOT: one partial sum of x . (A x) per block and vector
};

template <int NV, int MODE, bool DOT, bool FACES, bool REACT>
__global__ __launch_bounds__(MF_NT) void diffusion_mf_batch(MfBatchArgs<NV> ba) {
    static_assert(NV >= 2 && NV <= MF_BATCH_MAX, "one vector runs mf_march");
    static_assert(MODE == MODE_JACOBI || MODE == MODE_RESIDUAL || MODE == MODE_SPMV, "no Chebyshev step, no Gauss-Seidel");
    static_assert(!DOT || MODE == MODE_SPMV, "the partial sums are the SpMV's");
    const MfArgs& a = ba.a;
    const FreeBox& box = ba.box;
    constexpr double KPAD = FACES ? 0.0 : 1.0;      // a cell outside the grid
    __shared__ double sX[NV][4][MF_XS];
    __shared__ double sK[3][MF_KS];
    __shared__ double s_part[NV][MF_NT / WAVE];
    const int tid = threadIdx.x;
    const int lx = tid & 63, ly = tid >> 6;

    unsigned id;
    {
        const unsigned b = blockIdx.x, xcd = b & 7u, j = b >> 3, ch = a.ch;
        id = ((j / ch) * 8u + xcd) * ch + (j % ch);
    }
    double dot[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) dot[v] = 0.0;
    if (id < a.nitems) {
        const unsigned ntile = (unsigned)(a.ntx * a.nty);
        const int seg = (int)(id / ntile);
        const unsigned t = id % ntile;
        const int tix = (int)(t / (unsigned)a.nty), tiy = (int)(t % (unsigned)a.nty);
        const int z0 = seg * a.seglen, z1 = min(a.nz, z0 + a.seglen);
        const int tx0 = tix * MF_TX, ty0 = tiy * MF_TY;
        const int gi = tx0 + lx, gj = ty0 + ly;
        const bool on_grid = gi < a.nx && gj < a.ny;
        const bool inner_ij = FACES ? gi >= box.lo[0] && gi <= box.hi[0] && gj >= box.lo[1] && gj <= box.hi[1]
                                    : gi >= 1 && gi <= a.nx - 2 && gj >= 1 && gj <= a.ny - 2;
        const int64_t row_ij = (int64_t)gj * a.nx + gi;

        // the elements of the images this thread loads: e = tid and tid + MF_NT; -1: outside the grid (x: 0, kappa: KPAD)
        int64_t xo[2], ko[2];
        int xe[2], ke[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = tid + q * MF_NT;
            xe[q] = e < MF_XS ? e : -1;
            ke[q] = e < MF_KS ? e : -1;
            const int xi = tx0 - 1 + e % MF_XW, xj = ty0 - 1 + e / MF_XW;
            xo[q] = (e < MF_XS && xi >= 0 && xi < a.nx && xj >= 0 && xj < a.ny) ? (int64_t)xj * a.nx + xi : -1;
            const int ci = tx0 - 1 + e % MF_KW, cj = ty0 - 1 + e / MF_KW;
            ko[q] = (e < MF_KS && ci >= 0 && ci < a.N && cj >= 0 && cj < a.N) ? (int64_t)cj * a.N + ci : -1;
        }
        const int64_t KP = (int64_t)a.N * a.N;
        auto load_x = [&](int plane, double (&w)[NV][2]) {
            const bool ok = plane >= 0 && plane < a.nz;
#pragma unroll
            for (int v = 0; v < NV; ++v)
#pragma unroll
                for (int q = 0; q < 2; ++q) w[v][q] = ok && xo[q] >= 0 ? ba.x[v][(int64_t)plane * a.P + xo[q]] : 0.0;
        };
        auto load_k = [&](int cplane, double (&w)[2]) {
            const bool ok = cplane >= 0 && cplane < a.N;
#pragma unroll
            for (int q = 0; q < 2; ++q) w[q] = ok && ko[q] >= 0 ? a.kappa[(int64_t)cplane * KP + ko[q]] : KPAD;
        };
        auto park_x = [&](int plane, const double (&w)[NV][2]) {
            const int slot = (plane + 4) & 3;
#pragma unroll
            for (int v = 0; v < NV; ++v)
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    if (xe[q] >= 0) sX[v][slot][xe[q]] = w[v][q];
        };
        auto park_k = [&](int cplane, const double (&w)[2]) {
            double* const s = sK[(cplane + 3) % 3];
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if (ke[q] >= 0) s[ke[q]] = w[q];
        };
        constexpr bool WANT_F = MODE != MODE_SPMV;
        auto load_f = [&](int plane, double (&fv)[NV]) {
            const bool ok = on_grid && plane < a.nz;
            const int64_t r = (int64_t)plane * a.P + row_ij;
#pragma unroll
            for (int v = 0; v < NV; ++v) fv[v] = WANT_F && ok ? __builtin_nontemporal_load(ba.f[v] + r) : 0.0;
        };
        auto load_r = [&](int plane) { return on_grid && plane < a.nz ? ba.r[(int64_t)plane * a.P + row_ij] : 0.0; };

        // ---- warm-up: what step z0 finds in place ----
        double xr[NV][2], kr[2], f1[NV], f2[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) f2[v] = 0.0;
        double r1 = 0.0, r2 = 0.0;
        load_x(z0 - 1, xr); park_x(z0 - 1, xr);
        load_x(z0, xr); park_x(z0, xr);
        load_x(z0 + 1, xr); park_x(z0 + 1, xr);
        load_k(z0 - 1, kr); park_k(z0 - 1, kr);
        load_k(z0, kr); park_k(z0, kr);
        load_x(z0 + 2, xr);
        load_k(z0 + 1, kr);
        load_f(z0, f1);
        if constexpr (REACT) r1 = load_r(z0);
        __syncthreads();

        const int cx = (ly + 1) * MF_XW + lx + 1;       // this node in an x image
        const int ck = ly * MF_KW + lx;                 // cell (gi - 1, gj - 1) in a kappa image
        const double hh = a.h;

        for (int k = z0; k < z1; ++k) {
            park_x(k + 2, xr);
            park_k(k + 1, kr);
            load_x(k + 3, xr);
            load_k(k + 2, kr);
            if (k + 1 < z1) load_f(k + 1, f2);
            if constexpr (REACT)
                if (k + 1 < z1) r2 = load_r(k + 1);

            const int sa = (k + 3) & 3, sb = k & 3, sc = (k + 1) & 3;      // planes k-1, k, k+1
            const bool free_row = inner_ij && (FACES ? k >= box.lo[2] && k <= box.hi[2] : k >= 1 && k <= a.nz - 2);
            // the row, once: its entries in registers
            double diag = 1.0, azl = 0.0, ayl = 0.0, axl = 0.0, axu = 0.0, ayu = 0.0, azu = 0.0, ad = 1.0;
            if (free_row) {
                const double* const k0 = sK[(k + 2) % 3];   // cell plane k-1
                const double* const k1 = sK[k % 3];
                double K[2][2][2];
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        K[0][dy][dx] = k0[ck + dy * MF_KW + dx];
                        K[1][dy][dx] = k1[ck + dy * MF_KW + dx];
                    }
                double se[3][2];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    double t = 2.0 * K[0][0][s];
                    t = t + K[0][1][s]; t = t + K[1][0][s]; t = t + 2.0 * K[1][1][s];
                    se[0][s] = t;
                    t = 2.0 * K[0][s][0];
                    t = t + K[0][s][1]; t = t + K[1][s][0]; t = t + 2.0 * K[1][s][1];
                    se[1][s] = t;
                    t = 2.0 * K[s][0][0];
                    t = t + K[s][0][1]; t = t + K[s][1][0]; t = t + 2.0 * K[s][1][1];
                    se[2][s] = t;
                }
                double t = se[2][0];
                t = t + se[1][0]; t = t + se[0][0]; t = t + se[0][1]; t = t + se[1][1]; t = t + se[2][1];
                diag = mf_div6(t) * hh;
                if constexpr (REACT) diag = diag + r1;
                ad = diag;
                if constexpr (FACES) {
                    azl = k - 1 < box.lo[2] ? 0.0 : -(mf_div6(se[2][0]) * hh);
                    ayl = gj - 1 < box.lo[1] ? 0.0 : -(mf_div6(se[1][0]) * hh);
                    axl = gi - 1 < box.lo[0] ? 0.0 : -(mf_div6(se[0][0]) * hh);
                    axu = gi + 1 > box.hi[0] ? 0.0 : -(mf_div6(se[0][1]) * hh);
                    ayu = gj + 1 > box.hi[1] ? 0.0 : -(mf_div6(se[1][1]) * hh);
                    azu = k + 1 > box.hi[2] ? 0.0 : -(mf_div6(se[2][1]) * hh);
                } else {
                    azl = k - 1 == 0 ? 0.0 : -(mf_div6(se[2][0]) * hh);
                    ayl = gj - 1 == 0 ? 0.0 : -(mf_div6(se[1][0]) * hh);
                    axl = gi - 1 == 0 ? 0.0 : -(mf_div6(se[0][0]) * hh);
                    axu = gi + 1 == a.nx - 1 ? 0.0 : -(mf_div6(se[0][1]) * hh);
                    ayu = gj + 1 == a.ny - 1 ? 0.0 : -(mf_div6(se[1][1]) * hh);
                    azu = k + 1 == a.nz - 1 ? 0.0 : -(mf_div6(se[2][1]) * hh);
                }
            }
            const double d = diag != 0.0 ? diag : 1.0;
            const int64_t row = (int64_t)k * a.P + row_ij;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const double x0 = sX[v][sb][cx];
                double acc = 0.0;
                if (free_row) {
                    acc = fma(azl, sX[v][sa][cx], acc);
                    acc = fma(ayl, sX[v][sb][cx - MF_XW], acc);
                    acc = fma(axl, sX[v][sb][cx - 1], acc);
                    acc = fma(ad, x0, acc);
                    acc = fma(axu, sX[v][sb][cx + 1], acc);
                    acc = fma(ayu, sX[v][sb][cx + MF_XW], acc);
                    acc = fma(azu, sX[v][sc][cx], acc);
                } else {
                    // identity row: the stored zeros times finite neighbours leave +0, then 1 * x
                    acc = fma(1.0, x0, acc);
                }
                if (on_grid) {
                    double o;
                    if (MODE == MODE_SPMV) {
                        o = acc;
                        if (DOT) dot[v] += x0 * acc;
                    } else if (MODE == MODE_RESIDUAL) {
                        o = f1[v] - acc;
                    } else {
                        o = x0 + (a.omega * (1.0 / d)) * (f1[v] - acc);
                    }
                    ba.out[v][row] = o;
                }
                f1[v] = f2[v];
            }
            if constexpr (REACT) r1 = r2;
            __syncthreads();
        }
    }
    if (DOT) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const double w = wave_sum(dot[v]);
            if (lx == 0) s_part[v][ly] = w;
        }
        __syncthreads();
#pragma unroll
        for (int v = 0; v < NV; ++v)        // (thread v: the pointers are kernel arguments, indexed by constants only)
            if (tid == v) {
                double t = 0.0;
#pragma unroll
                for (int w = 0; w < MF_NT / WAVE; ++w) t += s_part[v][w];
                ba.partials[v][blockIdx.x] = t;
            }
    }
}

}  // namespace mgk
