// Matrix-free variable-coefficient diffusion levels for gfx950: the row of -div(kappa grad u) is rebuilt from kappa where
// it is needed instead of being streamed from memory.
//
// A generated 3-D diffusion level (gen_diffusion, mg_kernels.hip.h) is a function of one kappa per cell: 8 B per row
// instead of the 32 B per row of the symmetric diagonals.  One kernel, templated on the mode, marches a tile of
// MF_TX x MF_TY nodes through the planes of a z segment, one step per launch:
//     x of planes k-1, k, k+1 (tile + one ring) and kappa of cell planes k-1, k (tile + one ring of cells) live in LDS;
//     plane k+2 of x and cell plane k+1 of kappa are written to LDS at the start of step k, from registers whose loads
//     were issued a step earlier, and the loads of the step after are issued before the arithmetic of plane k starts;
//     the images rotate through 4 (x) and 3 (kappa) slots, so one barrier per step is enough.
// Per row and sweep: 8 (x) + 8 (f) + 8 (kappa) + 8 (out) = 32 B plus the tile rims, 24 B for the SpMV, 40 B for a
// Chebyshev step -- against 56 / 48 / 64 B of sdia_apply.
//
// The row is DEFINED by the stored level and the results carry its bits:
//   * edge sums and the diagonal sum in gen_diffusion's order (2 k00 + k10 + k01 + 2 k11 over the four cells of an edge in
//     ascending index; the diagonal: z-, y-, x-, x+, y+, z+), weights (s / 6.0) * h, diagonal (t / 6.0) * h;
//   * boundary rows are identity rows, an interior row has no column on the boundary (prune_zeros = 1);
//   * A x as sdia_body sums it: acc = 0, then fma(a, x, acc) over z-, y-, x-, the diagonal, x+, y+, z+ (an absent column
//     is a stored zero there: fma(0, x, acc)), and the output expressions of tile_epilogue, term for term
//     (x + (omega * (1.0 / d)) * (f - acc), cheb_term).  Built with -ffp-contract=off like everything else.
// x outside the grid is taken as 0 (the stored kernel reads a finite neighbour or zero slack there, times a stored zero):
// identical for finite iterates.
//
// t / 6.0 costs a full IEEE division (v_div_scale, v_rcp, four fma, v_div_fmas, v_div_fixup) seven times per row.
// mf_div6 computes the same bits in three operations, q = t * c, r = fma(-q, 6, t), q' = fma(r, c, q) with c = RN(1/6):
// q is faithful, r is exact, and t / 6 is never within 1/6 ulp of a rounding boundary without being on it, so the
// correction lands on RN(t / 6) (Markstein; Brisebarre, Muller, Raina 2004).  Outside [2^-900, 2^900] (r could underflow,
// q * 6 could overflow) it falls back to the division.  tests/test_diffusion_mf.py checks it against / 6.0 on the host.
// Round-to-nearest is symmetric in the sign, so the range test is on |t| and a negative t takes the same three operations
// (tests/test_diffusion_tangent.py: negated arguments, +-0 and subnormals); kappa > 0 never gets there, a direction does.
//
// TANGENT (MODE_SPMV only) is the derivative of that product in a direction of kappa, out = (dA/dkappa . dkappa) x
// (mg_diffusion_apply_dkappa): A is linear in kappa, so an interior row is the same row with kappa := dkappa, of any sign,
// and a boundary row -- the identity block does not depend on kappa -- is +0.0.  Everything else is the SpMV.
//
// ROWS_ALL / COLS_ALL (TANGENT only; mg_diffusion_apply_dkappa_ex) lift the two masks of that product one by one:
// out = M_rows A^(dkappa) M_cols x with A^ the natural P1 matrix of the cell field on all nodes, no boundary condition.
//   * ROWS_ALL: a boundary row is the row of A^ -- the same edge sums, diagonal sum, weights and fma chain, a cell outside
//     the grid counting as +0.0 (the kappa image is padded with 0.0 instead of 1.0; interior rows never read the pad) and a
//     neighbour outside the grid reading 0.  Without it a boundary row is +0.0 as above.
//   * COLS_ALL keeps the entries towards boundary neighbours.  Without it every entry whose column is a boundary node is
//     a zero in the chain: the six neighbours' and, on a boundary row, the row's own diagonal.
// <false, false> is the kernel above, expression for expression.
//
// FACES (diffusion_mf_faces; levels generated with a face set, mg_set_diffusion_faces) is the same march with the box of the
// free nodes in place of "1 <= index <= n - 2", in every mode and with every mask.  A free row on a no-flux face is rebuilt
// from kappa like an interior row: the kappa image is padded with 0.0, x outside the grid reads 0, and the entry towards a
// Dirichlet neighbour (or past the grid) is a zero in the fma chain -- the bits of the stored level's one-step kernel, whose
// row has the same sums.  Dirichlet rows are identity rows (TANGENT: +0.0).  ROWS_ALL / COLS_ALL: "boundary" reads
// "Dirichlet".  The bounds come from the host, six integers compared per axis: no bit of the set is tested in the loop.
// The instantiations without FACES are the kernels above, untouched: handles with the default set launch those.
//
// REACT (diffusion_mf_react; levels generated with a reaction term, mg_set_diffusion_reaction) is the operator A(kappa) +
// R(sigma) with R diagonal: every non-TANGENT mode, with and without the box of a face set.  The level keeps the nodal
// R(sigma) of reaction_diag (mg_kernels.hip.h) as one more row vector and not sigma itself.  The march loads r of a row where
// it loads f, one step ahead, with a plain load (every sweep reads it again), and a free row takes diag + r -- the stored
// level's diagonal, gen_diffusion's one more addition -- at the diagonal's place in the fma chain and as the d of the Jacobi
// and Chebyshev epilogues.  Identity rows do not read it.  No LDS image and no barrier is added.
// Per row and sweep: 8 (x) + 8 (f) + 8 (kappa) + 8 (r) + 8 (out) = 40 B instead of 32, 32 B instead of 24 for the SpMV, 48 B
// instead of 40 for a Chebyshev step.
// <..., REACT = false> are the kernels above, untouched: a level without a reaction term launches those.
//
// Robin fields (mg_set_diffusion_robin) need no kernel of their own: a level generated with them keeps the nodal
// B(alpha), or R(sigma) + B(alpha), of robin_diag (mg_kernels.hip.h) as that row vector and runs the REACT kernels as they
// are.  A variant that formed B of the rows on a field face from the face fields instead of streaming the vector (32 B per
// row) was measured slower than these and is not kept ("Robin faces").
#pragma once
#include "mg_kernels.hip.h"

namespace mgk {

constexpr int MF_TX = 64, MF_TY = 8, MF_NT = MF_TX * MF_TY;      // one wave per tile line
constexpr int MF_XW = MF_TX + 2, MF_XS = MF_XW * (MF_TY + 2);    // x image: tile + ring
constexpr int MF_KW = MF_TX + 1, MF_KS = MF_KW * (MF_TY + 1);    // kappa image: the cells around the tile's nodes

struct MfArgs {
    const double* x;        // row-based (x[row]); whole levels only
    const double* f;        // row-based
    const double* xp;       // MODE_CHEB: x_{k-1}, the same buffer as out
    double* out;            // row-based, != x
    const double* kappa;    // [N][N][N] cells, x fastest (TANGENT: the direction dkappa)
    double* partials;       // DOT: one partial sum of x . (A x) per block
    int nx, ny, nz, N;      // nodes per axis (N + 1 each), cells per axis
    int64_t P;              // nx * ny
    int ntx, nty, nseg, seglen;
    unsigned nitems, ch;    // tiles x segments; consecutive items per XCD at a time
    double h, omega, beta;
};

__device__ __forceinline__ double mf_div6(double t) {
    const double m = fabs(t);
    if (!(m >= 0x1p-900 && m <= 0x1p900)) return t / 6.0;
    const double c = 0x1.5555555555555p-3;      // RN(1 / 6)
    const double q = t * c;
    const double r = fma(-q, 6.0, t);
    return fma(r, c, q);
}

struct MfFaceArgs {
    MfArgs a;
    FreeBox box;            // the free nodes of the level's face set
};

struct MfReactArgs {
    MfArgs a;
    FreeBox box;            // the free nodes of the level's face set (the default set: the interior nodes)
    const double* r;        // nodal R(sigma), row-based
};

template <int MODE, bool DOT, bool TANGENT, bool ROWS_ALL, bool COLS_ALL, bool FACES, bool REACT = false>
__device__ __forceinline__ void mf_march(const MfArgs& a, const FreeBox& box, const double* react = nullptr) {
    static_assert(!REACT || !TANGENT, "the reaction term does not depend on kappa");
    static_assert(!TANGENT || (MODE == MODE_SPMV && !DOT), "the tangent is a plain SpMV with kappa := dkappa");
    static_assert(TANGENT || (!ROWS_ALL && !COLS_ALL), "only the tangent has rows and columns on the boundary");
    constexpr double KPAD = ROWS_ALL || FACES ? 0.0 : 1.0;      // a cell outside the grid
    __shared__ double sX[4][MF_XS];
    __shared__ double sK[3][MF_KS];
    __shared__ double s_part[MF_NT / WAVE];
    const int tid = threadIdx.x;
    const int lx = tid & 63, ly = tid >> 6;

    unsigned id;
    {
        const unsigned b = blockIdx.x, xcd = b & 7u, j = b >> 3, ch = a.ch;
        id = ((j / ch) * 8u + xcd) * ch + (j % ch);
    }
    double dot = 0.0;
    if (id < a.nitems) {
        const unsigned ntile = (unsigned)(a.ntx * a.nty);
        const int seg = (int)(id / ntile);
        const unsigned t = id % ntile;
        const int tix = (int)(t / (unsigned)a.nty), tiy = (int)(t % (unsigned)a.nty);      // y neighbours next to each other
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
        auto load_x = [&](int plane, double (&v)[2]) {
            const bool ok = plane >= 0 && plane < a.nz;
#pragma unroll
            for (int q = 0; q < 2; ++q) v[q] = ok && xo[q] >= 0 ? a.x[(int64_t)plane * a.P + xo[q]] : 0.0;
        };
        auto load_k = [&](int cplane, double (&v)[2]) {
            const bool ok = cplane >= 0 && cplane < a.N;
#pragma unroll
            for (int q = 0; q < 2; ++q) v[q] = ok && ko[q] >= 0 ? a.kappa[(int64_t)cplane * KP + ko[q]] : KPAD;
        };
        auto park_x = [&](int plane, const double (&v)[2]) {
            double* const s = sX[(plane + 4) & 3];
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if (xe[q] >= 0) s[xe[q]] = v[q];
        };
        auto park_k = [&](int cplane, const double (&v)[2]) {
            double* const s = sK[(cplane + 3) % 3];
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if (ke[q] >= 0) s[ke[q]] = v[q];
        };
        constexpr bool WANT_F = MODE != MODE_SPMV;
        const bool want_xp = MODE == MODE_CHEB && a.beta != 0.0;
        auto load_f = [&](int plane, double& fv, double& pv) {
            const bool ok = on_grid && plane < a.nz;
            const int64_t r = (int64_t)plane * a.P + row_ij;
            fv = WANT_F && ok ? __builtin_nontemporal_load(a.f + r) : 0.0;
            pv = want_xp && ok ? a.xp[r] : 0.0;
        };
        auto load_r = [&](int plane) { return on_grid && plane < a.nz ? react[(int64_t)plane * a.P + row_ij] : 0.0; };

        // ---- warm-up: what step z0 finds in place ----
        double xr[2], kr[2], f1, p1, f2 = 0.0, p2 = 0.0;
        double r1 = 0.0, r2 = 0.0;      // REACT: R(sigma) of this row in planes k and k + 1
        load_x(z0 - 1, xr); park_x(z0 - 1, xr);
        load_x(z0, xr); park_x(z0, xr);
        load_x(z0 + 1, xr); park_x(z0 + 1, xr);
        load_k(z0 - 1, kr); park_k(z0 - 1, kr);
        load_k(z0, kr); park_k(z0, kr);
        load_x(z0 + 2, xr);
        load_k(z0 + 1, kr);
        load_f(z0, f1, p1);
        if constexpr (REACT) r1 = load_r(z0);
        __syncthreads();

        const int cx = (ly + 1) * MF_XW + lx + 1;       // this node in an x image
        const int ck = ly * MF_KW + lx;                 // cell (gi - 1, gj - 1) in a kappa image
        const double hh = a.h;

        for (int k = z0; k < z1; ++k) {
            // plane k+2 of x and cell plane k+1 into the slots that step k-1 read last; then the loads of the step after
            park_x(k + 2, xr);
            park_k(k + 1, kr);
            load_x(k + 3, xr);
            load_k(k + 2, kr);
            if (k + 1 < z1) load_f(k + 1, f2, p2);     // (plane z1 is another workgroup's: it may be writing xp = out there)
            if constexpr (REACT)
                if (k + 1 < z1) r2 = load_r(k + 1);

            const double* const xa = sX[(k + 3) & 3];   // plane k-1
            const double* const xb = sX[k & 3];
            const double* const xc = sX[(k + 1) & 3];
            const double x0 = xb[cx];
            double acc = 0.0, diag = 1.0;
            if (ROWS_ALL ? on_grid : inner_ij && (FACES ? k >= box.lo[2] && k <= box.hi[2] : k >= 1 && k <= a.nz - 2)) {
                const double* const k0 = sK[(k + 2) % 3];   // cell plane k-1
                const double* const k1 = sK[k % 3];
                double K[2][2][2];      // K[dz][dy][dx]: cell (gi - 1 + dx, gj - 1 + dy, k - 1 + dz)
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
                double azl, ayl, axl, axu, ayu, azu, ad = diag;
                if constexpr (FACES) {
                    // as below with the box: a neighbour is a Dirichlet node if it has stepped out of the free range of its
                    // axis (past the grid included) or if the row itself is outside that of another axis
                    const bool bi = ROWS_ALL && !(gi >= box.lo[0] && gi <= box.hi[0]), bj = ROWS_ALL && !(gj >= box.lo[1] && gj <= box.hi[1]);
                    const bool bz = ROWS_ALL && !(k >= box.lo[2] && k <= box.hi[2]);
                    const bool mask = !COLS_ALL;
                    azl = mask && (bi || bj || k - 1 < box.lo[2]) ? 0.0 : -(mf_div6(se[2][0]) * hh);
                    ayl = mask && (bi || bz || gj - 1 < box.lo[1]) ? 0.0 : -(mf_div6(se[1][0]) * hh);
                    axl = mask && (bj || bz || gi - 1 < box.lo[0]) ? 0.0 : -(mf_div6(se[0][0]) * hh);
                    axu = mask && (bj || bz || gi + 1 > box.hi[0]) ? 0.0 : -(mf_div6(se[0][1]) * hh);
                    ayu = mask && (bi || bz || gj + 1 > box.hi[1]) ? 0.0 : -(mf_div6(se[1][1]) * hh);
                    azu = mask && (bi || bj || k + 1 > box.hi[2]) ? 0.0 : -(mf_div6(se[2][1]) * hh);
                    if (mask && (bi || bj || bz)) ad = 0.0;
                } else if constexpr (!ROWS_ALL && !COLS_ALL) {
                    // the stored entries -w, zero where the neighbour lies on the boundary
                    azl = k - 1 == 0 ? 0.0 : -(mf_div6(se[2][0]) * hh);
                    ayl = gj - 1 == 0 ? 0.0 : -(mf_div6(se[1][0]) * hh);
                    axl = gi - 1 == 0 ? 0.0 : -(mf_div6(se[0][0]) * hh);
                    axu = gi + 1 == a.nx - 1 ? 0.0 : -(mf_div6(se[0][1]) * hh);
                    ayu = gj + 1 == a.ny - 1 ? 0.0 : -(mf_div6(se[1][1]) * hh);
                    azu = k + 1 == a.nz - 1 ? 0.0 : -(mf_div6(se[2][1]) * hh);
                } else {
                    // the entries of A^: -w, where columns are masked zero towards a boundary node -- a neighbour is one if it
                    // has stepped onto (or past) a face or if the row itself lies on a face of another axis
                    const bool bi = ROWS_ALL && (gi < 1 || gi > a.nx - 2), bj = ROWS_ALL && (gj < 1 || gj > a.ny - 2);
                    const bool bz = ROWS_ALL && (k < 1 || k > a.nz - 2);
                    const bool mask = !COLS_ALL;
                    azl = mask && (bi || bj || k - 1 <= 0) ? 0.0 : -(mf_div6(se[2][0]) * hh);
                    ayl = mask && (bi || bz || gj - 1 <= 0) ? 0.0 : -(mf_div6(se[1][0]) * hh);
                    axl = mask && (bj || bz || gi - 1 <= 0) ? 0.0 : -(mf_div6(se[0][0]) * hh);
                    axu = mask && (bj || bz || gi + 1 >= a.nx - 1) ? 0.0 : -(mf_div6(se[0][1]) * hh);
                    ayu = mask && (bi || bz || gj + 1 >= a.ny - 1) ? 0.0 : -(mf_div6(se[1][1]) * hh);
                    azu = mask && (bi || bj || k + 1 >= a.nz - 1) ? 0.0 : -(mf_div6(se[2][1]) * hh);
                    if (mask && (bi || bj || bz)) ad = 0.0;
                }
                acc = fma(azl, xa[cx], acc);
                acc = fma(ayl, xb[cx - MF_XW], acc);
                acc = fma(axl, xb[cx - 1], acc);
                acc = fma(ad, x0, acc);
                acc = fma(axu, xb[cx + 1], acc);
                acc = fma(ayu, xb[cx + MF_XW], acc);
                acc = fma(azu, xc[cx], acc);
            } else if (!TANGENT) {
                // identity row: the stored zeros times finite neighbours leave +0, then 1 * x
                acc = fma(1.0, x0, acc);
            }                                               // (TANGENT: that block does not depend on kappa, +0.0)
            if (on_grid) {
                double o;
                if (MODE == MODE_SPMV) {
                    o = acc;
                    if (DOT) dot += x0 * acc;
                } else if (MODE == MODE_RESIDUAL) {
                    o = f1 - acc;
                } else {
                    const double d = diag != 0.0 ? diag : 1.0;
                    o = x0 + (a.omega * (1.0 / d)) * (f1 - acc);
                    if (MODE == MODE_CHEB && want_xp) o = cheb_term(o, x0, a.beta, p1);
                }
                a.out[(int64_t)k * a.P + row_ij] = o;
            }
            f1 = f2; p1 = p2;
            if constexpr (REACT) r1 = r2;
            __syncthreads();
        }
    }
    if (DOT) {
        dot = wave_sum(dot);
        if (lx == 0) s_part[ly] = dot;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < MF_NT / WAVE; ++w) t += s_part[w];
            a.partials[blockIdx.x] = t;
        }
    }
}

template <int MODE, bool DOT, bool TANGENT = false, bool ROWS_ALL = false, bool COLS_ALL = false>
__global__ __launch_bounds__(MF_NT) void diffusion_mf(MfArgs a) {
    mf_march<MODE, DOT, TANGENT, ROWS_ALL, COLS_ALL, false>(a, FreeBox{});
}

template <int MODE, bool DOT, bool TANGENT = false, bool ROWS_ALL = false, bool COLS_ALL = false>
__global__ __launch_bounds__(MF_NT) void diffusion_mf_faces(MfFaceArgs fa) {
    mf_march<MODE, DOT, TANGENT, ROWS_ALL, COLS_ALL, true>(fa.a, fa.box);
}

// the march with a reaction term, on the box of the level's face set (FACES) or on the interior nodes
template <int MODE, bool DOT, bool FACES>
__global__ __launch_bounds__(MF_NT) void diffusion_mf_react(MfReactArgs ra) {
    mf_march<MODE, DOT, false, false, false, FACES, true>(ra.a, ra.box, ra.r);
}

// Right-hand side (and, for the set-up paths that need it, 1 / diagonal) of the level gen_diffusion would store, without
// the matrix: the same expressions in the same order, one thread per node.  f / dinv may be null.
__global__ void gen_diffusion_rhs(DiffusionArgs d, double* f, double* dinv) {
    const GenArgs& a = d.ga;
    int i = 0, j = 0;
    if (!plane_node(a.g, &i, &j)) return;
    const int kl = blockIdx.y;
    const int k = a.g.k0 + kl;
    const int64_t lr = (int64_t)kl * a.g.plane + (int64_t)j * a.g.nx + i;
    const bool bnd = !free_node(d.box, i, j, k);        // a Dirichlet node
    double se[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    double diag = 1.0;
    if (!bnd) {
        double K[2][2][2];
        for (int dz = 0; dz < 2; ++dz)
            for (int dy = 0; dy < 2; ++dy)
                for (int dx = 0; dx < 2; ++dx) K[dz][dy][dx] = diff_kappa_in(d, i - 1 + dx, j - 1 + dy, k - 1 + dz);
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
        diag = (t / 6.0) * a.h;
        if (d.react) diag = diag + d.react[lr];
    }
    double b = bnd ? gen_g(a, i, j, k) : diff_load(d, i, j, k);
    if (!bnd) {
        // the axis offsets in the sorted order of the pattern: z-, y-, x-, x+, y+, z+
        const int off[6][3] = {{0, 0, -1}, {0, -1, 0}, {-1, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        for (int t = 0; t < 6; ++t) {
            const int ii = i + off[t][0], jj = j + off[t][1], kk = k + off[t][2];
            if (ii < 0 || ii >= a.g.nx || jj < 0 || jj >= a.g.ny || kk < 0 || kk >= a.g.nz) continue;
            if (free_node(d.box, ii, jj, kk)) continue;
            const int ax = off[t][0] != 0 ? 0 : (off[t][1] != 0 ? 1 : 2);
            const double s = se[ax][t >= 3 ? 1 : 0];
            const double w = (s / 6.0) * a.h;
            b = b - (-w) * gen_g(a, ii, jj, kk);
        }
    }
    if (f) f[lr] = b;
    if (dinv) dinv[lr] = 1.0 / diag;
}

}  // namespace mgk
