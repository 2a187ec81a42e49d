// Point sources and point observations for gfx950: the P1 interpolant of a nodal field at arbitrary points of the unit cube
// (mg_diffusion_point_sample, S), its transpose, the consistent point load int delta(x - x_m) phi_i (mg_diffusion_point_load,
// S^T), the gradient of the located simplex (mg_diffusion_point_gradient, G) and its transpose (mg_diffusion_point_gradient_t,
// G^T), on a whole 3-D grid level.  From the grid alone: no matrix, kappa or mask is read -- x is the field itself, Dirichlet
// values included, as with the cell gradient (mg_diffusion_flux.hip.h).
//
// N cells per axis, nodes lexicographic (k * n1 + j) * n1 + i with n1 = N + 1, pts M x 3 doubles, row m = (x, y, z) in [0, 1].
// Locate (pt_locate DEFINES the bits; every kernel below shares it), per axis d:
//     t = p_d * (double)N;   c_d = min((int)floor(t), N - 1);   xi_d = t - (double)c_d      (exact; p_d = 1: c_d = N - 1, xi_d = 1)
// pi = the permutation of (x, y, z) that sorts xi in descending order, stably (a tie: the lower axis first).  The point lies in
// the Kuhn simplex (0,0,0) -> +e_pi0 -> +e_pi1 -> (1,1,1) of cell c:
//     n0 = node(c), n1 = n0 + stride(pi0), n2 = n1 + stride(pi1), n3 = n2 + stride(pi2)                     (int64)
//     l0 = 1.0 - xi_pi0, l1 = xi_pi0 - xi_pi1, l2 = xi_pi1 - xi_pi2, l3 = xi_pi2
//   S(x)   -> M:      out_m = ((l0 * x[n0] + l1 * x[n1]) + l2 * x[n2]) + l3 * x[n3]
//   G(x)   -> M x 3:  component pi0 = (x[n1] - x[n0]) * Nd, pi1 = (x[n2] - x[n1]) * Nd, pi2 = (x[n3] - x[n2]) * Nd, Nd = (double)N
//   S^T(w) -> nodes:  point m contributes l_v * w_m to node n_v
//   G^T(p) -> nodes:  with P_a = p[m][pi_a], point m contributes (0.0 - P_0) * Nd, (P_0 - P_1) * Nd, (P_1 - P_2) * Nd, P_2 * Nd
//                     to n0 .. n3
// In both transposes a node starts at +0.0 and takes its contributions in ascending point index (a point touches a node at
// most once); an untouched node is +0.0.  Built with -ffp-contract=off: no product is fused into an add.
// poisson.diffusion_point_locate, _sample, _load, _gradient and _gradient_t restate all of it add for add.
//
// S, G: one thread per point, four loads through the caches.  The transposes use no floating-point atomic: out is zeroed, one
// thread per point writes its four (node, contribution) pairs at 4 m + v, a STABLE radix sort (rocPRIM, over the bits a node id
// of the level needs) orders the 4 M pairs by node -- equal nodes keep the order of 4 m + v, which is the order of m -- and one
// thread per run of equal nodes adds the run front to back and stores once.  Two calls give the same bits however many points
// share a node.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

namespace mgk {

constexpr int PT_BLOCK = 256;

struct PtArgs {
    const double* pts;      // M x 3
    const double* x;        // S, G: the nodal field; S^T: w (M); G^T: p (M x 3)
    double* out;            // S: M, G: 3 M; the contribution kernels: the 4 M values
    uint64_t* keys;         // the contribution kernels: the 4 M node ids
    int64_t M;
    int64_t nx, plane;      // strides of y and z
    int N;
};

struct PtLoc {
    int64_t n[4];           // the simplex's vertices along the Kuhn path
    double lam[4];          // their weights
    int pi[3];              // the axes in descending xi, stable
};

__device__ __forceinline__ PtLoc pt_locate(const double* __restrict__ pts, int64_t m, int N, int64_t nx, int64_t plane) {
    const double Nd = (double)N;
    double xi[3];
    int c[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double t = pts[3 * m + d] * Nd;
        const int f = (int)floor(t);
        c[d] = f < N - 1 ? f : N - 1;
        xi[d] = t - (double)c[d];
    }
    // stable insertion sort of three, descending: an axis moves ahead only of a strictly smaller xi
    int p0 = 0, p1 = 1, p2 = 2;
    if (xi[p0] < xi[p1]) { const int s = p0; p0 = p1; p1 = s; }
    if (xi[p1] < xi[p2]) {
        const int s = p1; p1 = p2; p2 = s;
        if (xi[p0] < xi[p1]) { const int s2 = p0; p0 = p1; p1 = s2; }
    }
    const double a = p0 == 0 ? xi[0] : p0 == 1 ? xi[1] : xi[2];
    const double b = p1 == 0 ? xi[0] : p1 == 1 ? xi[1] : xi[2];
    const double g = p2 == 0 ? xi[0] : p2 == 1 ? xi[1] : xi[2];
    const int64_t s0 = p0 == 0 ? 1 : p0 == 1 ? nx : plane;
    const int64_t s1 = p1 == 0 ? 1 : p1 == 1 ? nx : plane;
    const int64_t s2 = p2 == 0 ? 1 : p2 == 1 ? nx : plane;
    PtLoc q;
    q.pi[0] = p0; q.pi[1] = p1; q.pi[2] = p2;
    q.n[0] = (int64_t)c[2] * plane + (int64_t)c[1] * nx + c[0];
    q.n[1] = q.n[0] + s0;
    q.n[2] = q.n[1] + s1;
    q.n[3] = q.n[2] + s2;
    q.lam[0] = 1.0 - a;
    q.lam[1] = a - b;
    q.lam[2] = b - g;
    q.lam[3] = g;
    return q;
}

// the lowest point index with a coordinate that is not in [0, 1] (a NaN fails both comparisons): integer atomicMin, as kappa_check
__global__ void pt_check(const double* __restrict__ pts, int64_t n3, unsigned long long* first) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n3; q += (int64_t)gridDim.x * blockDim.x) {
        const double x = pts[q];
        if (!(x >= 0.0 && x <= 1.0)) atomicMin(first, (unsigned long long)(q / 3));
    }
}

// S: one thread per point
__global__ __launch_bounds__(PT_BLOCK) void pt_sample(PtArgs a) {
    const int64_t m = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (m >= a.M) return;
    const PtLoc q = pt_locate(a.pts, m, a.N, a.nx, a.plane);
    a.out[m] = ((q.lam[0] * a.x[q.n[0]] + q.lam[1] * a.x[q.n[1]]) + q.lam[2] * a.x[q.n[2]]) + q.lam[3] * a.x[q.n[3]];
}

// G: one thread per point; the three differences along the path land on the components pi0, pi1, pi2
__global__ __launch_bounds__(PT_BLOCK) void pt_gradient(PtArgs a) {
    const int64_t m = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (m >= a.M) return;
    const PtLoc q = pt_locate(a.pts, m, a.N, a.nx, a.plane);
    const double Nd = (double)a.N;
    const double u0 = a.x[q.n[0]], u1 = a.x[q.n[1]], u2 = a.x[q.n[2]], u3 = a.x[q.n[3]];
    a.out[3 * m + q.pi[0]] = (u1 - u0) * Nd;
    a.out[3 * m + q.pi[1]] = (u2 - u1) * Nd;
    a.out[3 * m + q.pi[2]] = (u3 - u2) * Nd;
}

// the (node, contribution) pairs of S^T (GRAD = false, a.x = w) or G^T (GRAD = true, a.x = p) at 4 m + v
template <bool GRAD>
__global__ __launch_bounds__(PT_BLOCK) void pt_contrib(PtArgs a) {
    const int64_t m = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (m >= a.M) return;
    const PtLoc q = pt_locate(a.pts, m, a.N, a.nx, a.plane);
    double v[4];
    if constexpr (GRAD) {
        const double Nd = (double)a.N;
        const double P0 = a.x[3 * m + q.pi[0]], P1 = a.x[3 * m + q.pi[1]], P2 = a.x[3 * m + q.pi[2]];
        v[0] = (0.0 - P0) * Nd;
        v[1] = (P0 - P1) * Nd;
        v[2] = (P1 - P2) * Nd;
        v[3] = P2 * Nd;
    } else {
        const double w = a.x[m];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = q.lam[k] * w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a.keys[4 * m + k] = (uint64_t)q.n[k];
        a.out[4 * m + k] = v[k];
    }
}

// one thread per sorted pair; the thread at the head of a run of equal nodes adds the run front to back onto +0.0 and stores it
__global__ __launch_bounds__(PT_BLOCK) void pt_run_sum(const uint64_t* __restrict__ keys, const double* __restrict__ vals, int64_t n,
                                                       double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    if (i > 0 && keys[i - 1] == key) return;
    double acc = 0.0;
    for (int64_t j = i; j < n && keys[j] == key; ++j) acc = acc + vals[j];
    out[key] = acc;
}

}  // namespace mgk

// ---- Located point sets (mg_points_*) ----------------------------------------------------------------------------------------
// A set keeps what depends on the point positions alone, so that a call with nb lanes launches only the kernels that touch the
// operands: the set's own copy of the points (the gathers locate from it with pt_locate, once per point and launch group), and,
// for the transposes, the 4 M slots 4 m + v in the stable order by node -- per sorted slot one PtSlot record -- with the runs of
// equal node: run_start[R + 1] (sorted positions) and run_node[R].  One thread per run walks its records front to back, which
// is ascending point index, reads each record once per launch group of up to PT_SET_NV lanes, adds onto +0.0 per lane and
// stores once per lane and node: the adds and their order are those of pt_contrib + pt_run_sum, so the bits are too.
namespace mgk {

constexpr int PT_SET_NV = 4;        // lanes per launch group ("Located point sets": the measured choice)

// One sorted slot.  S^T: contribution lam * w[m].  G^T: vertex v of the path takes (A - B) * Nd with A = p[3 m + a] (v = 0: 0.0)
// and B = p[3 m + b]; v = 3 takes p[3 m + a] * Nd.  code = v | a << 2 | b << 4, a = pi[v - 1], b = pi[v].
struct PtSlot {
    double lam;
    uint32_t m;
    uint32_t code;
};

// the pairs of the sort: key = node, value = slot 4 m + v
__global__ __launch_bounds__(PT_BLOCK) void pt_set_pairs(PtArgs a, uint64_t* __restrict__ slots) {
    const int64_t m = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (m >= a.M) return;
    const PtLoc q = pt_locate(a.pts, m, a.N, a.nx, a.plane);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a.keys[4 * m + k] = (uint64_t)q.n[k];
        slots[4 * m + k] = (uint64_t)(4 * m + k);
    }
}

// per sorted position: the record of its slot, and whether it heads a run of equal nodes
__global__ __launch_bounds__(PT_BLOCK) void pt_set_records(PtArgs a, const uint64_t* __restrict__ keys_s, const uint64_t* __restrict__ slots_s,
                                                           int64_t n, PtSlot* __restrict__ rec, unsigned char* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = slots_s[i];
    const int64_t m = (int64_t)(s >> 2);
    const int v = (int)(s & 3);
    const PtLoc q = pt_locate(a.pts, m, a.N, a.nx, a.plane);
    const int pa = v == 0 ? 0 : v == 1 ? q.pi[0] : v == 2 ? q.pi[1] : q.pi[2];
    const int pb = v == 0 ? q.pi[0] : v == 1 ? q.pi[1] : v == 2 ? q.pi[2] : 0;
    PtSlot r;
    r.lam = v == 0 ? q.lam[0] : v == 1 ? q.lam[1] : v == 2 ? q.lam[2] : q.lam[3];
    r.m = (uint32_t)m;
    r.code = (uint32_t)v | (uint32_t)pa << 2 | (uint32_t)pb << 4;
    rec[i] = r;
    head[i] = (i == 0 || keys_s[i - 1] != keys_s[i]) ? 1 : 0;
}

// run_start[R] = n, run_node[r] = the node of run r, and the longest run (an integer max)
__global__ __launch_bounds__(PT_BLOCK) void pt_set_runs(const uint64_t* __restrict__ keys_s, int64_t n, int64_t R, int64_t* __restrict__ run_start,
                                                        int64_t* __restrict__ run_node, unsigned long long* longest) {
    const int64_t r = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (r >= R) return;
    const int64_t s0 = run_start[r];
    const int64_t s1 = r + 1 < R ? run_start[r + 1] : n;    // (run_start[R] is written by the thread of the last run)
    if (r + 1 == R) run_start[R] = n;
    run_node[r] = (int64_t)keys_s[s0];
    atomicMax(longest, (unsigned long long)(s1 - s0));
}

template <int NV>
struct PtSetArgs {
    const double* pts;              // the set's copy, M x 3
    const PtSlot* rec;              // 4 M, sorted
    const int64_t* run_start;       // R + 1
    const int64_t* run_node;        // R
    const double* in[NV];
    double* out[NV];
    int64_t M, R;
    int64_t nx, plane;
    int N;
};

// S (GRAD false) or G (GRAD true) of NV fields: one thread per point, located once
template <bool GRAD, int NV>
__global__ __launch_bounds__(PT_BLOCK) void pt_set_gather(PtSetArgs<NV> a) {
    const int64_t m = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (m >= a.M) return;
    const PtLoc q = pt_locate(a.pts, m, a.N, a.nx, a.plane);
    const double Nd = (double)a.N;
#pragma unroll
    for (int b = 0; b < NV; ++b) {
        const double* __restrict__ x = a.in[b];
        const double u0 = x[q.n[0]], u1 = x[q.n[1]], u2 = x[q.n[2]], u3 = x[q.n[3]];
        if constexpr (GRAD) {
            a.out[b][3 * m + q.pi[0]] = (u1 - u0) * Nd;
            a.out[b][3 * m + q.pi[1]] = (u2 - u1) * Nd;
            a.out[b][3 * m + q.pi[2]] = (u3 - u2) * Nd;
        } else {
            a.out[b][m] = ((q.lam[0] * u0 + q.lam[1] * u1) + q.lam[2] * u2) + q.lam[3] * u3;
        }
    }
}

// S^T (GRAD false, in = w) or G^T (GRAD true, in = p) of NV operands onto zeroed outputs: one thread per run of equal node
template <bool GRAD, int NV>
__global__ __launch_bounds__(PT_BLOCK) void pt_set_scatter(PtSetArgs<NV> a) {
    const int64_t r = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (r >= a.R) return;
    const int64_t s0 = a.run_start[r], s1 = a.run_start[r + 1];
    const double Nd = (double)a.N;
    double acc[NV];
#pragma unroll
    for (int b = 0; b < NV; ++b) acc[b] = 0.0;
    for (int64_t j = s0; j < s1; ++j) {
        const PtSlot s = a.rec[j];
        const int64_t m = (int64_t)s.m;
        if constexpr (GRAD) {
            const int v = (int)(s.code & 3u);
            const int64_t ia = 3 * m + (int64_t)((s.code >> 2) & 3u), ib = 3 * m + (int64_t)((s.code >> 4) & 3u);
#pragma unroll
            for (int b = 0; b < NV; ++b) {
                const double A = v == 0 ? 0.0 : a.in[b][ia];
                const double c = v == 3 ? A * Nd : (A - a.in[b][ib]) * Nd;
                acc[b] = acc[b] + c;
            }
        } else {
#pragma unroll
            for (int b = 0; b < NV; ++b) {
                const double c = s.lam * a.in[b][m];
                acc[b] = acc[b] + c;
            }
        }
    }
    const int64_t node = a.run_node[r];
#pragma unroll
    for (int b = 0; b < NV; ++b) a.out[b][node] = acc[b];
}

}  // namespace mgk
