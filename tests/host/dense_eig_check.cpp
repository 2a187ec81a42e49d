// Stand-alone check of csrc/mg_dense_eig.h (the Rayleigh-Ritz step of mg_eigs) under the sanitizers: no GPU, no HIP.
//
// For every solved case it prints
//     orth  = max |C^T G_M C - I|
//     resid = max |G_K C - G_M C Theta| / ||G_K||_inf
// and checks both against   n^2 eps LIMIT_C,   LIMIT_C = 8 (sweeps + 1) + 32:
//   * a Jacobi sweep makes n (n - 1) / 2 rotations, and an entry of A (or of V) is in a rotated row or column in fewer than
//     2 n of them; a rotation replaces it by c a - s b, two products and a sum, at most 2 eps (|a| + |b|) off.  So a sweep moves
//     an entry by less than 4 n eps ||A||, `sweeps` sweeps and the final check sweep by 4 n eps (sweeps + 1) ||A||, and an entry
//     of the n-term products above collects n of them: 4 n^2 eps (sweeps + 1), taken twice for the two factors (A and V);
//   * the Cholesky factor and the two triangular solves with it add c n^2 eps cond(G_M) with c of order one; the cases here
//     keep cond(G_M) below about 20, hence 32.
// The sweep count is asserted to stay at or below 12 (the convergence is quadratic; 6 to 9 are seen).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../multigrid_dolfinx_amd/csrc/mg_dense_eig.h"

namespace {

int failures = 0;
uint64_t rng_state = 0x2545F4914F6CDD1Dull;

double uniform() {      // in [-1, 1)
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) * (1.0 / 4503599627370496.0) - 1.0;
}

using Mat = std::vector<double>;

// V^T diag(t) V for V of `len` rows and n columns (t null: the identity)
Mat gram(int n, int len, const Mat& v, const double* t) {
    Mat g((size_t)(n * n), 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double s = 0.0;
            for (int r = 0; r < len; ++r) s += v[(size_t)(r * n + i)] * (t ? t[r] : 1.0) * v[(size_t)(r * n + j)];
            g[(size_t)(i * n + j)] = s;
        }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) g[(size_t)(i * n + j)] = g[(size_t)(j * n + i)];
    return g;
}

void check_solved(const char* name, int n, const Mat& gk, const Mat& gm, const double* expect) {
    Mat theta((size_t)n), c((size_t)(n * n)), theta2((size_t)n), c2((size_t)(n * n));
    int sweeps = -1, sweeps2 = -1;
    if (!dense_sym_def_eig(n, gk.data(), gm.data(), theta.data(), c.data(), &sweeps)) {
        printf("FAIL %s: reported a failed Cholesky step on a definite pair\n", name);
        ++failures;
        return;
    }
    const bool again = dense_sym_def_eig(n, gk.data(), gm.data(), theta2.data(), c2.data(), &sweeps2);
    if (!again || sweeps != sweeps2 || memcmp(theta.data(), theta2.data(), (size_t)n * sizeof(double)) != 0 ||
        memcmp(c.data(), c2.data(), (size_t)(n * n) * sizeof(double)) != 0) {
        printf("FAIL %s: the same input twice gave other bytes\n", name);
        ++failures;
    }
    double norm_k = 0.0;
    for (int i = 0; i < n; ++i) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += std::fabs(gk[(size_t)(i * n + j)]);
        norm_k = std::fmax(norm_k, s);
    }
    Mat mc((size_t)(n * n)), kc((size_t)(n * n));
    for (int i = 0; i < n; ++i)
        for (int e = 0; e < n; ++e) {
            double sm = 0.0, sk = 0.0;
            for (int j = 0; j < n; ++j) {
                sm += gm[(size_t)(i * n + j)] * c[(size_t)(j * n + e)];
                sk += gk[(size_t)(i * n + j)] * c[(size_t)(j * n + e)];
            }
            mc[(size_t)(i * n + e)] = sm;
            kc[(size_t)(i * n + e)] = sk;
        }
    double orth = 0.0, resid = 0.0, value = 0.0;
    for (int e = 0; e < n; ++e) {
        for (int f = 0; f < n; ++f) {
            double s = 0.0;
            for (int i = 0; i < n; ++i) s += c[(size_t)(i * n + e)] * mc[(size_t)(i * n + f)];
            orth = std::fmax(orth, std::fabs(s - (e == f ? 1.0 : 0.0)));
        }
        for (int i = 0; i < n; ++i) resid = std::fmax(resid, std::fabs(kc[(size_t)(i * n + e)] - mc[(size_t)(i * n + e)] * theta[(size_t)e]));
        if (e > 0 && theta[(size_t)e] < theta[(size_t)(e - 1)]) {
            printf("FAIL %s: theta is not ascending at %d\n", name, e);
            ++failures;
        }
        if (expect) value = std::fmax(value, std::fabs(theta[(size_t)e] - expect[e]));
    }
    resid /= norm_k > 0.0 ? norm_k : 1.0;
    value /= norm_k > 0.0 ? norm_k : 1.0;
    const double limit = (double)(n * n) * std::numeric_limits<double>::epsilon() * (8.0 * (sweeps + 1) + 32.0);
    printf("%-28s n %2d sweeps %2d orth %.3e resid %.3e value %.3e limit %.3e\n", name, n, sweeps, orth, resid, value, limit);
    if (!(orth <= limit) || !(resid <= limit) || !(value <= limit) || sweeps > 12) {
        printf("FAIL %s: above the limit\n", name);
        ++failures;
    }
}

// a well-conditioned definite G_M = I + 0.25 E / n (|E_ij| <= 1: eigenvalues in [0.75, 1.25]) and a symmetric G_K
void random_pair(int n, Mat& gk, Mat& gm) {
    gk.assign((size_t)(n * n), 0.0);
    gm.assign((size_t)(n * n), 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = i; j < n; ++j) {
            gk[(size_t)(i * n + j)] = gk[(size_t)(j * n + i)] = 3.0 * uniform();
            gm[(size_t)(i * n + j)] = gm[(size_t)(j * n + i)] = (i == j ? 1.0 : 0.0) + 0.25 * uniform() / n;
        }
}

}  // namespace

int main() {
    Mat gk, gm;
    for (int n : {1, 2, 3, 12, 24}) {
        char name[64];
        snprintf(name, sizeof(name), "random pair, order %d", n);
        random_pair(n, gk, gm);
        check_solved(name, n, gk, gm, nullptr);
    }
    {   // a diagonal pair: theta_i = k_i / m_i, here descending on input
        const int n = 12;
        gk.assign((size_t)(n * n), 0.0);
        gm.assign((size_t)(n * n), 0.0);
        Mat expect((size_t)n);
        for (int i = 0; i < n; ++i) {
            gm[(size_t)(i * n + i)] = 1.0 + 0.125 * i;
            gk[(size_t)(i * n + i)] = (double)(n - i) * gm[(size_t)(i * n + i)];
            expect[(size_t)(n - 1 - i)] = (double)(n - i);
        }
        check_solved("diagonal pair", n, gk, gm, expect.data());
    }
    {   // a triple eigenvalue: G_M = V^T V, G_K = V^T diag(t) V with V square and orthogonal up to a column scale
        const int n = 12;
        Mat q((size_t)(n * n), 0.0);        // a product of plane rotations: orthogonal
        for (int i = 0; i < n; ++i) q[(size_t)(i * n + i)] = 1.0;
        for (int p = 0; p < n - 1; ++p)
            for (int r = p + 1; r < n; ++r) {
                const double a = 0.3 + 0.1 * p + 0.07 * r, cs = std::cos(a), sn = std::sin(a);
                for (int k = 0; k < n; ++k) {
                    const double x = q[(size_t)(k * n + p)], y = q[(size_t)(k * n + r)];
                    q[(size_t)(k * n + p)] = cs * x - sn * y;
                    q[(size_t)(k * n + r)] = sn * x + cs * y;
                }
            }
        for (int k = 0; k < n; ++k)
            for (int j = 0; j < n; ++j) q[(size_t)(k * n + j)] *= 1.0 + 0.05 * j;     // (column scale: G_M is not the identity)
        const double t[12] = {1.0, 2.0, 2.0, 2.0, 3.5, 4.0, 5.0, 6.25, 7.0, 8.0, 9.0, 11.0};
        gm = gram(n, n, q, nullptr);
        gk = gram(n, n, q, t);
        check_solved("triple eigenvalue", n, gk, gm, t);
    }
    Mat v((size_t)(64 * 24));
    {   // a Gram pair of 24 random vectors of length 64
        for (double& x : v) x = uniform();
        double t[64];
        for (int r = 0; r < 64; ++r) t[r] = 1.0 + r;
        gm = gram(24, 64, v, nullptr);
        gk = gram(24, 64, v, t);
        check_solved("Gram pair 24 of length 64", 24, gk, gm, nullptr);
    }
    {   // ... made singular to working precision: column 5 = column 2 + column 7.  To be reported, not solved.
        double t[64];
        for (int r = 0; r < 64; ++r) {
            t[r] = 1.0 + r;
            v[(size_t)(r * 24 + 5)] = v[(size_t)(r * 24 + 2)] + v[(size_t)(r * 24 + 7)];
        }
        gm = gram(24, 64, v, nullptr);
        gk = gram(24, 64, v, t);
        Mat theta(24), c(24 * 24);
        int pivot = -1;
        const bool solved = dense_sym_def_eig(24, gk.data(), gm.data(), theta.data(), c.data(), nullptr, &pivot);
        printf("%-28s %s (pivot %d)\n", "singular Gram pair", solved ? "SOLVED" : "reported as failed", pivot);
        if (solved || pivot != 7) {
            printf("FAIL singular Gram pair: a dependent basis must be reported at the pivot that completes the dependence (7)\n");
            ++failures;
        }
        gm.assign(24 * 24, 0.0);
        if (dense_sym_def_eig(24, gk.data(), gm.data(), theta.data(), c.data()) || dense_sym_def_eig(0, gk.data(), gm.data(), theta.data(), c.data()) ||
            dense_sym_def_eig(25, gk.data(), gm.data(), theta.data(), c.data())) {
            printf("FAIL: a zero G_M or an order outside 1..24 was not refused\n");
            ++failures;
        }
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("dense eigen-solver clean\n");
    return 0;
}
