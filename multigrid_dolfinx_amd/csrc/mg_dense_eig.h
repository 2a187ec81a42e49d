// Symmetric-definite generalised eigenproblem of small order on the host (plain C++17, no HIP): G_K c = theta G_M c, n <= 24.
// The Rayleigh-Ritz step of mg_eigs; a header of its own so that a stand-alone program can test it (tests/host/).
//
//   1. Cholesky G_M = L L^T.  A pivot <= n eps max_i G_M[i][i] is REPORTED (return false) instead of divided by: the
//      basis is dependent to working precision and the caller drops part of it.
//   2. A = L^-1 G_K L^-T, symmetrised as (A + A^T) / 2.
//   3. Cyclic Jacobi: sweeps over (p, q), p < q, in row order, each rotation the symmetric Schur decomposition of the
//      2 x 2 block (Golub & Van Loan, Algorithm 8.4.1), until a sweep meets no entry with |a_pq| > eps sqrt(|a_pp a_qq|)
//      or DENSE_EIG_MAX_SWEEPS sweeps are done (more than 12 sweeps are not seen on n <= 24: the convergence is quadratic).
//   4. theta ascending (a stable insertion sort: equal values keep their order), C = L^-T V, so that C^T G_M C = I.
// No random numbers, no threads, no dependence on anything but the input: the same input gives the same bytes.
#pragma once

#include <cmath>
#include <limits>
#include <utility>

constexpr int DENSE_EIG_MAX_N = 24;
constexpr int DENSE_EIG_MAX_SWEEPS = 30;

// gk, gm: n x n row-major, symmetric (the lower triangle is read through the upper: only entries [i][j], i <= j, are used).
// theta[n] ascending, c[n x n] row-major with the vectors in its COLUMNS.  sweeps (may be null): Jacobi sweeps done.
// false: n out of range, or the Cholesky factorisation of G_M met a pivot that is not positive to working precision
// (*bad_pivot, may be null: its index); theta and c are then unspecified.
inline bool dense_sym_def_eig(int n, const double* gk, const double* gm, double* theta, double* c, int* sweeps = nullptr,
                              int* bad_pivot = nullptr) {
    constexpr int NMAX = DENSE_EIG_MAX_N;
    if (sweeps) *sweeps = 0;
    if (bad_pivot) *bad_pivot = -1;
    if (n < 1 || n > NMAX) return false;
    const double eps = std::numeric_limits<double>::epsilon();
    auto sym = [n](const double* g, int i, int j) { return i <= j ? g[i * n + j] : g[j * n + i]; };

    // 1. Cholesky, lower factor in l
    double l[NMAX][NMAX] = {};
    double dmax = 0.0;
    for (int i = 0; i < n; ++i) dmax = std::fmax(dmax, gm[i * n + i]);
    if (!(dmax > 0.0) || !std::isfinite(dmax)) {
        if (bad_pivot) *bad_pivot = 0;
        return false;
    }
    const double floor_ = (double)n * eps * dmax;
    for (int j = 0; j < n; ++j) {
        double d = sym(gm, j, j);
        for (int k = 0; k < j; ++k) d -= l[j][k] * l[j][k];
        if (!(d > floor_)) {
            if (bad_pivot) *bad_pivot = j;
            return false;
        }
        l[j][j] = std::sqrt(d);
        for (int i = j + 1; i < n; ++i) {
            double s = sym(gm, i, j);
            for (int k = 0; k < j; ++k) s -= l[i][k] * l[j][k];
            l[i][j] = s / l[j][j];
        }
    }

    // 2. A = L^-1 G_K L^-T: B = L^-1 G_K by forward substitution on columns, then A^T = L^-1 B^T
    double a[NMAX][NMAX], b[NMAX][NMAX];
    for (int col = 0; col < n; ++col)
        for (int i = 0; i < n; ++i) {
            double s = sym(gk, i, col);
            for (int k = 0; k < i; ++k) s -= l[i][k] * b[k][col];
            b[i][col] = s / l[i][i];
        }
    for (int row = 0; row < n; ++row)
        for (int i = 0; i < n; ++i) {
            double s = b[row][i];
            for (int k = 0; k < i; ++k) s -= l[i][k] * a[row][k];
            a[row][i] = s / l[i][i];
        }
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const double m = 0.5 * (a[i][j] + a[j][i]);
            if (!std::isfinite(m)) return false;
            a[i][j] = a[j][i] = m;
        }

    // 3. cyclic Jacobi, V accumulates the rotations
    double v[NMAX][NMAX] = {};
    for (int i = 0; i < n; ++i) v[i][i] = 1.0;
    int sweep = 0;
    for (; sweep < DENSE_EIG_MAX_SWEEPS; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                if (std::fabs(apq) <= eps * std::sqrt(std::fabs(a[p][p] * a[q][q]))) {      // negligible: dropped, no rotation
                    a[p][q] = a[q][p] = 0.0;
                    continue;
                }
                rotated = true;
                const double tau = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = t * cs;
                for (int k = 0; k < n; ++k) {       // columns p, q of A
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = cs * akp - sn * akq;
                    a[k][q] = sn * akp + cs * akq;
                }
                for (int k = 0; k < n; ++k) {       // rows p, q of A
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = cs * apk - sn * aqk;
                    a[q][k] = sn * apk + cs * aqk;
                }
                a[p][q] = a[q][p] = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = cs * vkp - sn * vkq;
                    v[k][q] = sn * vkp + cs * vkq;
                }
            }
        if (!rotated) break;
    }
    if (sweeps) *sweeps = sweep;

    // 4. ascending theta, C = L^-T V
    int order[NMAX];
    for (int i = 0; i < n; ++i) order[i] = i;
    for (int i = 1; i < n; ++i)
        for (int j = i; j > 0 && a[order[j]][order[j]] < a[order[j - 1]][order[j - 1]]; --j) std::swap(order[j], order[j - 1]);
    for (int e = 0; e < n; ++e) {
        const int src = order[e];
        theta[e] = a[src][src];
        for (int i = n - 1; i >= 0; --i) {
            double s = v[i][src];
            for (int k = i + 1; k < n; ++k) s -= l[k][i] * c[k * n + e];
            c[i * n + e] = s / l[i][i];
        }
    }
    return true;
}
