"""NumPy statement of the Chebyshev smoother (MG_SMOOTH_CHEBYSHEV) and of its Lanczos estimate of lambda_max(D^-1 A), plus a
V-cycle with the P1 embedding and its transpose that uses it (test infrastructure).

Everything is in lexicographic grid numbering (x fastest), as the library keeps its vectors.  The step scalars are computed
in the library's order (mg_capi.hip: cheb_steps), so they are the same bits; one step is the library's expression

    x_{k+1} = (x_k + (alpha_k * (1 / d)) * (f - A x_k)) + beta_k * (x_k - x_{k-1})      (first step: no beta term)

with d the stored diagonal (1 where it is zero).  The estimate is Jacobi-preconditioned CG from the library's hashed start
vector; the Lanczos matrix of its coefficients gives lambda_max.
"""
import itertools

import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from multigrid_dolfinx_amd import poisson
from tests import p1_reference as p1

_M1, _M2, _M3 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB), np.uint64(0x9E3779B97F4A7C15)


def start_vector(gidx):
    """splitmix64 of the global lexicographic node index, top 53 bits as a number in [-1, 1) (mg_kernels.hip.h, cheb_hash)."""
    with np.errstate(over="ignore"):
        z = np.asarray(gidx, dtype=np.uint64) + _M3
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 4503599627370496.0) - 1.0


def diagonal(A):
    d = np.asarray(sp.csr_matrix(A).diagonal(), dtype=np.float64).copy()
    d[d == 0.0] = 1.0
    return d


def steps(lo, hi, m):
    """(alpha, beta) of the m steps on [lo, hi], in the library's order of operations."""
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    sigma = theta / delta
    rho = 1.0 / sigma
    al, be = [1.0 / theta], [0.0]
    for _ in range(1, m):
        rn = 1.0 / (2.0 * sigma - rho)
        al.append(2.0 * rn / delta)
        be.append(rn * rho)
        rho = rn
    return al[:m], be[:m]


def smooth(A, f, x, m, lo, hi):
    """Degree-m Chebyshev smoother from x (1-D arrays)."""
    d = diagonal(A)
    al, be = steps(lo, hi, m)
    x = np.asarray(x, dtype=np.float64).copy()
    xp = None
    for a, b in zip(al, be):
        new = x + (a * (1.0 / d)) * (f - A @ x)
        if b != 0.0:
            new = new + b * (x - xp)
        xp, x = x, new
    return x


def lanczos_lmax(A, eig_steps=10, gidx=None):
    """The library's estimate of lambda_max(D^-1 A): eig_steps steps of Jacobi-preconditioned CG, then eigvalsh of T."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    dinv = 1.0 / diagonal(A)
    r = start_vector(np.arange(n) if gidx is None else gidx)
    z = dinv * r
    p = z.copy()
    rz = float(r @ z)
    al, be = [], []
    for j in range(eig_steps):
        q = A @ p
        pq = float(p @ q)
        if not pq > 0.0:
            break
        alpha = rz / pq
        al.append(alpha)
        r = r - alpha * q
        z = dinv * r
        rz_new = float(r @ z)
        if not rz_new > 0.0 or j + 1 == eig_steps:
            break
        beta = rz_new / rz
        be.append(beta)
        rz = rz_new
        p = z + beta * p
    m = len(al)
    assert m >= 2
    dg = [1.0 / al[j] + (be[j - 1] / al[j - 1] if j > 0 else 0.0) for j in range(m)]
    off = [np.sqrt(be[j]) / al[j] for j in range(m - 1)]
    return float(scipy.linalg.eigvalsh_tridiagonal(np.array(dg), np.array(off))[-1])


def exact_lmax(A):
    """lambda_max(D^-1 A) = lambda_max(D^-1/2 A D^-1/2) by ARPACK."""
    s = sp.diags(1.0 / np.sqrt(diagonal(A)))
    B = sp.csr_matrix(s @ sp.csr_matrix(A) @ s)
    return float(spla.eigsh(B, k=1, which="LA", tol=1e-12, return_eigenvectors=False)[0])


def chebyshev_bound(m, lo, hi, lam):
    """|p_m(lam)| of the Chebyshev error polynomial on [lo, hi] (1 - lam t for the first step)."""
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    t = lambda y: np.sign(y) ** m * np.cosh(m * np.arccosh(abs(y))) if abs(y) >= 1 else np.cos(m * np.arccos(y))
    return abs(t((theta - lam) / delta) / t(theta / delta))


# ---- hierarchies ------------------------------------------------------------------------------------------------------
def poisson_matrices(dim, N0, nlev):
    """Rediscretised P1 Poisson levels N0 * 2^l, lexicographic, explicit zeros dropped (prune_zeros)."""
    out = []
    for l in range(nlev):
        A = sp.csr_matrix(poisson.make_level(N0 << l, dim).A)
        A.eliminate_zeros()
        A.sort_indices()
        out.append(A)
    return out


def kuhn_diffusion(N, dim, jump=1000.0):
    """P1 stiffness matrix of -div(k grad u) on the Kuhn mesh of poisson.py (squares cut along (1, 1), cubes into six
    simplices along the main diagonal), k = jump on elements whose centroid has x < 1/2 and 1 elsewhere, with identity rows
    and zeroed columns on the boundary.  Lexicographic numbering."""
    n1 = N + 1
    h = 1.0 / N
    strides = [1, n1, n1 * n1][:dim]
    simplices = []
    for perm in itertools.permutations(range(dim)):
        path = [np.zeros(dim, dtype=int)]
        for ax in perm:
            nxt = path[-1].copy()
            nxt[ax] = 1
            path.append(nxt)
        simplices.append(np.array(path))
    rows, cols, vals = [], [], []
    cells = np.array(list(itertools.product(range(N), repeat=dim)))[:, ::-1]      # (i, j[, k]) with x = i
    base = (cells * np.array(strides)).sum(axis=1)
    for S in simplices:
        X = S * h                                                                  # vertices of the reference cell
        E = (X[1:] - X[0]).T
        G = np.linalg.inv(E).T @ np.hstack([-np.ones((dim, 1)), np.eye(dim)])     # gradients of the barycentrics
        vol = abs(np.linalg.det(E)) / (2.0 if dim == 2 else 6.0)
        K = vol * (G.T @ G)
        cx = (cells[:, 0] + S[:, 0].mean()) * h
        coef = np.where(cx < 0.5, jump, 1.0)
        nodes = base[:, None] + (S * np.array(strides)).sum(axis=1)[None, :]
        for a in range(dim + 1):
            for b in range(dim + 1):
                rows.append(nodes[:, a])
                cols.append(nodes[:, b])
                vals.append(coef * K[a, b])
    n = n1 ** dim
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    interior = p1.interior(N, dim)
    keep = sp.diags(interior.astype(float))
    A = (keep @ A @ keep + sp.diags((~interior).astype(float))).tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def galerkin_matrices(A_top, dim, N0, nlev):
    """[A_0 .. A_top] with A_{l-1} = P^T A_l P as mg_galerkin_level builds them."""
    out = [A_top]
    for l in range(nlev - 1, 0, -1):
        out.insert(0, p1.galerkin(out[0], N0 << l, dim))
    return out


class Cycle:
    """V(mu1, mu2) cycles with the P1 embedding and R = P^T (p1_reference), the direct coarsest solve and either the
    Chebyshev smoother (intervals `bounds[l]` = (lo, hi), or upper_factor * lanczos_lmax with lower_ratio) or Jacobi."""

    def __init__(self, As, dim, N0, mu1=2, mu2=2, smoother="chebyshev", omega=2.0 / 3.0, lower_ratio=6.0,
                 upper_factor=1.1, eig_steps=10, bounds=None):
        self.As, self.dim, self.N0 = As, dim, N0
        self.mu1, self.mu2, self.smoother, self.omega = mu1, mu2, smoother, omega
        self.P = [None] + [p1.prolongation(N0 << (l - 1), dim) for l in range(1, len(As))]
        self.R = [None] + [p1.restriction(N0 << (l - 1), dim) for l in range(1, len(As))]
        self.lu = spla.splu(sp.csc_matrix(As[0]))
        self.bounds = dict(bounds or {})
        if smoother == "chebyshev":
            for l in range(1, len(As)):
                if l not in self.bounds:
                    hi = upper_factor * lanczos_lmax(As[l], eig_steps)
                    self.bounds[l] = (hi / lower_ratio, hi)

    def smooth(self, l, f, v, m):
        A = self.As[l]
        if m == 0:
            return v
        if self.smoother == "chebyshev":
            return smooth(A, f, v, m, *self.bounds[l])
        d = diagonal(A)
        for _ in range(m):
            v = v + (self.omega * (1.0 / d)) * (f - A @ v)
        return v

    def vcycle(self, l, f, v):
        if l == 0:
            return self.lu.solve(f)
        v = self.smooth(l, f, v, self.mu1)
        fc = self.R[l] @ (f - self.As[l] @ v)
        vc = self.vcycle(l - 1, fc, np.zeros_like(fc))
        v = v + self.P[l] @ vc
        return self.smooth(l, f, v, self.mu2)

    def history(self, f, ncycles, l=None):
        l = len(self.As) - 1 if l is None else l
        v = np.zeros_like(f)
        out = []
        for _ in range(ncycles):
            v = self.vcycle(l, f, v)
            out.append(float(np.linalg.norm(f - self.As[l] @ v)))
        return np.array(out)

    def pcg(self, f, rtol=1e-10, max_iter=100):
        """The recurrence of mg_pcg (tests/pcg_reference.py) with this cycle as preconditioner: ||r_k|| per iteration."""
        l = len(self.As) - 1
        A = self.As[l]
        x = np.zeros_like(f)
        r = f - A @ x
        tol = rtol * float(np.linalg.norm(f))
        z = self.vcycle(l, r, np.zeros_like(r))
        p = z.copy()
        rz = float(r @ z)
        hist = []
        while True:
            q = A @ p
            alpha = rz / float(p @ q)
            x = x + alpha * p
            r = r - alpha * q
            rn = float(np.linalg.norm(r))
            hist.append(rn)
            if rn <= tol or rn == 0.0 or len(hist) >= max_iter:
                break
            z = self.vcycle(l, r, np.zeros_like(r))
            beta = -alpha * float(z @ q) / rz
            rz = float(r @ z)
            p = z + beta * p
        return np.array(hist)


def contraction(hist, first=3, last=8):
    """Geometric mean of the residual ratio over cycles first..last (1-based)."""
    return float((hist[last - 1] / hist[first - 2]) ** (1.0 / (last - first + 1)))
