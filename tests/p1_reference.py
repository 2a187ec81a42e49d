"""NumPy / SciPy statement of the P1 natural-embedding transfers and of Galerkin coarse levels (test infrastructure).

P is built from the mesh itself -- every coarse edge (I, I + p), p in {0,1}^dim \\ {0}, puts 0.5 of each end on its midpoint
2I + p, every coarse node copies onto 2I -- and the restriction is SciPy's transpose of it, independently of the gather
formulas of `poisson.p1_*_table` and of the device kernels.  Matrices are in lexicographic grid numbering (x fastest).
"""
import itertools

import numpy as np
import scipy.sparse as sp

from multigrid_dolfinx_amd import poisson
from oracle.mg_oracle import Oracle


def _ijk(N, dim):
    n1 = N + 1
    idx = np.arange(n1 ** dim)
    return [idx % n1, (idx // n1) % n1] + ([idx // (n1 * n1)] if dim == 3 else [])


def interior(N, dim):
    m = np.ones((N + 1) ** dim, dtype=bool)
    for c in _ijk(N, dim):
        m &= (c > 0) & (c < N)
    return m


def prolongation(Nc, dim):
    """P: (2Nc+1)^dim x (Nc+1)^dim, the natural embedding of the coarse P1 space."""
    nc1, nf1 = Nc + 1, 2 * Nc + 1
    cI = _ijk(Nc, dim)
    rows, cols, vals = [], [], []
    lin_f = lambda c: c[0] + nf1 * c[1] + (nf1 * nf1 * c[2] if dim == 3 else 0)
    lin_c = lambda c: c[0] + nc1 * c[1] + (nc1 * nc1 * c[2] if dim == 3 else 0)
    rows.append(lin_f([2 * c for c in cI]))
    cols.append(lin_c(cI))
    vals.append(np.ones(cI[0].size))
    for p in itertools.product((0, 1), repeat=dim):
        if not any(p):
            continue
        ok = np.ones(cI[0].size, dtype=bool)
        for d in range(dim):
            ok &= cI[d] + p[d] <= Nc
        a = [c[ok] for c in cI]
        b = [c + q for c, q in zip(a, p)]
        mid = lin_f([2 * x + q for x, q in zip(a, p)])
        for end in (a, b):
            rows.append(mid)
            cols.append(lin_c(end))
            vals.append(np.full(mid.size, 0.5))
    P = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(nf1 ** dim, nc1 ** dim)).tocsr()
    P.sort_indices()
    return P


def restriction(Nc, dim):
    """R: interior coarse rows = rows of P^T restricted to interior fine columns; boundary coarse rows inject."""
    P = prolongation(Nc, dim)
    fi, ci = interior(2 * Nc, dim), interior(Nc, dim)
    PT = sp.csr_matrix(P.T)
    PT = sp.diags(ci.astype(float)) @ PT @ sp.diags(fi.astype(float))
    inj = sp.csr_matrix((np.ones((~ci).sum()), (np.flatnonzero(~ci), _coincident(Nc, dim)[~ci])),
                        shape=PT.shape)
    R = (PT + inj).tocsr()
    R.eliminate_zeros()
    R.sort_indices()
    return R


def _coincident(Nc, dim):
    nf1 = 2 * Nc + 1
    c = _ijk(Nc, dim)
    return 2 * c[0] + nf1 * 2 * c[1] + (nf1 * nf1 * 2 * c[2] if dim == 3 else 0)


def galerkin(A, Nf, dim):
    """P_i^T A_i P_i on the interior nodes (P restricted to interior fine and interior coarse nodes), identity rows on the
    boundary: the coarse matrix mg_galerkin_level builds, in lexicographic numbering (SciPy's product drops exact zeros)."""
    Nc = Nf // 2
    P = prolongation(Nc, dim)
    fi, ci = interior(Nf, dim), interior(Nc, dim)
    Pi = sp.csr_matrix(P[fi][:, ci])
    Ai = sp.csr_matrix(sp.csr_matrix(A)[fi][:, fi])
    G = sp.csr_matrix(Pi.T) @ Ai @ Pi
    n = (Nc + 1) ** dim
    emb = sp.csr_matrix((np.ones(ci.sum()), (np.flatnonzero(ci), np.arange(ci.sum()))), shape=(n, ci.sum()))
    out = (emb @ G @ emb.T + sp.diags((~ci).astype(float))).tocsr()
    out.eliminate_zeros()
    out.sort_indices()
    return out


def p1_oracle(bag, grid_index, dim):
    """The oracle's V-cycle with the P1 embedding and its transpose (restriction="table")."""
    orc = Oracle(bag, grid_index, dim=dim)
    orc.prolongation_table = poisson.p1_prolongation_table(dim)
    orc.restriction_table = poisson.p1_restriction_table(dim)
    return orc


def residual_history(orc, level, ncycles, restriction):
    """||f - A v||_2 after each of `ncycles` V-cycles from zero on `level`."""
    A = orc.A_sp_dict[level][0]
    f = orc.b_dict[level]
    v = np.zeros_like(f)
    out = []
    for _ in range(ncycles):
        v = orc.v_cycle(orc.A_jacobi_sp_dict[level], v, f, restriction=restriction)
        out.append(float(np.linalg.norm(f - A @ v)))
    return np.array(out)


def contraction(hist, first=5, last=12):
    """Geometric mean of the residual ratio over cycles first..last (1-based)."""
    return float((hist[last - 1] / hist[first - 2]) ** (1.0 / (last - first + 1)))
