"""Synthetic P1 Poisson hierarchies in the conventions of a dolfinx hand-off.

The reference builds its level inputs with dolfinx (`Multigrid_prototype.py:62-118`):
per level a `UnitSquareMesh`, a CG1 space, Dirichlet data `1 + x^2 + 2y^2` on the
whole boundary, `assemble_matrix(a, bcs=[bc])` exported with `getValuesCSR()` into a
SciPy CSR (`:92-96`), a lifted right-hand side reshaped to `(n, 1)` (`:100-110`) and a
two-way DoF<->coordinate dictionary (`:68-74`).  dolfinx is not installable here, so
this module synthesises inputs of exactly that shape:

* fp64 values, int32 `indices`/`indptr`, columns sorted within a row (PETSc AIJ),
* the full P1 sparsity pattern with the numerically-zero couplings kept as explicit
  0.0 (7 entries per interior row in 2-D, 15 in 3-D),
* symmetric Dirichlet treatment: boundary rows *and* columns zeroed, 1.0 on the
  boundary diagonal,
* right-hand side `f*h^d` on interior nodes, lifted by the boundary data, boundary
  entries set to the boundary data,
* an arbitrary DoF numbering (dolfinx numbering is not lexicographic and differs per
  level, `test/test_mesh.py:36`), related to the grid only through coordinates.

3-D has no reference counterpart; it is the dimension-consistent extension
(`g = 1 + x^2 + 2y^2 + 3z^2`, `f = -12`, Kuhn 6-tetrahedra split) of SURVEY.md §8(d).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np
import scipy.sparse as sp


def _offsets(dim: int):
    """P1 sparsity offsets (di, dj[, dk]) in ascending lexicographic-column order."""
    if dim == 2:
        offs = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1)]
        key = lambda o: (o[1], o[0])
    elif dim == 3:
        base = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
        offs = [(0, 0, 0)] + base + [tuple(-c for c in o) for o in base]
        key = lambda o: (o[2], o[1], o[0])
    else:
        raise ValueError("dim must be 2 or 3")
    return sorted(offs, key=key)


def boundary_data(coords: np.ndarray, dim: int) -> np.ndarray:
    """Dirichlet data / exact solution (`Multigrid_prototype.py:78`; 3-D extension)."""
    g = 1.0 + coords[:, 0] ** 2 + 2.0 * coords[:, 1] ** 2
    if dim == 3:
        g = g + 3.0 * coords[:, 2] ** 2
    return g


def source_term(dim: int) -> float:
    """Constant source `f` (`Multigrid_prototype.py:90`): -6 in 2-D, -12 in 3-D."""
    return -6.0 if dim == 2 else -12.0


@dataclass
class Level:
    """One level of a hierarchy, as the reference's script would hand it over."""
    N: int                      # elements per dimension
    dim: int
    A: sp.csr_matrix            # (n, n) fp64 / int32, explicit zeros kept, DoF numbering
    b: np.ndarray               # (n, 1) lifted right-hand side
    coords: np.ndarray          # (n, 3) DoF coordinates (z = 0 in 2-D), DoF numbering
    grid_index: np.ndarray      # (n,) int64: lexicographic node index of each DoF
    h: float

    @property
    def n(self) -> int:
        return self.A.shape[0]

    def exact(self) -> np.ndarray:
        return boundary_data(self.coords, self.dim).reshape(-1, 1)


def lexicographic_level(N: int, dim: int, keep_zeros: bool = True) -> Level:
    """Assemble one level in lexicographic numbering (x fastest)."""
    n1 = N + 1
    n = n1 ** dim
    h = 1.0 / N
    if n * 15 >= 2 ** 31 and dim == 3 and keep_zeros:
        raise ValueError("nnz would overflow int32 indptr; use the device generator")
    idx = np.arange(n, dtype=np.int64)
    ijk = [idx % n1, (idx // n1) % n1]
    if dim == 3:
        ijk.append(idx // (n1 * n1))
    on_bnd = np.zeros(n, dtype=bool)
    for c in ijk:
        on_bnd |= (c == 0) | (c == N)
    coords = np.zeros((n, 3))
    for d in range(dim):
        coords[:, d] = ijk[d] / N
    g = boundary_data(coords, dim)
    w = 1.0 if dim == 2 else h              # magnitude of an axis coupling
    diag = 4.0 if dim == 2 else 6.0 * h
    strides = [1, n1, n1 * n1][:dim]

    offs = _offsets(dim)
    valid, colv, valv = [], [], []
    b = np.where(on_bnd, g, source_term(dim) * h ** dim)
    for o in offs:
        ok = np.ones(n, dtype=bool)
        delta = 0
        for d in range(dim):
            if o[d] > 0:
                ok &= ijk[d] + o[d] <= N
            elif o[d] < 0:
                ok &= ijk[d] + o[d] >= 0
            delta += o[d] * strides[d]
        col = idx + delta
        nz_axis = sum(1 for c in o if c != 0)
        if nz_axis == 0:
            val = np.where(on_bnd, 1.0, diag)
        elif nz_axis == 1:
            colc = np.clip(col, 0, n - 1)
            both_int = ok & ~on_bnd & ~on_bnd[colc]
            val = np.where(both_int, -w, 0.0)
            lift = ok & ~on_bnd & on_bnd[colc]      # apply_lifting: b -= A_full[:, bc] g
            b = b + np.where(lift, w * g[colc], 0.0)
        else:
            val = np.zeros(n)
        if not keep_zeros:
            ok = ok & (val != 0.0)
        valid.append(ok)
        colv.append(col)
        valv.append(val)
    counts = np.zeros(n, dtype=np.int64)
    for ok in valid:
        counts += ok
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    nnz = int(indptr[-1])
    indices = np.empty(nnz, dtype=np.int32)
    data = np.empty(nnz, dtype=np.float64)
    pos = indptr[:-1].copy()
    for ok, col, val in zip(valid, colv, valv):
        p = pos[ok]
        indices[p] = col[ok]
        data[p] = val[ok]
        pos += ok
    A = sp.csr_matrix((data, indices, indptr.astype(np.int32)), shape=(n, n))
    A.has_sorted_indices = True
    return Level(N=N, dim=dim, A=A, b=b.reshape(n, 1), coords=coords, grid_index=idx.copy(), h=h)


def renumber(level: Level, numbering: np.ndarray) -> Level:
    """Re-express a lexicographic level in the DoF numbering `numbering[p] = dof`."""
    n = level.n
    numbering = np.asarray(numbering, dtype=np.int64)
    grid_index = np.empty(n, dtype=np.int64)
    grid_index[numbering] = np.arange(n, dtype=np.int64)
    A = level.A
    rows = np.repeat(numbering, np.diff(A.indptr))
    cols = numbering[A.indices]
    order = np.lexsort((cols, rows))
    counts = np.bincount(rows, minlength=n)
    indptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(counts, out=indptr[1:])
    A2 = sp.csr_matrix((A.data[order], cols[order].astype(np.int32), indptr), shape=(n, n))
    A2.has_sorted_indices = True
    b = np.empty_like(level.b)
    b[numbering] = level.b
    coords = np.empty_like(level.coords)
    coords[numbering] = level.coords
    return Level(N=level.N, dim=level.dim, A=A2, b=b, coords=coords, grid_index=grid_index, h=level.h)


def make_level(N: int, dim: int, seed: Optional[int] = None, keep_zeros: bool = True) -> Level:
    """One level; `seed` selects a reproducible random DoF numbering (None = lexicographic)."""
    lvl = lexicographic_level(N, dim, keep_zeros=keep_zeros)
    if seed is None:
        return lvl
    rng = np.random.default_rng(seed + 7919 * N)
    return renumber(lvl, rng.permutation(lvl.n))


def mesh_dof_dict(level: Level, decimals: int = 9) -> dict:
    """The reference's two-way dictionary `{dof: xyz} U {xyz: dof}` (`Multigrid_prototype.py:69-74`)."""
    d = {}
    for j in range(level.n):
        tup = tuple(round(float(c), decimals) for c in level.coords[j])
        d[j] = tup
        d[tup] = j
    return d


def grid_index_from_coords(coords: np.ndarray, N: int, dim: int) -> np.ndarray:
    """Lexicographic node index of every DoF from its coordinates.

    This replaces the reference's coordinate hashing (`multigrid.py:71-72`, `:78-79`,
    `:129-130`); rounding to the nearest grid line is valid for any N, unlike the
    reference's `int(x / h)` truncation.
    """
    coords = np.asarray(coords, dtype=np.float64)
    n1 = N + 1
    ijk = np.rint(coords[:, :dim] * N).astype(np.int64)
    if ijk.min() < 0 or ijk.max() > N:
        raise ValueError("coordinates outside the unit square/cube")
    gi = ijk[:, 0] + n1 * ijk[:, 1]
    if dim == 3:
        gi = gi + n1 * n1 * ijk[:, 2]
    if np.unique(gi).size != gi.size:
        raise ValueError("coordinates do not identify distinct grid nodes")
    return gi


@dataclass
class Hierarchy:
    """The 16-field attribute bag of `Var_initializer` (`Multigrid_prototype.py:15-32`)."""
    mesh_dof_list_dict: Dict[int, dict]
    element_size: Dict[int, float]
    coarsest_level_elements_per_dim: int
    coarsest_level: int
    finest_level: int
    A_sp_dict: Dict[int, tuple]
    A_jacobi_sp_dict: Dict[int, tuple]
    b_dict: Dict[int, np.ndarray]
    mu0: int
    mu1: int
    mu2: int
    omega: float
    residual_per_V_cycle_finest: list = field(default_factory=list)
    error_per_V_cycle_finest: list = field(default_factory=list)
    u_exact_fine: object = None
    V_fine_dolfx: object = None
    # extras (not part of the reference bag): the generated levels and the dimension
    levels: Dict[int, Level] = field(default_factory=dict)
    dim: int = 2


def make_hierarchy(dim: int, coarsest_level: int, finest_level: int, c: int = 8,
                   mu0: int = 2, mu1: int = 50, mu2: int = 50, omega: float = 2.0 / 3.0,
                   seed: Optional[int] = None, with_dicts: bool = False,
                   keep_zeros: bool = True) -> Hierarchy:
    """Level loop of `Multigrid_prototype.py:62-118` on synthetic inputs (N_l = c * 2**l).

    `A_jacobi_sp_dict` is left empty: it is filled by whichever `getJacobiMatrices`
    (the reference's, the oracle's or the HIP module's) the caller is exercising,
    as the script does at `Multigrid_prototype.py:135-136`.
    """
    levels, dicts, hs, As, bs = {}, {}, {}, {}, {}
    for l in range(coarsest_level, finest_level + 1):
        N = c * 2 ** l
        lvl = make_level(N, dim, seed=seed, keep_zeros=keep_zeros)
        levels[l] = lvl
        hs[l] = 1.0 / N
        As[l] = (lvl.A, l)
        bs[l] = lvl.b
        if with_dicts:
            dicts[l] = mesh_dof_dict(lvl)
    return Hierarchy(mesh_dof_list_dict=dicts, element_size=hs, coarsest_level_elements_per_dim=c,
                     coarsest_level=coarsest_level, finest_level=finest_level, A_sp_dict=As,
                     A_jacobi_sp_dict={}, b_dict=bs, mu0=mu0, mu1=mu1, mu2=mu2, omega=omega,
                     levels=levels, dim=dim)


# ---- P2 elements (BASELINE.json config 5; no reference implementation exists) ---------------------------------
def _p2_local_stiffness(verts: np.ndarray) -> np.ndarray:
    """Stiffness of one P2 simplex (triangle: 6 nodes, tetrahedron: 10 nodes) with vertex coordinates
    `verts` ((d+1, d)); node order: vertices, then edge midpoints (a, b) for a < b."""
    d = verts.shape[1]
    nv = d + 1
    T = np.hstack([np.ones((nv, 1)), verts])
    grad_lam = np.linalg.inv(T)[1:, :].T                 # (nv, d): gradient of each barycentric coordinate
    vol = abs(np.linalg.det(T)) / (2.0 if d == 2 else 6.0)
    edges = [(a, b) for a in range(nv) for b in range(a + 1, nv)]
    # degree-2 quadrature: triangle -> edge midpoints (weights 1/3); tetrahedron -> 4-point rule
    if d == 2:
        pts = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5]])
        wts = np.full(3, 1.0 / 3.0)
    else:
        a, b = 0.5854101966249685, 0.1381966011250105
        pts = np.full((4, 4), b) + (a - b) * np.eye(4)
        wts = np.full(4, 0.25)
    nn = nv + len(edges)
    K = np.zeros((nn, nn))
    for lam, w in zip(pts, wts):
        G = np.zeros((nn, d))
        for i in range(nv):
            G[i] = (4.0 * lam[i] - 1.0) * grad_lam[i]
        for e, (i, j) in enumerate(edges):
            G[nv + e] = 4.0 * (lam[i] * grad_lam[j] + lam[j] * grad_lam[i])
        K += w * vol * (G @ G.T)
    return K


def p2_level(N: int, dim: int, seed: Optional[int] = None) -> Level:
    """P2 Poisson level on the structured simplicial mesh with N cells per dimension: the DoFs are ALL points
    of the (2N+1)^dim lattice (vertices, edge / face-diagonal / body-diagonal midpoints), so `Level.N` is 2N and
    the lattice nests under refinement like the P1 grids do.  Same problem, boundary treatment and hand-off
    conventions as `lexicographic_level`; the stencil reaches two lattice planes.  Because P2 reproduces the
    quadratic manufactured solution exactly, the discrete solution equals the nodal exact values."""
    M = 2 * N
    n1 = M + 1
    n = n1 ** dim
    h = 1.0 / N
    idx = np.arange(n, dtype=np.int64)
    ijk = [idx % n1, (idx // n1) % n1] + ([idx // (n1 * n1)] if dim == 3 else [])
    coords = np.zeros((n, 3))
    for d in range(dim):
        coords[:, d] = ijk[d] / M
    on_bnd = np.zeros(n, dtype=bool)
    for cdir in ijk:
        on_bnd |= (cdir == 0) | (cdir == M)
    g = boundary_data(coords, dim)
    # reference simplices of one cell (right diagonal in 2-D, Kuhn split in 3-D), vertex offsets in cells
    import itertools
    simplices = []
    for perm in itertools.permutations(range(dim)):
        v = [np.zeros(dim, dtype=int)]
        for ax in perm:
            nxt = v[-1].copy()
            nxt[ax] += 1
            v.append(nxt)
        simplices.append(np.array(v))
    strides = np.array([1, n1, n1 * n1][:dim])
    cells = np.stack(np.meshgrid(*[np.arange(N)] * dim, indexing="ij"), axis=-1).reshape(-1, dim)
    rows, cols, vals = [], [], []
    load = np.zeros(n)
    f = source_term(dim)
    for sv in simplices:
        K = _p2_local_stiffness(sv * h)
        nv = dim + 1
        edges = [(a, b) for a in range(nv) for b in range(a + 1, nv)]
        local = [2 * sv[a] for a in range(nv)] + [sv[a] + sv[b] for a, b in edges]       # lattice offsets
        node = np.stack([(2 * cells + off) @ strides for off in local], axis=1)           # (ncells, nn)
        nn = node.shape[1]
        rows.append(np.repeat(node, nn, axis=1).reshape(-1))
        cols.append(np.tile(node, (1, nn)).reshape(-1))
        vals.append(np.tile(K.reshape(-1), cells.shape[0]))
        # load vector of a constant source: vertices get 0 (2-D) / -vol/20 (3-D), edge nodes vol/3 / vol/5
        vol = h ** dim / (2.0 if dim == 2 else 6.0)
        wv, we = (0.0, vol / 3.0) if dim == 2 else (-vol / 20.0, vol / 5.0)
        for a in range(nn):
            np.add.at(load, node[:, a], f * (wv if a < nv else we))
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    # symmetric Dirichlet treatment with explicit zeros kept, as assemble_matrix(bcs=[bc]) does
    b = load - A[:, on_bnd] @ g[on_bnd]
    b[on_bnd] = g[on_bnd]
    A = A.tolil()
    bidx = np.flatnonzero(on_bnd)
    keep = sp.diags((~on_bnd).astype(float))
    A = (keep @ A.tocsr() @ keep + sp.diags(on_bnd.astype(float))).tocsr()
    A.sort_indices()
    A = sp.csr_matrix((A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32)), shape=(n, n))
    lvl = Level(N=M, dim=dim, A=A, b=b.reshape(n, 1), coords=coords, grid_index=idx.copy(), h=h)
    if seed is None:
        return lvl
    rng = np.random.default_rng(seed + 7919 * N)
    return renumber(lvl, rng.permutation(n))


def p2_stencils(dim: int):
    """Interior rows of the P2 Poisson matrix per parity class of the lattice point, for mesh width h = 1 (cell
    size; lattice spacing 1/2): `(count[8], offsets[8, 64, 3], values[8, 64], load[8])` as `mg_gen_lattice_level` takes
    them, read off a small assembled level (`p2_level(4, dim)`, whose centre rows touch no boundary).  Values scale
    with h^(dim-2), the load with h^dim; for h a power of two both scalings are exact, so a level generated from these
    tables equals the assembled one bit for bit in its matrix."""
    N = 4
    L = p2_level(N, dim)
    M, n1 = L.N, L.N + 1
    h = 1.0 / N
    A = L.A.tocsr()
    count = np.zeros(8, dtype=np.int32)
    offsets = np.zeros((8, 64, 3), dtype=np.int32)
    values = np.zeros((8, 64))
    load = np.zeros(8)
    for cls in range(8):
        bits = (cls & 1, (cls >> 1) & 1, (cls >> 2) & 1)
        if dim == 2 and bits[1]:
            continue                                   # 2-D lattices are stored as (nx, 1, nz): j is always 0
        ijk = [4 + b for b in bits]                    # a centre node of this class
        if dim == 2:
            node = ijk[0] + n1 * ijk[2]
        else:
            node = ijk[0] + n1 * (ijk[1] + n1 * ijk[2])
        lo, hi = A.indptr[node], A.indptr[node + 1]
        cols, vals = A.indices[lo:hi], A.data[lo:hi]
        keep = vals != 0.0
        cols, vals = cols[keep], vals[keep]
        order = np.argsort(cols)
        cols, vals = cols[order], vals[order]
        count[cls] = cols.size
        for t, (cc, vv) in enumerate(zip(cols, vals)):
            ci = cc % n1
            cj = (cc // n1) % n1 if dim == 3 else 0
            ck = cc // (n1 * n1) if dim == 3 else cc // n1
            offsets[cls, t] = (ci - ijk[0], cj - ijk[1] if dim == 3 else 0, ck - ijk[2])
            values[cls, t] = vv / h ** (dim - 2)
        load[cls] = L.b[node, 0] / h ** dim
    return count, offsets, values, load


def p2_prolongation_table(dim: int):
    """The natural prolongation between nested P2 spaces on the structured simplicial meshes (coarse cells of four
    fine lattice steps per dimension): a fine lattice point takes the value of the coarse P2 function there.  That value
    only depends on the point's position inside its coarse cell, `(i mod 4, j mod 4, k mod 4)`, so the operator is a table
    `(count[64], offsets[64, 10, 3], weights[64, 10])`: for residue `ri + 4 rj + 16 rk` the `count` coarse lattice
    points `2 * floor((i, j, k) / 4) + offsets` (coarse lattice units, 0..2 per axis) and their weights -- the P2 basis
    functions `lambda_a (2 lambda_a - 1)` / `4 lambda_a lambda_b` of the Kuhn simplex that contains the point
    (`x_p1 >= x_p2 >= x_p3` for the simplex of axis permutation p, as `p2_level` splits the cells).  Coincident points
    copy, every other point combines up to 10 (3-D) / 6 (2-D) coarse values with weights like 3/8, 3/4, -1/8.
    2-D lattices use the residues with `rj = 0` (device storage `(nx, 1, nz)`).  NO REFERENCE COUNTERPART
    (`Interpolation2D` is bilinear, multigrid.py:59-120): BASELINE config 5's "higher-bandwidth transfer ops"."""
    import itertools
    axes = (0, 2) if dim == 2 else (0, 1, 2)            # lattice axes in use: (i, k) in 2-D
    count = np.zeros(64, dtype=np.int32)
    offsets = np.zeros((64, 10, 3), dtype=np.int32)
    weights = np.zeros((64, 10))
    for res in range(64):
        r = (res & 3, (res >> 2) & 3, (res >> 4) & 3)
        if dim == 2 and r[1]:
            continue
        x = np.array([r[a] / 4.0 for a in axes])         # position in the coarse cell
        perm = sorted(range(dim), key=lambda d: (-x[d], d))
        verts = [np.zeros(dim, dtype=int)]
        for d in perm:
            nxt = verts[-1].copy()
            nxt[d] += 1
            verts.append(nxt)
        xs = [x[d] for d in perm]
        lam = [1.0 - xs[0]] + [xs[t] - xs[t + 1] for t in range(dim - 1)] + [xs[-1]]
        entries = {}
        for a in range(dim + 1):
            w = lam[a] * (2.0 * lam[a] - 1.0)
            if w != 0.0:
                entries[tuple(2 * verts[a])] = entries.get(tuple(2 * verts[a]), 0.0) + w
        for a, b in itertools.combinations(range(dim + 1), 2):
            w = 4.0 * lam[a] * lam[b]
            if w != 0.0:
                key = tuple(verts[a] + verts[b])
                entries[key] = entries.get(key, 0.0) + w
        keys = sorted(entries, key=lambda kk: tuple(reversed(kk)))           # ascending coarse lexicographic order
        count[res] = len(keys)
        for t, kk in enumerate(keys):
            full = [0, 0, 0]
            for d, a in enumerate(axes):
                full[a] = kk[d]
            offsets[res, t] = full
            weights[res, t] = entries[kk]
    return count, offsets, weights


def p2_restriction_table(dim: int):
    """Transpose of `p2_prolongation_table`, gathered per coarse lattice point: `(count[8], offsets[8, M, 3],
    weights[8, M])` -- a coarse point A of type `(a & 1) + 2 (b & 1) + 4 (c & 1)` sums `weights[t] * r[2 A + offsets[t]]`
    over the fine lattice points whose prolongation uses it (the canonical finite-element restriction of a residual:
    `<R r, v> = <r, P v>`).  Entries in ascending fine lexicographic order.  NO REFERENCE COUNTERPART (the reference
    restricts by injection, multigrid.py:123-132, :251-252)."""
    count, offsets, weights = p2_prolongation_table(dim)
    fwd = {}
    for r in range(64):
        for t in range(count[r]):
            fwd[(r, tuple(int(x) for x in offsets[r, t]))] = weights[r, t]
    axes_on = (True, dim == 3, True)
    per_type = {}
    rng = range(-4, 5)
    for typ in range(8):
        t = (typ & 1, (typ >> 1) & 1, (typ >> 2) & 1)
        if dim == 2 and t[1]:
            continue
        ent = []
        for dk in rng:
            for dj in (rng if dim == 3 else (0,)):
                for di in rng:
                    d = (di, dj, dk)
                    res, need, ok = 0, [], True
                    for ax in range(3):
                        if not axes_on[ax]:
                            need.append(0)
                            continue
                        p = 2 * t[ax] + d[ax]                       # fine position relative to 4 q
                        res |= (p % 4) << (2 * ax)
                        o = t[ax] - 2 * (p // 4)                    # coarse offset that names A in that fine point's entry
                        if o < 0 or o > 2:
                            ok = False
                        need.append(o)
                    if ok and (res, tuple(need)) in fwd:
                        ent.append((d, fwd[(res, tuple(need))]))
        per_type[typ] = ent
    M = max(len(v) for v in per_type.values())
    rcount = np.zeros(8, dtype=np.int32)
    roff = np.zeros((8, M, 3), dtype=np.int32)
    rw = np.zeros((8, M))
    for typ, ent in per_type.items():
        rcount[typ] = len(ent)
        for e, (d, w) in enumerate(ent):
            roff[typ, e] = d
            rw[typ, e] = w
    return rcount, roff, rw


# ---- P1 natural embedding in the table format (no reference implementation exists) ---------------------------------
def kuhn_offsets(dim: int):
    """The P1 stencil of the structured simplicial mesh as device offsets (di, dj, dk) in ascending lexicographic order
    (dk, then dj, then di): `_offsets(dim)` with 2-D's (x, y) stored as (i, k).  The non-negative half are the mesh's edge
    directions: (1, 0), (0, 1), (1, 1) in 2-D; the seven non-zero p in {0,1}^3 in 3-D (six Kuhn simplices per cube)."""
    offs = []
    for o in _offsets(dim):
        offs.append((o[0], 0, o[1]) if dim == 2 else tuple(o))
    return offs


def p1_prolongation_table(dim: int):
    """The natural prolongation between nested P1 spaces on the structured simplicial meshes, in the table format of
    `p2_prolongation_table` (residue `ri + 4 rj + 16 rk` of `(i, j, k) mod 4` -> coarse points `2 * floor((i, j, k) / 4) +
    offsets`): fine node `2I + p` takes `v(I)` for p = 0 and `0.5 v(I) + 0.5 v(I + p)` otherwise -- every fine node is a
    coarse node or the midpoint of a coarse edge, which runs along p in {0,1}^dim.  The same operator as the device's
    `mg_set_prolongation_p1`; this table is its independent cross-check through `mg_set_prolongation_table`.  NO REFERENCE
    COUNTERPART (`Interpolation2D` is bilinear, multigrid.py:59-120, which on this mesh is not the embedding)."""
    axes = (0, 2) if dim == 2 else (0, 1, 2)
    count = np.zeros(64, dtype=np.int32)
    offsets = np.zeros((64, 10, 3), dtype=np.int32)
    weights = np.zeros((64, 10))
    for res in range(64):
        r = (res & 3, (res >> 2) & 3, (res >> 4) & 3)
        if dim == 2 and r[1]:
            continue
        base = [0, 0, 0]
        p = [0, 0, 0]
        for a in axes:
            base[a] = r[a] >> 1                      # floor(i / 2) - 2 floor(i / 4)
            p[a] = r[a] & 1
        if not any(p):
            entries = [(tuple(base), 1.0)]
        else:
            entries = [(tuple(base), 0.5), (tuple(b + q for b, q in zip(base, p)), 0.5)]
        count[res] = len(entries)
        for t, (o, w) in enumerate(entries):
            offsets[res, t] = o
            weights[res, t] = w
    return count, offsets, weights


def p1_restriction_table(dim: int):
    """Transpose of `p1_prolongation_table` in the format of `p2_restriction_table`: every interior coarse point, whatever
    its type, sums `w * r[2 A + d]` over the Kuhn pattern d (`kuhn_offsets`) in ascending fine lexicographic order, w = 1 for
    d = 0 and 0.5 otherwise.  The same operator as the device's MG_RESTRICT_P1_TRANSPOSE.  NO REFERENCE COUNTERPART."""
    offs = kuhn_offsets(dim)
    M = len(offs)
    count = np.full(8, M, dtype=np.int32)
    offsets = np.zeros((8, M, 3), dtype=np.int32)
    weights = np.zeros((8, M))
    for typ in range(8):
        for e, d in enumerate(offs):
            offsets[typ, e] = d
            weights[typ, e] = 1.0 if d == (0, 0, 0) else 0.5
    return count, offsets, weights


# ---- variable-coefficient diffusion, -div(kappa grad u) with one kappa per cell (no reference counterpart) ----------
def _kappa_cells(kappa, N: int, dim: int) -> np.ndarray:
    k = np.asarray(kappa, dtype=np.float64)
    if k.size != N ** dim:
        raise ValueError(f"kappa has {k.size} entries, the level has {N ** dim} cells")
    return k.reshape((N,) * dim)


def _edge_sums_3d(kp, n1):
    """Per node of the n1^3 grid, from the cell field padded by one cell: se[axis][side], the sum over the four cells of the
    edge towards the lower / upper neighbour on that axis in ascending index (n = 2, 1, 1, 2), and the sum of the six in
    ascending offset order -- `gen_diffusion`'s adds, one by one."""
    K = [[[kp[dz:dz + n1, dy:dy + n1, dx:dx + n1].reshape(-1) for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]
    se = [[None, None] for _ in range(3)]
    for s in (0, 1):
        se[0][s] = ((2.0 * K[0][0][s] + K[0][1][s]) + K[1][0][s]) + 2.0 * K[1][1][s]
        se[1][s] = ((2.0 * K[0][s][0] + K[0][s][1]) + K[1][s][0]) + 2.0 * K[1][s][1]
        se[2][s] = ((2.0 * K[s][0][0] + K[s][0][1]) + K[s][1][0]) + 2.0 * K[s][1][1]
    t = ((((se[2][0] + se[1][0]) + se[0][0]) + se[0][1]) + se[1][1]) + se[2][1]
    return se, t


FACE_BITS = {"x-": 1, "x+": 2, "y-": 4, "y+": 8, "z-": 16, "z+": 32}
ALL_FACES = 63


INSULATED = "insulated"


class _NoFaces(int):
    """What `face_set` makes of `INSULATED`: equal to 0, and the one zero `face_set` takes back, so the functions that hand a
    face set on as its integer keep working.  The plain integer 0 stays refused."""

    def __repr__(self):
        return "face_set('insulated')"


_NO_FACES = _NoFaces(0)


def face_set(dirichlet_faces) -> int:
    """The face set of `mg_set_diffusion_faces` as its integer: x- = 1, x+ = 2, y- = 4, y+ = 8, z- = 16, z+ = 32.  Takes the
    integer, None (all six) or names ("x-", "z+", ...).  `INSULATED` ("insulated") is the one spelling of the empty set, the
    body with no Dirichlet node of `mg_set_diffusion_insulated`: it gives 0.  The integer 0 is refused."""
    if dirichlet_faces is None:
        return ALL_FACES
    if isinstance(dirichlet_faces, _NoFaces) or (isinstance(dirichlet_faces, str) and dirichlet_faces == INSULATED):
        return _NO_FACES
    if isinstance(dirichlet_faces, (int, np.integer)):
        faces = int(dirichlet_faces)
    else:
        faces = 0
        for name in dirichlet_faces:
            if name not in FACE_BITS:
                raise ValueError(f"unknown face {name!r}: the faces are " + ", ".join(FACE_BITS))
            faces |= FACE_BITS[name]
    if faces < 0 or faces > ALL_FACES:
        raise ValueError(f"dirichlet_faces = {faces} is no face set (0..63)")
    if faces == 0:
        raise ValueError("dirichlet_faces = 0: without a Dirichlet face the operator is singular")
    return faces


def free_box(N: int, dirichlet_faces=ALL_FACES):
    """(lo, hi) per axis (x, y, z): a node is a free node of the face set iff lo[d] <= c[d] <= hi[d] on every axis -- the
    bounds the device kernels take instead of 1 and N - 1.  Every other node is a Dirichlet node."""
    faces = face_set(dirichlet_faces)
    lo = [1 if faces >> (2 * d) & 1 else 0 for d in range(3)]
    hi = [N - 1 if faces >> (2 * d + 1) & 1 else N for d in range(3)]
    return lo, hi


def dirichlet_mask(N: int, dirichlet_faces=ALL_FACES) -> np.ndarray:
    """True on the Dirichlet nodes of the face set (nodes on a face whose bit is set), (N + 1)^3 lexicographic."""
    lo, hi = free_box(N, dirichlet_faces)
    c = np.arange(N + 1)
    fr = [(c >= lo[d]) & (c <= hi[d]) for d in range(3)]
    free = fr[2][:, None, None] & fr[1][None, :, None] & fr[0][None, None, :]
    return ~free.reshape(-1)


def _cells_around_nodes(w, N: int):
    """W[dz][dy][dx]: per node (i, j, k) of the (N + 1)^3 grid the value of cell (i - 1 + dx, j - 1 + dy, k - 1 + dz), +0.0
    outside the grid."""
    n1 = N + 1
    wp = np.pad(_kappa_cells(w, N, 3), 1, constant_values=0.0)
    return [[[wp[dz:dz + n1, dy:dy + n1, dx:dx + n1].reshape(-1) for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]


def reaction_diag(N: int, w, dirichlet_faces=ALL_FACES) -> np.ndarray:
    """R(w): the diagonal of the lumped reaction term of a cell field `w` (N^3 values of any sign, cell order of
    `diffusion_level`) on the (N + 1)^3 nodes, as the device computes it (`reaction_diag`, mg_kernels.hip.h; same bits).  The
    row-sum lumped P1 mass of the Kuhn mesh with the weights of the load: over the 8 cells around a node in ascending index
    (dz, dy, dx), t * w_c with t = 6 where the node is the cell's (0,0,0) or (1,1,1) corner and 2 otherwise, a cell outside
    the grid counting as +0.0, added one by one; then (sum / 24.0) * h^3.  w == 1 gives h^3 (T / 24), the load of f == 1.
    Dirichlet nodes of `dirichlet_faces` (`face_set`) get +0.0: R acts on free rows only."""
    W = _cells_around_nodes(w, N)
    h = 1.0 / N
    s = None
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                t = (6.0 if dx == dy == dz else 2.0) * W[dz][dy][dx]
                s = t if s is None else s + t
    r = (s / 24.0) * h ** 3
    return np.where(dirichlet_mask(N, dirichlet_faces), 0.0, r)


def _one_face(face) -> int:
    """One face of the cube as its bit, from the bit or the name."""
    bit = FACE_BITS.get(face) if isinstance(face, str) else (int(face) if isinstance(face, (int, np.integer)) else None)
    if bit not in FACE_BITS.values():
        raise ValueError(f"{face!r} is not one face: the faces are " + ", ".join(f"{k} = {v}" for k, v in FACE_BITS.items()))
    return bit


def _robin_fields(N: int, robin, dirichlet_faces=None, signed: bool = False) -> dict:
    """`robin` (face name or bit -> N^2 values) as {bit: (N, N) array [cb][ca]} in ascending bit order, checked."""
    out = {}
    for face, alpha in robin.items():
        bit = _one_face(face)
        if bit in out:
            raise ValueError(f"face {bit} is given twice")
        if alpha is None:
            continue
        al = _kappa_cells(alpha, N, 2)
        if not signed and (not np.all(np.isfinite(al)) or np.any(al < 0.0)):
            raise ValueError("alpha must be finite and not negative")
        if dirichlet_faces is not None and face_set(dirichlet_faces) & bit:
            raise ValueError(f"face {bit} is a Dirichlet face of the set {face_set(dirichlet_faces)}: it cannot hold a Robin field")
        out[bit] = al
    return dict(sorted(out.items()))


def _face_cells_around_nodes(w, N: int) -> np.ndarray:
    """((sum over the 4 face-cells around an in-plane node, ascending (db, da), of t w) / 6.0) * h^2 on the (N + 1)^2 nodes
    [pb][pa] of a face: t = 2 where the node is the face-cell's in-plane (0,0) or (1,1) corner (da == db), else 1; a
    face-cell outside the face counts as +0.0; added one by one."""
    n1 = N + 1
    wp = np.pad(w, 1, constant_values=0.0)
    s = None
    for db in (0, 1):
        for da in (0, 1):
            t = (2.0 if da == db else 1.0) * wp[db:db + n1, da:da + n1]
            s = t if s is None else s + t
    h = 1.0 / N
    return (s / 6.0) * h ** 2


def _on_face(field2d, N: int, bit: int) -> np.ndarray:
    """The (N + 1)^3 nodal array [k][j][i] that holds `field2d` ([pb][pa], in-plane axes ascending) on the face and +0.0
    elsewhere."""
    n1 = N + 1
    out = np.zeros((n1, n1, n1))
    axis, side = (bit.bit_length() - 1) // 2, (bit.bit_length() - 1) % 2
    at = N if side else 0
    if axis == 0:
        out[:, :, at] = field2d
    elif axis == 1:
        out[:, at, :] = field2d
    else:
        out[at, :, :] = field2d
    return out


def _face_plane(nodal, N: int, bit: int) -> np.ndarray:
    """The (N + 1)^2 values [pb][pa] of a nodal vector on a face."""
    n1 = N + 1
    v = nodal.reshape(n1, n1, n1)
    axis, side = (bit.bit_length() - 1) // 2, (bit.bit_length() - 1) % 2
    at = N if side else 0
    return v[:, :, at] if axis == 0 else (v[:, at, :] if axis == 1 else v[at, :, :])


def robin_diag(N: int, robin, dirichlet_faces=ALL_FACES) -> np.ndarray:
    """B(alpha): the diagonal of the lumped Robin term kappa du/dn + alpha (u - u_ext) = 0 on the (N + 1)^3 nodes, as the
    device computes it (`robin_diag`, mg_kernels.hip.h; same bits).  `robin` maps a face (name or bit) to its N^2 values
    alpha >= 0, face-cell (ca, cb) at `cb * N + ca` with (a, b) the two in-plane axes in ascending order.  The Kuhn split
    cuts a boundary face-cell along the diagonal from its in-plane (0,0) to its (1,1) corner; the row-sum lumped P1 boundary
    mass gives, per face F,
        b_F(alpha)_i = ((sum over the 4 face-cells around node i, ascending (db, da), of t alpha_q) / 6.0) * h^2,
    t = 2 at the (0,0) and (1,1) corners, else 1, a face-cell outside the face counting as +0.0, added one by one.  B is the
    sum of b_F over the faces that contain the node in ascending face-bit order, the first term starting the accumulator;
    +0.0 on every node on no field face and on every Dirichlet node of `dirichlet_faces`.  A face of the Dirichlet set cannot
    hold a field."""
    fields = _robin_fields(N, robin, dirichlet_faces)
    n1 = N + 1
    B = np.zeros((n1, n1, n1))
    for bit, al in fields.items():          # (+0.0 + b is b: every term is >= +0.0)
        B = B + _on_face(_face_cells_around_nodes(al, N), N, bit)
    return np.where(dirichlet_mask(N, dirichlet_faces), 0.0, B.reshape(-1))


def coarsen_robin(robin):
    """The Robin fields of the coarse level (N / 2 face-cells per dimension) as the diffusion hierarchy calls compute them:
    the arithmetic mean of the 2 x 2 children in `coarsen_kappa`'s 2-D order, whatever the kappa averaging (boundary mass is
    additive).  Takes one field or a mapping of faces to fields and returns the same kind."""
    if isinstance(robin, dict):
        return {face: None if alpha is None else coarsen_kappa(alpha, 2, "arithmetic") for face, alpha in robin.items()}
    return coarsen_kappa(robin, 2, "arithmetic")


def diffusion_drobin(N: int, face, a, b, dirichlet_faces=ALL_FACES) -> np.ndarray:
    """D_alpha,F(a, b): d(a^T B(alpha) b) / d alpha_q for the N^2 face-cells of `face`, as `mg_diffusion_drobin` computes it
    (same bits).  With A~, B~ the values of `a`, `b` at a face-cell's corners (db, da), Dirichlet nodes of `dirichlet_faces`
    taken as 0: t * (A~ * B~) with t = 2 at (0,0) and (1,1) and 1 elsewhere, added one by one in ascending (db, da), times
    h^2 / 6.0.  The adjoint of `diffusion_apply_drobin`: a . T(w, x) = w . D(a, x)."""
    bit = _one_face(face)
    if face_set(dirichlet_faces) & bit:
        raise ValueError(f"face {bit} is a Dirichlet face of the set {face_set(dirichlet_faces)}")
    n1 = N + 1
    free = ~dirichlet_mask(N, dirichlet_faces)

    def corners(x):
        v = np.array(x, dtype=np.float64).reshape(-1)
        if v.size != n1 ** 3:
            raise ValueError(f"vector has {v.size} entries, the level has {n1 ** 3} nodes")
        m = _face_plane(np.where(free, v, 0.0), N, bit)
        return [[m[db:db + N, da:da + N] for da in (0, 1)] for db in (0, 1)]

    A, Bc = corners(a), corners(b)
    s = None
    for db in (0, 1):
        for da in (0, 1):
            t = (2.0 if da == db else 1.0) * (A[db][da] * Bc[db][da])
            s = t if s is None else s + t
    h = 1.0 / N
    return np.ascontiguousarray((s * (h ** 2 / 6.0)).reshape(-1))


def diffusion_apply_drobin(N: int, face, dalpha, x, dirichlet_faces=ALL_FACES) -> np.ndarray:
    """T_alpha,F(dalpha, x)_i = b_F(dalpha)_i x_i on the free nodes of `face`, +0.0 on every other node, as
    `mg_diffusion_apply_drobin` computes it (same bits: `robin_diag`'s face sum, then one product).  `dalpha`: N^2 values of
    any sign.  With dalpha = alpha and x = u_ext it is the ambient load alpha u_ext int phi_i that the caller adds to f."""
    bit = _one_face(face)
    if face_set(dirichlet_faces) & bit:
        raise ValueError(f"face {bit} is a Dirichlet face of the set {face_set(dirichlet_faces)}")
    n1 = N + 1
    v = np.array(x, dtype=np.float64).reshape(-1)
    if v.size != n1 ** 3:
        raise ValueError(f"vector has {v.size} entries, the level has {n1 ** 3} nodes")
    w = _kappa_cells(dalpha, N, 2)
    bF = _on_face(_face_cells_around_nodes(w, N), N, bit).reshape(-1)
    on = _on_face(np.ones((n1, n1)), N, bit).reshape(-1) > 0.0
    return np.where(on & ~dirichlet_mask(N, dirichlet_faces), bF * v, 0.0)


def diffusion_level(N: int, dim: int, kappa, keep_zeros: bool = True, dirichlet_faces=ALL_FACES, sigma=None, robin=None) -> Level:
    """The level `mg_gen_diffusion_level` generates, assembled on the host in the kernel's operation order (same bits), in
    the hand-off conventions of `lexicographic_level`.  `kappa` holds one positive value per cell: cube (ci, cj, ck) at
    `(ck * N + cj) * N + ci`, square (ci, cy) at `cy * N + ci`.  On the Kuhn mesh the P1 stiffness of -div(kappa grad u)
    couples axis neighbours only: the edge towards a neighbour gets -(sum_c n_c kappa_c) h / 6 (3-D) or -(sum_c kappa_c) / 2
    (2-D) over the cells holding the edge in ascending index (n_c = 2 where the cell's other two local coordinates at the
    edge are equal, else 1), the diagonal the sum of the row's edge sums in ascending offset order, scaled the same way.
    Identity rows, zeroed columns and the lifted right-hand side as `lexicographic_level`, which kappa == 1 reproduces bit
    for bit.

    `dirichlet_faces` (3-D; `face_set`, the set of `mg_set_diffusion_faces`): only nodes on those faces are identity rows.
    A free node on another face gets the natural row: the same sums with a cell outside the grid counting as +0.0, no
    column outside the grid, and the load fh * (T / 24.0) with T the number of Kuhn simplices at the node inside the grid
    (6 for an in-grid cell of which the node is the (0,0,0) or (1,1,1) corner, 2 for every other; 24 inside).  63, the
    default, is the level above byte for byte.

    `sigma` (3-D; `mg_set_diffusion_reaction`): one finite value >= 0 per cell, the operator A(kappa) + R(sigma).  A free row's
    diagonal is the stiffness diagonal above plus `reaction_diag(N, sigma)` of its node, one more addition; identity rows, the
    off-diagonals, the lifted right-hand side and the load do not change.  None, the default, is the level above byte for
    byte.

    `robin` (3-D; `mg_set_diffusion_robin`): a mapping of faces outside the Dirichlet set to N^2 values alpha >= 0 each, the
    condition kappa du/dn + alpha (u - u_ext) = 0 there.  A free row's diagonal gets one nodal term by one more addition:
    `robin_diag(N, robin)` of its node, or `reaction_diag + robin_diag`, formed as that sum, with a `sigma`.  Nothing else
    changes; the ambient load is the caller's (`diffusion_apply_drobin`).  None, the default, is the level above byte for
    byte."""
    faces = face_set(dirichlet_faces)
    if faces != ALL_FACES and dim != 3:
        raise ValueError("a face set other than all six faces is 3-D only")
    if sigma is not None:
        if dim != 3:
            raise ValueError("the reaction term is 3-D only")
        sig = _kappa_cells(sigma, N, 3)
        if not np.all(np.isfinite(sig)) or np.any(sig < 0.0):
            raise ValueError("sigma must be finite and not negative")
    if robin is not None and dim != 3:
        raise ValueError("Robin faces are 3-D only")
    kap = _kappa_cells(kappa, N, dim)
    if np.any(~(kap > 0.0)) or not np.all(np.isfinite(kap)):
        raise ValueError("kappa must be positive and finite")
    # node (i, ..) -> cells i - 1 + d: padded index i + d (the pad is read by rows on the boundary only)
    kp = np.pad(kap, 1, constant_values=1.0 if faces == ALL_FACES else 0.0)
    n1 = N + 1
    h = 1.0 / N
    if dim == 3:
        se, t = _edge_sums_3d(kp, n1)
        diag = (t / 6.0) * h
        if robin is not None and _robin_fields(N, robin, faces):
            B = robin_diag(N, robin, faces)
            diag = diag + (reaction_diag(N, sig, faces) + B if sigma is not None else B)
        elif sigma is not None:
            diag = diag + reaction_diag(N, sig, faces)
        weight = lambda s: (s / 6.0) * h
    else:
        K = [[kp[dy:dy + n1, dx:dx + n1].reshape(-1) for dx in (0, 1)] for dy in (0, 1)]
        se = [[K[0][s] + K[1][s] for s in (0, 1)], [K[s][0] + K[s][1] for s in (0, 1)]]
        t = ((se[1][0] + se[0][0]) + se[0][1]) + se[1][1]
        diag = t / 2.0
        weight = lambda s: s / 2.0

    n = n1 ** dim
    idx = np.arange(n, dtype=np.int64)
    ijk = [idx % n1, (idx // n1) % n1]
    if dim == 3:
        ijk.append(idx // (n1 * n1))
    on_bnd = np.zeros(n, dtype=bool)            # the Dirichlet nodes
    for d, c in enumerate(ijk):
        on_bnd |= ((c == 0) & bool(faces >> (2 * d) & 1)) | ((c == N) & bool(faces >> (2 * d + 1) & 1))
    coords = np.zeros((n, 3))
    for d in range(dim):
        coords[:, d] = ijk[d] / N
    g = boundary_data(coords, dim)
    strides = [1, n1, n1 * n1][:dim]
    load = source_term(dim) * h ** dim
    if faces != ALL_FACES:
        inside = np.pad(np.ones((N, N, N)), 1, constant_values=0.0)
        T = np.zeros(n)
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    T += (6.0 if dx == dy == dz else 2.0) * inside[dz:dz + n1, dy:dy + n1, dx:dx + n1].reshape(-1)
        load = load * (T / 24.0)
    b = np.where(on_bnd, g, load)
    valid, colv, valv = [], [], []
    for o in _offsets(dim):
        ok = np.ones(n, dtype=bool)
        delta = 0
        for d in range(dim):
            if o[d] > 0:
                ok &= ijk[d] + o[d] <= N
            elif o[d] < 0:
                ok &= ijk[d] + o[d] >= 0
            delta += o[d] * strides[d]
        col = idx + delta
        axes = [d for d in range(dim) if o[d] != 0]
        if not axes:
            val = np.where(on_bnd, 1.0, diag)
        elif len(axes) == 1:
            ax = axes[0]
            a = -weight(se[ax][1 if o[ax] > 0 else 0])
            colc = np.clip(col, 0, n - 1)
            both_int = ok & ~on_bnd & ~on_bnd[colc]
            val = np.where(both_int, a, 0.0)
            lift = ok & ~on_bnd & on_bnd[colc]
            b = np.where(lift, b - a * g[colc], b)
        else:
            val = np.zeros(n)
        if not keep_zeros:
            ok = ok & (val != 0.0)
        valid.append(ok)
        colv.append(col)
        valv.append(val)
    counts = np.zeros(n, dtype=np.int64)
    for ok in valid:
        counts += ok
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    nnz = int(indptr[-1])
    indices = np.empty(nnz, dtype=np.int32)
    data = np.empty(nnz, dtype=np.float64)
    pos = indptr[:-1].copy()
    for ok, col, val in zip(valid, colv, valv):
        p = pos[ok]
        indices[p] = col[ok]
        data[p] = val[ok]
        pos += ok
    A = sp.csr_matrix((data, indices, indptr.astype(np.int32)), shape=(n, n))
    A.has_sorted_indices = True
    return Level(N=N, dim=dim, A=A, b=b.reshape(n, 1), coords=coords, grid_index=idx.copy(), h=h)


def coarsen_kappa(kappa, dim: int, averaging: str = "arithmetic") -> np.ndarray:
    """kappa of the coarse cells (N / 2 per dimension) as `mg_gen_diffusion_hierarchy` computes it: the 2^dim children in
    ascending lexicographic order summed one by one (explicit adds, so the order is pinned), then x 2^-dim ("arithmetic")
    or 2^dim / sum of 1 / kappa ("harmonic").  Flat array in the cell order of `diffusion_level`."""
    k = np.asarray(kappa, dtype=np.float64)
    N = int(round(k.size ** (1.0 / dim)))
    kap = _kappa_cells(k, N, dim)
    if N % 2:
        raise ValueError("coarsening needs an even number of cells per dimension")
    if averaging not in ("arithmetic", "harmonic"):
        raise ValueError("averaging must be 'arithmetic' or 'harmonic'")
    if dim == 3:
        children = [kap[c::2, b::2, a::2] for c in (0, 1) for b in (0, 1) for a in (0, 1)]
    else:
        children = [kap[b::2, a::2] for b in (0, 1) for a in (0, 1)]
    s = None
    for x in children:
        term = 1.0 / x if averaging == "harmonic" else x
        s = term.copy() if s is None else s + term
    m = float(2 ** dim)
    out = m / s if averaging == "harmonic" else s * (1.0 / m)
    return np.ascontiguousarray(out.reshape(-1))


def coarsen_sigma(sigma, averaging: str = "arithmetic") -> np.ndarray:
    """sigma of the coarse cells (N / 2 per dimension) as the diffusion hierarchy calls compute it: the arithmetic mean of the
    2^3 children in `coarsen_kappa`'s order, whatever `averaging` says for kappa -- mass is additive.  `averaging` is taken so
    that the two fields can be coarsened by one call pattern, and only checked."""
    if averaging not in ("arithmetic", "harmonic"):
        raise ValueError("averaging must be 'arithmetic' or 'harmonic'")
    return coarsen_kappa(sigma, 3, "arithmetic")


def diffusion_dsigma(N: int, a, b, dirichlet_faces=ALL_FACES) -> np.ndarray:
    """D_sigma(a, b): d(a^T R(sigma) b) / d sigma_c for the N^3 cells, as `mg_diffusion_dsigma` computes it (same bits).  With
    A~, B~ the values of `a`, `b` at a cell's corners (dz, dy, dx), the Dirichlet nodes of `dirichlet_faces` taken as 0:
    t * (A~ * B~) with t = 6 at (0,0,0) and (1,1,1) and 2 elsewhere, added one by one in ascending (dz, dy, dx), times
    h^3 / 24.0.  R is linear in sigma: no sigma is read.  The adjoint of `diffusion_apply_dsigma`:
    a . T_sigma(w, x) = w . D_sigma(a, x)."""
    n1 = N + 1
    free = ~dirichlet_mask(N, dirichlet_faces)

    def corners(x):
        v = np.array(x, dtype=np.float64).reshape(-1)
        if v.size != n1 ** 3:
            raise ValueError(f"vector has {v.size} entries, the level has {n1 ** 3} nodes")
        m = np.where(free, v, 0.0).reshape(n1, n1, n1)
        return [[[m[dz:dz + N, dy:dy + N, dx:dx + N] for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]

    A, B = corners(a), corners(b)
    s = None
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                t = (6.0 if dx == dy == dz else 2.0) * (A[dz][dy][dx] * B[dz][dy][dx])
                s = t if s is None else s + t
    h = 1.0 / N
    return np.ascontiguousarray((s * (h ** 3 / 24.0)).reshape(-1))


def diffusion_apply_dsigma(N: int, dsigma, x, dirichlet_faces=ALL_FACES) -> np.ndarray:
    """T_sigma(dsigma, x) = R(dsigma) x on the free nodes of `dirichlet_faces`, +0.0 on its Dirichlet nodes, as
    `mg_diffusion_apply_dsigma` computes it (same bits: `reaction_diag`'s sum, then one product).  The derivative of
    (A(kappa) + R(sigma)) x in the direction `dsigma`, of any sign; with dsigma = 1 / dt it is the M u / dt of an implicit
    Euler step."""
    n1 = N + 1
    v = np.array(x, dtype=np.float64).reshape(-1)
    if v.size != n1 ** 3:
        raise ValueError(f"vector has {v.size} entries, the level has {n1 ** 3} nodes")
    W = _cells_around_nodes(dsigma, N)
    s = None
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                t = (6.0 if dx == dy == dz else 2.0) * W[dz][dy][dx]
                s = t if s is None else s + t
    r = (s / 24.0) * (1.0 / N) ** 3
    return np.where(dirichlet_mask(N, dirichlet_faces), 0.0, r * v)


_NODE_SETS = ("interior", "all")


def _node_set_all(name, what: str) -> bool:
    if name not in _NODE_SETS:
        raise ValueError(f"{what} must be 'interior' or 'all' (got {name!r})")
    return name == "all"


def diffusion_dkappa(N: int, a, b, a_nodes: str = "interior", b_nodes: str = "interior", dirichlet_faces=ALL_FACES) -> np.ndarray:
    """d(a^T A(kappa) b) / d kappa_c for the N^3 cells of the 3-D `diffusion_level`, as `mg_diffusion_dkappa` computes it (same
    bits: explicit adds in the order of `dk_cell`, mg_diffusion_adj.hip.h).  `a`, `b`: nodal values in lexicographic order;
    their boundary entries count as 0 (boundary rows are identity rows and interior rows have no boundary column: that block
    does not depend on kappa).  A is linear in kappa, so the result needs no kappa: with A~, B~ the masked values at a cell's
    corners (dz, dy, dx), an axis edge contributes (A~_upper - A~_lower) * (B~_upper - B~_lower), times 2 where the cell's two
    other local coordinates at the edge are equal; the x edges at (dz, dy) = (0,0), (0,1), (1,0), (1,1), then the y edges at
    (dz, dx), then the z edges at (dy, dx) are added one by one and the sum is scaled by (1 / N) / 6.  Flat array in the cell
    order of `diffusion_level`.

    `a_nodes`, `b_nodes` ("interior" / "all") are the masks of `mg_diffusion_dkappa_ex`, D(a, b; A, B)_c =
    d / d w_c (M_A a)^T A^(w) (M_B b) with A^ = `diffusion_natural_matrix`: "all" keeps the boundary entries of that
    vector.  The mask acts on the values at the corners and nowhere else, so these are the device's bits as well.

    `dirichlet_faces` (`face_set`): "interior" is the set of the free nodes of that face set -- the entries on the Dirichlet
    nodes count as 0, those on free boundary nodes are kept.  63 is the boundary."""
    n1 = N + 1
    lo, hi = free_box(N, dirichlet_faces)
    box = tuple(slice(lo[d], hi[d] + 1) for d in (2, 1, 0))

    def corners(x, keep_boundary):
        v = np.array(x, dtype=np.float64).reshape(-1)
        if v.size != n1 ** 3:
            raise ValueError(f"vector has {v.size} entries, the level has {n1 ** 3} nodes")
        v = v.reshape(n1, n1, n1)
        m = v
        if not keep_boundary:
            m = np.zeros_like(v)
            m[box] = v[box]
        return [[[m[dz:dz + N, dy:dy + N, dx:dx + N] for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]

    A, B = corners(a, _node_set_all(a_nodes, "a_nodes")), corners(b, _node_set_all(b_nodes, "b_nodes"))
    edge = lambda hi, lo: (A[hi[0]][hi[1]][hi[2]] - A[lo[0]][lo[1]][lo[2]]) * (B[hi[0]][hi[1]][hi[2]] - B[lo[0]][lo[1]][lo[2]])
    s = None
    for axis in (0, 1, 2):                      # x, y, z edges; (p, q): the two other coordinates, slower one first
        for p in (0, 1):
            for q in (0, 1):
                if axis == 0:
                    hi, lo = (p, q, 1), (p, q, 0)
                elif axis == 1:
                    hi, lo = (p, 1, q), (p, 0, q)
                else:
                    hi, lo = (1, p, q), (0, p, q)
                t = edge(hi, lo)
                if p == q:
                    t = 2.0 * t
                s = t if s is None else s + t
    return np.ascontiguousarray((s * ((1.0 / N) / 6.0)).reshape(-1))


def _cell_gradient_axes(N: int, x):
    """[G_x, G_y, G_z], each [N][N][N]: the mean of grad x_h over the six Kuhn simplices of every cell, with the adds of
    `cg_grad` (mg_diffusion_flux.hip.h): per axis one accumulator over the cell's four edges of that axis in `dk_cell`'s edge
    order with the weights 2, 1, 1, 2, times N / 6.0.  No mask."""
    n1 = N + 1
    v = np.array(x, dtype=np.float64).reshape(-1)
    if v.size != n1 ** 3:
        raise ValueError(f"vector has {v.size} entries, the level has {n1 ** 3} nodes")
    v = v.reshape(n1, n1, n1)
    U = [[[v[dz:dz + N, dy:dy + N, dx:dx + N] for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]
    s = N / 6.0
    G = []
    for axis in (0, 1, 2):                      # x, y, z edges; (p, q): the two other coordinates, slower one first
        acc = None
        for p in (0, 1):
            for q in (0, 1):
                if axis == 0:
                    hi, lo = (p, q, 1), (p, q, 0)
                elif axis == 1:
                    hi, lo = (p, 1, q), (p, 0, q)
                else:
                    hi, lo = (1, p, q), (0, p, q)
                t = U[hi[0]][hi[1]][hi[2]] - U[lo[0]][lo[1]][lo[2]]
                if p == q:
                    t = 2.0 * t
                acc = t if acc is None else acc + t
        G.append(acc * s)
    return G


def _cell_field3(p, N: int) -> np.ndarray:
    v = np.array(p, dtype=np.float64).reshape(-1)
    if v.size != 3 * N ** 3:
        raise ValueError(f"a 3-component cell field has {3 * N ** 3} entries (got {v.size})")
    return v.reshape(3, N, N, N)


def diffusion_cell_gradient(N: int, w, x) -> np.ndarray:
    """F(w, x), 3 N^3: F_{d,c} = w_c * G_d(x)_c with G(x)_c the mean of grad x_h over the six Kuhn simplices of cell c, as
    `mg_diffusion_cell_gradient` computes it (same bits: the adds of `cg_cell_f`, mg_diffusion_flux.hip.h).  `w`: N^3 cell values
    of any sign in the cell order of `diffusion_level`, or None (F = G, no product); `x`: nodal values in lexicographic order,
    read as they are (no mask).  Component d in (x, y, z) at d * N^3 + cell.  -F(kappa, u) is the cell average of the flux
    -kappa grad u_h."""
    G = _cell_gradient_axes(N, x)
    if w is not None:
        wc = _kappa_cells(w, N, 3)
        G = [wc * g for g in G]
    return np.ascontiguousarray(np.stack(G).reshape(-1))


def diffusion_cell_gradient_dot(N: int, p, x) -> np.ndarray:
    """C(p, x), N^3: out_c = ((p_{x,c} * G_x) + p_{y,c} * G_y) + p_{z,c} * G_z, as `mg_diffusion_cell_gradient_dot` computes it
    (same bits).  <w, C(p, x)> = <p, F(w, x)> up to rounding."""
    G = _cell_gradient_axes(N, x)
    P = _cell_field3(p, N)
    return np.ascontiguousarray((((P[0] * G[0]) + P[1] * G[1]) + P[2] * G[2]).reshape(-1))


def diffusion_cell_gradient_t(N: int, w, p) -> np.ndarray:
    """F^T(w, p), (N + 1)^3 nodes: the transpose of `diffusion_cell_gradient` in x, as `mg_diffusion_cell_gradient_t` computes it
    (same bits: the order of `cg_node_t`, mg_diffusion_flux.hip.h).  One accumulator per node starts at +0.0 and takes the cells
    (k + oz, j + oy, i + ox) around node (i, j, k) in ascending (oz, oy, ox), each offset -1 then 0, cells outside the grid
    adding nothing; inside a cell q_d = w_c * p_{d,c} (p_{d,c} with `w` None), then for x, y, z: + or - (2.0 * q_d where the
    node's two other local coordinates in the cell are equal, else q_d), + where the offset along that axis is -1; the sum
    times N / 6.0."""
    n1 = N + 1
    Q = _cell_field3(p, N)
    if w is not None:
        wc = _kappa_cells(w, N, 3)
        Q = np.stack([wc * Q[d] for d in range(3)])
    pad = np.zeros((3, N + 2, N + 2, N + 2))            # (a cell outside the grid adds 0.0: the accumulator is never -0.0)
    pad[:, 1:-1, 1:-1, 1:-1] = Q
    acc = np.zeros((n1, n1, n1))
    for oz in (-1, 0):
        for oy in (-1, 0):
            for ox in (-1, 0):
                q = pad[:, 1 + oz:1 + oz + n1, 1 + oy:1 + oy + n1, 1 + ox:1 + ox + n1]
                for d, (off, same) in enumerate(((ox, oy == oz), (oy, ox == oz), (oz, ox == oy))):
                    t = 2.0 * q[d] if same else q[d]
                    acc = acc + t if off < 0 else acc - t
    return np.ascontiguousarray((acc * (N / 6.0)).reshape(-1))


def _points(pts) -> np.ndarray:
    P = np.array(pts, dtype=np.float64)
    if P.ndim != 2 or P.shape[1] != 3 or P.shape[0] < 1:
        raise ValueError(f"points are an (M, 3) array with M >= 1 (got shape {P.shape})")
    bad = np.flatnonzero(~((P >= 0.0) & (P <= 1.0)).all(axis=1))
    if bad.size:
        m = int(bad[0])
        raise ValueError(f"a point must lie in the unit cube, every coordinate finite and in [0, 1]: point {m} is "
                         f"({P[m, 0]!r}, {P[m, 1]!r}, {P[m, 2]!r})")
    return P


def _nodal(x, N: int) -> np.ndarray:
    v = np.array(x, dtype=np.float64).reshape(-1)
    if v.size != (N + 1) ** 3:
        raise ValueError(f"vector has {v.size} entries, the level has {(N + 1) ** 3} nodes")
    return v


def diffusion_point_locate(N: int, pts):
    """The Kuhn simplex of the 3-D `diffusion_level` mesh that holds each point, as `pt_locate` (mg_diffusion_points.hip.h) finds
    it, same bits.  `pts`: (M, 3), row m = (x, y, z) in [0, 1]^3 (anything else is a ValueError that names the lowest
    offending point).  Per axis d: t = p_d * float(N), c_d = min(int(floor(t)), N - 1), xi_d = t - float(c_d) (exact; p_d = 1
    gives c_d = N - 1, xi_d = 1).  pi sorts xi in descending order, stably: on a tie the lower axis comes first.  Returns
    (nodes, weights, pi): nodes (M, 4) int64 = n0 = node(c), n1 = n0 + stride(pi0), n2 = n1 + stride(pi1), n3 = n2 + stride(pi2)
    with the strides (1, N + 1, (N + 1)^2) of x, y, z; weights (M, 4) = 1.0 - xi_pi0, xi_pi0 - xi_pi1, xi_pi1 - xi_pi2, xi_pi2;
    pi (M, 3) int64."""
    P = _points(pts)
    n1 = N + 1
    t = P * float(N)
    c = np.minimum(np.floor(t).astype(np.int64), N - 1)
    xi = t - c.astype(np.float64)
    pi = np.argsort(-xi, axis=1, kind="stable").astype(np.int64)
    s = np.take_along_axis(xi, pi, axis=1)
    stride = np.array([1, n1, n1 * n1], dtype=np.int64)[pi]
    n0 = (c[:, 2] * n1 + c[:, 1]) * n1 + c[:, 0]
    nodes = np.stack([n0, n0 + stride[:, 0], n0 + stride[:, 0] + stride[:, 1], n0 + stride[:, 0] + stride[:, 1] + stride[:, 2]], axis=1)
    lam = np.stack([1.0 - s[:, 0], s[:, 0] - s[:, 1], s[:, 1] - s[:, 2], s[:, 2]], axis=1)
    return nodes, lam, pi


def diffusion_point_sample(N: int, pts, x) -> np.ndarray:
    """S(x, pts), M values: the P1 interpolant of the nodal field `x` (lexicographic, read as it is: no mask) at the points, as
    `mg_diffusion_point_sample` computes it (same bits): out_m = ((l0 * x[n0] + l1 * x[n1]) + l2 * x[n2]) + l3 * x[n3] with
    the vertices and weights of `diffusion_point_locate`."""
    n, lam, _ = diffusion_point_locate(N, pts)
    v = _nodal(x, N)
    return ((lam[:, 0] * v[n[:, 0]] + lam[:, 1] * v[n[:, 1]]) + lam[:, 2] * v[n[:, 2]]) + lam[:, 3] * v[n[:, 3]]


def diffusion_point_gradient(N: int, pts, x) -> np.ndarray:
    """G(x, pts), (M, 3): the gradient of x_h in the simplex that holds each point, as `mg_diffusion_point_gradient` computes it
    (same bits): component pi0 = (x[n1] - x[n0]) * float(N), pi1 = (x[n2] - x[n1]) * float(N), pi2 = (x[n3] - x[n2]) * float(N)."""
    n, _, pi = diffusion_point_locate(N, pts)
    v = _nodal(x, N)
    out = np.empty((n.shape[0], 3))
    rows = np.arange(n.shape[0])
    for a in range(3):
        out[rows, pi[:, a]] = (v[n[:, a + 1]] - v[n[:, a]]) * float(N)
    return out


def _point_scatter(N: int, nodes, contrib) -> np.ndarray:
    """Every node starts at +0.0 and takes the contributions of the points in ascending point index.  `np.add.at` is unbuffered
    and walks its indices front to back, so this is a SEQUENTIAL sum over the points, one vertex column at a time; the four
    vertices of one point are distinct nodes, so the column order does not show in any node's sum."""
    out = np.zeros((N + 1) ** 3)
    np.add.at(out, nodes.reshape(-1), contrib.reshape(-1))          # index 4 m + v: ascending m
    return out


def diffusion_point_load(N: int, pts, w) -> np.ndarray:
    """S^T(w, pts), (N + 1)^3 nodes: the consistent point load sum_m w_m int delta(x - x_m) phi_i, as `mg_diffusion_point_load`
    computes it (same bits).  Point m contributes l_v * w_m to node n_v (`diffusion_point_locate`); a node starts at +0.0 and
    takes its contributions in ascending point index -- a sequential loop over the points (`np.add.at`, unbuffered, front to
    back), which is what the device's stable sort by node and one add per run reproduce.  Untouched nodes are +0.0."""
    n, lam, _ = diffusion_point_locate(N, pts)
    wv = np.array(w, dtype=np.float64).reshape(-1)
    if wv.size != n.shape[0]:
        raise ValueError(f"{n.shape[0]} points need {n.shape[0]} weights (got {wv.size})")
    return _point_scatter(N, n, lam * wv[:, None])


def diffusion_point_gradient_t(N: int, pts, p) -> np.ndarray:
    """G^T(p, pts), (N + 1)^3 nodes: the transpose of `diffusion_point_gradient` in x, as `mg_diffusion_point_gradient_t`
    computes it (same bits).  With P_a = p[m][pi_a] point m contributes (0.0 - P_0) * float(N), (P_0 - P_1) * float(N),
    (P_1 - P_2) * float(N), P_2 * float(N) to n0 .. n3; the nodes are summed as in `diffusion_point_load`: sequentially, in
    ascending point index, from +0.0."""
    n, _, pi = diffusion_point_locate(N, pts)
    pv = np.array(p, dtype=np.float64).reshape(-1)
    if pv.size != 3 * n.shape[0]:
        raise ValueError(f"{n.shape[0]} points need {3 * n.shape[0]} components (got {pv.size})")
    P = np.take_along_axis(pv.reshape(-1, 3), pi, axis=1)
    Nd = float(N)
    contrib = np.stack([(0.0 - P[:, 0]) * Nd, (P[:, 0] - P[:, 1]) * Nd, (P[:, 1] - P[:, 2]) * Nd, P[:, 2] * Nd], axis=1)
    return _point_scatter(N, n, contrib)


def diffusion_point_runs(N: int, pts):
    """What a located point set (`mg_points_create`) keeps for the transposes: the 4 M slots 4 m + v (vertex v of point m, node
    `diffusion_point_locate(N, pts)[0][m, v]`) in the STABLE order by node, and the runs of equal node in that order.  Returns
    (slot_order, run_start, run_node): slot_order (4 M,) int64, a permutation along which the nodes do not decrease and, inside
    a run, the slots -- so the point indices -- ascend; run_start (R + 1,) int64, run r being slot_order[run_start[r] :
    run_start[r + 1]], run_start[R] = 4 M; run_node (R,) int64, strictly ascending.  Adding a run's contributions front to back
    onto +0.0 is the sequential sum of `diffusion_point_load` and `diffusion_point_gradient_t`.  R and the longest run are what
    `mg_points_info` reports."""
    nodes, _, _ = diffusion_point_locate(N, pts)
    flat = nodes.reshape(-1)
    slot_order = np.argsort(flat, kind="stable").astype(np.int64)
    along = flat[slot_order]
    heads = np.flatnonzero(np.concatenate(([True], along[1:] != along[:-1])))
    run_start = np.concatenate((heads, [flat.size])).astype(np.int64)
    return slot_order, run_start, along[heads].astype(np.int64)


def diffusion_apply_dkappa(N: int, dkappa, x, rows: str = "interior", cols: str = "interior", dirichlet_faces=ALL_FACES) -> np.ndarray:
    """(dA/dkappa . dkappa) x for the 3-D `diffusion_level`: the derivative of A(kappa) x in the direction `dkappa` (N^3 values in
    the cell order of `diffusion_level`, of any sign), as `mg_diffusion_apply_dkappa` computes it.  A is linear in kappa, so an
    interior row is the row of `diffusion_level` with kappa := dkappa -- the edge sums and the diagonal sum in its order,
    weights (s / 6.0) * h, entries towards boundary neighbours zero -- applied as the device sums it: acc = 0, then
    a * x + acc over z-, y-, x-, the diagonal, x+, y+, z+.  Boundary rows are 0: the identity block does not depend on kappa.
    The same operations in the same order, but NumPy has no fma: every product here is rounded before its add, on the
    device it is not, so this restates the kernel to a rounding bound (a few ulps of the sum of the absolute values of a
    row's terms), not to the bit.  `x`: nodal values in lexicographic order, boundary entries included (an interior row has
    no boundary column, so they do not count).

    `rows`, `cols` ("interior" / "all") are the masks of `mg_diffusion_apply_dkappa_ex`, T(w, x; R, C) = M_R A^(w) M_C x with
    A^ = `diffusion_natural_matrix`.  rows = "all": a boundary row is the row of A^, summed like an interior row with a cell
    outside the grid counting as 0 and a neighbour outside it reading 0.  cols = "all" keeps the entries towards boundary
    neighbours; cols = "interior" zeroes every entry whose column is a boundary node, a boundary row's own diagonal
    included.

    `dirichlet_faces` (`face_set`): "interior" is the set of the free nodes of that face set, rows and columns alike.  A free
    row on the boundary is the row of A^ (cells outside the grid count as 0, a neighbour outside it reads 0) with the
    entries towards Dirichlet nodes zeroed; a Dirichlet row is 0 unless rows = "all".  63 is the boundary."""
    n1 = N + 1
    lo, hi = free_box(N, dirichlet_faces)
    all_faces = face_set(dirichlet_faces) == ALL_FACES
    rows_all, cols_all = _node_set_all(rows, "rows"), _node_set_all(cols, "cols")
    dk = _kappa_cells(dkappa, N, 3)
    v = np.array(x, dtype=np.float64).reshape(-1)
    if v.size != n1 ** 3:
        raise ValueError(f"vector has {v.size} entries, the level has {n1 ** 3} nodes")
    h = 1.0 / N
    se, t = _edge_sums_3d(np.pad(dk, 1, constant_values=0.0 if rows_all or not all_faces else 1.0), n1)
    idx = np.arange(n1 ** 3, dtype=np.int64)
    ijk = [idx % n1, (idx // n1) % n1, idx // (n1 * n1)]
    on_face = [(c < lo[d]) | (c > hi[d]) for d, c in enumerate(ijk)]
    inner = ~(on_face[0] | on_face[1] | on_face[2])
    strides = (1, n1, n1 * n1)
    xp = np.concatenate([np.zeros(strides[2]), v, np.zeros(strides[2])])       # a neighbour outside the grid reads 0
    nb = lambda delta: xp[strides[2] + delta:strides[2] + delta + v.size]

    def masked(axis, stepped_onto_face):
        """Is the column of the neighbour along `axis` a boundary node that `cols` masks?"""
        if cols_all:
            return np.zeros(n1 ** 3, dtype=bool)
        others = [on_face[d] for d in range(3) if d != axis]
        return stepped_onto_face | others[0] | others[1]

    acc = np.zeros(n1 ** 3)
    for axis in (2, 1, 0):                      # z-, y-, x-
        a = np.where(masked(axis, ijk[axis] - 1 < lo[axis]), 0.0, -((se[axis][0] / 6.0) * h))
        acc = a * nb(-strides[axis]) + acc
    acc = np.where(inner | cols_all, (t / 6.0) * h, 0.0) * v + acc
    for axis in (0, 1, 2):                      # x+, y+, z+
        a = np.where(masked(axis, ijk[axis] + 1 > hi[axis]), 0.0, -((se[axis][1] / 6.0) * h))
        acc = a * nb(strides[axis]) + acc
    return acc if rows_all else np.where(inner, acc, 0.0)


def diffusion_natural_matrix(N: int, cells) -> sp.csr_matrix:
    """A^(w): the natural P1 stiffness matrix of the cell field `cells` (N^3 values of any sign, cell order of `diffusion_level`)
    on all (N + 1)^3 nodes of the Kuhn mesh, lexicographic, without boundary condition.  Assembled cell by cell (vectorised
    over the cells): each of a cell's twelve axis edges e = (i, j) adds n_{c,e} w_c h / 6 to (i, i) and (j, j) and its negative
    to (i, j) and (j, i), n = 2 where the cell's two other local coordinates at the edge are equal, else 1 -- the weights of
    `diffusion_level`, whose interior block this matrix shares up to the order of the adds.  Rows sum to zero."""
    w = _kappa_cells(cells, N, 3)
    n1 = N + 1
    h = 1.0 / N
    ck, cj, ci = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    node = lambda dx, dy, dz: (((ck + dz) * n1 + (cj + dy)) * n1 + (ci + dx)).reshape(-1)
    wc = w.reshape(-1)
    lower, upper, vals = [], [], []
    for axis in range(3):
        for p in (0, 1):
            for q in (0, 1):                    # (p, q): the two other coordinates, slower one first
                if axis == 0:
                    lo, hi = (0, q, p), (1, q, p)
                elif axis == 1:
                    lo, hi = (q, 0, p), (q, 1, p)
                else:
                    lo, hi = (q, p, 0), (q, p, 1)
                lower.append(node(*lo))
                upper.append(node(*hi))
                vals.append(((2.0 if p == q else 1.0) * wc) * h / 6.0)
    i, j, we = np.concatenate(lower), np.concatenate(upper), np.concatenate(vals)
    shape = (n1 ** 3, n1 ** 3)
    above = sp.coo_matrix((-we, (i, j)), shape=shape).tocsr()       # i < j; its transpose has the same sums: A^ is symmetric to the bit
    diagonal = sp.coo_matrix((np.concatenate([we, we]), (np.concatenate([i, j]), np.concatenate([i, j]))), shape=shape).tocsr()
    A = (diagonal + above + above.T).tocsr()
    A.sort_indices()
    return A


def diffusion_lift(N: int, kappa, g, dirichlet_faces=ALL_FACES) -> np.ndarray:
    """A_IB(kappa) g_B on interior rows, 0 on boundary rows: T(kappa, g_B; interior, all) with g_B = `g` on the boundary and 0
    inside.  The right-hand side of -div(kappa grad u) = f with u = g on the boundary is f - lift on interior rows (and g on
    the identity rows), as `diffusion_level` folds `boundary_data` into its own.  With `dirichlet_faces` (`face_set`) the
    boundary is the set of its Dirichlet nodes and the interior that of its free nodes."""
    n1 = N + 1
    gv = np.array(g, dtype=np.float64).reshape(-1)
    if gv.size != n1 ** 3:
        raise ValueError(f"vector has {gv.size} entries, the level has {n1 ** 3} nodes")
    gb = np.where(dirichlet_mask(N, dirichlet_faces), gv, 0.0)
    return diffusion_apply_dkappa(N, kappa, gb, "interior", "all", dirichlet_faces)


def diffusion_eigs_reference(N: int, kappa, k: int, rho=None, dirichlet_faces=ALL_FACES, sigma=None, robin=None):
    """The `k` smallest eigenpairs of K u = lambda M(rho) u on the host: K the free block of `diffusion_level(N, 3, kappa, ...)`
    (A(kappa) + R(sigma) + B(alpha)), M(rho) = `reaction_diag(N, rho)` on the free nodes (rho = 1: None), by
    `scipy.sparse.linalg.eigsh` in shift-invert mode at 0.  Returns (lam, U): lam ascending, U of shape (k, (N + 1)^3) with
    u^T M u = 1 and +0.0 on the Dirichlet nodes.  The host statement of what `mg_eigs` computes; the sign of a vector and the
    basis of a degenerate cluster are eigsh's."""
    from scipy.sparse.linalg import eigsh
    n1 = N + 1
    free = np.flatnonzero(~dirichlet_mask(N, dirichlet_faces))
    A = diffusion_level(N, 3, kappa, dirichlet_faces=dirichlet_faces, sigma=sigma, robin=robin).A.tocsr()
    K = A[free][:, free].tocsc()
    m = reaction_diag(N, np.ones(N ** 3) if rho is None else rho, dirichlet_faces)[free]
    if not np.all(m > 0.0):
        raise ValueError("rho must be positive")
    if not 1 <= k < free.size:
        raise ValueError(f"k = {k} is outside 1..{free.size - 1}")
    v0 = np.cos(np.arange(free.size) * 0.7311 + 0.3)          # (a fixed start: the same call gives the same numbers)
    lam, V = eigsh(K, k=k, M=sp.diags(m).tocsc(), sigma=0.0, which="LM", v0=v0, tol=0)
    order = np.argsort(lam, kind="stable")
    lam, V = lam[order], V[:, order]
    V = V / np.sqrt(np.einsum("ij,i,ij->j", V, m, V))
    U = np.zeros((k, n1 ** 3))
    U[:, free] = V.T
    return lam, U


def insulated_solve_reference(N: int, kappa, f, sigma=None, robin=None, averaging: str = "arithmetic") -> np.ndarray:
    """The host statement of the insulated solve (`mg_set_diffusion_insulated`; DESIGN.md, "Insulated bodies"): u on the
    (N + 1)^3 nodes for the load `f`, with A = `diffusion_level(N, 3, kappa, dirichlet_faces=INSULATED, sigma=.., robin=..).A`.

    Regular case -- `sigma` given, or `robin` with at least one field: A is regular and u = A^-1 f, a plain sparse solve.
    Singular case -- neither: A has zero row sums.  With w = `reaction_diag(N, ones, INSULATED)` (w_i = the integral of the
    hat function) and s = w.1, u = Q A^+ Q^T f, Q = I - 1 w^T / s, the solution of the bordered system

        [[A, w], [w^T, 0]] [u; mu] = [f; 0]:       A u = f - w (1.f) / s,   w.u = 0   (mu = (1.f) / s),

    followed by u - 1 (w.u) / s, which takes the rounding of the factorisation out of w.u.

    `averaging` is the coarsening of the device hierarchy and does not enter a one-level solve; it is taken so that a call
    reads like the device's."""
    from scipy.sparse.linalg import spsolve
    if averaging not in ("arithmetic", "harmonic"):
        raise ValueError("unknown kappa averaging")
    n = (N + 1) ** 3
    fv = np.array(f, dtype=np.float64).reshape(-1)
    if fv.size != n:
        raise ValueError(f"vector has {fv.size} entries, the level has {n} nodes")
    has_robin = robin is not None and bool(_robin_fields(N, robin, _NO_FACES))
    A = diffusion_level(N, 3, kappa, dirichlet_faces=INSULATED, sigma=sigma, robin=robin if has_robin else None).A.tocsc()
    if sigma is not None or has_robin:
        return np.asarray(spsolve(A, fv)).reshape(-1)
    w = reaction_diag(N, np.ones(N ** 3), INSULATED)
    K = sp.bmat([[A, sp.csc_matrix(w.reshape(-1, 1))], [sp.csc_matrix(w.reshape(1, -1)), None]], format="csc")
    u = np.asarray(spsolve(K, np.concatenate([fv, [0.0]]))).reshape(-1)[:n]
    return u - (w @ u) / w.sum()                # (Q once more: the sparse LU leaves w.u at its own rounding, not at that of u)
