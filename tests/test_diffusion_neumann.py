"""No-flux (Neumann) faces of the diffusion solves (mg_set_diffusion_faces): only the faces of the set carry the Dirichlet
condition, every other node is a free node with the natural P1 row.  The host restatements of poisson.py against the natural
matrix, the stored level against its restatement, the matrix-free march against the stored level, the P1-transpose
restriction, the sensitivity operators with "interior" = the free nodes, mg_pcg against spsolve, DiffusionSolver against a
host adjoint (tests/diffusion_neumann_workers.py), the default set leaving everything as it was, and the refusals."""
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from multigrid_dolfinx_amd import poisson
from tests.diffusion_neumann_workers import FACE_SETS, free_mask
from tests.diffusion_workers import lognormal_kappa

EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEUMANN_SETS = tuple(s for s in FACE_SETS if s != 63)
KERNEL_N = (8, 36, 72, 128)     # smaller than a 64 x 8 tile; partial tiles; a second tile column; several z segments
PAIRS = [(r, c) for r in ("interior", "all") for c in ("interior", "all")]
# the stored handle's one-step kernel whose bits the matrix-free march carries (tests/test_diffusion_mf.py)
STORED_ONE_STEP = {"row_classes": 0, "fuse_sweeps": 0}


@functools.lru_cache(maxsize=None)
def _kappa(N):
    return lognormal_kappa(N, 3, seed=3)


@functools.lru_cache(maxsize=8)
def _host_level(N, faces):
    return poisson.diffusion_level(N, 3, _kappa(N), dirichlet_faces=faces)


def _csr_bytes(A):
    A = A.tocsr()
    return A.indptr.tobytes(), A.indices.tobytes(), A.data.tobytes()


# ---- host ---------------------------------------------------------------------------------------------------------------------
def test_face_set_names_and_boxes():
    assert poisson.face_set(None) == 63 and poisson.face_set(("x-", "x+", "y-", "y+", "z-", "z+")) == 63
    assert poisson.face_set(("x+", "z-")) == 18 and poisson.face_set(12) == 12
    assert poisson.free_box(8, 63) == ([1, 1, 1], [7, 7, 7]) and poisson.free_box(8, 18) == ([0, 0, 1], [7, 8, 8])
    for bad in (0, 64, -1, ("w-",)):
        with pytest.raises(ValueError):
            poisson.face_set(bad)
    with pytest.raises(ValueError, match="3-D only"):
        poisson.diffusion_level(4, 2, np.ones(16), dirichlet_faces=1)
    m = poisson.dirichlet_mask(4, 1).reshape(5, 5, 5)
    assert m[:, :, 0].all() and not m[:, :, 1:].any()


@pytest.mark.parametrize("dim,N", [(2, 6), (3, 6), (3, 8)])
@pytest.mark.parametrize("keep_zeros", [True, False])
def test_default_set_is_the_level_without_the_keyword(dim, N, keep_zeros):
    kappa = lognormal_kappa(N, dim, seed=3)
    a = poisson.diffusion_level(N, dim, kappa, keep_zeros)
    for faces in (63, None):
        b = poisson.diffusion_level(N, dim, kappa, keep_zeros, dirichlet_faces=faces)
        assert _csr_bytes(a.A) == _csr_bytes(b.A) and a.b.tobytes() == b.b.tobytes()


def _simplices_at_nodes(N):
    """T by enumeration: the six Kuhn simplices of every cell are the paths 0 -> e_p -> e_p + e_q -> (1,1,1)."""
    n1 = N + 1
    T = np.zeros((n1, n1, n1))
    ck, cj, ci = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    for perm in itertools.permutations(range(3)):
        v = [0, 0, 0]
        corners = [tuple(v)]
        for axis in perm:
            v[axis] = 1
            corners.append(tuple(v))
        for dx, dy, dz in corners:
            np.add.at(T, (ck + dz, cj + dy, ci + dx), 1.0)
    return T.reshape(-1)


@pytest.mark.parametrize("N", [6, 8])
@pytest.mark.parametrize("faces", NEUMANN_SETS)
def test_level_against_the_natural_matrix(N, faces):
    """The free block is that of A^(kappa) up to the order of the adds: per entry within 4 eps times the sum of the absolute
    values of its terms (four cell terms per edge, twenty-four on the diagonal, each rounded once; A^(|kappa|) holds those
    sums); symmetric bit for bit; Dirichlet rows are identity rows and no free row keeps a Dirichlet column; the right-hand side
    is the load of the simplices inside the grid less A^_FD g_D."""
    kappa = _kappa(N)
    L = _host_level(N, faces)
    free = free_mask(N, faces)
    A, Ahat = L.A.tocsr(), poisson.diffusion_natural_matrix(N, kappa)
    AF, HF = A[free][:, free], Ahat[free][:, free]
    bound = 4 * EPS * abs(HF)
    assert (abs(AF - HF) - bound).max() <= 0.0
    assert abs(AF - HF).max() > 0.0 or N < 3          # (the orders do differ: the comparison is not of a matrix with itself)
    assert (AF != AF.T).nnz == 0
    assert (A[~free] != sp.identity(A.shape[0], format="csr")[~free]).nnz == 0
    assert abs(A[free][:, ~free]).sum() == 0.0
    g = poisson.boundary_data(L.coords, 3)
    load = -12.0 * (1.0 / N) ** 3 * _simplices_at_nodes(N) / 24.0
    FD = Ahat[free][:, ~free]
    want = load[free] - FD @ g[~free]
    slack = 8 * EPS * (abs(load[free]) + abs(FD) @ abs(g[~free]))
    assert np.all(np.abs(L.b.reshape(-1)[free] - want) <= slack)
    assert np.array_equal(L.b.reshape(-1)[~free], g[~free])
    lift = poisson.diffusion_lift(N, kappa, g, faces)
    assert np.all(np.abs(lift[free] - FD @ g[~free]) <= slack) and not lift[~free].any()


def _face_flux_load(N, grad, faces):
    """The load of the flux q = grad . n of a linear function on the no-flux faces of the set: q times the integral of phi_i
    over the face, (h^2 / 6) times the number of the face's triangles at the node (every boundary square is cut along its
    (0,0)-(1,1) diagonal: two triangles at those corners, one at the others)."""
    n1, h = N + 1, 1.0 / N
    load = np.zeros((n1, n1, n1))           # [z, y, x]
    tri = np.zeros((n1, n1))
    for a in (0, 1):
        for b in (0, 1):
            tri[a:a + N, b:b + N] += 2.0 if a == b else 1.0     # the squares whose corner (a, b) the node is
    for axis in range(3):
        for side in (0, 1):
            if faces >> (2 * axis + side) & 1:
                continue
            q = grad[axis] * (1.0 if side else -1.0)
            index = [slice(None)] * 3
            index[2 - axis] = N if side else 0
            load[tuple(index)] += q * (h * h / 6.0) * tri
    return load.reshape(-1)


@pytest.mark.parametrize("N", [6, 8])
@pytest.mark.parametrize("faces", NEUMANN_SETS)
def test_linear_solution_is_reproduced(N, faces):
    """kappa = 1, f = 0, u = 1 + 2 x - 3 y + z / 2: Dirichlet data on the faces of the set, its flux as load on the others.  P1
    reproduces linears, so spsolve returns u up to cond(A) eps (cond computed densely)."""
    L = poisson.diffusion_level(N, 3, np.ones(N ** 3), dirichlet_faces=faces)
    grad = (2.0, -3.0, 0.5)
    u = 1.0 + L.coords @ np.array(grad)
    free = free_mask(N, faces)
    rhs = np.where(free, _face_flux_load(N, grad, faces) - poisson.diffusion_lift(N, np.ones(N ** 3), u, faces), u)
    x = spl.spsolve(L.A.tocsc(), rhs)
    cond = np.linalg.cond(L.A.toarray())
    print("faces", faces, "N", N, "cond", cond, "error", np.abs(x - u).max() / np.abs(u).max())
    assert np.linalg.norm(x - u) <= cond * EPS * np.linalg.norm(u)


def _abs_natural(N, w):
    return abs(poisson.diffusion_natural_matrix(N, np.abs(w)))


@pytest.mark.parametrize("faces", NEUMANN_SETS)
def test_adjoint_identities_of_the_restatements(faces):
    """w . D(a, x; R, C) = a . T(w, x; R, C) and y . T(w, x; R, C) = x . T(w, y; C, R) with "interior" = the free nodes of the
    set, to 64 eps |a|^T |A^(|w|)| |x|; and T and D with a masked vector are those of the vector zeroed on the Dirichlet nodes."""
    N = 6
    rng = np.random.default_rng(5)
    n = (N + 1) ** 3
    a, x, y, w = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(N ** 3)
    free = free_mask(N, faces)
    M = _abs_natural(N, w)
    for R, Cn in PAIRS:
        D = poisson.diffusion_dkappa(N, a, x, R, Cn, faces)
        T = poisson.diffusion_apply_dkappa(N, w, x, R, Cn, faces)
        assert abs(w @ D - a @ T) <= 64 * EPS * (np.abs(a) @ (M @ np.abs(x)))
        Tt = poisson.diffusion_apply_dkappa(N, w, y, Cn, R, faces)
        assert abs(y @ T - x @ Tt) <= 64 * EPS * (np.abs(y) @ (M @ np.abs(x)))
        am = a if R == "all" else np.where(free, a, 0.0)
        xm = x if Cn == "all" else np.where(free, x, 0.0)
        assert np.array_equal(D, poisson.diffusion_dkappa(N, am, xm, "all", "all", faces))
        full = poisson.diffusion_apply_dkappa(N, w, xm, "all", "all", faces)
        assert np.allclose(T, full if R == "all" else np.where(free, full, 0.0), rtol=0, atol=64 * EPS * (M @ np.abs(x)).max())
        if R == "interior":
            assert not T[~free].any()
    # and against the natural matrix itself
    want = poisson.diffusion_natural_matrix(N, w) @ x
    got = poisson.diffusion_apply_dkappa(N, w, x, "all", "all", faces)
    assert np.all(np.abs(got - want) <= 16 * EPS * (M @ np.abs(x)))


# ---- device -------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.tobytes() == b.tobytes()


_INFO = ("n_global", "nnz_stored", "nnz_nonzero", "ell_width", "offset_codes", "symmetric_diagonals", "row_classes")


def _outputs(h, l, v, f):
    out = [h.get_vector(l, "f")]
    h.set_vector(l, "v", v)
    h.set_vector(l, "f", f)
    h.residual(l)
    out.append(h.get_vector(l, "r"))
    h.smooth(l, 1)
    out.append(h.get_vector(l, "v"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("N", KERNEL_N)
@pytest.mark.parametrize("faces", FACE_SETS)
def test_device_level_equals_host_restatement(faces, N):
    """As tests/test_diffusion.py compares them: the generated level against a handle fed the host restatement's CSR -- the
    same storage figures, F to the bit, and residual and one sweep to the bit."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    host = _host_level(N, faces)
    with DeviceHierarchy(3, 0, 1, c=N // 2) as d, DeviceHierarchy(3, 0, 1, c=N // 2) as s:
        d.set_diffusion_faces(faces)
        assert d.diffusion_faces() == faces
        d.gen_diffusion_level(1, _kappa(N))
        s.set_level(1, host.A, prune_zeros=True)
        for h in (d, s):
            h.set_params(2, 2, 2.0 / 3.0)
        assert {k: d.level_info(1)[k] for k in _INFO} == {k: s.level_info(1)[k] for k in _INFO}
        sd, ss = d.level_storage(1), s.level_storage(1)
        assert sd["symmetric"] == 1 and sd["max_pair_ulps"] == 0 and ss["symmetric"] == 1
        assert _same(d.get_vector(1, "f"), host.b)
        rng = np.random.default_rng(11)
        v, f = rng.standard_normal(d.n_dofs(1)), host.b.reshape(-1)
        a, b = _outputs(d, 1, v, f), _outputs(s, 1, v, f)
        for x, y in zip(a[1:], b[1:]):
            assert _same(x, y)
        r = f - host.A @ v
        assert np.linalg.norm(a[1].reshape(-1) - r) <= 1e-14 * np.linalg.norm(r)


@pytest.mark.gpu
@pytest.mark.parametrize("N", KERNEL_N)
@pytest.mark.parametrize("faces", FACE_SETS)
def test_matrix_free_bits_against_the_stored_level(faces, N):
    """F, the residual, one Jacobi sweep, Chebyshev steps and the SpMV of the matrix-free level: the bytes of the stored level's
    one-step kernel.  The SpMV's dot is summed per workgroup, so it agrees to the worst-case bound of two summation orders,
    2 n eps sum |x_i (A x)_i|.  The launch counts say which kernels ran."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    kappa = _kappa(N)
    with DeviceHierarchy(3, 0, 1, c=N // 2, **STORED_ONE_STEP) as s, DeviceHierarchy(3, 0, 1, c=N // 2) as m:
        for h in (s, m):
            h.set_diffusion_faces(faces)
        s.gen_diffusion_level(1, kappa)
        m.gen_diffusion_level(1, kappa, matrix_free=True)
        assert m.level_matrix_free(1) and not s.level_matrix_free(1)
        assert s.level_info(1)["nnz_nonzero"] == m.level_info(1)["nnz_nonzero"]
        assert _same(s.get_vector(1, "f"), m.get_vector(1, "f"))
        rng = np.random.default_rng(11)
        v, f = rng.standard_normal(s.n_dofs(1)), rng.standard_normal(s.n_dofs(1))
        for smoother, sweeps in (("jacobi", (1,)), ("chebyshev", (1, 2))):
            for h in (s, m):
                h.set_params(2, 2, 2.0 / 3.0, smoother=smoother)
                h.set_chebyshev_bounds(1, 0.25, 2.125)
                h.reset_smoother_launches()
            for nw in sweeps:
                got = []
                for h in (s, m):
                    h.set_vector(1, "v", v)
                    h.set_vector(1, "f", f)
                    h.residual(1)
                    r = h.get_vector(1, "r")
                    h.smooth(1, nw)
                    got.append((r, h.get_vector(1, "v")))
                assert np.all(np.isfinite(got[0][1]))
                assert np.array_equal(got[0][0], got[1][0]), (smoother, nw, "residual")
                assert np.array_equal(got[0][1], got[1][1]), (smoother, nw, np.flatnonzero(got[0][1] != got[1][1])[:5])
            total = sum(sweeps)
            assert s.smoother_launches(1) == {"slice": (total, total, 0)}
            assert m.smoother_launches(1) == {"matrix_free": (total, total, 0)}
        spmv = []
        for h in (s, m):
            h.set_vector(1, "v", v)
            spmv.append((h.quadratic_form(1, "v"), h.get_vector(1, "r")))
        assert np.array_equal(spmv[0][1], spmv[1][1])
        terms = np.abs(v * spmv[0][1].reshape(-1)).sum()
        print("x . A x stored / matrix-free:", spmv[0][0], spmv[1][0])
        assert abs(spmv[0][0] - spmv[1][0]) <= 2 * v.size * EPS * terms
        assert abs(spmv[0][0] - v @ spmv[0][1].reshape(-1)) <= 2 * v.size * EPS * terms


_KUHN = [o for o in poisson.kuhn_offsets(3)]


def _restrict_numpy(r, Nc, faces):
    """restrict_p1t with a face set: a free coarse node sums w * r[2 I + d] over the Kuhn pattern in ascending fine
    lexicographic order, w = 1 for d = 0 and 0.5 otherwise, multiply then add, offsets outside the grid skipped; a Dirichlet
    coarse node takes the coincident fine value."""
    nf, nc = 2 * Nc + 1, Nc + 1
    rf = np.pad(r.reshape(nf, nf, nf), 1)                   # [z, y, x]; (the pad is never added: masked below)
    K, J, I = np.meshgrid(np.arange(nc), np.arange(nc), np.arange(nc), indexing="ij")
    out = None
    started = np.zeros((nc, nc, nc), dtype=bool)
    for di, dj, dk in _KUHN:
        fi, fj, fk = 2 * I + di, 2 * J + dj, 2 * K + dk
        inside = (fi >= 0) & (fi < nf) & (fj >= 0) & (fj < nf) & (fk >= 0) & (fk < nf)
        term = (1.0 if (di, dj, dk) == (0, 0, 0) else 0.5) * rf[fk + 1, fj + 1, fi + 1]
        if out is None:
            out = np.where(inside, term, 0.0)
        else:
            out = np.where(inside, np.where(started, out + term, term), out)
        started |= inside
    free = free_mask(Nc, faces).reshape(nc, nc, nc)
    return np.where(free, out, r.reshape(nf, nf, nf)[::2, ::2, ::2]).reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("N", KERNEL_N)
@pytest.mark.parametrize("faces", FACE_SETS)
def test_restriction_with_a_face_set(faces, N):
    """MG_RESTRICT_P1_TRANSPOSE between levels generated with the set: the NumPy restatement to the bit, and
    <P e, r> = <e, P^T r> over the free nodes (e zero on the Dirichlet nodes) to 64 eps times the sum of the absolute values of
    the terms, <P |e|, |r|>."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    Nc = N // 2
    kappa = _kappa(N)
    with DeviceHierarchy(3, 0, 1, c=Nc) as h:
        h.set_diffusion_faces(faces)
        h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
        h.set_prolongation("p1")
        h.gen_diffusion_hierarchy(kappa)
        rng = np.random.default_rng(7)
        r = rng.standard_normal(h.n_dofs(1))
        e = np.where(free_mask(Nc, faces), rng.standard_normal(h.n_dofs(0)), 0.0)
        h.set_vector(1, "r", r)
        h.restrict(1, "p1_transpose")
        got = h.get_vector(0, "f").reshape(-1)
        assert _same(got, _restrict_numpy(r, Nc, faces))
        Pe = []
        for x in (e, np.abs(e)):
            h.set_vector(0, "v", x)
            h.prolong(1, add=False)
            Pe.append(h.get_vector(1, "err").reshape(-1))
        fine_free = free_mask(N, faces)
        assert not Pe[0][~fine_free].any()
        lhs, rhs = Pe[0][fine_free] @ r[fine_free], e @ got
        assert abs(lhs - rhs) <= 64 * EPS * (Pe[1] @ np.abs(r))


def _row_terms(N, w, x, rows, cols, faces):
    """The seven products a row of M_rows A^(w) M_cols x sums, M the mask of the free nodes of the set ("interior") or the
    identity ("all"): tests/diffusion_dirichlet_workers.natural_row_terms with that mask."""
    from tests.diffusion_dirichlet_workers import _EDGES
    n1, h = N + 1, 1.0 / N
    free = free_mask(N, faces).astype(np.float64)
    mask = lambda nodes: free if nodes == "interior" else np.ones(n1 ** 3)
    se, t = poisson._edge_sums_3d(np.pad(np.asarray(w, dtype=np.float64).reshape(N, N, N), 1, constant_values=0.0), n1)
    xm = np.asarray(x, dtype=np.float64).reshape(-1) * mask(cols)
    idx = np.arange(n1 ** 3, dtype=np.int64)
    ijk = [idx % n1, (idx // n1) % n1, idx // (n1 * n1)]
    strides = (1, n1, n1 * n1)
    xp = np.concatenate([np.zeros(strides[2]), xm, np.zeros(strides[2])])
    terms = [((t / 6.0) * h) * xm]
    for axis, side in _EDGES:
        delta = strides[axis] if side else -strides[axis]
        outside = ijk[axis] + 1 > N if side else ijk[axis] - 1 < 0
        terms.append(-((se[axis][side] / 6.0) * h) * np.where(outside, 0.0, xp[strides[2] + delta:strides[2] + delta + xm.size]))
    return np.array(terms) * mask(rows)


def _row_bound(N, w, x, rows, cols, faces):
    """tests/diffusion_tangent_workers.row_bound, evaluated with the free-node mask: 16 eps times the sum of the absolute values
    of a row's seven products, taken on |w| and |x|."""
    return 16 * EPS * np.abs(_row_terms(N, np.abs(w), np.abs(x), rows, cols, faces)).sum(axis=0)


@pytest.mark.gpu
@pytest.mark.parametrize("N", KERNEL_N)
@pytest.mark.parametrize("faces", FACE_SETS)
def test_sensitivities_with_a_face_set(faces, N):
    """mg_diffusion_dkappa[_ex] (march and gather) to the bit of its restatement; the tangent within the per-row bound; T(kappa,
    x; interior, interior) with the bits of the negated residual of kappa's level on the free rows; and both adjoint identities
    with both sides from the device."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    kappa = _kappa(N)
    rng = np.random.default_rng(13)
    n = (N + 1) ** 3
    a, x, y, w = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(N ** 3)
    free = free_mask(N, faces)
    with DeviceHierarchy(3, 0, 1, c=N // 2, **STORED_ONE_STEP) as h:
        h.set_diffusion_faces(faces)
        h.gen_diffusion_level(1, kappa)
        for R, Cn in PAIRS:
            want = poisson.diffusion_dkappa(N, a, x, R, Cn, faces)
            for gather in (0, 1):
                h.set_tuning("dkappa_gather", gather)
                assert _same(h.diffusion_dkappa(1, a, x, a_nodes=R, b_nodes=Cn), want), (R, Cn, gather)
            D = h.diffusion_dkappa(1, a, x, a_nodes=R, b_nodes=Cn)
            T = h.diffusion_apply_dkappa(1, w, x, rows=R, cols=Cn)
            bound = _row_bound(N, w, x, R, Cn, faces)
            assert np.all(np.abs(T - poisson.diffusion_apply_dkappa(N, w, x, R, Cn, faces)) <= bound), (R, Cn)
            if R == "interior":
                assert not T[~free].any()
            terms = np.abs(a) @ (bound / (16 * EPS))
            assert abs(w @ D - a @ T) <= 64 * EPS * terms, (R, Cn)
            Tt = h.diffusion_apply_dkappa(1, w, y, rows=Cn, cols=R)
            assert abs(y @ T - x @ Tt) <= 64 * EPS * (np.abs(y) @ (bound / (16 * EPS))), (R, Cn)
        assert _same(h.diffusion_dkappa(1, a, x), poisson.diffusion_dkappa(N, a, x, dirichlet_faces=faces))
        h.set_params(2, 2, 2.0 / 3.0)
        h.set_vector(1, "v", x)
        h.set_vector(1, "f", np.zeros(n))
        h.residual(1)
        r = h.get_vector(1, "r").reshape(-1)
        T = h.diffusion_apply_dkappa(1, kappa, x)
        assert np.array_equal(T[free], -r[free])


@functools.lru_cache(maxsize=None)
def _host_solution(N, faces):
    """(A^-1 b, cond(A)) of the restated level: one SuperLU factorisation (what spsolve runs; minimum-degree ordering on
    A^T + A, a quarter of the default ordering's fill on these 3-D levels) serves the solve and, as the shift-invert operator
    of Lanczos, lambda_min; lambda_max by Lanczos on A.  The level is symmetric positive definite, identity rows included."""
    host = _host_level(N, faces)
    A = host.A.tocsc()
    A.eliminate_zeros()
    lu = spl.splu(A, permc_spec="MMD_AT_PLUS_A")
    lo = spl.eigsh(A, k=1, sigma=0.0, which="LM", return_eigenvectors=False, OPinv=spl.LinearOperator(A.shape, matvec=lu.solve))[0]
    hi = spl.eigsh(A, k=1, which="LA", return_eigenvectors=False)[0]
    return lu.solve(host.b.reshape(-1)), float(hi / lo)


@pytest.mark.gpu
@pytest.mark.parametrize("N,nlev", [(16, 3), (32, 4)])
@pytest.mark.parametrize("faces", [1, 18])
def test_pcg_with_a_face_set_against_spsolve(faces, N, nlev):
    """mg_pcg on generated hierarchies, stored and matrix-free, log-normal kappa: rtol 1e-10 within DiffusionSolver's max_iter
    (200), and the solution within cond(A) rtol of the sparse direct solve of the restated level in relative l2, cond computed
    on the host for this N.  The iteration counts are printed beside those of the default set, which only iterates here."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    rtol, top = 1e-10, nlev - 1
    kappa = _kappa(N)
    counts = {}
    for set_ in (faces, 63):
        host = _host_level(N, set_)
        f = host.b.reshape(-1)
        for name, min_rows in (("stored", None), ("matrix_free", 0)):
            with DeviceHierarchy(3, 0, top, c=N >> top) as h:
                h.set_diffusion_faces(set_)
                h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
                h.set_prolongation("p1")
                h.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=min_rows)
                assert h.level_matrix_free(top) == (name == "matrix_free")
                assert _same(h.get_vector(top, "f"), host.b)
                h.zero_vector(top, "v")
                hist = h.pcg(rtol=rtol, max_iter=200, level=top)
                x = h.get_vector(top, "v").reshape(-1)
            assert len(hist) < 200 and hist[-1] <= rtol * np.linalg.norm(f)
            counts[(set_, name)] = len(hist)
            if set_ == 63:
                continue
            want, cond = _host_solution(N, set_)
            err = np.linalg.norm(x - want) / np.linalg.norm(want)
            print("faces", set_, name, "N", N, "iterations", len(hist), "cond %.3e" % cond, "rel l2 error %.3e" % err)
            assert err <= cond * rtol
    print("iterations (face set, storage):", counts)


def _snapshot(h, top, f):
    out = [h.get_vector(l, "f").tobytes() for l in range(top + 1)]
    out += [repr(sorted(h.level_info(l).items())) for l in range(top + 1)]
    rng = np.random.default_rng(3)
    v = rng.standard_normal(h.n_dofs(top))
    h.set_vector(top, "v", v)
    h.set_vector(top, "f", f)
    h.residual(top)
    out.append(h.get_vector(top, "r").tobytes())
    h.smooth(top, 1)
    out.append(h.get_vector(top, "v").tobytes())
    h.zero_vector(top, "v")
    out.append(h.pcg(rtol=1e-9, max_iter=50, level=top).tobytes())
    out.append(h.get_vector(top, "v").tobytes())
    return out, h.memory_bytes(), [h.smoother_launches(l) for l in range(top + 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("min_rows", [None, 0])
def test_default_set_changes_nothing(min_rows):
    """A handle that sets all six faces and one that never calls the entry: levels, residual, one sweep and a pcg history and
    iterate byte for byte, mg_memory_bytes and mg_smoother_launches equal."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N, top = 32, 2
    kappa = _kappa(N)
    f = np.random.default_rng(9).standard_normal((N + 1) ** 3)
    got = []
    for call in (False, True):
        with DeviceHierarchy(3, 0, top, c=N >> top) as h:
            if call:
                h.set_diffusion_faces(("x-", "x+", "y-", "y+", "z-", "z+"))
            assert h.diffusion_faces() == 63
            h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
            h.set_prolongation("p1")
            h.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=min_rows)
            got.append(_snapshot(h, top, f))
    assert got[0][0] == got[1][0]
    assert got[0][1] == got[1][1]
    assert got[0][2] == got[1][2]


def _refused(call, text):
    from multigrid_dolfinx_amd._capi import MgError
    with pytest.raises(MgError, match=text):
        call()


def _untouched(h, call, text, vectors=()):
    """`call` is refused with `text`; counters() and the given (level, name, bytes) vectors are as they were."""
    before = h.counters()
    faces = h.diffusion_faces()
    _refused(call, text)
    assert h.counters() == before and h.diffusion_faces() == faces
    for level, name, want in vectors:
        assert h.get_vector(level, name).tobytes() == want, (level, name)


@pytest.mark.gpu
def test_refusals_leave_the_handle_as_it_was():
    """Every refusal by message; counters(), the face set and, where the handle has levels, V and F unchanged by it."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N, top = 16, 2
    kappa = _kappa(N)
    nothing = lambda *args: None
    with DeviceHierarchy(2, 0, 1, c=4) as h2:
        _untouched(h2, lambda: h2.set_diffusion_faces(3), "3-D only")
        h2.set_diffusion_faces(63)
        assert h2.diffusion_faces() == 63
    with DeviceHierarchy(3, 0, 1, c=4) as slab:
        slab.set_comm_callbacks(0, 2, nothing, nothing, nothing)
        _untouched(slab, lambda: slab.set_diffusion_faces(3), "whole \\(not slab\\) handle")
        slab.set_diffusion_faces(63)
        assert slab.diffusion_faces() == 63
    with DeviceHierarchy(3, 0, 1, c=4) as late:         # a slab handle made after the set was set: refused where the set is read
        late.set_diffusion_faces(18)
        late.set_comm_callbacks(0, 2, nothing, nothing, nothing)
        _untouched(late, lambda: late.gen_diffusion_level(1, _kappa(8)), "face set 18 .*whole \\(not slab\\) handle")
        _untouched(late, lambda: late.gen_diffusion_level(1, _kappa(8), matrix_free=True), "whole \\(not slab\\) handle")
    with DeviceHierarchy(3, 0, top, c=N >> top) as h:
        h.set_diffusion_faces(18)
        h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
        h.set_prolongation("p1")
        h.gen_diffusion_hierarchy(kappa)
        v = np.random.default_rng(1).standard_normal(h.n_dofs(top))
        h.set_vector(top, "v", v)
        state = [(top, "v", v.tobytes()), (top, "f", h.get_vector(top, "f").tobytes()), (top - 1, "f", h.get_vector(top - 1, "f").tobytes())]
        untouched = lambda call, text: _untouched(h, call, text, state)
        untouched(lambda: h.set_diffusion_faces(0), "singular")
        untouched(lambda: h.set_diffusion_faces(64), "no face set")
        untouched(lambda: h.set_diffusion_faces(-1), "no face set")
        # the transfers: anything but the P1 prolongation with its transpose, in cycles and in single calls
        for restriction, prolongation in (("direct", "p1"), ("full_weighting", "p1"), ("p1_transpose", "q1")):
            h.set_params(2, 2, 2.0 / 3.0, restriction=restriction)
            h.set_prolongation(prolongation)
            untouched(lambda: h.vcycle(top, 1), "P1 transfers")
            untouched(lambda: h.prepare_cycle(top), "P1 transfers")
            untouched(lambda: h.fmg(1), "P1 transfers")
            untouched(lambda: h.pcg(level=top), "P1 transfers")
            if restriction != "p1_transpose":
                untouched(lambda: h.restrict(top, restriction), "P1 transfers")
            if prolongation != "p1":
                untouched(lambda: h.prolong(top), "P1 transfers")
        h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
        h.set_prolongation("p1")
        untouched(lambda: h.galerkin_level(top), "mg_galerkin_level.*face set 18")
        # a refresh under another set
        h.set_diffusion_faces(63)
        untouched(lambda: h.refresh_diffusion_hierarchy(kappa), "generated with the face set 18")
        h.set_diffusion_faces(18)
        h.refresh_diffusion_hierarchy(kappa)
        assert h.get_vector(top, "f").tobytes() == state[1][2]
        h.zero_vector(top, "v")
        assert len(h.pcg(rtol=1e-8, max_iter=100, level=top)) < 100
        # levels of two sets in one cycle or one transfer
        h.set_diffusion_faces(1)
        h.gen_diffusion_level(top, kappa)
        h.set_vector(top, "v", v)
        state = [(top, "v", v.tobytes()), (top, "f", h.get_vector(top, "f").tobytes()), (top - 1, "f", h.get_vector(top - 1, "f").tobytes())]
        untouched(lambda: h.vcycle(top, 1), "different face sets")
        untouched(lambda: h.pcg(level=top), "different face sets")
        untouched(lambda: h.restrict(top, "p1_transpose"), "different face sets")
        untouched(lambda: h.prolong(top), "different face sets")


def _torch_first(worker):
    code = "import torch, sys; sys.path.insert(0, %r); import tests.diffusion_neumann_workers as w; w.%s()" % (ROOT, worker)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.gpu
def test_diffusion_solver_with_no_flux_faces_against_the_host():
    """DiffusionSolver with dirichlet_faces = ("x-", "x+") and ("z+",), N = 16, stored and matrix-free: u, the gradients with
    respect to kappa, f and g and a Hessian-vector product against the host adjoint built on spsolve, n_solves 2 and 4, the
    gradient of g zero off the Dirichlet nodes (`solver_worker`, whose NEUMANN_LIMIT holds the measured figures)."""
    assert "solver ok" in _torch_first("solver_worker")
