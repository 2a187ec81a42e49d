"""Robin (convective) faces of the diffusion solves (mg_set_diffusion_robin): kappa du/dn + alpha (u - u_ext) = 0 on faces
outside the Dirichlet set, as the lumped boundary diagonal B(alpha).  The host restatements of poisson.py against an enumeration
of the boundary triangles of the Kuhn simplices, the stored level against its restatement, the matrix-free march (B folded into
the level's nodal diagonal term) against the stored level, alpha == 0 and cleared fields changing
nothing, mg_pcg against a sparse direct solve, the refresh path, the two sensitivity kernels, the refusals, the timing names,
and DiffusionSolver with Robin fields against host adjoints (tests/diffusion_robin_workers.py)."""
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
from tests.diffusion_neumann_workers import free_mask
from tests.diffusion_reaction_workers import reaction_sigma
from tests.diffusion_robin_workers import CONFIGS, robin_alpha, robin_fields
from tests.diffusion_workers import lognormal_kappa

EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_N = (8, 36, 72)          # 9^3 nodes: part of one 64 x 8 tile; 37^3: the y tiles; 73^3: the x+ face lies in the second x tile
# the stored handle's one-step kernel whose bits the matrix-free march carries (tests/test_diffusion_mf.py)
STORED_ONE_STEP = {"row_classes": 0, "fuse_sweeps": 0}
# (the march splits z into segments of at least sixteen planes where that fills the device better: 37 and 73 planes run in
# more than one segment)


@functools.lru_cache(maxsize=None)
def _kappa(N):
    return lognormal_kappa(N, 3, seed=3)


@functools.lru_cache(maxsize=None)
def _sigma(N):
    return reaction_sigma(N)


def _robin(N, config, seed=0):
    return robin_fields(N, CONFIGS[config][1], seed)


@functools.lru_cache(maxsize=8)
def _host_level(N, config, react=False, robin=True):
    return poisson.diffusion_level(N, 3, _kappa(N), dirichlet_faces=CONFIGS[config][0], sigma=_sigma(N) if react else None,
                                   robin=_robin(N, config) if robin else None)


def _csr_bytes(A):
    A = A.tocsr()
    return A.indptr.tobytes(), A.indices.tobytes(), A.data.tobytes()


def _same(a, b):
    return a.tobytes() == b.tobytes()


# ---- host ---------------------------------------------------------------------------------------------------------------------
def _boundary_mass_by_triangles(N, robin):
    """(B(alpha), the same sum over |alpha|) at all (N + 1)^3 nodes by enumeration, and the set of diagonals found: the six Kuhn
    simplices of a cell are the paths 0 -> e_p -> e_p + e_q -> (1,1,1); a triangle of a simplex lies in a face of the cell if
    its three vertices share a coordinate; on a boundary cell it is a boundary triangle of area h^2 / 2, and the row-sum lumped
    P1 boundary mass gives each of its three vertices |T| / 3 times the face-cell's alpha."""
    n1, h = N + 1, 1.0 / N
    B, S = np.zeros((n1, n1, n1)), np.zeros((n1, n1, n1))
    diagonals = set()
    for perm in itertools.permutations(range(3)):
        v = [0, 0, 0]
        corners = [tuple(v)]
        for axis in perm:
            v[axis] = 1
            corners.append(tuple(v))
        for tri in itertools.combinations(corners, 3):
            for axis in range(3):
                for side in (0, 1):
                    if any(c[axis] != side for c in tri):
                        continue
                    a, b = [d for d in range(3) if d != axis]
                    # the edge of the triangle that is no edge of the square is the diagonal the split cuts along
                    for p, q in itertools.combinations(tri, 2):
                        if p[a] != q[a] and p[b] != q[b]:
                            diagonals.add(frozenset(((p[a], p[b]), (q[a], q[b]))))
                    bit = 1 << (2 * axis + side)
                    if bit not in robin:
                        continue
                    alpha = np.asarray(robin[bit]).reshape(N, N)
                    for cb in range(N):
                        for ca in range(N):
                            cell = [0, 0, 0]
                            cell[axis], cell[a], cell[b] = (N - 1 if side else 0), ca, cb
                            for c in tri:
                                node = (cell[2] + c[2], cell[1] + c[1], cell[0] + c[0])
                                B[node] += alpha[cb, ca] * (h * h / 2.0) / 3.0
                                S[node] += abs(alpha[cb, ca]) * (h * h / 2.0) / 3.0
    return B.reshape(-1), S.reshape(-1), diagonals


@pytest.mark.parametrize("N", [4, 6])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_robin_diag_against_the_kuhn_boundary_triangles(config, N):
    """Every boundary face-cell is cut along the diagonal from its in-plane (0,0) to its (1,1) corner; robin_diag is within
    12 eps of the sum of the absolute values of its (at most 18) triangle terms of the enumeration on free nodes, +0.0 on
    Dirichlet nodes and off the field faces; alpha == 1 on a face sums to the face's area; the level with the fields is the
    level without plus diag(B) on the free rows and nothing else, symmetric to the bit."""
    faces, fields = CONFIGS[config]
    robin = _robin(N, config)
    want, terms, diagonals = _boundary_mass_by_triangles(N, robin)
    assert diagonals == {frozenset(((0, 0), (1, 1)))}
    free = free_mask(N, faces)
    B = poisson.robin_diag(N, robin, faces)
    assert np.all(np.abs(B[free] - want[free]) <= 12 * EPS * terms[free])
    assert not B[~free].any() and np.array_equal(B == 0.0, ~free | (terms == 0.0))
    assert np.all(B >= 0.0) and not np.signbit(B).any()
    # by name and by bit, and one face at a time: B is the sum over the faces in ascending bit order
    names = {name: robin[bit] for name, bit in poisson.FACE_BITS.items() if bit in robin}
    assert _same(poisson.robin_diag(N, names, faces), B)
    total = None
    for bit in sorted(robin):
        one = poisson.robin_diag(N, {bit: robin[bit]}, faces)
        total = one if total is None else total + one
    assert _same(total, B)
    # alpha == 1: the face load of q == 1, which sums to the area of the face (no Dirichlet node masked: a set without the
    # face's neighbours)
    for bit in fields:
        other = 1 << ((bit.bit_length() - 1) ^ 1)       # the opposite face as the only Dirichlet face
        ones = poisson.robin_diag(N, {bit: np.ones(N * N)}, other)
        assert abs(ones.sum() - 1.0) <= 4 * (N + 1) ** 2 * EPS
    L0 = poisson.diffusion_level(N, 3, _kappa(N), dirichlet_faces=faces)
    L1 = poisson.diffusion_level(N, 3, _kappa(N), dirichlet_faces=faces, robin=robin)
    A0, A1 = L0.A.tocsr(), L1.A.tocsr()
    assert A0.indptr.tobytes() == A1.indptr.tobytes() and A0.indices.tobytes() == A1.indices.tobytes()
    assert L0.b.tobytes() == L1.b.tobytes()
    d0, d1 = A0.diagonal(), A1.diagonal()
    assert ((A0 - sp.diags(d0)) != (A1 - sp.diags(d1))).nnz == 0
    assert np.array_equal(d1, np.where(free, d0 + B, 1.0)) and (A1 != A1.T).nnz == 0
    # with a reaction field the one nodal term is R + B, formed as that sum
    sigma = _sigma(N)
    L2 = poisson.diffusion_level(N, 3, _kappa(N), dirichlet_faces=faces, sigma=sigma, robin=robin)
    R = poisson.reaction_diag(N, sigma, faces)
    assert np.array_equal(L2.A.diagonal(), np.where(free, d0 + (R + B), 1.0))


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_robin_none_and_zero_fields_are_byte_identical(config):
    N = 6
    faces, fields = CONFIGS[config]
    for sigma in (None, _sigma(N)):
        plain = poisson.diffusion_level(N, 3, _kappa(N), dirichlet_faces=faces, sigma=sigma)
        for robin in (None, {}, {bit: np.zeros(N * N) for bit in fields}, {fields[0]: None}):
            level = poisson.diffusion_level(N, 3, _kappa(N), dirichlet_faces=faces, sigma=sigma, robin=robin)
            assert _csr_bytes(level.A) == _csr_bytes(plain.A) and level.b.tobytes() == plain.b.tobytes()
    for bad in (-1.0, np.nan, np.inf):
        field = robin_alpha(N, fields[0])
        field[5] = bad
        with pytest.raises(ValueError, match="alpha must be finite and not negative"):
            poisson.diffusion_level(N, 3, _kappa(N), dirichlet_faces=faces, robin={fields[0]: field})
    dirichlet = faces & -faces
    with pytest.raises(ValueError, match="Dirichlet face"):
        poisson.diffusion_level(N, 3, _kappa(N), dirichlet_faces=faces, robin={dirichlet: np.ones(N * N)})
    with pytest.raises(ValueError, match="Dirichlet face"):
        poisson.diffusion_level(N, 3, _kappa(N), robin={1: np.ones(N * N)})       # (the default set: all six)
    with pytest.raises(ValueError, match="not one face"):
        poisson.robin_diag(N, {3: np.ones(N * N)}, faces)
    with pytest.raises(ValueError, match="3-D only"):
        poisson.diffusion_level(4, 2, np.ones(16), robin={1: np.ones(4)})


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_adjoint_identity_of_the_robin_restatements(config):
    """a . T_alpha,F(w, x) = w . D_alpha,F(a, x).  Both sides sum the products t w_q a_i x_i h^2 / 6 over the (face-cell, free
    corner) pairs; S, the sum of their absolute values, is |a| . T(|w|, |x|).  Either side rounds each term a fixed number of
    times (the four-term sum, the scale, the products: at most 12) and then adds at most n of them, n the number of nodes of
    the face: the difference is within 2 (n + 12) eps S."""
    N = 6
    faces, fields = CONFIGS[config]
    rng = np.random.default_rng(5)
    n = (N + 1) ** 3
    a, x = rng.standard_normal(n), rng.standard_normal(n)
    free = free_mask(N, faces)
    for bit in fields:
        w = rng.standard_normal(N * N)
        T = poisson.diffusion_apply_drobin(N, bit, w, x, faces)
        D = poisson.diffusion_drobin(N, bit, a, x, faces)
        S = np.abs(a) @ poisson.diffusion_apply_drobin(N, bit, np.abs(w), np.abs(x), faces)
        assert S > 0.0 and abs(a @ T - w @ D) <= 2 * ((N + 1) ** 2 + 12) * EPS * S
        on_face = poisson._on_face(np.ones((N + 1, N + 1)), N, bit).reshape(-1) > 0
        assert not T[~(free & on_face)].any() and np.count_nonzero(T) == np.count_nonzero(free & on_face)
        assert np.array_equal(D, poisson.diffusion_drobin(N, bit, np.where(free, a, 0.0), np.where(free, x, 0.0), faces))
        assert np.array_equal(D, poisson.diffusion_drobin(N, bit, x, a, faces))
        assert np.array_equal(poisson.diffusion_apply_drobin(N, bit, -w, x, faces), -T)
        # with alpha >= 0 it is the field's share of the diagonal
        alpha = robin_alpha(N, bit)
        assert np.array_equal(poisson.diffusion_apply_drobin(N, bit, alpha, x, faces), poisson.robin_diag(N, {bit: alpha}, faces) * x)
    dirichlet = faces & -faces
    with pytest.raises(ValueError, match="Dirichlet face"):
        poisson.diffusion_drobin(N, dirichlet, a, x, faces)
    with pytest.raises(ValueError, match="Dirichlet face"):
        poisson.diffusion_apply_drobin(N, dirichlet, np.ones(N * N), x, faces)


def test_coarsen_robin_is_the_mean_of_the_children():
    N = 8
    robin = _robin(N, "a")
    coarse = poisson.coarsen_robin(robin)
    assert sorted(coarse) == sorted(robin)
    for bit, alpha in robin.items():
        assert _same(coarse[bit], poisson.coarsen_kappa(alpha, 2, "arithmetic")) and _same(coarse[bit], poisson.coarsen_robin(alpha))
        mean = alpha.reshape(N // 2, 2, N // 2, 2).mean(axis=(1, 3)).reshape(-1)
        assert np.all(np.abs(coarse[bit] - mean) <= 4 * EPS * mean)
    # boundary mass is additive: the coarse face carries the fine face's total
    for bit in robin:
        assert abs(coarse[bit].sum() / (N // 2) ** 2 - robin[bit].sum() / N ** 2) <= 4 * N * N * EPS * robin[bit].sum() / N ** 2
    assert poisson.coarsen_robin({1: None}) == {1: None}


def test_a_linear_solution_with_its_ambient_load_is_reproduced():
    """u = a + b z solves -div(kappa grad u) = 0 for constant kappa with u = a on z-, no flux through the side faces and
    kappa b + alpha (u(1) - u_ext) = 0 on z+.  P1 represents u and the lumping is exact on a function that is constant over the
    face, so the discrete solve with the load T_alpha(alpha, u_ext) gives u to rounding: within cond(A) eps of it, cond from the
    extreme eigenvalues of the free block."""
    N = 8
    kappa0, alpha0, a, b = 1.75, 3.5, 0.25, -1.5
    u_ext = (a + b) + kappa0 * b / alpha0
    faces = 16
    robin = {"z+": np.full(N * N, alpha0)}
    level = poisson.diffusion_level(N, 3, np.full(N ** 3, kappa0), dirichlet_faces=faces, robin=robin)
    n1 = N + 1
    z = (np.arange(n1 ** 3) // (n1 * n1)) / N
    u = a + b * z
    free = free_mask(N, faces)
    A = level.A.tocsr()
    load = poisson.diffusion_apply_drobin(N, "z+", robin["z+"], np.full(n1 ** 3, u_ext), faces)
    # (the level's columns towards Dirichlet nodes are lifted into its own right-hand side for its own data: ours by hand)
    lift = poisson.diffusion_lift(N, np.full(N ** 3, kappa0), np.where(free, 0.0, a), faces)
    rhs = np.where(free, load - lift, a)
    got = spl.spsolve(A.tocsc(), rhs)
    Aff = A[free][:, free].tocsc()
    hi = spl.eigsh(Aff, k=1, which="LA", return_eigenvectors=False)[0]
    lo = spl.eigsh(Aff, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0]
    err = np.abs(got - u).max() / np.abs(u).max()
    print("linear solution: max relative error %.3e, cond %.3e" % (err, hi / lo))
    assert err <= (hi / lo) * EPS
    # ... and the residual of u itself vanishes to rounding, row by row
    r = (A @ u - rhs)[free]
    assert np.all(np.abs(r) <= 16 * EPS * (abs(A) @ np.abs(u))[free])


# ---- device -------------------------------------------------------------------------------------------------------------------
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


def _handle(N, nlev, **tuning):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    top = nlev - 1
    h = DeviceHierarchy(3, 0, top, c=N >> top, **tuning)
    h.set_prolongation("p1")
    h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
    return h


def _device_array(h, host):
    from multigrid_dolfinx_amd.hierarchy import _DeviceArray
    host = np.ascontiguousarray(host, dtype=np.float64).reshape(-1)
    return _DeviceArray(h._lib, h.device, host.size, host)


def _set_fields(h, robin):
    for face, alpha in robin.items():
        h.set_diffusion_robin(face, alpha)


@pytest.mark.gpu
@pytest.mark.parametrize("N", KERNEL_N)
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_device_level_with_robin_fields_equals_host_restatement(config, N):
    """The level generated with Robin fields against a handle fed the host restatement's CSR: the same storage figures, F to the
    byte, and residual and one Jacobi sweep to the byte -- without and with a reaction field (d = B and d = R + B)."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    faces, fields = CONFIGS[config]
    robin = _robin(N, config)
    for react in (False, True):
        host = _host_level(N, config, react)
        with DeviceHierarchy(3, 0, 1, c=N // 2) as d, DeviceHierarchy(3, 0, 1, c=N // 2) as s:
            d.set_diffusion_faces(faces)
            assert d.diffusion_robin() == (0, 0)
            _set_fields(d, robin)
            assert d.diffusion_robin() == (sum(fields), N)
            if react:
                d.set_diffusion_reaction(_sigma(N))
            d.gen_diffusion_level(1, _kappa(N))
            assert d.level_robin(1) == sum(fields) and d.level_reaction(1) == react and not d.level_matrix_free(1)
            s.set_level(1, host.A, prune_zeros=True)
            assert s.level_robin(1) == 0
            for h in (d, s):
                h.set_params(2, 2, 2.0 / 3.0)
            assert {k: d.level_info(1)[k] for k in _INFO} == {k: s.level_info(1)[k] for k in _INFO}
            sd = d.level_storage(1)
            assert sd["symmetric"] == 1 and sd["max_pair_ulps"] == 0
            assert _same(d.get_vector(1, "f"), host.b)
            rng = np.random.default_rng(11)
            v, f = rng.standard_normal(d.n_dofs(1)), host.b.reshape(-1)
            a, b = _outputs(d, 1, v, f), _outputs(s, 1, v, f)
            for x, y in zip(a[1:], b[1:]):
                assert _same(x, y)
            r = f - host.A @ v
            assert np.linalg.norm(a[1].reshape(-1) - r) <= 1e-14 * np.linalg.norm(r)
            plain = f - _host_level(N, config, react, False).A @ v
            assert np.linalg.norm(a[1].reshape(-1) - plain) > 1e-6 * np.linalg.norm(r)


@pytest.mark.gpu
@pytest.mark.parametrize("N", KERNEL_N)
@pytest.mark.parametrize("react", [False, True])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_matrix_free_robin_bits_against_the_stored_level(config, react, N):
    """F, the residual, one Jacobi sweep, Chebyshev steps (1, 2) and the SpMV vector of the matrix-free level with Robin fields:
    the bytes of the stored level's one-step kernels, over more than one z segment.  The level's nodal vector holds B, or R + B
    with a reaction field: one vector of 8 bytes per row that a level with neither does not have, and none beyond the reaction
    term's; the path and its counts are those of the reaction term.  The SpMV's dot is summed per workgroup: within the
    worst-case bound of two summation orders, 2 n eps sum |x_i (A x)_i|."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    faces, fields = CONFIGS[config]
    kappa, robin = _kappa(N), _robin(N, config)
    with DeviceHierarchy(3, 0, 1, c=N // 2, **STORED_ONE_STEP) as s, DeviceHierarchy(3, 0, 1, c=N // 2) as m, \
            DeviceHierarchy(3, 0, 1, c=N // 2) as bare:
        for h in (s, m, bare):
            h.set_diffusion_faces(faces)
            if react:
                h.set_diffusion_reaction(_sigma(N))
        bare.gen_diffusion_level(1, kappa, matrix_free=True)
        for h in (s, m):
            _set_fields(h, robin)
        s.gen_diffusion_level(1, kappa)
        m.gen_diffusion_level(1, kappa, matrix_free=True)
        assert m.level_matrix_free(1) and not s.level_matrix_free(1)
        assert m.level_robin(1) == s.level_robin(1) == sum(fields)
        assert m.level_reaction(1) == s.level_reaction(1) == react
        # the handle's fields, and the level's nodal vector where the reaction term has not brought one
        assert m.memory_bytes() - bare.memory_bytes() == 8 * N * N * len(fields) + (0 if react else 8 * (N + 1) ** 3)
        assert s.level_info(1)["nnz_nonzero"] == m.level_info(1)["nnz_nonzero"]
        assert _same(s.get_vector(1, "f"), m.get_vector(1, "f"))
        rng = np.random.default_rng(11)
        v, f = rng.standard_normal(s.n_dofs(1)), rng.standard_normal(s.n_dofs(1))
        for smoother, sweeps in (("jacobi", (1,)), ("chebyshev", (1, 2))):
            for h in (s, m, bare):
                h.set_params(2, 2, 2.0 / 3.0, smoother=smoother)
                h.set_chebyshev_bounds(1, 0.25, 2.125)
                h.reset_smoother_launches()
            for nw in sweeps:
                got = []
                for h in (s, m, bare):
                    h.set_vector(1, "v", v)
                    h.set_vector(1, "f", f)
                    h.residual(1)
                    r = h.get_vector(1, "r")
                    h.smooth(1, nw)
                    got.append((r, h.get_vector(1, "v")))
                assert np.all(np.isfinite(got[0][1]))
                assert np.array_equal(got[0][0], got[1][0]), (smoother, nw, "residual")
                assert np.array_equal(got[0][1], got[1][1]), (smoother, nw, np.flatnonzero(got[0][1] != got[1][1])[:5])
                assert not np.array_equal(got[2][1], got[1][1])
            total = sum(sweeps)
            assert s.smoother_launches(1) == {"slice": (total, total, 0)}
            assert m.smoother_launches(1) == {"matrix_free": (total, total, 0)} == bare.smoother_launches(1)
        spmv = []
        for h in (s, m):
            h.set_vector(1, "v", v)
            spmv.append((h.quadratic_form(1, "v"), h.get_vector(1, "r")))
        assert np.array_equal(spmv[0][1], spmv[1][1])
        terms = np.abs(v * spmv[0][1].reshape(-1)).sum()
        assert abs(spmv[0][0] - spmv[1][0]) <= 2 * v.size * EPS * terms
        assert abs(spmv[0][0] - v @ spmv[0][1].reshape(-1)) <= 2 * v.size * EPS * terms
        want = _host_level(N, config, react).A @ v
        assert np.linalg.norm(spmv[1][1].reshape(-1) - want) <= 1e-14 * np.linalg.norm(want)


def _cycles(h, top):
    """F of every level, then iterate and residual history of two V(2,2) cycles from zero, then an mg_pcg history."""
    F = [h.get_vector(l, "f").tobytes() for l in range(top + 1)]
    h.zero_vector(top, "v")
    hist = h.vcycle(top, 2, residuals=True)
    x = h.get_vector(top, "v").tobytes()
    h.zero_vector(top, "v")
    pcg = h.pcg(rtol=1e-10, max_iter=100, level=top)
    return F, x, hist.tobytes(), pcg


@pytest.mark.gpu
@pytest.mark.parametrize("min_rows", [None, 0])
def test_zero_fields_and_cleared_fields_change_no_bit(min_rows):
    """N = 16, three levels, configuration (a): a handle with alpha == 0 on both faces against a handle that never had a field
    -- F of every level and two V(2,2) cycles (iterate and residual history) byte for byte, the launch counts the same, and
    mg_memory_bytes larger by exactly the handle's fields and the matrix-free levels' nodal vectors.  A handle whose
    fields were set and cleared again is the handle without: bits, mg_memory_bytes and launch counts."""
    N, nlev, top = 16, 3, 2
    faces, fields = CONFIGS["a"]
    kappa = _kappa(N)
    with _handle(N, nlev) as first:
        first.set_diffusion_faces(faces)
        first.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=min_rows)
        assert first.diffusion_robin() == (0, 0) and not any(first.level_robin(l) for l in range(nlev))
        want = _cycles(first, top)
        memory = first.memory_bytes()
        launches = [first.smoother_launches(l) for l in range(nlev)]
    with _handle(N, nlev) as zero:
        zero.set_diffusion_faces(faces)
        _set_fields(zero, {bit: np.zeros(N * N) for bit in fields})
        zero.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=min_rows)
        assert all(zero.level_robin(l) == sum(fields) for l in range(nlev))
        got = _cycles(zero, top)
        rows = sum(zero.n_dofs(l) for l in range(1, nlev)) if min_rows is not None else 0
        assert zero.memory_bytes() == memory + 8 * len(fields) * N * N + 8 * rows
        assert [zero.smoother_launches(l) for l in range(nlev)] == launches
    assert got[:3] == want[:3]
    assert len(got[3]) == len(want[3]) and np.all(np.abs(got[3] - want[3]) <= 1e-12 * np.abs(want[3]))
    with _handle(N, nlev) as cleared:
        cleared.set_diffusion_faces(faces)
        _set_fields(cleared, _robin(N, "a"))
        for bit in fields:
            cleared.set_diffusion_robin(bit, None)
        assert cleared.diffusion_robin() == (0, 0)
        cleared.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=min_rows)
        again = _cycles(cleared, top)
        assert again[:3] == want[:3] and again[3].tobytes() == want[3].tobytes()
        assert cleared.memory_bytes() == memory
        assert [cleared.smoother_launches(l) for l in range(nlev)] == launches


@functools.lru_cache(maxsize=None)
def _host_solution(N, config, react):
    """(A^-1 b, cond(A)) of the restated level, as tests/test_diffusion_reaction.py computes them."""
    host = _host_level(N, config, react)
    A = host.A.tocsc()
    A.eliminate_zeros()
    lu = spl.splu(A, permc_spec="MMD_AT_PLUS_A")
    lo = spl.eigsh(A, k=1, sigma=0.0, which="LM", return_eigenvectors=False, OPinv=spl.LinearOperator(A.shape, matvec=lu.solve))[0]
    hi = spl.eigsh(A, k=1, which="LA", return_eigenvectors=False)[0]
    return lu.solve(host.b.reshape(-1)), float(hi / lo)


@pytest.mark.gpu
@pytest.mark.parametrize("N,nlev", [(16, 3), (32, 4)])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_pcg_with_robin_fields_against_the_direct_solve(config, N, nlev):
    """mg_pcg on generated hierarchies with Robin fields, stored and matrix-free, without and with a reaction field: rtol 1e-10
    within max_iter 200, and the solution within cond(A) rtol of the sparse direct solve of the restated level in relative l2,
    cond computed on the host for this case."""
    rtol, top = 1e-10, nlev - 1
    faces, fields = CONFIGS[config]
    kappa = _kappa(N)
    for react in (False, True):
        host = _host_level(N, config, react)
        f = host.b.reshape(-1)
        want, cond = _host_solution(N, config, react)
        for name, min_rows in (("stored", None), ("matrix_free", 0)):
            with _handle(N, nlev) as h:
                h.set_diffusion_faces(faces)
                _set_fields(h, _robin(N, config))
                if react:
                    h.set_diffusion_reaction(_sigma(N))
                h.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=min_rows)
                assert h.level_matrix_free(top) == (name == "matrix_free")
                assert all(h.level_robin(l) == sum(fields) for l in range(nlev))
                assert _same(h.get_vector(top, "f"), host.b)
                h.zero_vector(top, "v")
                hist = h.pcg(rtol=rtol, max_iter=200, level=top)
                x = h.get_vector(top, "v").reshape(-1)
            assert len(hist) < 200 and hist[-1] <= rtol * np.linalg.norm(f)
            err = np.linalg.norm(x - want) / np.linalg.norm(want)
            print("config", config, "sigma", react, name, "N", N, "iterations", len(hist), "cond %.3e" % cond, "rel l2 error %.3e" % err)
            assert err <= cond * rtol


@pytest.mark.gpu
@pytest.mark.parametrize("react", [False, True])
@pytest.mark.parametrize("min_rows", [None, 0])
def test_refresh_with_new_fields_equals_a_fresh_generation(min_rows, react):
    """N = 16, three levels, kappa and the fields in device memory: generate, refresh with other alpha and the same kappa; F of
    every level, mg_memory_bytes and the iterate of two cycles are those of a fresh generation with those fields, byte for byte.
    The coarse levels rediscretise with the mean of the 2 x 2 children whatever the averaging of kappa.  A refresh after a field
    was cleared is refused by name and leaves the handle usable."""
    N, nlev, top = 16, 3, 2
    faces, fields = CONFIGS["b"]
    kappa, r1, r2 = _kappa(N), _robin(N, "b"), _robin(N, "b", seed=9)
    with _handle(N, nlev) as A, _handle(N, nlev) as B:
        held = {"kappa": _device_array(A, kappa)}
        for bit in fields:
            held[(1, bit)], held[(2, bit)] = _device_array(A, r1[bit]), _device_array(A, r2[bit])
        try:
            kp = held["kappa"].ptr.value
            for h in (A, B):
                h.set_diffusion_faces(faces)
                if react:
                    h.set_diffusion_reaction(_sigma(N))
            for bit in fields:
                A.set_diffusion_robin(bit, held[(1, bit)].ptr.value, N=N)
            A.gen_diffusion_hierarchy(kp, matrix_free_min_rows=min_rows)
            first = _cycles(A, top)
            memory = A.memory_bytes()
            for bit in fields:
                A.set_diffusion_robin(bit, held[(2, bit)].ptr.value, N=N)
            assert A.memory_bytes() == memory
            A.refresh_diffusion_hierarchy(kp)
            assert all(A.level_robin(l) == sum(fields) for l in range(nlev))
            second = _cycles(A, top)
            assert A.memory_bytes() == memory
            for bit in fields:
                B.set_diffusion_robin(bit, r2[bit])
            B.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=min_rows)
            fresh = _cycles(B, top)
            assert B.memory_bytes() == memory
            assert all(held[(2, bit)].download().tobytes() == r2[bit].tobytes() for bit in fields)
            assert first[1] != fresh[1]
            assert second[:3] == fresh[:3] and second[3].tobytes() == fresh[3].tobytes()
            with _handle(N, nlev) as H:
                H.set_diffusion_faces(faces)
                _set_fields(H, r2)
                if react:
                    H.set_diffusion_reaction(_sigma(N))
                H.gen_diffusion_hierarchy(kappa, "harmonic", matrix_free_min_rows=min_rows)
                level = poisson.diffusion_level(N // 2, 3, poisson.coarsen_kappa(kappa, 3, "harmonic"), dirichlet_faces=faces,
                                                sigma=poisson.coarsen_sigma(_sigma(N)) if react else None, robin=poisson.coarsen_robin(r2))
                v = np.random.default_rng(2).standard_normal(H.n_dofs(top - 1))
                H.set_vector(top - 1, "v", v)
                H.set_vector(top - 1, "f", np.zeros(v.size))
                H.residual(top - 1)
                want = -(level.A @ v)
                assert np.linalg.norm(H.get_vector(top - 1, "r").reshape(-1) - want) <= 1e-14 * np.linalg.norm(want)
            A.set_diffusion_robin(fields[0], None)
            _untouched(A, lambda: A.refresh_diffusion_hierarchy(kp), "generated with Robin fields on the faces %d, the handle holds fields on the faces %d" % (sum(fields), fields[1]))
            assert _cycles(A, top)[1:3] == fresh[1:3]
        finally:
            for d in held.values():
                d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("N", KERNEL_N)
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_robin_sensitivity_kernels(config, N):
    """mg_diffusion_drobin and mg_diffusion_apply_drobin to the byte of their restatements (fixed-order sums and plain products,
    no fma) for every field face, on a grid-only level, a stored and a matrix-free level alike; the adjoint identity with both
    sides from the device, within the bound of test_adjoint_identity_of_the_robin_restatements; and T_alpha(alpha, x) is what
    the field adds to the product of the generated level."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    faces, fields = CONFIGS[config]
    rng = np.random.default_rng(13)
    n = (N + 1) ** 3
    a, x = rng.standard_normal(n), rng.standard_normal(n)
    free = free_mask(N, faces)
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.set_diffusion_faces(faces)
        h.set_level_grid(1)
        for bit in fields:
            w = rng.standard_normal(N * N)
            want_D, want_T = poisson.diffusion_drobin(N, bit, a, x, faces), poisson.diffusion_apply_drobin(N, bit, w, x, faces)
            D, T = h.diffusion_drobin(1, bit, a, x), h.diffusion_apply_drobin(1, bit, w, x)
            assert _same(D, want_D) and _same(T, want_T)
            assert not T[~free].any()
            S = np.abs(a) @ h.diffusion_apply_drobin(1, bit, np.abs(w), np.abs(x))
            assert abs(a @ T - w @ D) <= 2 * ((N + 1) ** 2 + 12) * EPS * S
            assert _same(h.diffusion_drobin(1, bit, a, a), poisson.diffusion_drobin(N, bit, a, a, faces))
            if N == KERNEL_N[0]:
                for matrix_free in (False, True):
                    h.gen_diffusion_level(1, _kappa(N), matrix_free=matrix_free)
                    assert _same(h.diffusion_drobin(1, bit, a, x), want_D) and _same(h.diffusion_apply_drobin(1, bit, w, x), want_T)
        robin = _robin(N, config)
        h.set_params(2, 2, 2.0 / 3.0)
        prods = []
        for on in (False, True):
            if on:
                _set_fields(h, robin)
            h.gen_diffusion_level(1, _kappa(N))
            h.set_vector(1, "v", x)
            h.set_vector(1, "f", np.zeros(n))
            h.residual(1)
            prods.append(-h.get_vector(1, "r").reshape(-1))
        # (each product rounds at most eight times on partial sums of a row's terms, each T at most seven times on a term of
        # the row with the fields, and up to three T are added: within 32 eps of the sum of the absolute values of the terms)
        T = sum(h.diffusion_apply_drobin(1, bit, robin[bit], x) for bit in fields)
        terms = abs(_host_level(N, config).A) @ np.abs(x)
        assert np.all(np.abs((prods[1] - prods[0]) - T) <= 32 * EPS * terms)
        assert np.count_nonzero(T) > 0


def _refused(call, text):
    from multigrid_dolfinx_amd._capi import MgError
    with pytest.raises(MgError, match=text):
        call()


def _untouched(h, call, text, vectors=()):
    """`call` is refused with `text`; counters(), the face set, the reaction and Robin state, mg_memory_bytes and the given
    (level, name, bytes) vectors are as they were."""
    before = h.counters()
    state = h.diffusion_faces(), h.diffusion_reaction(), h.diffusion_robin(), h.memory_bytes()
    _refused(call, text)
    assert h.counters() == before
    assert (h.diffusion_faces(), h.diffusion_reaction(), h.diffusion_robin(), h.memory_bytes()) == state
    for level, name, want in vectors:
        assert h.get_vector(level, name).tobytes() == want, (level, name)


@pytest.mark.gpu
def test_robin_refusals_leave_the_handle_as_it_was():
    """Every refusal by message; counters(), the face set, the fields and, where the handle has levels, V and F unchanged."""
    import ctypes as C
    from multigrid_dolfinx_amd._capi import MgError, check
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N, nlev, top = 16, 3, 2
    faces, fields = CONFIGS["a"]
    kappa, robin = _kappa(N), _robin(N, "a")
    nothing = lambda *args: None
    with DeviceHierarchy(2, 0, 1, c=4) as h2:
        _untouched(h2, lambda: h2.set_diffusion_robin("z+", np.ones(64)), "3-D only")
        h2.set_diffusion_robin("z+", None)
        h2.gen_poisson_level(1)
        buf = _device_array(h2, np.ones(9 ** 3))
        try:
            p = buf.ptr.value
            _untouched(h2, lambda: h2.diffusion_drobin(1, 32, p, p, p), "Robin sensitivity is 3-D only")
            _untouched(h2, lambda: h2.diffusion_apply_drobin(1, 32, p, p, p), "Robin sensitivity is 3-D only")
        finally:
            buf.free()
    with DeviceHierarchy(3, 0, 1, c=4) as slab:
        slab.set_comm_callbacks(0, 2, nothing, nothing, nothing)
        _untouched(slab, lambda: slab.set_diffusion_robin("z+", np.ones(64)), "whole \\(not slab\\) handle")
        buf = _device_array(slab, np.ones(9 ** 3))
        try:
            p = buf.ptr.value
            _untouched(slab, lambda: slab.set_diffusion_robin(32, p, N=8), "whole \\(not slab\\) handle")
            _untouched(slab, lambda: slab.diffusion_drobin(1, 32, p, p, p), "whole \\(not slab\\) handle")
            _untouched(slab, lambda: slab.diffusion_apply_drobin(1, 32, p, p, p), "whole \\(not slab\\) handle")
        finally:
            buf.free()
    with DeviceHierarchy(3, 0, 0, c=16) as flat:
        flat.set_flat_level(poisson.lexicographic_level(4, 2).A)
        buf = _device_array(flat, np.ones(125))
        try:
            p = buf.ptr.value
            _untouched(flat, lambda: flat.diffusion_drobin(0, 32, p, p, p), "flat")
            _untouched(flat, lambda: flat.diffusion_apply_drobin(0, 32, p, p, p), "flat")
        finally:
            buf.free()
    with _handle(N, nlev) as h:
        h.set_diffusion_faces(faces)
        _set_fields(h, robin)
        h.gen_diffusion_hierarchy(kappa)
        v = np.random.default_rng(1).standard_normal(h.n_dofs(top))
        h.set_vector(top, "v", v)
        state = [(top, "v", v.tobytes()), (top, "f", h.get_vector(top, "f").tobytes()), (top - 1, "f", h.get_vector(top - 1, "f").tobytes())]
        untouched = lambda call, text: _untouched(h, call, text, state)
        # a face that is not exactly one bit
        for bad_face in (0, 3, 33, 63, 64, -1):
            untouched(lambda: check(h._lib.mg_set_diffusion_robin(h._h, N, bad_face, robin[32].ctypes.data_as(C.c_void_p))), "is not exactly one face")
            untouched(lambda: check(h._lib.mg_set_diffusion_robin(h._h, N, bad_face, None)), "is not exactly one face")
        # the field itself: the first bad face-cell, named alike by both variants
        cell = 7 * N + 3
        for bad in (-1.0, np.nan, np.inf, -np.inf):
            field = robin[32].copy()
            field[cell], field[cell + 20] = bad, -2.0
            msg = "alpha must be finite and not negative: face-cell \\(3, 7\\) of face 32 = index %d holds" % cell
            untouched(lambda: h.set_diffusion_robin("z+", field), msg)
            buf = _device_array(h, field)
            try:
                untouched(lambda: h.set_diffusion_robin("z+", buf.ptr.value, N=N), msg)
                names = []
                for arg in (field, buf.ptr.value):
                    try:
                        h.set_diffusion_robin(32, arg, N=N)
                    except MgError as exc:
                        names.append(str(exc).split(": ", 1)[1])
                assert len(names) == 2 and names[0] == names[1], names
            finally:
                buf.free()
        good = _device_array(h, robin[32])
        held = [good]
        try:
            p = good.ptr.value
            untouched(lambda: h.set_diffusion_robin(32, robin[32].ctypes.data, N=N), "not device memory")
            untouched(lambda: check(h._lib.mg_set_diffusion_robin(h._h, N, 32, C.c_void_p(p))), "not host memory")
            untouched(lambda: h.set_diffusion_robin(32, p, N=0), "elements_per_dim must be positive")
            untouched(lambda: h.set_diffusion_robin(32, robin_alpha(N // 2, 32)), "the fields the handle holds on other faces have %d face-cells" % N)
            untouched(lambda: h.set_diffusion_robin(2, robin_alpha(N // 2, 2)), "the fields the handle holds on other faces have %d face-cells" % N)
            # the face set 0 is still singular with fields in place
            untouched(lambda: h.set_diffusion_faces(0), "singular")
            kbuf = _device_array(h, kappa)
            held.append(kbuf)
            calls = (lambda: h.gen_diffusion_level(top, kappa), lambda: h.gen_diffusion_level(top, kappa, matrix_free=True),
                     lambda: h.gen_diffusion_hierarchy(kappa), lambda: h.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=0),
                     lambda: h.gen_diffusion_hierarchy(kbuf.ptr.value), lambda: h.refresh_diffusion_hierarchy(kbuf.ptr.value))
            # a field on a face of the Dirichlet set, at every generating call
            h.set_diffusion_faces(faces | 32)
            for call in calls[:5]:
                untouched(call, "face 32 cannot be both")
            h.set_diffusion_faces(faces)
            # fields of another size than the level (the top level of a hierarchy), at every generating call
            for bit in fields:
                h.set_diffusion_robin(bit, None)
            for bit in fields:
                h.set_diffusion_robin(bit, robin_alpha(N // 2, bit))
            for call in calls:
                untouched(call, "elements_per_dim = %d, the Robin fields .* have %d face-cells per dimension" % (N, N // 2))
            # a refresh with another set of field faces than the levels'
            h.set_diffusion_robin(fields[0], None)
            h.set_diffusion_robin(fields[1], None)
            untouched(lambda: h.refresh_diffusion_hierarchy(kbuf.ptr.value), "generated with Robin fields on the faces %d, the handle holds fields on the faces 0" % sum(fields))
            _set_fields(h, robin)
            h.refresh_diffusion_hierarchy(kbuf.ptr.value)
            assert h.get_vector(top, "f").tobytes() == state[1][2]
            with _handle(N, nlev) as plain:
                plain.set_diffusion_faces(faces)
                plain.gen_diffusion_hierarchy(kappa)
                plain.set_diffusion_robin(32, robin[32])
                _untouched(plain, lambda: plain.refresh_diffusion_hierarchy(kappa), "generated with Robin fields on the faces 0, the handle holds fields on the faces 32")
            # the sensitivity entries
            n = h.n_dofs(top)
            nodes, cells, out = _device_array(h, v), _device_array(h, robin[32]), _device_array(h, np.zeros(n))
            held += [nodes, cells, out]
            a, w, o = nodes.ptr.value, cells.ptr.value, out.ptr.value
            h.set_vector(top, "v", v)
            for call, text in ((lambda: h.diffusion_drobin(top, 32, 0, a, o), "null pointer \\(a\\)"),
                               (lambda: h.diffusion_drobin(top, 32, a, 0, o), "null pointer \\(b\\)"),
                               (lambda: h.diffusion_drobin(top, 32, a, a, 0), "null pointer \\(out\\)"),
                               (lambda: h.diffusion_apply_drobin(top, 32, 0, a, o), "null pointer \\(dalpha\\)"),
                               (lambda: h.diffusion_apply_drobin(top, 32, w, 0, o), "null pointer \\(x\\)"),
                               (lambda: h.diffusion_apply_drobin(top, 32, w, a, 0), "null pointer \\(out\\)"),
                               (lambda: h.diffusion_drobin(top, 32, v.ctypes.data, a, o), "a is not device memory"),
                               (lambda: h.diffusion_drobin(top, 32, a, a, v.ctypes.data), "out is not device memory"),
                               (lambda: h.diffusion_apply_drobin(top, 32, robin[32].ctypes.data, a, o), "dalpha is not device memory"),
                               (lambda: h.diffusion_apply_drobin(top, 32, w, v.ctypes.data, o), "x is not device memory"),
                               (lambda: h.diffusion_drobin(top, 32, a, a, a), "out overlaps a"),
                               (lambda: h.diffusion_drobin(top, 32, o, a, a + 8), "out overlaps b"),
                               (lambda: h.diffusion_apply_drobin(top, 32, w, a, a), "out overlaps x"),
                               (lambda: h.diffusion_apply_drobin(top, 32, w, a, w), "out overlaps dalpha"),
                               (lambda: h.diffusion_drobin(top, 16, a, a, o), "face 16 is a Dirichlet face"),
                               (lambda: h.diffusion_apply_drobin(top, 16, w, a, o), "face 16 is a Dirichlet face"),
                               (lambda: check(h._lib.mg_diffusion_drobin(h._h, top, 48, C.c_void_p(a), C.c_void_p(a), C.c_void_p(o))), "is not exactly one face"),
                               (lambda: check(h._lib.mg_diffusion_apply_drobin(h._h, top, 0, C.c_void_p(w), C.c_void_p(a), C.c_void_p(o))), "is not exactly one face")):
                untouched(call, text)
            assert out.download().tobytes() == np.zeros(n).tobytes()
            h.zero_vector(top, "v")
            assert len(h.pcg(rtol=1e-8, max_iter=100, level=top)) < 100
        finally:
            for d in held:
                d.free()


@pytest.mark.gpu
def test_the_timing_names_run():
    """mg_time_kernel takes "drobin" and "apply_drobin" (face z+) on a level whose handle has z+ outside its Dirichlet set, and
    refuses them by name where z+ is a Dirichlet face; the march keys time the march on a level that has fields."""
    N = 16
    faces, fields = CONFIGS["a"]
    with _handle(N, 2) as h:
        h.set_diffusion_faces(faces)
        _set_fields(h, _robin(N, "a"))
        h.gen_diffusion_hierarchy(_kappa(N), matrix_free_min_rows=0)
        for name in ("drobin", "apply_drobin", "diffusion_mf:jacobi"):
            t = h.time_kernel(name, 1, reps=2)
            assert np.isfinite(t) and t > 0.0, name
    with _handle(N, 2) as h:
        h.gen_diffusion_hierarchy(_kappa(N))
        for name in ("drobin", "apply_drobin"):
            _refused(lambda: h.time_kernel(name, 1, reps=1), "face 32 is a Dirichlet face")


def _torch_first(worker):
    code = "import torch, sys; sys.path.insert(0, %r); import tests.diffusion_robin_workers as w; w.%s()" % (ROOT, worker)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.gpu
def test_diffusion_solver_with_robin_fields_against_the_host():
    """DiffusionSolver with Robin fields, configurations (a) and (b), N = 16, stored and matrix-free, the fields on the device
    and on the CPU: u, J, the gradients with respect to kappa, alpha, sigma, f and g and the kappa-kappa, kappa-alpha,
    alpha-kappa and alpha-alpha blocks of Hessian-vector products against the host adjoint, n_solves 2, 4 and 6
    (`solver_worker`; ROBIN_LIMIT holds the measured figure)."""
    assert "solver ok" in _torch_first("solver_worker")


@pytest.mark.gpu
def test_diffusion_solver_tangent_with_every_direction_against_the_host():
    """`tangent` with df, g and dg, sigma and dsigma, Robin fields on both field faces and drobin on one of them, and the same
    call with g = None, dg = None: configuration (a), N = 16, stored and matrix-free, u and du against HostOperator
    (`tangent_worker`; TANGENT_LIMIT holds the measured figure)."""
    assert "tangent ok" in _torch_first("tangent_worker")


@pytest.mark.gpu
def test_diffusion_solver_switches_between_sets_of_field_faces():
    assert "switch ok" in _torch_first("switch_worker")
