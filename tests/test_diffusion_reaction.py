"""The lumped reaction term of the diffusion solves (mg_set_diffusion_reaction): the operator A(kappa) + R(sigma) with R the
row-sum lumped P1 mass of the Kuhn mesh weighted by one sigma per cell.  The host restatements of poisson.py against an
independent assembly over the Kuhn simplices, the stored level against its restatement, the matrix-free march with the reaction
diagonal against the stored level, sigma == 0 and handles without a field changing nothing, mg_pcg against a sparse direct
solve, the refresh path, the two sensitivity kernels, the refusals, and DiffusionSolver with sigma, reaction_apply and
same_operator against host adjoints (tests/diffusion_reaction_workers.py)."""
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
from tests.diffusion_workers import lognormal_kappa

EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACE_SETS = (63, 18, 1)
KERNEL_N = (8, 36, 72)          # 9^3 nodes: part of one 64 x 8 tile; 37^3: the y tiles; 73^3: past the 64-node tile edge in x
# the stored handle's one-step kernel whose bits the matrix-free march carries (tests/test_diffusion_mf.py)
STORED_ONE_STEP = {"row_classes": 0, "fuse_sweeps": 0}


@functools.lru_cache(maxsize=None)
def _kappa(N):
    return lognormal_kappa(N, 3, seed=3)


@functools.lru_cache(maxsize=None)
def _sigma(N):
    return reaction_sigma(N)


@functools.lru_cache(maxsize=8)
def _host_level(N, faces, react=True):
    return poisson.diffusion_level(N, 3, _kappa(N), dirichlet_faces=faces, sigma=_sigma(N) if react else None)


def _csr_bytes(A):
    A = A.tocsr()
    return A.indptr.tobytes(), A.indices.tobytes(), A.data.tobytes()


# ---- host ---------------------------------------------------------------------------------------------------------------------
def _lumped_mass_by_simplices(N, w):
    """(R(w), the same sum over |w|) at all (N + 1)^3 nodes by enumeration: the six Kuhn simplices of a cell are the paths
    0 -> e_p -> e_p + e_q -> (1,1,1), each of volume h^3 / 6; the row-sum lumped P1 mass gives each of a simplex's four
    vertices |T| / 4 times the cell's w."""
    n1, h = N + 1, 1.0 / N
    cells = np.asarray(w, dtype=np.float64).reshape(N, N, N)
    R, S = np.zeros((n1, n1, n1)), np.zeros((n1, n1, n1))
    ck, cj, ci = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    for perm in itertools.permutations(range(3)):
        v = [0, 0, 0]
        corners = [tuple(v)]
        for axis in perm:
            v[axis] = 1
            corners.append(tuple(v))
        for dx, dy, dz in corners:
            np.add.at(R, (ck + dz, cj + dy, ci + dx), cells * (h ** 3 / 6.0) / 4.0)
            np.add.at(S, (ck + dz, cj + dy, ci + dx), np.abs(cells) * (h ** 3 / 6.0) / 4.0)
    return R.reshape(-1), S.reshape(-1)


def _reaction_diag_everywhere(N, w):
    """`poisson.reaction_diag` masks the Dirichlet nodes of a face set, and no face set is empty: the nodes of the x- face from
    the set {x+}, every other node from the set {x-}."""
    return np.where(poisson.dirichlet_mask(N, 1), poisson.reaction_diag(N, w, 2), poisson.reaction_diag(N, w, 1))


@pytest.mark.parametrize("N", [4, 6])
@pytest.mark.parametrize("faces", FACE_SETS)
def test_level_with_sigma_against_the_simplex_assembly(N, faces):
    """diffusion_level(sigma=...) is the level without sigma plus diag(R(sigma)) on the free rows and nothing elsewhere, R within
    24 eps of the sum of the absolute values of its (at most 24) simplex terms of an independent assembly; the matrix is
    symmetric to the bit; sigma=None is today's call byte for byte; and R sums to h^3 sum_c w_c over all nodes."""
    kappa, sigma = _kappa(N), _sigma(N)
    free = free_mask(N, faces)
    L0 = poisson.diffusion_level(N, 3, kappa, dirichlet_faces=faces)
    L1 = poisson.diffusion_level(N, 3, kappa, dirichlet_faces=faces, sigma=sigma)
    none = poisson.diffusion_level(N, 3, kappa, dirichlet_faces=faces, sigma=None)
    assert _csr_bytes(L0.A) == _csr_bytes(none.A) and L0.b.tobytes() == none.b.tobytes()
    if faces == 63:
        plain = poisson.diffusion_level(N, 3, kappa)
        assert _csr_bytes(L0.A) == _csr_bytes(plain.A) and L0.b.tobytes() == plain.b.tobytes()
    A0, A1 = L0.A.tocsr(), L1.A.tocsr()
    assert A0.indptr.tobytes() == A1.indptr.tobytes() and A0.indices.tobytes() == A1.indices.tobytes()
    assert L0.b.tobytes() == L1.b.tobytes()
    d0, d1 = A0.diagonal(), A1.diagonal()
    off0, off1 = A0 - sp.diags(d0), A1 - sp.diags(d1)
    assert (off0 != off1).nnz == 0
    assert np.array_equal(d1[~free], d0[~free]) and np.all(d1[~free] == 1.0)
    R = poisson.reaction_diag(N, sigma, faces)
    assert np.array_equal(d1[free], d0[free] + R[free]) and not R[~free].any()
    assert (A1 != A1.T).nnz == 0
    want, terms = _lumped_mass_by_simplices(N, sigma)
    assert np.all(np.abs(R[free] - want[free]) <= 24 * EPS * terms[free])
    assert np.all(R[free] > 0.0)
    # the sum over all nodes, to n eps sum |terms| with n the number of additions
    for w in (sigma, np.random.default_rng(3).standard_normal(N ** 3)):
        everywhere = _reaction_diag_everywhere(N, w)
        total, bound = (1.0 / N) ** 3 * np.sum(w), (1.0 / N) ** 3 * np.sum(np.abs(w))
        n = (N + 1) ** 3 + N ** 3 + 16
        assert abs(np.sum(everywhere) - total) <= n * EPS * bound
    # w == 1 is the load of f == 1 on a free node: diffusion_level's load is -12 times that (rows with no Dirichlet neighbour,
    # whose right-hand side is the load alone; the two round the same three factors in another order)
    ones = poisson.reaction_diag(N, np.ones(N ** 3), faces)
    c = np.arange(N + 1)
    deep = (c >= 2) & (c <= N - 2)
    deep = (deep[:, None, None] & deep[None, :, None] & deep[None, None, :]).reshape(-1)
    assert deep.any() and np.all(np.abs(L0.b.reshape(-1)[deep] - -12.0 * ones[deep]) <= 4 * EPS * 12.0 * ones[deep])
    assert np.allclose(ones[free], _lumped_mass_by_simplices(N, np.ones(N ** 3))[0][free], rtol=24 * EPS, atol=0)


@pytest.mark.parametrize("faces", [63, 18, 1, 12])
def test_adjoint_identity_of_the_reaction_restatements(faces):
    """a . T_sigma(w, x) = w . D_sigma(a, x).  Both sides sum the products t w_c a_i x_i h^3 / 24 over the (cell, free corner)
    pairs; S, the sum of their absolute values, is |a| . T_sigma(|w|, |x|).  Either side rounds each term a fixed number of times
    (the eight-term sum, the scale, the products: at most 16) and then adds at most n of them, n the number of nodes: the
    difference is within 2 (n + 16) eps S.  The masks are those of the vectors zeroed on the Dirichlet nodes."""
    N = 6
    rng = np.random.default_rng(5)
    n = (N + 1) ** 3
    a, x, w = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(N ** 3)
    free = free_mask(N, faces)
    T = poisson.diffusion_apply_dsigma(N, w, x, faces)
    D = poisson.diffusion_dsigma(N, a, x, faces)
    S = np.abs(a) @ poisson.diffusion_apply_dsigma(N, np.abs(w), np.abs(x), faces)
    assert S > 0.0 and abs(a @ T - w @ D) <= 2 * (n + 16) * EPS * S
    assert not T[~free].any()
    assert np.array_equal(D, poisson.diffusion_dsigma(N, np.where(free, a, 0.0), np.where(free, x, 0.0), faces))
    assert np.array_equal(T[free], (poisson.reaction_diag(N, w, faces) * x)[free])
    # symmetric in its two vectors, and linear in w
    assert np.array_equal(D, poisson.diffusion_dsigma(N, x, a, faces))
    assert np.array_equal(poisson.diffusion_apply_dsigma(N, -w, x, faces), -T)


def test_coarsen_sigma_is_arithmetic_and_sigma_is_3d_only():
    N = 8
    sigma = _sigma(N)
    want = poisson.coarsen_kappa(sigma, 3, "arithmetic")
    for averaging in ("arithmetic", "harmonic"):
        assert poisson.coarsen_sigma(sigma, averaging).tobytes() == want.tobytes()
    mean = sigma.reshape(N // 2, 2, N // 2, 2, N // 2, 2).mean(axis=(1, 3, 5)).reshape(-1)
    assert np.all(np.abs(want - mean) <= 8 * EPS * mean)
    assert np.abs(want - poisson.coarsen_kappa(sigma, 3, "harmonic")).max() > 0.0
    with pytest.raises(ValueError):
        poisson.coarsen_sigma(sigma, "geometric")
    with pytest.raises(ValueError, match="3-D only"):
        poisson.diffusion_level(4, 2, np.ones(16), sigma=np.ones(16))
    for bad in (-1.0, np.nan, np.inf):
        field = _sigma(4).copy()
        field[5] = bad
        with pytest.raises(ValueError, match="sigma must be finite and not negative"):
            poisson.diffusion_level(4, 3, _kappa(4), sigma=field)
    zero = poisson.diffusion_level(4, 3, _kappa(4), sigma=np.zeros(64))
    plain = poisson.diffusion_level(4, 3, _kappa(4))
    assert _csr_bytes(zero.A) == _csr_bytes(plain.A) and zero.b.tobytes() == plain.b.tobytes()


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


@pytest.mark.gpu
@pytest.mark.parametrize("N", KERNEL_N)
@pytest.mark.parametrize("faces", FACE_SETS)
def test_device_level_with_sigma_equals_host_restatement(faces, N):
    """As tests/test_diffusion_neumann.py compares them: the level generated with a reaction field against a handle fed the host
    restatement's CSR -- the same storage figures, F to the byte, and residual and one Jacobi sweep to the byte."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    host = _host_level(N, faces)
    with DeviceHierarchy(3, 0, 1, c=N // 2) as d, DeviceHierarchy(3, 0, 1, c=N // 2) as s:
        d.set_diffusion_faces(faces)
        assert d.diffusion_reaction() == (0, 0)
        d.set_diffusion_reaction(_sigma(N))
        assert d.diffusion_reaction() == (1, N)
        d.gen_diffusion_level(1, _kappa(N))
        assert d.level_reaction(1) and not d.level_matrix_free(1)
        s.set_level(1, host.A, prune_zeros=True)
        assert not s.level_reaction(1)
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
        # ... and it is not the level without the field
        plain = f - _host_level(N, faces, False).A @ v
        assert np.linalg.norm(a[1].reshape(-1) - plain) > 1e-6 * np.linalg.norm(r)


@pytest.mark.gpu
@pytest.mark.parametrize("N", KERNEL_N)
@pytest.mark.parametrize("faces", [63, 18])
def test_matrix_free_reaction_bits_against_the_stored_level(faces, N):
    """F, the residual, one Jacobi sweep, Chebyshev steps (1, 2) and the SpMV vector of the matrix-free level with a reaction
    diagonal: the bytes of the stored level's one-step kernels.  The SpMV's dot is summed per workgroup: within the worst-case
    bound of two summation orders, 2 n eps sum |x_i (A x)_i|.  The launch counts name the matrix-free march."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    kappa, sigma = _kappa(N), _sigma(N)
    with DeviceHierarchy(3, 0, 1, c=N // 2, **STORED_ONE_STEP) as s, DeviceHierarchy(3, 0, 1, c=N // 2) as m:
        for h in (s, m):
            h.set_diffusion_faces(faces)
            h.set_diffusion_reaction(sigma)
        s.gen_diffusion_level(1, kappa)
        m.gen_diffusion_level(1, kappa, matrix_free=True)
        assert m.level_matrix_free(1) and not s.level_matrix_free(1)
        assert m.level_reaction(1) and s.level_reaction(1)
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
        # the vector is that of the restated operator, not of the one without the field
        want = _host_level(N, faces).A @ v
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
def test_a_zero_field_and_no_field_change_no_bit(min_rows):
    """N = 16, three levels: a handle with sigma == 0 against a handle without a field -- F of every level and two V(2,2) cycles
    (iterate and residual history) byte for byte, the mg_pcg history to 1e-12 relative.  A handle without a field reports (0, 0)
    and its mg_memory_bytes is that of an identical handle built before any field was set on any handle."""
    N, nlev, top = 16, 3, 2
    kappa = _kappa(N)
    with _handle(N, nlev) as first:
        first.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=min_rows)
        assert first.diffusion_reaction() == (0, 0)
        assert not any(first.level_reaction(l) for l in range(nlev))
        want = _cycles(first, top)
        memory = first.memory_bytes()
        launches = [first.smoother_launches(l) for l in range(nlev)]
    with _handle(N, nlev) as zero:
        zero.set_diffusion_reaction(np.zeros(N ** 3))
        assert zero.diffusion_reaction() == (1, N)
        zero.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=min_rows)
        assert all(zero.level_reaction(l) for l in range(nlev))
        assert [zero.level_matrix_free(l) for l in range(nlev)] == [False] + [min_rows is not None] * top
        got = _cycles(zero, top)
        rows = sum(zero.n_dofs(l) for l in range(1, nlev)) if min_rows is not None else 0
        assert zero.memory_bytes() == memory + 8 * N ** 3 + 8 * rows      # the handle's field, R(sigma) of the matrix-free levels
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
    assert len(got[3]) == len(want[3]) and np.all(np.abs(got[3] - want[3]) <= 1e-12 * np.abs(want[3]))
    with _handle(N, nlev) as later:
        later.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=min_rows)
        assert later.diffusion_reaction() == (0, 0)
        again = _cycles(later, top)
        assert later.memory_bytes() == memory
        assert [later.smoother_launches(l) for l in range(nlev)] == launches
    assert again[:3] == want[:3] and again[3].tobytes() == want[3].tobytes()
    # a field set and cleared again leaves a handle without one
    with _handle(N, nlev) as cleared:
        cleared.set_diffusion_reaction(_sigma(N))
        cleared.set_diffusion_reaction(None)
        assert cleared.diffusion_reaction() == (0, 0)
        cleared.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=min_rows)
        assert _cycles(cleared, top)[:3] == want[:3] and cleared.memory_bytes() == memory


@functools.lru_cache(maxsize=None)
def _host_solution(N, faces, react):
    """(A^-1 b, cond(A)) of the restated level, as tests/test_diffusion_neumann.py computes them: one SuperLU factorisation
    serves the solve and, as the shift-invert operator of Lanczos, lambda_min; lambda_max by Lanczos on A."""
    host = _host_level(N, faces, react)
    A = host.A.tocsc()
    A.eliminate_zeros()
    lu = spl.splu(A, permc_spec="MMD_AT_PLUS_A")
    lo = spl.eigsh(A, k=1, sigma=0.0, which="LM", return_eigenvectors=False, OPinv=spl.LinearOperator(A.shape, matvec=lu.solve))[0]
    hi = spl.eigsh(A, k=1, which="LA", return_eigenvectors=False)[0]
    return lu.solve(host.b.reshape(-1)), float(hi / lo)


@pytest.mark.gpu
@pytest.mark.parametrize("N,nlev", [(16, 3), (32, 4)])
@pytest.mark.parametrize("faces", [63, 18])
def test_pcg_with_a_reaction_term_against_the_direct_solve(faces, N, nlev):
    """mg_pcg on generated hierarchies with a reaction field, stored and matrix-free: rtol 1e-10 within max_iter 200, and the
    solution within cond(A) rtol of the sparse direct solve of the restated level in relative l2, cond computed on the host for
    this case.  The iteration counts are printed beside those without a field (recorded in DESIGN.md, not asserted)."""
    rtol, top = 1e-10, nlev - 1
    kappa = _kappa(N)
    counts = {}
    for react in (True, False):
        host = _host_level(N, faces, react)
        f = host.b.reshape(-1)
        for name, min_rows in (("stored", None), ("matrix_free", 0)):
            with _handle(N, nlev) as h:
                h.set_diffusion_faces(faces)
                if react:
                    h.set_diffusion_reaction(_sigma(N))
                h.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=min_rows)
                assert h.level_matrix_free(top) == (name == "matrix_free")
                assert all(h.level_reaction(l) == react for l in range(nlev))
                assert _same(h.get_vector(top, "f"), host.b)
                h.zero_vector(top, "v")
                hist = h.pcg(rtol=rtol, max_iter=200, level=top)
                x = h.get_vector(top, "v").reshape(-1)
            assert len(hist) < 200 and hist[-1] <= rtol * np.linalg.norm(f)
            counts[("sigma" if react else "no sigma", name)] = len(hist)
            if not react:
                continue
            want, cond = _host_solution(N, faces, react)
            err = np.linalg.norm(x - want) / np.linalg.norm(want)
            print("faces", faces, name, "N", N, "iterations", len(hist), "cond %.3e" % cond, "rel l2 error %.3e" % err)
            assert err <= cond * rtol
    print("iterations N", N, "faces", faces, counts)


@pytest.mark.gpu
@pytest.mark.parametrize("min_rows", [None, 0])
def test_refresh_with_a_new_sigma_equals_a_fresh_generation(min_rows):
    """N = 16, three levels, kappa and sigma in device memory: generate, refresh with another sigma and the same kappa; F of every
    level, mg_memory_bytes and the iterate of two cycles are those of a fresh generation with that sigma, byte for byte.  A
    refresh after the field was cleared is refused by name and leaves the handle usable."""
    N, nlev, top = 16, 3, 2
    kappa, s1, s2 = _kappa(N), _sigma(N), reaction_sigma(N, seed=9)
    with _handle(N, nlev) as A, _handle(N, nlev) as B:
        held = [_device_array(A, x) for x in (kappa, s1, s2)]
        try:
            kp, p1, p2 = (d.ptr.value for d in held)
            A.set_diffusion_reaction(p1, N=N)
            A.gen_diffusion_hierarchy(kp, matrix_free_min_rows=min_rows)
            first = _cycles(A, top)
            memory = A.memory_bytes()
            A.set_diffusion_reaction(p2, N=N)
            assert A.memory_bytes() == memory
            A.refresh_diffusion_hierarchy(kp)
            assert all(A.level_reaction(l) for l in range(nlev))
            second = _cycles(A, top)
            assert A.memory_bytes() == memory
            B.set_diffusion_reaction(p2, N=N)
            B.gen_diffusion_hierarchy(kp, matrix_free_min_rows=min_rows)
            fresh = _cycles(B, top)
            assert B.memory_bytes() == memory
            assert held[2].download().tobytes() == s2.tobytes() and held[0].download().tobytes() == kappa.tobytes()
            assert first[1] != fresh[1]
            assert second[:3] == fresh[:3] and second[3].tobytes() == fresh[3].tobytes()
            # host hand-off of both fields: the same hierarchy
            with _handle(N, nlev) as C:
                C.set_diffusion_reaction(s2)
                C.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=min_rows)
                assert _cycles(C, top)[:3] == fresh[:3]
            # the coarse levels rediscretise with the arithmetic mean of sigma, whatever the averaging of kappa
            with _handle(N, nlev) as H:
                H.set_diffusion_reaction(s2)
                H.gen_diffusion_hierarchy(kappa, "harmonic", matrix_free_min_rows=min_rows)
                ks = poisson.coarsen_kappa(kappa, 3, "harmonic")
                level = poisson.diffusion_level(N // 2, 3, ks, sigma=poisson.coarsen_sigma(s2, "harmonic"))
                assert _same(H.get_vector(top - 1, "f"), level.b)
                v = np.random.default_rng(2).standard_normal(H.n_dofs(top - 1))
                H.set_vector(top - 1, "v", v)
                H.set_vector(top - 1, "f", np.zeros(v.size))
                H.residual(top - 1)
                want = -(level.A @ v)
                assert np.linalg.norm(H.get_vector(top - 1, "r").reshape(-1) - want) <= 1e-14 * np.linalg.norm(want)
            A.set_diffusion_reaction(None)
            _untouched(A, lambda: A.refresh_diffusion_hierarchy(kp), "generated with a reaction term, the handle has no reaction field")
            assert _cycles(A, top)[1:3] == fresh[1:3]       # (the cycles before have overwritten the coarse levels' F)
        finally:
            for d in held:
                d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("N", KERNEL_N)
@pytest.mark.parametrize("faces", FACE_SETS)
def test_sigma_sensitivity_kernels(faces, N):
    """mg_diffusion_dsigma and mg_diffusion_apply_dsigma to the byte of their restatements (fixed-order sums and plain products,
    no fma), on a stored level, a matrix-free level and a grid-only level alike; and the adjoint identity with both sides from
    the device, within the bound of test_adjoint_identity_of_the_reaction_restatements."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    rng = np.random.default_rng(13)
    n = (N + 1) ** 3
    a, x, w = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(N ** 3)
    free = free_mask(N, faces)
    want_D, want_T = poisson.diffusion_dsigma(N, a, x, faces), poisson.diffusion_apply_dsigma(N, w, x, faces)
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.set_diffusion_faces(faces)
        h.set_level_grid(1)
        D, T = h.diffusion_dsigma(1, a, x), h.diffusion_apply_dsigma(1, w, x)
        assert _same(D, want_D) and _same(T, want_T)
        assert not T[~free].any()
        S = np.abs(a) @ h.diffusion_apply_dsigma(1, np.abs(w), np.abs(x))
        assert abs(a @ T - w @ D) <= 2 * (n + 16) * EPS * S
        assert _same(h.diffusion_dsigma(1, a, a), poisson.diffusion_dsigma(N, a, a, faces))
        if N == KERNEL_N[0]:
            for matrix_free in (False, True):
                h.gen_diffusion_level(1, _kappa(N), matrix_free=matrix_free)
                assert _same(h.diffusion_dsigma(1, a, x), want_D) and _same(h.diffusion_apply_dsigma(1, w, x), want_T)
        # T_sigma(sigma, x) is what the reaction field adds to the product of the generated level
        sigma = _sigma(N)
        h.set_params(2, 2, 2.0 / 3.0)
        prods = []
        for field in (None, sigma):
            h.set_diffusion_reaction(field)
            h.gen_diffusion_level(1, _kappa(N))
            h.set_vector(1, "v", x)
            h.set_vector(1, "f", np.zeros(n))
            h.residual(1)
            prods.append(-h.get_vector(1, "r").reshape(-1))
        # (each product rounds at most eight times on partial sums of a row's terms, T at most eleven times on a term of the
        # row with the field: within 32 eps of the sum of the absolute values of that row's terms)
        T = h.diffusion_apply_dsigma(1, sigma, x)
        terms = abs(_host_level(N, faces).A) @ np.abs(x)
        assert np.all(np.abs((prods[1] - prods[0]) - T) <= 32 * EPS * terms)
        assert np.abs(T[free]).min() > 0.0


def _refused(call, text):
    from multigrid_dolfinx_amd._capi import MgError
    with pytest.raises(MgError, match=text):
        call()


def _untouched(h, call, text, vectors=()):
    """`call` is refused with `text`; counters(), the face set, the reaction state and the given (level, name, bytes) vectors are
    as they were."""
    before = h.counters()
    faces, react, memory = h.diffusion_faces(), h.diffusion_reaction(), h.memory_bytes()
    _refused(call, text)
    assert h.counters() == before and h.diffusion_faces() == faces and h.diffusion_reaction() == react
    assert h.memory_bytes() == memory
    for level, name, want in vectors:
        assert h.get_vector(level, name).tobytes() == want, (level, name)


@pytest.mark.gpu
def test_reaction_refusals_leave_the_handle_as_it_was():
    """Every refusal by message; counters(), the face set, the reaction field and, where the handle has levels, V and F unchanged."""
    from multigrid_dolfinx_amd._capi import MgError
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N, nlev, top = 16, 3, 2
    kappa, sigma = _kappa(N), _sigma(N)
    nothing = lambda *args: None
    with DeviceHierarchy(2, 0, 1, c=4) as h2:
        _untouched(h2, lambda: h2.set_diffusion_reaction(np.ones(8 ** 3)), "3-D only")
        h2.set_diffusion_reaction(None)
        h2.gen_poisson_level(1)
        buf = _device_array(h2, np.ones(9 ** 3))
        try:
            p = buf.ptr.value
            _untouched(h2, lambda: h2.diffusion_dsigma(1, p, p, p), "sigma sensitivity is 3-D only")
            _untouched(h2, lambda: h2.diffusion_apply_dsigma(1, p, p, p), "sigma sensitivity is 3-D only")
        finally:
            buf.free()
    with DeviceHierarchy(3, 0, 1, c=4) as slab:
        slab.set_comm_callbacks(0, 2, nothing, nothing, nothing)
        _untouched(slab, lambda: slab.set_diffusion_reaction(np.ones(8 ** 3)), "whole \\(not slab\\) handle")
        buf = _device_array(slab, np.ones(9 ** 3))
        try:
            p = buf.ptr.value
            _untouched(slab, lambda: slab.set_diffusion_reaction(p, N=8), "whole \\(not slab\\) handle")
            _untouched(slab, lambda: slab.diffusion_dsigma(1, p, p, p), "whole \\(not slab\\) handle")
            _untouched(slab, lambda: slab.diffusion_apply_dsigma(1, p, p, p), "whole \\(not slab\\) handle")
        finally:
            buf.free()
    with DeviceHierarchy(3, 0, 1, c=4) as late:         # a slab handle made after the field was set: refused where it is read
        late.set_diffusion_reaction(np.ones(8 ** 3))
        late.set_comm_callbacks(0, 2, nothing, nothing, nothing)
        _untouched(late, lambda: late.gen_diffusion_level(1, _kappa(8)), "reaction term .*whole \\(not slab\\) handle")
        _untouched(late, lambda: late.gen_diffusion_level(1, _kappa(8), matrix_free=True), "whole \\(not slab\\) handle")
    with DeviceHierarchy(3, 0, 0, c=16) as flat:
        flat.set_flat_level(poisson.lexicographic_level(4, 2).A)
        buf = _device_array(flat, np.ones(125))
        try:
            p = buf.ptr.value
            _untouched(flat, lambda: flat.diffusion_dsigma(0, p, p, p), "flat")
            _untouched(flat, lambda: flat.diffusion_apply_dsigma(0, p, p, p), "flat")
        finally:
            buf.free()
    with _handle(N, nlev) as h:
        h.set_diffusion_faces(18)
        h.set_diffusion_reaction(sigma)
        h.gen_diffusion_hierarchy(kappa)
        v = np.random.default_rng(1).standard_normal(h.n_dofs(top))
        h.set_vector(top, "v", v)
        state = [(top, "v", v.tobytes()), (top, "f", h.get_vector(top, "f").tobytes()), (top - 1, "f", h.get_vector(top - 1, "f").tobytes())]
        untouched = lambda call, text: _untouched(h, call, text, state)
        # the field itself: the first bad cell, named alike by both variants
        cell = (5 * N + 7) * N + 3
        names = {}
        for bad in (-1.0, np.nan, np.inf, -np.inf):
            field = sigma.copy()
            field[cell], field[cell + 100] = bad, -2.0
            untouched(lambda: h.set_diffusion_reaction(field), "sigma must be finite and not negative: cell \\(3, 7, 5\\) = index %d holds" % cell)
            buf = _device_array(h, field)
            try:
                untouched(lambda: h.set_diffusion_reaction(buf.ptr.value, N=N), "sigma must be finite and not negative: cell \\(3, 7, 5\\) = index %d holds" % cell)
                for variant, arg in (("host", field), ("device", buf.ptr.value)):
                    try:
                        h.set_diffusion_reaction(arg, N=N)
                    except MgError as exc:
                        names[(bad if bad == bad else "nan", variant)] = str(exc).split(": ", 1)[1]
            finally:
                buf.free()
            key = bad if bad == bad else "nan"
            assert names[(key, "host")] == names[(key, "device")], names
        good = _device_array(h, sigma)
        held = [good]
        try:
            p = good.ptr.value
            untouched(lambda: h.set_diffusion_reaction(sigma.ctypes.data, N=N), "not device memory")
            from multigrid_dolfinx_amd._capi import check
            import ctypes as C
            untouched(lambda: check(h._lib.mg_set_diffusion_reaction(h._h, N, C.c_void_p(p))), "not host memory")
            untouched(lambda: h.set_diffusion_reaction(p, N=0), "elements_per_dim must be positive")
            # the face set 0 is still singular with a field in place
            untouched(lambda: h.set_diffusion_faces(0), "singular")
            # a field of another size than the level (the top level of a hierarchy), at every generating call
            h.set_diffusion_reaction(reaction_sigma(N // 2))
            msg = "elements_per_dim = %d, the reaction field .* has %d cells per dimension" % (N, N // 2)
            kbuf = _device_array(h, kappa)
            held.append(kbuf)
            untouched(lambda: h.gen_diffusion_level(top, kappa), msg)
            untouched(lambda: h.gen_diffusion_level(top, kappa, matrix_free=True), msg)
            untouched(lambda: h.gen_diffusion_hierarchy(kappa), msg)
            untouched(lambda: h.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=0), msg)
            untouched(lambda: h.gen_diffusion_hierarchy(kbuf.ptr.value), msg)
            untouched(lambda: h.refresh_diffusion_hierarchy(kbuf.ptr.value), msg)
            # a refresh with another has-sigma state than the levels'
            h.set_diffusion_reaction(None)
            untouched(lambda: h.refresh_diffusion_hierarchy(kbuf.ptr.value), "generated with a reaction term, the handle has no reaction field")
            h.set_diffusion_reaction(sigma)
            h.refresh_diffusion_hierarchy(kbuf.ptr.value)
            assert h.get_vector(top, "f").tobytes() == state[1][2]
            with _handle(N, nlev) as plain:
                plain.gen_diffusion_hierarchy(kappa)
                plain.set_diffusion_reaction(sigma)
                _untouched(plain, lambda: plain.refresh_diffusion_hierarchy(kappa), "generated without a reaction term, the handle has a reaction field")
            # the sensitivity entries
            n = h.n_dofs(top)
            nodes, cells, out = _device_array(h, v), _device_array(h, sigma), _device_array(h, np.zeros(n))
            held += [nodes, cells, out]
            a, w, o = nodes.ptr.value, cells.ptr.value, out.ptr.value
            h.set_vector(top, "v", v)
            for call, text in ((lambda: h.diffusion_dsigma(top, 0, a, o), "null pointer \\(a\\)"),
                               (lambda: h.diffusion_dsigma(top, a, 0, o), "null pointer \\(b\\)"),
                               (lambda: h.diffusion_dsigma(top, a, a, 0), "null pointer \\(out\\)"),
                               (lambda: h.diffusion_apply_dsigma(top, 0, a, o), "null pointer \\(dsigma\\)"),
                               (lambda: h.diffusion_apply_dsigma(top, w, 0, o), "null pointer \\(x\\)"),
                               (lambda: h.diffusion_apply_dsigma(top, w, a, 0), "null pointer \\(out\\)"),
                               (lambda: h.diffusion_dsigma(top, v.ctypes.data, a, o), "a is not device memory"),
                               (lambda: h.diffusion_dsigma(top, a, a, v.ctypes.data), "out is not device memory"),
                               (lambda: h.diffusion_apply_dsigma(top, sigma.ctypes.data, a, o), "dsigma is not device memory"),
                               (lambda: h.diffusion_apply_dsigma(top, w, v.ctypes.data, o), "x is not device memory"),
                               (lambda: h.diffusion_dsigma(top, a, a, a), "out overlaps a"),
                               (lambda: h.diffusion_dsigma(top, o, a, a + 8), "out overlaps b"),
                               (lambda: h.diffusion_apply_dsigma(top, w, a, a), "out overlaps x"),
                               (lambda: h.diffusion_apply_dsigma(top, w, a, w), "out overlaps dsigma")):
                untouched(call, text)
            assert out.download().tobytes() == np.zeros(n).tobytes()
            h.zero_vector(top, "v")
            assert len(h.pcg(rtol=1e-8, max_iter=100, level=top)) < 100
        finally:
            for d in held:
                d.free()


def _torch_first(worker):
    code = "import torch, sys; sys.path.insert(0, %r); import tests.diffusion_reaction_workers as w; w.%s()" % (ROOT, worker)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.gpu
def test_diffusion_solver_with_sigma_against_the_host():
    """DiffusionSolver with sigma, all six faces and ("x-", "x+"), N = 16, stored and matrix-free, kappa and sigma on the device
    and on the CPU: u, J, the gradients with respect to kappa, sigma, f and g and the kappa-, sigma- and mixed blocks of
    Hessian-vector products against the host adjoint, n_solves 2, 4 and 6 (`solver_worker`; REACTION_LIMIT holds the measured
    figure)."""
    assert "solver ok" in _torch_first("solver_worker")


@pytest.mark.gpu
def test_diffusion_solver_switches_between_sigma_and_none():
    assert "switch ok" in _torch_first("switch_worker")


@pytest.mark.gpu
def test_implicit_euler_by_composition_against_the_host_march():
    """Three implicit Euler steps written with solve, reaction_apply and same_operator: u^3 and the gradients with respect to
    kappa, u^0 and dt against a host march with its adjoint recursion; one generation, six solves (`euler_worker`)."""
    assert "euler ok" in _torch_first("euler_worker")
