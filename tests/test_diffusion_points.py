"""Point sources and point observations: the P1 evaluation S, the consistent point load S^T, the simplex gradient G and its
transpose G^T (mg_diffusion_point_sample, _load, _gradient, _gradient_t; mg_diffusion_points.hip.h) against their host
restatements in poisson.py, the restatements against exact fields and independent barycentric coordinates, and
DiffusionSolver.sample / point_load / sample_gradient through autograd."""
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from multigrid_dolfinx_amd import poisson
from tests.diffusion_points_workers import special_points, tie_points
from tests.diffusion_workers import lognormal_kappa
from tests.test_diffusion_flux import _simplex_mean_gradient

EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- host ------------------------------------------------------------------------------------------------------------------
def test_affine_field_is_reproduced_exactly():
    """u = c0 + a . x at N = 8 with dyadic a and c0, 200 points whose coordinates are multiples of 1/64 (0 and 1 among them):
    p * 8, the local coordinates, the weights, every product and every partial sum are dyadic numbers of a few bits, so
    `sample` is c0 + a . x and `sample_gradient` is a, both exactly."""
    N = 8
    a, c0 = np.array([0.5, -1.25, 3.0]), 0.75
    t = np.arange(N + 1) / N
    u = c0 + a[0] * t[None, None, :] + a[1] * t[None, :, None] + a[2] * t[:, None, None]
    rng = np.random.default_rng(0)
    pts = rng.integers(0, 65, (200, 3)) / 64.0
    pts[:8] = np.array(list(itertools.product((0.0, 1.0), repeat=3)))
    assert pts.min() == 0.0 and pts.max() == 1.0
    want = c0 + pts @ a
    got = poisson.diffusion_point_sample(N, pts, u)
    assert np.array_equal(got, want), np.abs(got - want).max()
    G = poisson.diffusion_point_gradient(N, pts, u)
    assert G.shape == (200, 3) and np.array_equal(G, np.broadcast_to(a, (200, 3)))


def test_points_at_the_nodes_return_the_field():
    """Points at all nodes of N = 5: one weight is 1.0, three are 0.0, and `sample` returns u to the bit."""
    N = 5
    n1 = N + 1
    ids = np.arange(n1 ** 3)
    pts = np.stack([ids % n1, (ids // n1) % n1, ids // (n1 * n1)], axis=1) / N
    u = np.random.default_rng(1).standard_normal(n1 ** 3)
    nodes, lam, _ = poisson.diffusion_point_locate(N, pts)
    assert np.array_equal(np.sort(lam, axis=1), np.broadcast_to([0.0, 0.0, 0.0, 1.0], lam.shape))
    assert np.array_equal(nodes[np.arange(ids.size), np.argmax(lam, axis=1)], ids)
    assert poisson.diffusion_point_sample(N, pts, u).tobytes() == u.tobytes()


def test_ties_take_the_stable_permutation_and_the_field_is_continuous():
    """Points with xi_x = xi_y, xi_y = xi_z, xi_x = xi_z and all three equal, on cell faces, edges, the main diagonal and the
    faces between simplices (N = 8: p * N is exact).  The located permutation is the stable descending one -- on a tie the
    lower axis first --, and the value is that of EVERY simplex of the cell that contains the point, within 4 ulp of
    sum |l_v u_v|: u_h is continuous, and each side is four products and three adds."""
    N = 8
    n1 = N + 1
    cells = [(0, 0, 0), (N - 1, N - 1, N - 1), (3, 0, 6)]
    pts = tie_points(N, cells)
    u = np.random.default_rng(2).standard_normal(n1 ** 3)
    nodes, lam, pi = poisson.diffusion_point_locate(N, pts)
    got = poisson.diffusion_point_sample(N, pts, u)
    stride = (1, n1, n1 * n1)
    tied = set()
    for m, p in enumerate(pts):
        t = p * N
        c = np.minimum(np.floor(t), N - 1)
        xi = t - c
        # the stable descending order, written out: by -xi, then by axis
        want_pi = sorted(range(3), key=lambda d: (-xi[d], d))
        assert list(pi[m]) == want_pi, (m, xi, pi[m])
        n_alternatives = 0
        for perm in itertools.permutations(range(3)):
            s = xi[list(perm)]
            if not (s[0] >= s[1] >= s[2]):
                continue                                     # the point does not lie in this simplex
            n_alternatives += 1
            n0 = int((c[2] * n1 + c[1]) * n1 + c[0])
            verts = [n0, n0 + stride[perm[0]], n0 + stride[perm[0]] + stride[perm[1]], n0 + sum(stride)]
            l = [1.0 - s[0], s[0] - s[1], s[1] - s[2], s[2]]
            terms = [l[v] * u[verts[v]] for v in range(4)]
            other = ((terms[0] + terms[1]) + terms[2]) + terms[3]
            assert abs(got[m] - other) <= 4 * EPS * sum(abs(t_) for t_ in terms), (m, perm, got[m], other)
        assert n_alternatives >= 2, (m, xi)                  # every one of these points ties
        tied.add(n_alternatives)
    assert tied == {2, 6}                                    # one pair equal: two simplices; all three equal: all six
    assert nodes.min() >= 0 and nodes.max() < n1 ** 3 and (lam >= 0.0).all()


def _exact_points(N, rng, count):
    """Points p whose product p * N is exactly c + xi with xi a multiple of 1/64: random (c, xi), p = (c + xi) / N rounded, kept
    where the product gives c + xi back.  Locate and the weights are then exact on both sides of the comparison below."""
    kept = []
    while len(kept) < count:
        want = rng.integers(0, N, 3) + rng.integers(0, 65, 3) / 64.0
        p = want / N
        if np.array_equal(p * float(N), want) and p.max() <= 1.0:
            kept.append(p)
    return np.array(kept)


@pytest.mark.parametrize("N", [3, 4])
def test_sample_and_gradient_against_barycentric_coordinates(N):
    """Random u, 300 points whose local coordinates are exact (`_exact_points`): per point the simplex is set up from its
    vertices as `_simplex_mean_gradient` does -- the gradients of the barycentrics through np.linalg.inv of the edge matrix
    times h, the barycentrics themselves through np.linalg.inv of the edge matrix in cell units applied to p * N - vertex 0 --
    and S and G are the sums over the four vertices.  The weights are exact on both sides and the inverses are of
    unimodular 0/1 matrices (times h), so each side carries the roundings of four products and three adds: the bound is
    8 eps times the sum of the absolute values of the terms, computed alongside.  Then the mean of G at the six simplex
    centroids of every cell (xi = 3/4, 1/2, 1/4 along the path) against the cell gradient, with that test's bound."""
    rng = np.random.default_rng(N)
    n1, h = N + 1, 1.0 / N
    u = rng.standard_normal(n1 ** 3)
    U = u.reshape(n1, n1, n1)
    pts = _exact_points(N, rng, 300)
    got_s = poisson.diffusion_point_sample(N, pts, u)
    got_g = poisson.diffusion_point_gradient(N, pts, u)
    _, _, pi = poisson.diffusion_point_locate(N, pts)
    worst_s = worst_g = 0.0
    for m, p in enumerate(pts):
        t = p * float(N)
        c = np.minimum(np.floor(t), N - 1).astype(int)
        path = [np.zeros(3, dtype=int)]
        for ax in pi[m]:
            nxt = path[-1].copy()
            nxt[ax] = 1
            path.append(nxt)
        S = np.array(path)                                                      # the simplex's vertices in the cell, (x, y, z)
        vals = np.array([U[c[2] + sz, c[1] + sy, c[0] + sx] for sx, sy, sz in S])
        E = (S[1:] - S[0]).T.astype(np.float64)
        B = np.linalg.inv(E * h).T @ np.hstack([-np.ones((3, 1)), np.eye(3)])    # gradients of the barycentrics
        inner = np.linalg.inv(E) @ (t - (c + S[0]))
        bary = np.concatenate([[1.0 - inner.sum()], inner])
        assert (bary >= 0.0).all(), (m, bary)                                   # the located simplex contains the point
        want_s, size_s = float(bary @ vals), float(np.abs(bary * vals).sum())
        worst_s = max(worst_s, abs(got_s[m] - want_s) / (8 * EPS * size_s))
        for d in range(3):
            want_g, size_g = float(B[d] @ vals), float(np.abs(B[d] * vals).sum())
            worst_g = max(worst_g, abs(got_g[m, d] - want_g) / (8 * EPS * size_g))
    print("N", N, "largest |difference| / bound: S", worst_s, "G", worst_g)
    assert worst_s <= 1.0 and worst_g <= 1.0
    # the six centroids of every cell
    ck, cj, ci = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    cells = np.stack([ci, cj, ck], axis=-1).reshape(-1, 3).astype(np.float64)
    mean = np.zeros((3, N ** 3))
    for perm in itertools.permutations(range(3)):
        xi = np.zeros(3)
        xi[list(perm)] = (0.75, 0.5, 0.25)
        cent = (cells + xi) / N
        _, _, located = poisson.diffusion_point_locate(N, cent)
        assert (located == np.array(perm)).all()
        mean += poisson.diffusion_point_gradient(N, cent, u).T
    mean /= 6.0
    want, size = _simplex_mean_gradient(N, u)
    ratio = (np.abs(mean.reshape(3, N, N, N) - poisson.diffusion_cell_gradient(N, None, u).reshape(3, N, N, N)) / (64 * EPS * size)).max()
    print("N", N, "centroid mean against the cell gradient: largest |difference| / bound", ratio)
    assert ratio <= 1.0
    assert (np.abs(mean.reshape(3, N, N, N) - want) / (64 * EPS * size)).max() <= 1.0


@pytest.mark.parametrize("N", [6, 8])
def test_the_operators_are_adjoint(N):
    """<w, S(u)> = <u, S^T(w)> and <p, G(u)> = <u, G^T(p)> with M = 300 random points, within 4 (M + 8) eps times the sum of the
    absolute values of the terms of both sides."""
    M = 300
    rng = np.random.default_rng(60 + N)
    pts = rng.random((M, 3))
    u, w, p = rng.standard_normal((N + 1) ** 3), rng.standard_normal(M), rng.standard_normal((M, 3))
    pairs = {"S": (w * poisson.diffusion_point_sample(N, pts, u), u * poisson.diffusion_point_load(N, pts, w)),
             "G": ((p * poisson.diffusion_point_gradient(N, pts, u)).reshape(-1), u * poisson.diffusion_point_gradient_t(N, pts, p))}
    for name, (ta, tb) in pairs.items():
        assert tb.size == (N + 1) ** 3
        bound = 4 * (M + 8) * EPS * (np.abs(ta).sum() + np.abs(tb).sum())
        print("N", N, name, ta.sum(), tb.sum(), "difference", abs(ta.sum() - tb.sum()), "bound", bound)
        assert abs(ta.sum() - tb.sum()) <= bound


def test_a_node_sums_its_points_in_ascending_order():
    """1000 points in one cell: `point_load` and `point_gradient_t` equal an explicit ascending Python loop to the bit, and the
    same points in reverse order change bits somewhere -- an order-free sum would not."""
    N, M = 5, 1000
    rng = np.random.default_rng(4)
    pts = (np.array([2.0, 4.0, 0.0]) + rng.random((M, 3))) / N
    w, p = rng.standard_normal(M), rng.standard_normal((M, 3))
    nodes, lam, pi = poisson.diffusion_point_locate(N, pts)
    assert np.unique(nodes).size == 8
    load, grad_t = np.zeros((N + 1) ** 3), np.zeros((N + 1) ** 3)
    for m in range(M):
        P = p[m][pi[m]]
        contrib = [(0.0 - P[0]) * float(N), (P[0] - P[1]) * float(N), (P[1] - P[2]) * float(N), P[2] * float(N)]
        for v in range(4):
            load[nodes[m, v]] = load[nodes[m, v]] + lam[m, v] * w[m]
            grad_t[nodes[m, v]] = grad_t[nodes[m, v]] + contrib[v]
    assert poisson.diffusion_point_load(N, pts, w).tobytes() == load.tobytes()
    assert poisson.diffusion_point_gradient_t(N, pts, p).tobytes() == grad_t.tobytes()
    assert poisson.diffusion_point_load(N, pts[::-1], w[::-1]).tobytes() != load.tobytes()
    assert poisson.diffusion_point_gradient_t(N, pts[::-1], p[::-1]).tobytes() != grad_t.tobytes()
    assert np.allclose(poisson.diffusion_point_load(N, pts[::-1], w[::-1]), load, rtol=0, atol=1e-10)


def test_host_restatements_refuse_points_outside_the_cube():
    pts = np.full((6, 3), 0.5)
    pts[4, 1], pts[2, 0], pts[3, 2] = 1.0 + 2.0 ** -52, np.nan, -0.25
    with pytest.raises(ValueError, match="point 2 is"):
        poisson.diffusion_point_locate(4, pts)
    with pytest.raises(ValueError, match=r"\(M, 3\)"):
        poisson.diffusion_point_locate(4, np.zeros(3))


# ---- device ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kernel_case(N):
    rng = np.random.default_rng(300 + N)
    pts = special_points(N, seed=N)
    M = pts.shape[0]
    x, w, p = rng.standard_normal((N + 1) ** 3), rng.standard_normal(M), rng.standard_normal((M, 3))
    want = {"sample": poisson.diffusion_point_sample(N, pts, x), "load": poisson.diffusion_point_load(N, pts, w),
            "gradient": poisson.diffusion_point_gradient(N, pts, x).reshape(-1), "gradient_t": poisson.diffusion_point_gradient_t(N, pts, p)}
    for a in (pts, x, w, p, *want.values()):
        a.setflags(write=False)
    return pts, x, w, p, want


def _check_entries(h, level, N, label):
    pts, x, w, p, want = _kernel_case(N)
    M = pts.shape[0]
    assert h.elements(level) == N
    calls = {"sample": lambda: h.diffusion_point_sample(level, M, pts, x), "load": lambda: h.diffusion_point_load(level, M, pts, w),
             "gradient": lambda: h.diffusion_point_gradient(level, M, pts, x),
             "gradient_t": lambda: h.diffusion_point_gradient_t(level, M, pts, p)}
    for name, call in calls.items():
        got = call()
        bad = np.flatnonzero(got != want[name])
        assert got.tobytes() == want[name].tobytes(), (label, name, bad[:5], bad.size)
        if name in ("load", "gradient_t"):
            assert call().tobytes() == got.tobytes(), (label, name, "a second call gave other bytes")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [8, 36, 72])
def test_kernels_match_the_host_restatements_to_the_bit(N):
    """The top level at N = 8 (fewer points per node plane than a block, every node among the points), 36 and 72 (off powers of
    two: p * N rounds), as a grid-only, a stored and a matrix-free level: 1000 random points and the special ones (nodes, ties,
    coordinates 0 and 1, 1000 points in one cell), all four entries with the bytes of the host restatements, each transpose
    twice with the same bytes."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.set_level_grid(1)
        _check_entries(h, 1, N, "grid-only")
    for matrix_free in (False, True):
        with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
            h.gen_diffusion_level(1, lognormal_kappa(N, 3, seed=1), matrix_free=matrix_free)
            assert h.level_matrix_free(1) == matrix_free
            _check_entries(h, 1, N, "matrix-free" if matrix_free else "stored")


@pytest.mark.gpu
def test_kernels_on_the_level_below_the_top():
    """A hierarchy with N = 36 on top: the entries on the level below it (N = 18), grid-only, stored and matrix-free."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 36
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.set_level_grid(0)
        h.set_level_grid(1)
        _check_entries(h, 0, N // 2, "grid-only, below the top")
    for min_rows in (None, 0):
        with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
            h.gen_diffusion_hierarchy(lognormal_kappa(N, 3, seed=1), matrix_free_min_rows=min_rows)
            _check_entries(h, 0, N // 2, "generated, below the top")
            _check_entries(h, 1, N, "generated, the top")


def _device_array(h, n, host=None):
    """n float64 on the handle's device without torch (which must not be imported after libmg_hip.so is loaded)."""
    from multigrid_dolfinx_amd.hierarchy import _DeviceArray
    return _DeviceArray(h._lib, h.device, n, host)


@pytest.mark.gpu
def test_refusals_name_their_cause_and_their_entry():
    import ctypes as C
    from multigrid_dolfinx_amd import _capi
    from multigrid_dolfinx_amd._capi import MgError
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N, M = 12, 40
    n = (N + 1) ** 3
    rng = np.random.default_rng(8)
    names = ("sample", "load", "gradient", "gradient_t")
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.gen_diffusion_level(1, np.ones(N ** 3), matrix_free=True)
        v = rng.standard_normal(n)
        h.set_vector(1, "v", v)
        good = rng.random((M, 3))
        bad = good.copy()
        bad[31, 1], bad[17, 2], bad[23, 0] = 1.0 + 2.0 ** -52, np.nan, -0.25
        sentinel = np.full(n, 7.0)
        bufs = [_device_array(h, 3 * M, good), _device_array(h, n, rng.standard_normal(n)), _device_array(h, n, sentinel),
                _device_array(h, 3 * M, bad)]
        try:
            pts, b, o, pts_bad = (d.ptr.value for d in bufs)
            host = np.zeros(n).ctypes.data
            entries = {"mg_diffusion_point_" + k: getattr(h, "diffusion_point_" + k) for k in names}
            counters = h.counters()
            for name, call in entries.items():
                for args in ((host, b, o), (pts, host, o), (pts, b, host)):
                    with pytest.raises(MgError, match=name + ": .* is not device memory"):
                        call(1, M, *args)
                for args in ((0, b, o), (pts, 0, o), (pts, b, 0)):
                    with pytest.raises(MgError, match=name + ": null pointer"):
                        call(1, M, *args)
                for args in ((pts, b, pts), (pts, b, b), (pts, b, pts + 8 * (3 * M - 1))):
                    with pytest.raises(MgError, match=name + ": out overlaps"):
                        call(1, M, *args)
                for count in (0, -3):
                    with pytest.raises(MgError, match=name + ": M = %d" % count):
                        call(1, count, pts, b, o)
                with pytest.raises(MgError, match=name + ": level 0 has not been set"):
                    call(0, M, pts, b, o)
                # (the Python layer refuses these two itself: straight to the library)
                raw = lambda handle, level: _capi.check(getattr(h._lib, name)(handle, level, C.c_int64(M), C.c_void_p(pts),
                                                                              C.c_void_p(b), C.c_void_p(o)))
                with pytest.raises(MgError, match=name + ": level 5 out of range"):
                    raw(h._h, 5)
                with pytest.raises(MgError, match=name + ": null handle"):
                    raw(None, 1)
                # 1 + 2^-52 at point 31, a NaN at 17, -0.25 at 23: the lowest index is named and out is unwritten
                with pytest.raises(MgError, match=name + ": a point must lie in the unit cube.*: point 17 is"):
                    call(1, M, pts_bad, b, o)
                assert bufs[2].download().tobytes() == sentinel.tobytes(), name
                with pytest.raises(TypeError):
                    call(1, M, pts, np.zeros(n), o)
            assert h.counters() == counters
            assert h.get_vector(1, "v").tobytes() == v.tobytes()
            with DeviceHierarchy(2, 0, 1, c=16) as h2:
                h2.gen_poisson_level(1)
                for name in entries:
                    with pytest.raises(MgError, match=name + ": .*2-D"):
                        getattr(h2, name[3:])(1, M, pts, b, o)
            with DeviceHierarchy(3, 0, 1, c=16) as hs:
                nothing = lambda *args: None
                hs.set_comm_callbacks(0, 2, nothing, nothing, nothing, replicate_below=0)
                for name in entries:
                    with pytest.raises(MgError, match=name + " needs a whole .*slab"):
                        getattr(hs, name[3:])(1, M, pts, b, o)
            with DeviceHierarchy(3, 0, 0, c=16) as hf:
                hf.set_flat_level(poisson.lexicographic_level(4, 2).A)
                for name in entries:
                    with pytest.raises(MgError, match=name + ": .*flat"):
                        getattr(hf, name[3:])(0, M, pts, b, o)
        finally:
            for d in bufs:
                d.free()
        # the handle that refused all of that still computes
        _check_entries(h, 1, N, "after the refusals")


def test_capi_names_the_four_entries():
    """Header and binding agree on the four new names (the library's side: tests/test_capi_symbols)."""
    from multigrid_dolfinx_amd import _capi
    header = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    for k in ("sample", "load", "gradient", "gradient_t"):
        name = "mg_diffusion_point_" + k
        assert "int %s(mg_handle h, int level, int64_t M, const double* pts_dev" % name in header
        assert len(_capi.SIGNATURES[name]) == 6


# ---- DiffusionSolver: in a process of its own that imports torch FIRST (see tests/test_diffusion_adjoint.py) -----------------
def _torch_first(worker):
    code = "import torch, sys; sys.path.insert(0, %r); import tests.diffusion_points_workers as w; w.%s()" % (ROOT, worker)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.gpu
def test_point_functions_pass_gradcheck_and_gradgradcheck():
    """gradcheck and gradgradcheck at torch's default tolerances on `sample`, `point_load` and `sample_gradient`, in the fields
    and in the points, N = 4 with 12 points kept away from simplex faces (`gradcheck_worker`)."""
    assert "gradcheck ok" in _torch_first("gradcheck_worker")


@pytest.mark.gpu
def test_source_position_gradient_against_central_differences():
    """N = 8, three levels, rtol 1e-12: dJ/dx_s of the receiver misfit of a point-source solve against central differences,
    1e-6 relative; the solution is 0 on the boundary although the load is not; `n_solves` counts the solves only
    (`end_to_end_worker`)."""
    assert "end to end ok" in _torch_first("end_to_end_worker")


@pytest.mark.gpu
def test_sampling_leaves_the_hierarchy_alone():
    """`sample`, `point_load` and `sample_gradient` before any solve leave `n_generations` and `n_solves` at 0, and the solve
    after them has the bytes of a solver that never called them (`idle_worker`)."""
    assert "idle ok" in _torch_first("idle_worker")
