"""The kappa tangent of the diffusion operator, T(dkappa, x) = (dA/dkappa . dkappa) x (mg_diffusion_apply_dkappa: the SpMV
march of mg_diffusion_mf.hip.h with kappa := dkappa and zero boundary rows; host restatement
poisson.diffusion_apply_dkappa), the tangent solve and the second derivatives of torch_diffusion.DiffusionSolver against
host references built on scipy's spsolve (tests/diffusion_tangent_workers.py)."""
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from multigrid_dolfinx_amd import poisson
from tests.diffusion_adjoint_workers import host_adjoint
from tests.diffusion_tangent_workers import host_hessian_vector, row_bound, row_terms
from tests.diffusion_workers import lognormal_kappa
from tests.test_diffusion_mf import STORED_ONE_STEP, _fma

EPS = np.finfo(np.float64).eps


def _inner(N):
    m = np.zeros((N + 1,) * 3, dtype=bool)
    m[1:-1, 1:-1, 1:-1] = True
    return m.reshape(-1)


def _within_row_bound(N, dkappa, x, got, want, what):
    """|got - want| <= row_bound per row; prints the largest ratio of error to bound."""
    bound = row_bound(N, dkappa, x)
    err = np.abs(got - want)
    some = bound > 0.0          # (0 on boundary rows and on the 2^3 rows inside a block of 3^3 zero cells: the error must be 0 there)
    assert some.sum() >= _inner(N).sum() - 8
    print(what, "N", N, "largest error / bound", float((err[some] / bound[some]).max()), "largest error", float(err.max()))
    assert np.all(err <= bound), (what, int(np.argmax(err - bound)))


def _adjoint_identity(N, dkappa, D, a, x, T, what):
    """dkappa . D(a, x) = a~ . T(dkappa, x) to 64 eps times the sum of the absolute values of the terms of both sides: the
    cells' products on the left, the products of the rows' entries on the right."""
    at = np.where(_inner(N), a, 0.0)
    lhs_terms = dkappa * D
    rhs_abs = float((np.abs(at) * np.abs(row_terms(N, dkappa, x))).sum())
    lhs, rhs = float(lhs_terms.sum()), float(at @ T)
    bound = 64 * EPS * (float(np.abs(lhs_terms).sum()) + rhs_abs)
    print(what, "N", N, "lhs", lhs, "rhs", rhs, "difference", abs(lhs - rhs), "bound", bound)
    assert abs(lhs - rhs) <= bound, what


# ---- host ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [6, 8])
def test_restatement_against_assembled_matrices(N):
    """T(kappa_1 - kappa_2, x) = (A(kappa_1) - A(kappa_2)) x on interior rows, within the per-row bound
    16 eps (h / 6) sum_e (sum_c n_c |dkappa_c|)(|x_i| + |x~_j|), and exactly 0 on boundary rows, x with non-zero boundary."""
    rng = np.random.default_rng(N)
    k1, k2 = np.exp(rng.standard_normal(N ** 3)), np.exp(rng.standard_normal(N ** 3))
    x = rng.standard_normal((N + 1) ** 3)
    assert np.all(x != 0.0)
    got = poisson.diffusion_apply_dkappa(N, k1 - k2, x)
    assert got.shape == ((N + 1) ** 3,)
    inner = _inner(N)
    assert not got[~inner].any() and got[inner].all()
    want = (poisson.diffusion_level(N, 3, k1).A - poisson.diffusion_level(N, 3, k2).A) @ x
    _within_row_bound(N, k1 - k2, x, got, np.where(inner, want, 0.0), "restatement against A(k1) - A(k2)")
    # the boundary entries of x do not count: an interior row has no boundary column
    assert poisson.diffusion_apply_dkappa(N, k1 - k2, np.where(inner, x, 0.0)).tobytes() == got.tobytes()


@pytest.mark.parametrize("N", [6, 8])
def test_adjoint_identity_on_the_host(N):
    """dkappa . D(a, x) = a~ . T(dkappa, x) for standard-normal dkappa: T is the transpose of D in its first argument."""
    rng = np.random.default_rng(40 + N)
    dkappa = rng.standard_normal(N ** 3)
    a, x = rng.standard_normal((N + 1) ** 3), rng.standard_normal((N + 1) ** 3)
    _adjoint_identity(N, dkappa, poisson.diffusion_dkappa(N, a, x), a, x, poisson.diffusion_apply_dkappa(N, dkappa, x), "host")


def _div6(t):
    """mf_div6 of mg_diffusion_mf.hip.h, operation for operation: the range test is on |t|."""
    if not (2.0 ** -900 <= abs(t) <= 2.0 ** 900):
        return t / 6.0
    c = float.fromhex("0x1.5555555555555p-3")
    q = t * c
    r = _fma(-q, 6.0, t)
    return _fma(r, c, q)


def test_division_by_six_shortcut_for_negative_zero_and_subnormal_arguments():
    """The method of test_division_by_six_shortcut_is_correctly_rounded on the negated arguments (10^6 random mantissas across
    the exponents of the fast range, its edges, powers of two, multiples of six and their neighbours), on +-0 and on
    subnormals of both signs: the bits of / 6.0, the sign of a zero included."""
    rng = np.random.default_rng(0)
    m = rng.integers(1 << 52, 1 << 53, size=1_000_000).astype(np.float64)
    e = rng.integers(-899, 900, size=m.size)
    cases = (-np.ldexp(m, e - 52)).tolist()
    edge = [0.0, -0.0]
    for p in list(range(-1074, -1000, 3)) + list(range(-905, -895)) + list(range(-60, 61)) + list(range(895, 905)) + [1020, 1023]:
        x = 2.0 ** p
        for y in (x, np.nextafter(x, 0.0), np.nextafter(x, np.inf), 3.0 * x, 6.0 * x if p < 1020 else x,
                  np.nextafter(6.0 * x if p < 1020 else x, 0.0), np.nextafter(6.0 * x if p < 1020 else x, np.inf)):
            edge.append(-float(y))
    tiny = np.finfo(np.float64).tiny
    for y in (5e-324, 3 * 5e-324, 6 * 5e-324, 7 * 5e-324, tiny / 2, np.nextafter(tiny, 0.0), tiny, np.nextafter(tiny, 1.0),
              np.finfo(np.float64).max):
        edge += [float(y), -float(y)]
    sub = np.ldexp(rng.integers(1, 1 << 52, size=1000).astype(np.float64), -1074)
    assert np.all(sub < tiny)
    edge += sub.tolist() + (-sub).tolist()
    bad = [(t, _div6(t), t / 6.0) for t in cases + edge if struct.pack("<d", _div6(t)) != struct.pack("<d", t / 6.0)]
    assert not bad, bad[:5]
    assert struct.pack("<d", _div6(-0.0)) == struct.pack("<d", -0.0)


def test_host_hessian_vector_product_against_finite_differences():
    """J = 1/2 ||u - d||^2 at N = 6 with spsolve: along three relative directions the discrepancy (l2) between the
    four-solve Hessian-vector product and central differences of host_adjoint's gradient falls by a factor between 3 and
    5 from step 0.01 to 0.005 -- second-order convergence towards the product, the test and the band of
    test_host_adjoint_gradient_against_finite_differences."""
    N, eps = 6, 0.01
    rng = np.random.default_rng(3)
    kappa = np.exp(rng.standard_normal(N ** 3))
    f, d = rng.standard_normal((N + 1) ** 3), rng.standard_normal((N + 1) ** 3)
    grad = lambda k: host_adjoint(N, k, f, d)[2]
    lam = lambda k: host_adjoint(N, k, f, d)[3]
    for t in range(3):
        v = np.random.default_rng(10 + t).standard_normal(N ** 3) * kappa
        v /= np.abs(v / kappa).max()
        hk, hf = host_hessian_vector(N, kappa, f, d, v)
        err = [float(np.linalg.norm((grad(kappa + s * v) - grad(kappa - s * v)) / (2 * s) - hk)) for s in (eps, eps / 2)]
        erf = [float(np.linalg.norm((lam(kappa + s * v) - lam(kappa - s * v)) / (2 * s) - hf)) for s in (eps, eps / 2)]
        print("direction", t, "|H v|", float(np.linalg.norm(hk)), "discrepancies", err, "ratio", err[0] / err[1],
              "f block", erf, "ratio", erf[0] / erf[1])
        assert 3.0 <= err[0] / err[1] <= 5.0, (t, err)
        assert 3.0 <= erf[0] / erf[1] <= 5.0, (t, erf)


# ---- device: the kernel ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kernel_case(N):
    rng = np.random.default_rng(200 + N)
    x, a = rng.standard_normal((N + 1) ** 3), rng.standard_normal((N + 1) ** 3)
    dkappa = rng.standard_normal(N ** 3)
    dkappa[rng.random(N ** 3) < 0.1] = 0.0                  # exact zeros, and a block of 3^3 zero cells around a node
    dkappa.reshape(N, N, N)[2:5, 1:4, 3:6] = 0.0
    kappa = lognormal_kappa(N, 3, seed=1)
    for v in (x, a, dkappa, kappa):
        v.setflags(write=False)
    return kappa, dkappa, x, a


def _levels(N, kappa):
    """The three kinds of 3-D level the entry runs on: (name, a handle whose level 1 is of that kind)."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    for name in ("stored", "matrix_free", "poisson"):
        with DeviceHierarchy(3, 0, 1, c=N // 2, **(STORED_ONE_STEP if name == "stored" else {})) as h:
            if name == "poisson":
                h.gen_poisson_level(1)
            else:
                h.gen_diffusion_level(1, kappa, matrix_free=name == "matrix_free")
                assert h.level_matrix_free(1) == (name == "matrix_free")
            yield name, h


SHAPES = [8, 36, 72, 128]       # smaller than a tile; partial tiles in x and y and a second tile column; several z segments


@pytest.mark.gpu
@pytest.mark.parametrize("N", SHAPES)
def test_kernel_carries_the_bits_of_the_residual(N):
    """With dkappa := a log-normal kappa the interior rows of T(kappa, x) are the negated residual of that kappa's level with
    V = x and F = 0 (0 - acc is exact), of the stored level's one-step kernel and of the matrix-free march, on a stored,
    a matrix-free and a grid-only level; boundary rows are exactly zero although x is not."""
    kappa, _, x, _ = _kernel_case(N)
    assert np.all(x != 0.0)
    inner = _inner(N)
    got, residual = {}, {}
    for name, h in _levels(N, kappa):
        got[name] = h.diffusion_apply_dkappa(1, kappa, x)
        if name != "poisson":
            h.set_vector(1, "v", x)
            h.zero_vector(1, "f")
            h.residual(1)
            residual[name] = h.get_vector(1, "r").reshape(-1)
    for name, T in got.items():
        assert not T[~inner].any(), name
        for level, r in residual.items():
            bad = np.flatnonzero(T[inner] != -r[inner])
            assert np.array_equal(T[inner], -r[inner]), (name, level, bad[:5], bad.size)


@pytest.mark.gpu
@pytest.mark.parametrize("N", SHAPES)
def test_kernel_sign_symmetry_restatement_and_adjoint_identity(N):
    """Standard-normal dkappa with exact zeros and a 3^3 block of zero cells: T(-dkappa, x) = -T(dkappa, x) to the bit (the
    division by six takes the same operations for both signs), T within the per-row bound of the host restatement, and
    dkappa . D(a, x) = a~ . T(dkappa, x) with both sides from the device."""
    kappa, dkappa, x, a = _kernel_case(N)
    want = poisson.diffusion_apply_dkappa(N, dkappa, x)
    first = None
    for name, h in _levels(N, kappa):
        T = h.diffusion_apply_dkappa(1, dkappa, x)
        assert np.array_equal(h.diffusion_apply_dkappa(1, -dkappa, x), -T), name
        if first is None:
            first = T
            _within_row_bound(N, dkappa, x, T, want, "device against the restatement")
            _adjoint_identity(N, dkappa, h.diffusion_dkappa(1, a, x), a, x, T, "device")
        assert T.tobytes() == first.tobytes(), name         # the level's kind does not matter


def _device_array(h, n, host=None):
    from multigrid_dolfinx_amd.hierarchy import _DeviceArray
    return _DeviceArray(h._lib, h.device, n, host)


@pytest.mark.gpu
def test_refusals_name_their_cause():
    from multigrid_dolfinx_amd._capi import MgError
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 32
    with DeviceHierarchy(3, 0, 1, c=16) as h:
        h.gen_diffusion_level(1, np.ones(N ** 3), matrix_free=True)
        n = (N + 1) ** 3
        bufs = [_device_array(h, n, np.zeros(n)), _device_array(h, n, np.zeros(n)), _device_array(h, 2 * n, np.zeros(2 * n))]
        try:
            k, p, o = (b.ptr.value for b in bufs)
            host = np.zeros(n)
            h.set_vector(1, "v", np.arange(n, dtype=np.float64))
            before = h.get_vector(1, "v").copy()
            counters = h.counters()
            for call in (lambda: h.diffusion_apply_dkappa(1, host.ctypes.data, p, o), lambda: h.diffusion_apply_dkappa(1, k, host.ctypes.data, o),
                         lambda: h.diffusion_apply_dkappa(1, k, p, host.ctypes.data)):
                with pytest.raises(MgError, match="mg_diffusion_apply_dkappa.*not device memory"):
                    call()
            for call in (lambda: h.diffusion_apply_dkappa(1, 0, p, o), lambda: h.diffusion_apply_dkappa(1, k, 0, o),
                         lambda: h.diffusion_apply_dkappa(1, k, p, 0)):
                with pytest.raises(MgError, match="mg_diffusion_apply_dkappa.*null pointer"):
                    call()
            # out on x, out beginning inside x, x beginning inside out; and out on the direction
            for call in (lambda: h.diffusion_apply_dkappa(1, k, p, p), lambda: h.diffusion_apply_dkappa(1, k, o, o + 8 * (n - 1)),
                         lambda: h.diffusion_apply_dkappa(1, k, o + 8 * (n - 1), o)):
                with pytest.raises(MgError, match="mg_diffusion_apply_dkappa: out overlaps x"):
                    call()
            with pytest.raises(MgError, match="mg_diffusion_apply_dkappa: out overlaps dkappa"):
                h.diffusion_apply_dkappa(1, k, p, k)
            assert h.counters() == counters
            assert h.get_vector(1, "v").tobytes() == before.tobytes()
            for call in (lambda: h.diffusion_apply_dkappa(1, k, host, o), lambda: h.diffusion_apply_dkappa(1, host, p, o),
                         lambda: h.diffusion_apply_dkappa(1, k, p), lambda: h.diffusion_apply_dkappa(1, host[:N ** 3], host, o)):
                with pytest.raises(TypeError):
                    call()
            h.diffusion_apply_dkappa(1, k, o + 8 * n, o)        # next to each other is not overlapping
            with DeviceHierarchy(2, 0, 1, c=16) as h2:
                h2.gen_poisson_level(1)
                with pytest.raises(MgError, match="mg_diffusion_apply_dkappa.*2-D"):
                    h2.diffusion_apply_dkappa(1, k, p, o)
            with DeviceHierarchy(3, 0, 1, c=16) as hs:
                nothing = lambda *a: None
                hs.set_comm_callbacks(0, 2, nothing, nothing, nothing, replicate_below=0)
                with pytest.raises(MgError, match="mg_diffusion_apply_dkappa.*slab"):
                    hs.diffusion_apply_dkappa(1, k, p, o)
            with DeviceHierarchy(3, 0, 0, c=16) as hf:
                hf.set_flat_level(poisson.lexicographic_level(4, 2).A)
                with pytest.raises(MgError, match="mg_diffusion_apply_dkappa.*flat"):
                    hf.diffusion_apply_dkappa(0, k, p, o)
        finally:
            for b in bufs:
                b.free()


@pytest.mark.gpu
def test_timing_name_runs_the_kernel():
    """ "apply_dkappa" takes dkappa from the first N^3 entries of F and x from V, and leaves in R what the entry returns."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 36
    kappa, dkappa, x, _ = _kernel_case(N)
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.gen_diffusion_level(1, kappa, matrix_free=True)
        want = h.diffusion_apply_dkappa(1, dkappa, x)
        assert np.count_nonzero(want) >= _inner(N).sum() - 8    # (the 2^3 rows inside the block of zero cells are 0)
        h.set_vector(1, "v", x)
        h.set_vector(1, "f", np.concatenate([dkappa, np.full((N + 1) ** 3 - N ** 3, np.nan)]))
        h.set_vector(1, "r", np.full((N + 1) ** 3, np.nan))
        assert h.time_kernel("apply_dkappa", 1, reps=2) > 0.0
        assert h.get_vector(1, "r").reshape(-1).tobytes() == want.tobytes()


# ---- DiffusionSolver: in a process of its own that imports torch FIRST (see tests/test_diffusion_adjoint.py) ----------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_first(worker):
    code = "import torch, sys; sys.path.insert(0, %r); import tests.diffusion_tangent_workers as w; w.%s()" % (ROOT, worker)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.gpu
def test_tangent_solve_against_the_host():
    """N = 16, two levels, log-normal kappa, rtol 1e-12: du of DiffusionSolver.tangent against spsolve(A, df - T(dkappa, u)) in
    relative l2, stored and matrix-free; one generation and two solves (`tangent_worker`, whose SECOND_ORDER_LIMIT holds the
    measured figures)."""
    assert "tangent ok" in _torch_first("tangent_worker")


@pytest.mark.gpu
def test_hessian_vector_product_against_the_host():
    """g = grad(J, kappa, create_graph=True), then grad(g . v, (kappa, f)): against the host's four-solve product and its f
    block, in four solves on one generation, stored and matrix-free (`hessian_worker`)."""
    assert "hessian ok" in _torch_first("hessian_worker")


@pytest.mark.gpu
def test_first_order_backward_is_unchanged():
    """A plain J.backward() takes two solves in all and reports them as "forward" and "adjoint"; a double backward on the same
    solver leaves the kept warm-start solutions alone (`first_order_worker`)."""
    assert "first order ok" in _torch_first("first_order_worker")
