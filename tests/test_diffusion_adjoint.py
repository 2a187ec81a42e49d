"""Differentiable diffusion solves: the kappa sensitivity of the operator (mg_diffusion_dkappa, mg_diffusion_adj.hip.h, and its
host restatement poisson.diffusion_dkappa), the device-pointer vector calls, and the adjoint gradient of
torch_diffusion.DiffusionSolver against a host adjoint built on scipy's spsolve."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spl

from multigrid_dolfinx_amd import poisson
from tests.diffusion_adjoint_workers import host_adjoint as _host_adjoint, host_solve as _host_solve
from tests.diffusion_workers import lognormal_kappa

EPS = np.finfo(np.float64).eps


def _masked(N, x):
    """x with the boundary nodes of the (N + 1)^3 grid set to zero."""
    v = np.array(x, dtype=np.float64).reshape(N + 1, N + 1, N + 1)
    m = np.zeros_like(v)
    m[1:-1, 1:-1, 1:-1] = v[1:-1, 1:-1, 1:-1]
    return m.reshape(-1)


# ---- host ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [6, 8])
def test_dkappa_against_assembled_matrices(N):
    """(kappa_1 - kappa_2) . out = a~^T (A(kappa_1) - A(kappa_2)) b~ with the matrices of poisson.diffusion_level, a and b random
    with non-zero boundary entries.  Both sides are sums of products; the bound is 64 eps times the sum of the absolute
    values of the terms of both sides (a rounding bound: every term carries a few roundings of its own -- the kappa sums,
    the division by six, the differences -- and the sums are far shorter than 1 / eps)."""
    rng = np.random.default_rng(N)
    k1, k2 = np.exp(rng.standard_normal(N ** 3)), np.exp(rng.standard_normal(N ** 3))
    a, b = rng.standard_normal((N + 1) ** 3), rng.standard_normal((N + 1) ** 3)
    assert np.all(a != 0.0) and np.all(b != 0.0)
    out = poisson.diffusion_dkappa(N, a, b)
    assert out.shape == (N ** 3,)
    D = (poisson.diffusion_level(N, 3, k1).A - poisson.diffusion_level(N, 3, k2).A).tocoo()
    at, bt = _masked(N, a), _masked(N, b)
    lhs_terms = (k1 - k2) * out
    rhs_terms = at[D.row] * D.data * bt[D.col]
    bound = 64 * EPS * (np.abs(lhs_terms).sum() + np.abs(rhs_terms).sum())
    print("N", N, "lhs", lhs_terms.sum(), "rhs", rhs_terms.sum(), "difference", abs(lhs_terms.sum() - rhs_terms.sum()), "bound", bound)
    assert abs(lhs_terms.sum() - rhs_terms.sum()) <= bound
    # the boundary entries of a and b do not matter, and the result is symmetric in (a, b)
    assert poisson.diffusion_dkappa(N, at, bt).tobytes() == out.tobytes()
    assert poisson.diffusion_dkappa(N, b, a).tobytes() == out.tobytes()


def test_host_adjoint_gradient_against_finite_differences():
    """J = 1/2 ||u - d||^2 at N = 6 with spsolve: along three random directions the discrepancy between the adjoint
    gradient and central differences falls by a factor between 3 and 5 from step eps to eps / 2 -- second-order
    convergence towards the adjoint value.  Directions are relative (|v / kappa| <= 1) and eps = 0.01: truncation
    (about 1e-4 here) is then far above the round-off of the difference quotient (about 1e-14 / eps)."""
    N, eps = 6, 0.01
    rng = np.random.default_rng(3)
    kappa = np.exp(rng.standard_normal(N ** 3))
    f, d = rng.standard_normal((N + 1) ** 3), rng.standard_normal((N + 1) ** 3)
    J = lambda k: 0.5 * float(np.sum((_host_solve(N, k, f) - d) ** 2))
    _, _, g, _ = _host_adjoint(N, kappa, f, d)
    for t in range(3):
        v = np.random.default_rng(10 + t).standard_normal(N ** 3) * kappa
        v /= np.abs(v / kappa).max()
        err = [abs((J(kappa + s * v) - J(kappa - s * v)) / (2 * s) - g @ v) for s in (eps, eps / 2)]
        print("direction", t, "g.v", g @ v, "discrepancies", err, "ratio", err[0] / err[1])
        assert 3.0 <= err[0] / err[1] <= 5.0, (t, err)


# ---- device ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kernel_case(N):
    rng = np.random.default_rng(100 + N)
    a, b = rng.standard_normal((N + 1) ** 3), rng.standard_normal((N + 1) ** 3)
    want = {"ab": poisson.diffusion_dkappa(N, a, b), "aa": poisson.diffusion_dkappa(N, a, a)}
    for x in (a, b, *want.values()):
        x.setflags(write=False)
    return a, b, want


@pytest.mark.gpu
@pytest.mark.parametrize("N", [8, 36, 72, 128])
def test_kernel_matches_the_host_restatement_to_the_bit(N):
    """8: a level smaller than one tile; 36 / 72: 37 / 73 nodes per line, partial tiles in x and y and a second tile column;
    128: several z segments.  The plane march and the plain form ("dkappa_gather"), on a stored and on a matrix-free level,
    a != b and a and b the same pointer: the bytes of poisson.diffusion_dkappa every time."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    a, b, want = _kernel_case(N)
    assert np.all(a != 0.0) and np.all(b != 0.0)    # (the boundary entries are non-zero: the mask matters)
    kappa = lognormal_kappa(N, 3, seed=1)
    for matrix_free in (False, True):
        with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
            h.gen_diffusion_level(1, kappa, matrix_free=matrix_free)
            assert h.level_matrix_free(1) == matrix_free
            for gather in (0, 1):
                h.set_tuning("dkappa_gather", gather)
                got = h.diffusion_dkappa(1, a, b)
                bad = np.flatnonzero(got != want["ab"])
                assert got.tobytes() == want["ab"].tobytes(), (matrix_free, gather, bad[:5], bad.size)
                got = h.diffusion_dkappa(1, a, a)
                assert got.tobytes() == want["aa"].tobytes(), (matrix_free, gather, "a is b")


@pytest.mark.gpu
def test_timing_names_run_both_kernels():
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 36
    a, b, want = _kernel_case(N)
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.gen_diffusion_level(1, lognormal_kappa(N, 3, seed=1), matrix_free=True)
        for name in ("dkappa", "dkappa_gather"):
            h.set_vector(1, "v", a)
            h.set_vector(1, "f", b)
            h.zero_vector(1, "r")
            assert h.time_kernel(name, 1, reps=2) > 0.0
            assert h.get_vector(1, "r").reshape(-1)[:N ** 3].tobytes() == want["ab"].tobytes(), name


def _device_array(h, n, host=None):
    """n float64 on the handle's device without torch (which must not be imported after libmg_hip.so is loaded)."""
    from multigrid_dolfinx_amd.hierarchy import _DeviceArray
    return _DeviceArray(h._lib, h.device, n, host)


def _round_trips(h, level, n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n)
    dev, back = _device_array(h, n, x), _device_array(h, n, np.full(n, np.nan))
    try:
        before = h.counters()
        h.set_vector_device(level, "v", dev.ptr.value)
        h.get_vector_device(level, "v", back.ptr.value)
        assert h.counters() == before
        assert back.download().tobytes() == x.tobytes()
        assert h.get_vector(level, "v").tobytes() == x.tobytes()            # set by pointer, read through the host
        y = rng.standard_normal(n)
        h.set_vector(level, "f", y)                                         # set through the host, read by pointer
        before = h.counters()
        h.get_vector_device(level, "f", back.ptr.value)
        assert h.counters() == before
        assert back.download().tobytes() == y.tobytes()
    finally:
        dev.free()
        back.free()
    return x


@pytest.mark.gpu
def test_pointer_round_trips_on_a_generated_level():
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 32
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.gen_diffusion_level(1, lognormal_kappa(N, 3, seed=2))
        _round_trips(h, 1, h.n_dofs(1))


@pytest.mark.gpu
def test_pointer_round_trips_on_a_permuted_level():
    """A level handed over in a shuffled DoF numbering: the device calls permute like the host calls, and the library's own
    (lexicographic) copy is the permuted vector."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    lvl = poisson.make_level(16, 2, seed=7)
    assert not np.array_equal(lvl.grid_index, np.arange(lvl.grid_index.size))
    with DeviceHierarchy(2, 1, 1, c=8) as h, DeviceHierarchy(2, 1, 1, c=8) as lex:
        h.set_level(1, lvl.A, lvl.grid_index)
        x = _round_trips(h, 1, h.n_dofs(1))
        # the same vector in lexicographic numbering gives the same norm bits on a lexicographic handle
        plain = poisson.lexicographic_level(16, 2)
        lex.set_level(1, plain.A, plain.grid_index)
        xl = np.empty_like(x)
        xl[lvl.grid_index] = x
        lex.set_vector(1, "v", xl)
        assert h.norm2(1, "v") == lex.norm2(1, "v")


@pytest.mark.gpu
def test_refusals_name_their_cause():
    from multigrid_dolfinx_amd._capi import MgError
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    with DeviceHierarchy(3, 0, 1, c=16) as h:
        h.gen_diffusion_level(1, np.ones(32 ** 3), matrix_free=True)
        buf = _device_array(h, 33 ** 3, np.zeros(33 ** 3))
        try:
            p = buf.ptr.value
            host = np.zeros(33 ** 3)
            before = h.get_vector(1, "v").copy()
            counters = h.counters()
            for call in (lambda: h.set_vector_device(1, "v", host.ctypes.data), lambda: h.get_vector_device(1, "v", host.ctypes.data),
                         lambda: h.diffusion_dkappa(1, host.ctypes.data, p, p), lambda: h.diffusion_dkappa(1, p, host.ctypes.data, p),
                         lambda: h.diffusion_dkappa(1, p, p, host.ctypes.data)):
                with pytest.raises(MgError, match="not device memory"):
                    call()
            for call in (lambda: h.diffusion_dkappa(1, 0, p, p), lambda: h.diffusion_dkappa(1, p, p, 0),
                         lambda: h.set_vector_device(1, "v", 0)):
                with pytest.raises(MgError, match="null pointer"):
                    call()
            assert h.counters() == counters
            assert h.get_vector(1, "v").tobytes() == before.tobytes()
            with pytest.raises(TypeError):
                h.diffusion_dkappa(1, p, host, p)
            with DeviceHierarchy(2, 0, 1, c=16) as h2:
                h2.gen_poisson_level(1)
                with pytest.raises(MgError, match="2-D"):
                    h2.diffusion_dkappa(1, p, p, p)
            with DeviceHierarchy(3, 0, 1, c=16) as hs:
                nothing = lambda *a: None
                hs.set_comm_callbacks(0, 2, nothing, nothing, nothing, replicate_below=0)
                with pytest.raises(MgError, match="slab"):
                    hs.diffusion_dkappa(1, p, p, p)
                with pytest.raises(MgError, match="slab"):
                    hs.set_vector_device(1, "v", p)
                with pytest.raises(MgError, match="slab"):
                    hs.get_vector_device(1, "v", p)
            with DeviceHierarchy(3, 0, 0, c=16) as hf:
                hf.set_flat_level(poisson.lexicographic_level(4, 2).A)
                with pytest.raises(MgError, match="flat"):
                    hf.diffusion_dkappa(0, p, p, p)
        finally:
            buf.free()


# ---- DiffusionSolver: in a process of its own that imports torch FIRST ----------------------------------------------------
# torch ships its own HIP runtime under the soname libmg_hip.so links against.  A process that imports torch first has one
# runtime, shared by torch and the library, and device pointers mean the same to both; the test session loaded libmg_hip.so
# long before, bound to the system's runtime, and torch could not even initialise beside it.  The bodies are in
# tests/diffusion_adjoint_workers.py; each prints its figures and exits non-zero on a failed assertion.
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_first(worker):
    code = "import torch, sys; sys.path.insert(0, %r); import tests.diffusion_adjoint_workers as w; w.%s()" % (ROOT, worker)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.gpu
def test_device_gradient_against_the_host_adjoint():
    """N = 16, two levels, log-normal kappa, J = 1/2 ||u - d||^2: grad_kappa and grad_f of DiffusionSolver (rtol 1e-12)
    against the host adjoint (spsolve) in relative l2, with a stored and with a matrix-free top level, and the two device
    gradients against each other (`gradient_worker`, whose GRADIENT_LIMIT holds the measured figures)."""
    assert "gradient ok" in _torch_first("gradient_worker")


@pytest.mark.gpu
def test_two_sgd_steps_on_log_kappa_lower_the_misfit():
    """N = 32, three levels: two steps of torch.optim.SGD on log kappa lower J = 1/2 ||u(kappa) - d||^2, every time, and the
    kappa gradient is finite and non-zero in every cell (`sgd_worker`)."""
    assert "sgd ok" in _torch_first("sgd_worker")


@pytest.mark.gpu
def test_a_solve_that_cannot_converge_raises():
    """A max_iter too small for the adjoint solve, or for the forward solve, raises NotConverged and leaves no gradient
    (`max_iter_worker`)."""
    assert "max_iter ok" in _torch_first("max_iter_worker")


@pytest.mark.gpu
def test_library_loaded_before_torch_is_refused_by_name():
    """In this session libmg_hip.so is loaded and torch is not the runtime it uses: DiffusionSolver says so instead of failing
    somewhere inside torch."""
    code = ("import sys; sys.path.insert(0, %r); from multigrid_dolfinx_amd import _capi; _capi.load();\n"
            "from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver\n"
            "try:\n    DiffusionSolver(16, 2)\nexcept RuntimeError as exc:\n    print('refused:', exc)\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "refused:" in out.stdout and "import torch before" in out.stdout, out.stdout
