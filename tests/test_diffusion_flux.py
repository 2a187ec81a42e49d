"""Cell gradients and fluxes of diffusion solutions: F(w, x), its transpose F^T(w, p) and the contraction C(p, x)
(mg_diffusion_cell_gradient, _t, _dot; mg_diffusion_flux.hip.h) against their host restatements in poisson.py, the restatements
against independent assembly, and DiffusionSolver.gradient / flux against a host adjoint built on scipy's spsolve."""
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from multigrid_dolfinx_amd import poisson
from tests.diffusion_flux_workers import host_flux_adjoint, host_flux_misfit
from tests.diffusion_workers import lognormal_kappa

EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- host ------------------------------------------------------------------------------------------------------------------
def test_affine_field_has_its_slope_in_every_cell():
    """u = c0 + a . x at N = 8 with dyadic a and c0: node values, differences and weighted sums are exact, the accumulator
    is 6 a_d / 8 exactly, and the only roundings are N / 6.0 and one product -- G_d = a_d within 2 ulp in every cell."""
    N = 8
    a, c0 = (0.5, -1.25, 3.0), 0.75
    t = np.arange(N + 1) / N
    u = c0 + a[0] * t[None, None, :] + a[1] * t[None, :, None] + a[2] * t[:, None, None]
    G = poisson.diffusion_cell_gradient(N, None, u).reshape(3, N ** 3)
    for d in range(3):
        worst = np.abs(G[d] - a[d]).max()
        print("axis", d, "slope", a[d], "largest deviation", worst, "in ulp", worst / np.spacing(abs(a[d])))
        assert worst <= 2 * np.spacing(abs(a[d]))


def _simplex_mean_gradient(N, u):
    """The mean over the six Kuhn simplices of a cell of the gradient of the P1 interpolant, and the sum of the absolute
    values of the terms that make it, both (3, N, N, N): barycentric gradients through np.linalg.inv, as
    tests/cheb_reference.kuhn_diffusion builds its element matrices."""
    h = 1.0 / N
    U = np.asarray(u).reshape(N + 1, N + 1, N + 1)
    mean, size = np.zeros((3, N, N, N)), np.zeros((3, N, N, N))
    for perm in itertools.permutations(range(3)):
        path = [np.zeros(3, dtype=int)]
        for ax in perm:
            nxt = path[-1].copy()
            nxt[ax] = 1
            path.append(nxt)
        S = np.array(path)                                                      # vertices (x, y, z) of the simplex
        E = ((S[1:] - S[0]) * h).T
        B = np.linalg.inv(E).T @ np.hstack([-np.ones((3, 1)), np.eye(3)])       # gradients of the barycentrics
        for v, (sx, sy, sz) in enumerate(S):
            corner = U[sz:sz + N, sy:sy + N, sx:sx + N]
            for d in range(3):
                mean[d] += B[d, v] * corner / 6.0
                size[d] += np.abs(B[d, v] * corner) / 6.0
    return mean, size


@pytest.mark.parametrize("N", [3, 4])
def test_gradient_against_independent_assembly(N):
    """Random u: G equals the mean over the six Kuhn simplices of gradients built with np.linalg.inv.  Both sides are short
    sums of products of magnitude |B_dv u_v| / 6; each term carries a few roundings (the inverse of a matrix of condition
    below ten, the product, the division, against the restatement's differences, N / 6.0 and one product), so the bound is 64
    eps times the sum of the absolute values of the terms, cell by cell."""
    u = np.random.default_rng(N).standard_normal((N + 1) ** 3)
    want, size = _simplex_mean_gradient(N, u)
    got = poisson.diffusion_cell_gradient(N, None, u).reshape(3, N, N, N)
    ratio = (np.abs(got - want) / (64 * EPS * size)).max()
    print("N", N, "largest |difference| / bound", ratio)
    assert ratio <= 1.0
    w = np.random.default_rng(N + 10).standard_normal(N ** 3)
    assert poisson.diffusion_cell_gradient(N, w, u).tobytes() == (w.reshape(N, N, N) * got).tobytes()


@pytest.mark.parametrize("N", [6, 8])
def test_the_three_operators_are_adjoint(N):
    """<p, F(w, x)> = <x, F^T(w, p)> = <w, C(p, x)> with random w of both signs, within 64 eps times the sum of the absolute
    values of the terms of both sides (the bound of test_dkappa_against_assembled_matrices); F(None, x) == F(ones, x) bytewise,
    and F^T alike."""
    rng = np.random.default_rng(40 + N)
    w, x, p = rng.standard_normal(N ** 3), rng.standard_normal((N + 1) ** 3), rng.standard_normal(3 * N ** 3)
    assert (w > 0).any() and (w < 0).any()
    sides = {"<p, F(w, x)>": p * poisson.diffusion_cell_gradient(N, w, x),
             "<x, F^T(w, p)>": x * poisson.diffusion_cell_gradient_t(N, w, p),
             "<w, C(p, x)>": w * poisson.diffusion_cell_gradient_dot(N, p, x)}
    assert [v.size for v in sides.values()] == [3 * N ** 3, (N + 1) ** 3, N ** 3]
    for (na, ta), (nb, tb) in itertools.combinations(sides.items(), 2):
        bound = 64 * EPS * (np.abs(ta).sum() + np.abs(tb).sum())
        print("N", N, na, ta.sum(), nb, tb.sum(), "difference", abs(ta.sum() - tb.sum()), "bound", bound)
        assert abs(ta.sum() - tb.sum()) <= bound
    ones = np.ones(N ** 3)
    assert poisson.diffusion_cell_gradient(N, None, x).tobytes() == poisson.diffusion_cell_gradient(N, ones, x).tobytes()
    assert poisson.diffusion_cell_gradient_t(N, None, p).tobytes() == poisson.diffusion_cell_gradient_t(N, ones, p).tobytes()


def test_host_flux_adjoint_against_finite_differences():
    """J(kappa) = 1/2 h^3 ||flux(kappa, u(kappa)) - q_obs||^2 at N = 6 with spsolve and the restatements: along three relative
    directions the discrepancy between the adjoint gradient and central differences falls by a factor between 3 and 5 from
    step 0.01 to 0.005 -- the criterion of test_host_adjoint_gradient_against_finite_differences."""
    N, eps = 6, 0.01
    rng = np.random.default_rng(3)
    kappa = np.exp(rng.standard_normal(N ** 3))
    f, q_obs = rng.standard_normal((N + 1) ** 3), rng.standard_normal(3 * N ** 3)
    J = lambda k: host_flux_misfit(N, k, f, q_obs)[0]
    _, _, g, _ = host_flux_adjoint(N, kappa, f, q_obs)
    for t in range(3):
        v = np.random.default_rng(10 + t).standard_normal(N ** 3) * kappa
        v /= np.abs(v / kappa).max()
        err = [abs((J(kappa + s * v) - J(kappa - s * v)) / (2 * s) - g @ v) for s in (eps, eps / 2)]
        print("direction", t, "g.v", g @ v, "discrepancies", err, "ratio", err[0] / err[1])
        assert 3.0 <= err[0] / err[1] <= 5.0, (t, err)


# ---- device ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kernel_case(N):
    rng = np.random.default_rng(200 + N)
    w, x, p = rng.standard_normal(N ** 3), rng.standard_normal((N + 1) ** 3), rng.standard_normal(3 * N ** 3)
    want = {("f", True): poisson.diffusion_cell_gradient(N, w, x), ("f", False): poisson.diffusion_cell_gradient(N, None, x),
            ("t", True): poisson.diffusion_cell_gradient_t(N, w, p), ("t", False): poisson.diffusion_cell_gradient_t(N, None, p),
            ("c", True): poisson.diffusion_cell_gradient_dot(N, p, x)}
    for a in (w, x, p, *want.values()):
        a.setflags(write=False)
    return w, x, p, want


def _check_entries(h, level, N, label):
    w, x, p, want = _kernel_case(N)
    for weighted in (True, False):
        got = h.diffusion_cell_gradient(level, w if weighted else None, x)
        bad = np.flatnonzero(got != want["f", weighted])
        assert got.tobytes() == want["f", weighted].tobytes(), (label, "F", weighted, bad[:5], bad.size)
        got = h.diffusion_cell_gradient_t(level, w if weighted else None, p)
        bad = np.flatnonzero(got != want["t", weighted])
        assert got.tobytes() == want["t", weighted].tobytes(), (label, "F^T", weighted, bad[:5], bad.size)
    got = h.diffusion_cell_gradient_dot(level, p, x)
    bad = np.flatnonzero(got != want["c", True])
    assert got.tobytes() == want["c", True].tobytes(), (label, "C", bad[:5], bad.size)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [8, 36, 72, 128])
def test_kernels_match_the_host_restatements_to_the_bit(N):
    """8: a plane smaller than one block; 36 / 72: planes that are no multiple of the block, 37 / 73 nodes per line; 128:
    many blocks per plane.  Each of the three entries, w given and null, on a grid-only level and on a matrix-free generated
    level: the bytes of the poisson restatement every time.  (The sizes are those the plane-march forms were tested at before
    the measurements retired them; there is one form per entry and no tuning key.)"""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.set_level_grid(1)
        _check_entries(h, 1, N, "grid-only")
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.gen_diffusion_level(1, lognormal_kappa(N, 3, seed=1), matrix_free=True)
        assert h.level_matrix_free(1)
        _check_entries(h, 1, N, "matrix-free")


@pytest.mark.gpu
def test_timing_names_run_every_entry():
    """The mg_time_kernel names of the family run and leave the bytes of the restatements in MG_VEC_R: w = F[:N^3], x = V and
    p = (V, F, V)[:N^3] per component."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 36
    n, cells = (N + 1) ** 3, N ** 3
    rng = np.random.default_rng(7)
    v, f = rng.standard_normal(n), rng.standard_normal(n)
    w, p = f[:cells], np.concatenate([v[:cells], f[:cells], v[:cells]])
    want = {"cell_grad": poisson.diffusion_cell_gradient(N, w, v)[:n], "cell_grad_nw": poisson.diffusion_cell_gradient(N, None, v)[:n],
            "cell_grad_dot": poisson.diffusion_cell_gradient_dot(N, p, v), "cell_grad_t": poisson.diffusion_cell_gradient_t(N, w, p)}
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.gen_diffusion_level(1, lognormal_kappa(N, 3, seed=1), matrix_free=True)
        for name in ("cell_grad", "cell_grad_nw", "cell_grad_dot", "cell_grad_t"):
            h.set_vector(1, "v", v)
            h.set_vector(1, "f", f)
            h.zero_vector(1, "r")
            assert h.time_kernel(name, 1, reps=2) > 0.0
            expect = want[name]
            assert h.get_vector(1, "r").reshape(-1)[:expect.size].tobytes() == expect.tobytes(), name


def _device_array(h, n, host=None):
    """n float64 on the handle's device without torch (which must not be imported after libmg_hip.so is loaded)."""
    from multigrid_dolfinx_amd.hierarchy import _DeviceArray
    return _DeviceArray(h._lib, h.device, n, host)


@pytest.mark.gpu
def test_refusals_name_their_cause_and_their_entry():
    from multigrid_dolfinx_amd._capi import MgError
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 32
    n, cells = (N + 1) ** 3, N ** 3
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.gen_diffusion_level(1, np.ones(cells), matrix_free=True)
        bufs = [_device_array(h, 3 * cells, np.zeros(3 * cells)) for _ in range(3)]
        try:
            a, b, o = (d.ptr.value for d in bufs)
            host = np.zeros(3 * cells).ctypes.data
            entries = {"mg_diffusion_cell_gradient": h.diffusion_cell_gradient, "mg_diffusion_cell_gradient_t": h.diffusion_cell_gradient_t,
                       "mg_diffusion_cell_gradient_dot": h.diffusion_cell_gradient_dot}
            counters = h.counters()
            for name, call in entries.items():
                for args in ((host, b, o), (a, host, o), (a, b, host)):
                    with pytest.raises(MgError, match=name + ": .* is not device memory"):
                        call(1, *args)
                for args in ((a, 0, o), (a, b, 0)):
                    with pytest.raises(MgError, match=name + ": null pointer"):
                        call(1, *args)
                for args in ((a, b, a), (a, b, b), (a, b, b + 8 * (cells - 1))):
                    with pytest.raises(MgError, match=name + ": out overlaps"):
                        call(1, *args)
                with pytest.raises(TypeError):
                    call(1, a, np.zeros(3 * cells), o)
            with pytest.raises(MgError, match="mg_diffusion_cell_gradient_dot: null pointer"):
                h.diffusion_cell_gradient_dot(1, 0, b, o)           # (only w may be null)
            assert h.counters() == counters
            with DeviceHierarchy(2, 0, 1, c=16) as h2:
                h2.gen_poisson_level(1)
                for name, call in ((k, getattr(h2, v.__name__)) for k, v in entries.items()):
                    with pytest.raises(MgError, match=name + ": .*2-D"):
                        call(1, a, b, o)
            with DeviceHierarchy(3, 0, 1, c=16) as hs:
                nothing = lambda *args: None
                hs.set_comm_callbacks(0, 2, nothing, nothing, nothing, replicate_below=0)
                for name, call in ((k, getattr(hs, v.__name__)) for k, v in entries.items()):
                    with pytest.raises(MgError, match=name + " needs a whole .*slab"):
                        call(1, a, b, o)
            with DeviceHierarchy(3, 0, 0, c=16) as hf:
                hf.set_flat_level(poisson.lexicographic_level(4, 2).A)
                for name, call in ((k, getattr(hf, v.__name__)) for k, v in entries.items()):
                    with pytest.raises(MgError, match=name + ": .*flat"):
                        call(0, a, b, o)
        finally:
            for d in bufs:
                d.free()
        # the handle that refused all of that still computes
        _check_entries(h, 1, N, "after the refusals")


# ---- DiffusionSolver: in a process of its own that imports torch FIRST (see tests/test_diffusion_adjoint.py) -----------------
def _torch_first(worker):
    code = "import torch, sys; sys.path.insert(0, %r); import tests.diffusion_flux_workers as w; w.%s()" % (ROOT, worker)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.gpu
def test_gradient_and_flux_pass_gradcheck_and_gradgradcheck():
    """torch.autograd.gradcheck and gradgradcheck at torch's default tolerances on `gradient` and `flux`, N = 4, two levels,
    weight None and given, kappa on the device and on the CPU (`gradcheck_worker`)."""
    assert "gradcheck ok" in _torch_first("gradcheck_worker")


@pytest.mark.gpu
def test_flux_misfit_gradients_against_the_host_adjoint():
    """N = 16, two levels, log-normal kappa, rtol 1e-12, stored and matrix-free: grad_kappa and grad_f of
    J = 1/2 h^3 ||flux(kappa, u(kappa)) - q_obs||^2 against the host adjoint, and the solve counts of a gradient and of a
    Hessian-vector product (`end_to_end_worker`, whose FLUX_GRADIENT_LIMIT holds the measured figures)."""
    assert "end to end ok" in _torch_first("end_to_end_worker")


@pytest.mark.gpu
def test_gradient_leaves_the_hierarchy_alone():
    """`gradient` works before any solve, and the solve after it has the bytes of a solver that never called it
    (`non_interference_worker`)."""
    assert "non-interference ok" in _torch_first("non_interference_worker")
