"""Chebyshev polynomial smoother (MG_SMOOTH_CHEBYSHEV) with per-level Lanczos estimates of lambda_max(D^-1 A).
No reference counterpart: the reference smooths with weighted Jacobi only.

CPU: the binding, the NumPy reference (tests/cheb_reference.py) against the Chebyshev bound and ARPACK, NumPy cycles.
GPU: the estimate and the smoother against the NumPy reference on every storage format, first steps on a poisoned x_{k-1},
V-cycle / mg_pcg histories, symmetry of the cycle, scale, slabs and memory.
"""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from multigrid_dolfinx_amd import _capi, poisson
from tests import cheb_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mg_set_chebyshev", "mg_set_chebyshev_bounds", "mg_chebyshev_bounds", "mg_chebyshev_estimate_bytes")


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_binding_and_library():
    text = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    assert re.search(r"MG_SMOOTH_CHEBYSHEV\s*=\s*3", text)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _capi.SIGNATURES, name
        assert getattr(_capi.load(), name) is not None
    assert _capi.MG_SMOOTH_CHEBYSHEV == 3
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    for m in ("set_chebyshev", "set_chebyshev_bounds", "chebyshev_bounds"):
        assert callable(getattr(DeviceHierarchy, m))


def test_start_vector_is_splitmix64():
    # splitmix64(0) = 0xE220A8397B1DCDAF (the generator's published first output for seed 0)
    z = 0xE220A8397B1DCDAF
    assert ref.start_vector([0])[0] == (z >> 11) / 2.0 ** 52 - 1.0
    v = ref.start_vector(np.arange(100000))
    assert v.min() >= -1.0 and v.max() < 1.0 and abs(v.mean()) < 0.01


def test_step_scalars_reproduce_the_chebyshev_polynomial():
    """The three-term recurrence of the scalars is the scaled Chebyshev polynomial: on D^-1 A = lam, error e -> p_m(lam) e."""
    lo, hi = 0.3, 2.2
    for m in (1, 2, 3, 6):
        for lam in (0.35, 1.0, 1.7, 2.2):
            A = sp.csr_matrix(np.array([[1.0, lam - 1.0], [lam - 1.0, 1.0]]))     # D = I, (1, 1) has eigenvalue lam
            e = ref.smooth(A, np.zeros(2), np.ones(2), m, lo, hi)[0]
            assert abs(abs(e) - ref.chebyshev_bound(m, lo, hi, lam)) <= 1e-13, (m, lam)


@pytest.mark.parametrize("dim,N", [(2, 32), (3, 12)])
@pytest.mark.parametrize("m", [2, 3, 5])
def test_numpy_smoother_meets_the_chebyshev_bound(dim, N, m):
    """Error components with lambda(D^-1 A) in [a, b] shrink by at most max |p_m| on [a, b]."""
    A = ref.poisson_matrices(dim, N, 1)[0]
    d = ref.diagonal(A)
    s = sp.diags(1.0 / np.sqrt(d))
    w, V = np.linalg.eigh((s @ A @ s).toarray())
    hi = 1.1 * w[-1]
    lo = hi / 6.0
    sel = (w >= lo) & (w <= hi)
    e0 = (s @ V[:, sel]) @ np.random.default_rng(m).standard_normal(sel.sum())       # D^-1/2 eigenvectors of the range
    e = ref.smooth(A, np.zeros_like(e0), e0, m, lo, hi)
    bound = max(ref.chebyshev_bound(m, lo, hi, x) for x in np.linspace(lo, hi, 2001))
    dn = lambda x: np.linalg.norm(np.sqrt(d) * x)
    assert dn(e) <= bound * dn(e0) * (1 + 1e-9), (dn(e) / dn(e0), bound)


@pytest.mark.parametrize("dim,N", [(2, 32), (2, 64), (3, 8), (3, 16)])
def test_numpy_estimate_brackets_lambda_max(dim, N):
    A = ref.poisson_matrices(dim, N, 1)[0]
    est = 1.1 * ref.lanczos_lmax(A, 10)
    lam = ref.exact_lmax(A)
    assert lam <= est <= 1.25 * lam, (est, lam)


@pytest.mark.parametrize("dim,N0,nlev", [(2, 4, 5), (3, 4, 4)])       # 65^2, 33^3
@pytest.mark.parametrize("m", [2, 4])
def test_numpy_cycle_contracts_faster_than_jacobi(dim, N0, nlev, m):
    As = ref.poisson_matrices(dim, N0, nlev)
    f = np.random.default_rng(1).standard_normal(As[-1].shape[0])
    rho_j = ref.contraction(ref.Cycle(As, dim, N0, mu1=m, mu2=m, smoother="jacobi").history(f, 10))
    rho_c = ref.contraction(ref.Cycle(As, dim, N0, mu1=m, mu2=m).history(f, 10))
    assert rho_c < rho_j, (rho_c, rho_j)


def test_kuhn_assembly_is_the_poisson_matrix_without_jump():
    for dim, N in ((2, 16), (3, 8)):
        assert abs(ref.kuhn_diffusion(N, dim, jump=1.0) - ref.poisson_matrices(dim, N, 1)[0]).max() <= 1e-14


@pytest.mark.parametrize("dim,N0,nlev", [(2, 4, 5), (3, 4, 3)])
def test_numpy_cycle_on_a_coefficient_jump_with_galerkin_levels(dim, N0, nlev):
    """P1 diffusion with a 1 : 1000 jump, Galerkin coarse levels: both smoothers converge (factors in DESIGN.md)."""
    As = ref.galerkin_matrices(ref.kuhn_diffusion(N0 << (nlev - 1), dim), dim, N0, nlev)
    f = np.random.default_rng(2).standard_normal(As[-1].shape[0])
    for smoother in ("chebyshev", "jacobi"):
        rho = ref.contraction(ref.Cycle(As, dim, N0, smoother=smoother).history(f, 10))
        assert rho < 0.9, (smoother, rho)


# ---- GPU -------------------------------------------------------------------------------------------------------------
def _handle(As, dim, N0, smoother="chebyshev", mu=2, **tuning):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    h = DeviceHierarchy(dim, 0, len(As) - 1, c=N0, **tuning)
    for l, A in enumerate(As):
        h.set_level(l, A)
    h.set_params(mu, mu, 2.0 / 3.0, restriction="p1_transpose", smoother=smoother)
    h.set_prolongation("p1")
    return h


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@pytest.mark.gpu
@pytest.mark.parametrize("dim,N0,nlev", [(2, 4, 5), (3, 4, 6)])          # C1 (65^2) and 3-D levels 9^3 .. 129^3
def test_device_estimate_matches_numpy(dim, N0, nlev):
    As = ref.poisson_matrices(dim, N0, nlev)
    got = {}
    for graph in (0, 1):
        with _handle(As, dim, N0, graph=graph) as h:
            if graph:
                # the estimate runs from mg_prepare_cycle ahead of the first (captured) cycle; replays use its scalars
                top = nlev - 1
                h.set_vector(top, "f", np.ones(As[-1].shape[0]))
                h.zero_vector(top, "v")
                h.vcycle(top, 2)
                assert h.counters()["graph_replays"] >= 1
            got[graph] = [h.chebyshev_bounds(l) for l in range(1, nlev)]
            again = [h.chebyshev_bounds(l) for l in range(1, nlev)]
            assert again == got[graph]
    assert got[0] == got[1]                         # the same bits whether or not the estimate ran before captured cycles
    for l in range(1, nlev):
        b = got[0][l - 1]
        want = ref.lanczos_lmax(As[l], 10)
        assert abs(b["lmax_estimate"] - want) <= 1e-10 * want, (l, b, want)
        assert b["lmax"] == 1.1 * b["lmax_estimate"] and b["lmin"] == b["lmax"] / 6.0
        if As[l].shape[0] <= 65 ** 3:
            assert b["lmax"] >= ref.exact_lmax(As[l]), l


@pytest.mark.gpu
@pytest.mark.parametrize("dim,N", [(2, 64), (3, 16), (3, 32)])
@pytest.mark.parametrize("fmt", [dict(), dict(row_classes=0), dict(symmetric_storage=0),
                                 dict(symmetric_storage=0, offset_codes=0)])
def test_device_smoother_matches_numpy_on_every_format(dim, N, fmt):
    As = ref.poisson_matrices(dim, N // 4, 3)
    A = As[-1]
    rng = np.random.default_rng(N + dim)
    v0, f = rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0])
    lo, hi = 0.31, 2.17
    with _handle(As, dim, N // 4, **fmt) as h:
        h.set_chebyshev_bounds(2, lo, hi)
        assert h.chebyshev_bounds(2)["lmax"] == hi
        for m in range(1, 7):
            h.set_vector(2, "v", v0)
            h.set_vector(2, "f", f)
            h.reset_smoother_launches()
            h.smooth(2, m)
            got = h.get_vector(2, "v")[:, 0]
            want = ref.smooth(A, f, v0, m, lo, hi)
            assert _rel(got, want) <= 1e-12, (m, _rel(got, want))
            runs = h.smoother_launches(2)
            # (the default format takes the fused paths for m >= 2: small level / 2-D kernel; the others one step per launch)
            assert sum(w for _, w, _ in runs.values()) == m and set(runs) <= {"slice", "sweep1c", "small", "k2d"}, runs
            if fmt:
                assert set(runs) <= {"slice", "sweep1c"}, runs


@pytest.mark.gpu
def test_device_smoother_on_the_large_plane_march_and_a_p2_lattice():
    """The sdia_sweep1c plane march (a 3-D level above "march_min_rows", here forced low) and a P2 lattice level through
    the lattice march ("lattice_march_min_rows" low) and through its stencil classes."""
    As = ref.poisson_matrices(3, 16, 2)
    A = As[-1]
    rng = np.random.default_rng(9)
    v0, f = rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0])
    with _handle(As, 3, 16, march_min_rows=1000) as h:
        h.set_chebyshev_bounds(1, 0.25, 2.0)
        for m in (1, 2, 5):
            h.set_vector(1, "v", v0)
            h.set_vector(1, "f", f)
            h.reset_smoother_launches()
            h.smooth(1, m)
            assert _rel(h.get_vector(1, "v")[:, 0], ref.smooth(A, f, v0, m, 0.25, 2.0)) <= 1e-12
            assert h.smoother_launches(1) == {"sweep1c": (m, m, 0)}
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    lvl = poisson.p2_level(16, 3)
    A2 = sp.csr_matrix(lvl.A)
    v0, f = rng.standard_normal(A2.shape[0]), rng.standard_normal(A2.shape[0])
    for march in (1, 0):
        with DeviceHierarchy(3, 0, 0, c=32, lattice_march_min_rows=1000, lattice_march=march) as h:
            h.set_level(0, A2, lvl.grid_index if hasattr(lvl, "grid_index") else None)
            # which kernel a one-step launch takes: the lattice march exactly where "lattice" can be timed
            if march:
                h.time_kernel("lattice", 0, 1)
            else:
                with pytest.raises(_capi.MgError, match="lattice march"):
                    h.time_kernel("lattice", 0, 1)
            h.set_params(0, 0, 1.0, smoother="chebyshev")
            h.set_chebyshev_bounds(0, 0.2, 2.5)
            for m in (1, 4):
                h.set_vector(0, "v", v0)
                h.set_vector(0, "f", f)
                h.smooth(0, m)
                assert _rel(h.get_vector(0, "v")[:, 0], ref.smooth(A2, f, v0, m, 0.2, 2.5)) <= 1e-12, (march, m)


def _fused_pair(dim, lo, hi, levels, degrees, knob, **tuning):
    """V for each (level, degree) with `knob` 1 and 0; the smoother_launches of both."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    out = {}
    for on in (1, 0):
        with DeviceHierarchy.synthetic(dim, lo, hi, c=8, mu1=2, mu2=2, **{knob: on}, **tuning) as h:
            h.set_params(2, 2, 0.0, restriction="p1_transpose", smoother="chebyshev")
            for l in levels:
                h.set_chebyshev_bounds(l, 0.33, 2.05)
            rng = np.random.default_rng(8)
            for l in levels:
                n = h.n_dofs(l)
                v0, f = rng.standard_normal(n), rng.standard_normal(n)
                for m in degrees:
                    h.set_vector(l, "v", v0)
                    h.set_vector(l, "f", f)
                    h.reset_smoother_launches()
                    h.smooth(l, m)
                    out[(on, l, m)] = (h.get_vector(l, "v")[:, 0], h.smoother_launches(l))
    return out


@pytest.mark.gpu
def test_fused_small_level_steps_bit_identical_to_one_step():
    """The 17^2 and 33^2 levels of C1's kind: all steps of a call in one launch of one workgroup (32 per launch: 40 = 32 + 8, the second
    launch continuing from x_{k-1}) equal one step per launch bit for bit."""
    degrees = (1, 2, 3, 5, 6, 40)
    out = _fused_pair(2, 0, 3, (1, 2), degrees, "fuse_small", fuse_2d=0)
    for l in (1, 2):
        for m in degrees:
            (a, na), (b, nb) = out[(1, l, m)], out[(0, l, m)]
            assert np.array_equal(a, b), (l, m)
            assert nb == {"slice": (m, m, 0)}, nb
            want = {"small": ((m + 31) // 32, m, 0)} if m >= 2 else {"slice": (1, 1, 0)}
            assert na == want, (l, m, na)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_fused_2d_steps_bit_identical_to_one_step(k):
    """65^2 .. 1025^2: a whole call of at most fuse_2d_k steps in one launch of sdia_jacobik2d equals one step per launch bit for
    bit; longer calls (tails) run one step per launch."""
    degrees = tuple(range(1, k + 2))
    levels = (3, 5, 7)
    out = _fused_pair(2, 2, 7, levels, degrees, "fuse_2d", fuse_2d_k=k, fuse_small=0)
    for l in levels:
        for m in degrees:
            (a, na), (b, nb) = out[(1, l, m)], out[(0, l, m)]
            assert np.array_equal(a, b), (l, m)
            assert nb == {"slice": (m, m, 0)}, nb
            assert na == ({"k2d": (1, m, 0)} if 2 <= m <= k else {"slice": (m, m, 0)}), (l, m, na)


@pytest.mark.gpu
def test_first_step_ignores_a_poisoned_previous_iterate():
    As = ref.poisson_matrices(2, 8, 3)
    n = As[-1].shape[0]
    rng = np.random.default_rng(3)
    v0, f = rng.standard_normal(n), rng.standard_normal(n)
    out = {}
    for poison in (0.0, np.nan):
        with _handle(As, 2, 8) as h:
            h.set_chebyshev_bounds(2, 0.3, 2.2)
            h.set_vector(2, "r", np.full(n, poison))            # MG_VEC_R is the buffer that holds x_{k-1}
            h.set_vector(2, "v", v0)
            h.set_vector(2, "f", f)
            h.smooth(2, 3)
            out[poison == 0.0] = h.get_vector(2, "v")[:, 0]
    assert np.all(np.isfinite(out[False])) and np.array_equal(out[False], out[True])


def _device_histories(As, dim, N0, ncycles, f, **kw):
    with _handle(As, dim, N0, **kw) as h:
        top = len(As) - 1
        h.zero_vector(top, "v")
        h.set_vector(top, "f", f)
        hv = h.vcycle(top, ncycles, residuals=True)
        h.zero_vector(top, "v")
        hp = h.pcg(rtol=1e-10, max_iter=60)
    return hv, hp


def _galerkin_handle(dim, N0, nlev, **tuning):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    A = ref.kuhn_diffusion(N0 << (nlev - 1), dim)
    return A, DeviceHierarchy.galerkin_from_matrix(dim, 0, nlev - 1, A=A, c=N0, smoother="chebyshev", **tuning)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["c1", "33cube", "jump2d", "jump3d"])
def test_device_cycle_and_pcg_histories_match_numpy(case):
    dim, N0, nlev = {"c1": (2, 4, 5), "33cube": (3, 4, 4), "jump2d": (2, 4, 5), "jump3d": (3, 4, 4)}[case]
    bounds = None
    if case.startswith("jump"):
        A, h = _galerkin_handle(dim, N0, nlev)
        As = ref.galerkin_matrices(A, dim, N0, nlev)
        f = np.random.default_rng(4).standard_normal(A.shape[0])
        with h:
            if dim == 3:
                # the device's 3-D Galerkin levels of this operator are symmetric to round-off only (mg_level_storage: not
                # bit for bit), so the estimate refuses them: the caller sets their intervals
                bounds = {l: (1.1 * ref.lanczos_lmax(As[l]) / 6.0, 1.1 * ref.lanczos_lmax(As[l])) for l in range(1, nlev)}
                for l, (lo, hi) in bounds.items():
                    h.set_chebyshev_bounds(l, lo, hi)
            top = nlev - 1
            h.zero_vector(top, "v")
            h.set_vector(top, "f", f)
            hv = h.vcycle(top, 12, residuals=True)
            h.zero_vector(top, "v")
            hp = h.pcg(rtol=1e-10, max_iter=60)
    else:
        As = ref.poisson_matrices(dim, N0, nlev)
        f = np.random.default_rng(4).standard_normal(As[-1].shape[0])
        hv, hp = _device_histories(As, dim, N0, 12, f)
    cyc = ref.Cycle(As, dim, N0, bounds=bounds)
    want_v, want_p = cyc.history(f, 12), cyc.pcg(f, 1e-10, 60)
    keep = want_v >= 1e-4 * want_v[0]
    assert np.all(np.abs(hv[keep] - want_v[keep]) <= 1e-10 * want_v[keep]), (hv, want_v)
    keep = want_p >= 1e-4 * want_p[0]
    assert len(hp) == len(want_p)
    assert np.all(np.abs(hp[keep] - want_p[keep]) <= 1e-10 * want_p[keep]), (hp, want_p)
    assert hv[-1] < 1e-3 * hv[0]


@pytest.mark.gpu
@pytest.mark.parametrize("dim,N0,nlev", [(2, 4, 5), (3, 4, 4)])
def test_device_cycle_is_symmetric(dim, N0, nlev):
    """mu1 = mu2, direct coarsest solve, zero start: B is symmetric, |w.Bu - u.Bw| <= 1e-12 (|w||Bu| + |u||Bw|), on the
    interior unknowns (the Dirichlet rows are identity rows that the P1 prolongation reads and P^T does not)."""
    from tests import p1_reference as p1
    As = ref.poisson_matrices(dim, N0, nlev)
    n = As[-1].shape[0]
    rng = np.random.default_rng(6)
    inner = p1.interior(N0 << (nlev - 1), dim)
    u, w = rng.standard_normal(n) * inner, rng.standard_normal(n) * inner
    with _handle(As, dim, N0, mu=3) as h:
        top = nlev - 1

        def B(x):
            h.zero_vector(top, "v")
            h.set_vector(top, "f", x)
            h.vcycle(top, 1)
            return h.get_vector(top, "v")[:, 0]
        Bu, Bw = B(u), B(w)
    err = abs(w @ Bu - u @ Bw)
    assert err <= 1e-12 * (np.linalg.norm(w) * np.linalg.norm(Bu) + np.linalg.norm(u) * np.linalg.norm(Bw)), err


@pytest.mark.gpu
@pytest.mark.parametrize("dim,lo,hi", [(3, 1, 6), (2, 4, 11)])        # C3 257^3 (c = 4 -> 8 .. 256), C2 2049^2
def test_device_pcg_at_scale(dim, lo, hi):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    with DeviceHierarchy.synthetic(dim, lo, hi, c=4 if dim == 3 else 2, mu1=2, mu2=2) as h:
        h.set_params(2, 2, 0.0, restriction="p1_transpose", smoother="chebyshev")
        h.set_prolongation("p1")
        h.zero_vector(hi, "v")
        hist = h.pcg(rtol=1e-10, max_iter=100)
        assert len(hist) < 100 and hist[-1] <= 1e-10 * h.norm2(hi, "f") * (1 + 1e-12), (len(hist), hist[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("world,dim,c", [(2, 3, 4), (3, 2, 8)])
def test_device_chebyshev_on_slabs(world, dim, c):
    import torch.multiprocessing as mp
    from tests.dist_helpers import free_port
    from tests.cheb_workers import gpu_cheb_slab_worker
    mp.spawn(gpu_cheb_slab_worker, args=(world, free_port(), dim, 1, 3, c, 0), nprocs=world, join=True)


@pytest.mark.gpu
def test_device_memory_unchanged_by_the_estimate():
    As = ref.poisson_matrices(3, 4, 4)
    with _handle(As, 3, 4, smoother="jacobi") as h:
        h.prepare_cycle(3)
        before = h.memory_bytes()
        h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose", smoother="chebyshev")
        h.prepare_cycle(3)
        assert h.chebyshev_bounds(3)["lmax_estimate"] > 0
        assert h.memory_bytes() == before
        assert h.chebyshev_estimate_bytes() >= 4 * 8 * As[-1].shape[0]


@pytest.mark.gpu
def test_device_refuses_what_it_cannot_estimate():
    """A non-symmetric level is refused unless its interval is set; the caller's interval then works."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    As = ref.poisson_matrices(2, 8, 2)
    A = As[1].tolil()
    A[40, 41] *= 1.5
    A = sp.csr_matrix(A)
    with DeviceHierarchy(2, 0, 1, c=8) as h:         # (the coarsest level gets no symmetry test: level 1 carries the matrix)
        h.set_level(0, As[0])
        h.set_level(1, A)
        assert h.level_storage(1)["symmetric"] == 0
        h.set_params(0, 0, 1.0, smoother="chebyshev")
        with pytest.raises(_capi.MgError, match="not symmetric"):
            h.smooth(1, 2)
        h.set_chebyshev_bounds(1, 0.3, 2.2)
        v0 = np.ones(A.shape[0])
        h.set_vector(1, "v", v0)
        h.set_vector(1, "f", np.zeros(A.shape[0]))
        h.smooth(1, 2)
        assert _rel(h.get_vector(1, "v")[:, 0], ref.smooth(A, np.zeros(A.shape[0]), v0, 2, 0.3, 2.2)) <= 1e-12
