"""Flexible CG preconditioned by one V-cycle per iteration (`mg_pcg`, `DeviceHierarchy.pcg`, `MultigridPCG`).

CPU: the binding and the NumPy recurrence (tests/pcg_reference.py) -- the iteration counts it reaches on the reference's
own parameters.  GPU: the device solve against that recurrence, its contract (vector roles, counters, errors), determinism,
convergence against plain V-cycles at scale, and slabs."""
import numpy as np
import pytest

from multigrid_dolfinx_amd import _capi, poisson
from tests.helpers import bag_from_fixture, load_golden, rel_l2
from tests.pcg_reference import fcg

FULL = ["c1_lex", "c1_perm"]


def _c1(name):
    from oracle.mg_oracle import Oracle
    bag, gi, _ = bag_from_fixture(load_golden(name))
    return bag, gi, Oracle(bag, gi, dim=2)


def _p1_3d(mu, seed=None):
    from oracle.mg_oracle import Oracle
    bag = poisson.make_hierarchy(3, 1, 3, c=4, mu1=mu, mu2=mu, seed=seed)
    gi = {l: L.grid_index for l, L in bag.levels.items()}
    return bag, gi, Oracle(bag, gi, dim=3)


def _true_rel_residual(bag, x):
    hi = bag.finest_level
    b = bag.b_dict[hi].reshape(-1, 1)
    return float(np.linalg.norm(b - bag.A_sp_dict[hi][0].dot(np.asarray(x).reshape(-1, 1))) / np.linalg.norm(b))


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_pcg_is_declared_bound_and_exported():
    import ctypes as C
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mg_hip.h")).read()
    assert "int mg_pcg(mg_handle h, int level, double rtol, int max_iter, double* resid_hist, int* iterations);" in header
    assert _capi.SIGNATURES["mg_pcg"] == [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    assert _capi.load().mg_pcg.argtypes == _capi.SIGNATURES["mg_pcg"]


@pytest.mark.parametrize("name", FULL)
def test_reference_recurrence_on_the_c1_fixture(name):
    """The reference's own 64^2 case, V(50,50) with injection: 15 flexible CG iterations to 1e-11 ||b|| (plain V-cycles
    do not get there in 80)."""
    bag, _, orc = _c1(name)
    x, hist = fcg(orc, bag.b_dict[bag.finest_level], rtol=1e-11, max_iter=80)
    assert len(hist) == 15
    assert hist[-1] <= 1e-11 * np.linalg.norm(bag.b_dict[bag.finest_level])
    assert _true_rel_residual(bag, x) <= 2e-11


def test_reference_recurrence_in_3d():
    """3-D, 32^3 elements on levels 1..3, V(50,50): 10 iterations."""
    bag, _, orc = _p1_3d(50)
    x, hist = fcg(orc, bag.b_dict[3], rtol=1e-11, max_iter=80)
    assert len(hist) == 10
    assert _true_rel_residual(bag, x) <= 2e-11


def test_reference_recurrence_start_and_limits():
    """A start that already solves the system takes no iteration; max_iter bounds the count; rtol <= 0 runs exactly
    max_iter iterations."""
    bag, _, orc = _c1("c1_lex")
    b = bag.b_dict[3]
    x, hist = fcg(orc, b, rtol=1e-11, max_iter=80)
    _, again = fcg(orc, b, rtol=1e-6, max_iter=80, x0=x)
    assert len(again) == 0
    assert len(fcg(orc, b, rtol=1e-11, max_iter=3)[1]) == 3
    assert len(fcg(orc, b, rtol=0.0, max_iter=4)[1]) == 4


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _device_run(dev, hi, f, rtol, max_iter, v0=None):
    dev.set_vector(hi, "v", np.zeros_like(f) if v0 is None else v0)
    dev.set_vector(hi, "f", f)
    hist = dev.pcg(rtol=rtol, max_iter=max_iter, level=hi)
    return hist, dev.get_vector(hi, "v")


def _match(hist, x, want_hist, want_x):
    assert len(hist) == len(want_hist)
    assert np.all(np.abs(hist - want_hist) <= 1e-6 * want_hist), np.max(np.abs(hist - want_hist) / want_hist)
    assert rel_l2(x, want_x) <= 1e-8, rel_l2(x, want_x)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FULL)
def test_device_pcg_matches_reference_on_c1(name):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    bag, gi, orc = _c1(name)
    f = bag.b_dict[3]
    want_x, want_hist = fcg(orc, f, rtol=0.0, max_iter=12)
    with DeviceHierarchy.from_bag(bag, dim=2, grid_index=gi) as dev:
        hist, x = _device_run(dev, 3, f, 0.0, 12)
    _match(hist, x, want_hist, want_x)


@pytest.mark.gpu
@pytest.mark.parametrize("mu,restriction,iters", [(50, "direct", 8), (2, "direct", 15), (2, "full_weighting", 15),
                                                  (50, "full_weighting", 8)])
def test_device_pcg_matches_reference_in_3d(mu, restriction, iters):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    bag, gi, orc = _p1_3d(mu, seed=2)
    f = bag.b_dict[3]
    want_x, want_hist = fcg(orc, f, rtol=0.0, max_iter=iters, restriction=restriction)
    with DeviceHierarchy.from_bag(bag, dim=3, grid_index=gi) as dev:
        dev.set_params(mu, mu, bag.omega, restriction=restriction)
        hist, x = _device_run(dev, 3, f, 0.0, iters)
    _match(hist, x, want_hist, want_x)


@pytest.mark.gpu
def test_device_pcg_matches_reference_with_red_black_gauss_seidel():
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    from oracle.mg_oracle import Oracle
    bag = poisson.make_hierarchy(3, 1, 3, c=4, mu1=2, mu2=2, omega=1.0, seed=6)
    gi = {l: L.grid_index for l, L in bag.levels.items()}
    orc = Oracle(bag, gi, dim=3)
    f = bag.b_dict[3]
    want_x, want_hist = fcg(orc, f, rtol=0.0, max_iter=12, smoother="rbgs")
    with DeviceHierarchy.from_bag(bag, dim=3, grid_index=gi) as dev:
        dev.set_params(2, 2, 1.0, smoother="rbgs")
        hist, x = _device_run(dev, 3, f, 0.0, 12)
    _match(hist, x, want_hist, want_x)


@pytest.mark.gpu
def test_device_pcg_matches_reference_on_p2_with_table_transfers():
    """P2 lattice levels, nine-colour Gauss-Seidel V(2,2), the P2 prolongation and its transpose: the preconditioner is
    whatever cycle the handle has."""
    import types
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    from oracle.mg_oracle import Oracle
    dim, lo, hi, c = 3, 1, 3, 4                        # lattices of 4, 8, 16 steps per dimension
    levels = {l: poisson.p2_level(c * 2 ** l // 2, dim) for l in range(lo, hi + 1)}
    bag = types.SimpleNamespace(
        mesh_dof_list_dict={}, element_size={l: 1.0 / L.N for l, L in levels.items()}, coarsest_level_elements_per_dim=c,
        coarsest_level=lo, finest_level=hi, A_sp_dict={l: (L.A, l) for l, L in levels.items()}, A_jacobi_sp_dict={},
        b_dict={l: L.b for l, L in levels.items()}, mu0=1, mu1=2, mu2=2, omega=1.0,
        residual_per_V_cycle_finest=[], error_per_V_cycle_finest=[], u_exact_fine=None, V_fine_dolfx=None, levels=levels)
    orc = Oracle(bag, {l: L.grid_index for l, L in levels.items()}, dim=dim)
    orc.prolongation_table = poisson.p2_prolongation_table(dim)
    orc.restriction_table = poisson.p2_restriction_table(dim)
    f = bag.b_dict[hi]
    want_x, want_hist = fcg(orc, f, rtol=0.0, max_iter=12, smoother="mcgs", restriction="table")
    with DeviceHierarchy.synthetic_p2(dim, lo, hi, c=c, mu1=2, mu2=2, omega=1.0, transfers="p2",
                                      restriction="table") as dev:
        dev.zero_vector(hi, "v")
        hist = dev.pcg(rtol=0.0, max_iter=12)
        x = dev.get_vector(hi, "v")
    _match(hist, x, want_hist, want_x)


@pytest.mark.gpu
def test_device_pcg_beats_plain_cycles_on_c1():
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    bag, gi, _ = _c1("c1_lex")
    f = bag.b_dict[3]
    bn = float(np.linalg.norm(f))
    with DeviceHierarchy.from_bag(bag, dim=2, grid_index=gi) as dev:
        hist, x = _device_run(dev, 3, f, 1e-11, 200)
        assert len(hist) <= 20 and hist[-1] <= 1e-11 * bn
        assert _true_rel_residual(bag, x) <= 2e-11
        dev.zero_vector(3, "v")
        plain = dev.vcycle(3, 80, residuals=True)
        assert plain[-1] > 1e-10 * bn


@pytest.mark.gpu
def test_device_pcg_contract():
    """F bit for bit, R = F - A x, V = x, a nonzero start, max_iter, errors, no whole-vector copies."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    bag, gi, orc = _c1("c1_perm")
    A, f = bag.A_sp_dict[3][0], bag.b_dict[3]
    rng = np.random.default_rng(11)
    v0 = rng.standard_normal(f.shape)
    with DeviceHierarchy.from_bag(bag, dim=2, grid_index=gi) as dev:
        dev.set_vector(3, "v", v0)
        dev.set_vector(3, "f", f)
        f_before = dev.get_vector(3, "f")
        before = dev.counters()
        hist = dev.pcg(rtol=0.0, max_iter=8)
        after = dev.counters()
        assert (after["uploads"], after["downloads"]) == (before["uploads"], before["downloads"])
        assert np.array_equal(dev.get_vector(3, "f"), f_before)
        x = dev.get_vector(3, "v")
        want_x, want_hist = fcg(orc, f, rtol=0.0, max_iter=8, x0=v0)
        _match(hist, x, want_hist, want_x)
        r = dev.get_vector(3, "r")
        r_sp = f.reshape(-1, 1) - A.dot(x.reshape(-1, 1))
        scale = float(np.linalg.norm(abs(A).dot(np.abs(x).reshape(-1, 1))))
        assert float(np.linalg.norm(r.reshape(-1, 1) - r_sp)) <= 1e-13 * scale
        # max_iter reached is no error; a start that meets the tolerance takes no iteration and keeps V
        assert len(dev.pcg(rtol=1e-30, max_iter=3)) == 3
        x3 = dev.get_vector(3, "v")
        assert len(dev.pcg(rtol=1.0, max_iter=5)) == 0
        assert np.array_equal(dev.get_vector(3, "v"), x3)
        with pytest.raises(_capi.MgError, match="level 0"):
            dev.pcg(level=1)
        with pytest.raises(_capi.MgError, match="max_iter"):
            dev.pcg(max_iter=-1)
    with DeviceHierarchy(2, 0, 1, c=8) as flat:
        flat.set_flat_level(A)
        with pytest.raises(_capi.MgError, match="flat"):
            flat.pcg(level=0)


@pytest.mark.gpu
def test_device_pcg_is_deterministic_and_graph_neutral():
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    bag, gi, _ = _p1_3d(2, seed=4)
    f = bag.b_dict[3]
    runs = []
    for graph in (1, 1, 0):
        with DeviceHierarchy.from_bag(bag, dim=3, grid_index=gi, graph=graph) as dev:
            hist, x = _device_run(dev, 3, f, 1e-10, 100)
            if graph:
                assert dev.counters()["graph_replays"] > 0
            again, x2 = _device_run(dev, 3, f, 1e-10, 100)
            assert np.array_equal(hist, again) and np.array_equal(x, x2)
            runs.append((hist, x))
    for hist, x in runs[1:]:
        assert np.array_equal(hist, runs[0][0]) and np.array_equal(x, runs[0][1])


@pytest.mark.gpu
@pytest.mark.parametrize("dim,lo,hi,mu", [(3, 2, 5, 2), (2, 4, 8, 50)])
def test_device_pcg_at_scale(dim, lo, hi, mu):
    """257^3 (C3) at V(2,2) and 2049^2 (C2) at V(50,50), generated on the device: after k = 30 iterations / cycles the
    PCG residual is below the plain cycles'; to rtol = 1e-8 the true residual is within 2 rtol ||b||."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    k = 30
    with DeviceHierarchy.synthetic(dim, lo, hi, c=8, mu1=mu, mu2=mu) as dev:
        bn = dev.norm2(hi, "f")
        dev.zero_vector(hi, "v")
        plain = dev.vcycle(hi, k, residuals=True)
        dev.zero_vector(hi, "v")
        hist = dev.pcg(rtol=0.0, max_iter=k)
        assert len(hist) == k and hist[-1] < plain[-1], (hist[-1], plain[-1])
        dev.zero_vector(hi, "v")
        hist = dev.pcg(rtol=1e-8, max_iter=400)
        true = dev.norm2(hi, "r")
        print(f"\npcg C{'3' if dim == 3 else '2'} V({mu},{mu}): {len(hist)} iterations to 1e-8 "
              f"(recursive {hist[-1] / bn:.3e}, true {true / bn:.3e}); after {k}: pcg {hist[min(k, len(hist)) - 1] / bn:.3e}, "
              f"plain {plain[-1] / bn:.3e}")
        if hist[-1] <= 1e-8 * bn:
            assert true <= 2e-8 * bn


@pytest.mark.gpu
@pytest.mark.parametrize("world,dim,c", [(2, 3, 4), (3, 2, 8)])
def test_device_pcg_on_slabs_matches_single_handle(world, dim, c):
    """2 and 3 processes share the GPU through the host-staged callback transport."""
    import torch.multiprocessing as mp
    from tests.dist_helpers import free_port
    from tests.pcg_workers import gpu_pcg_slab_worker
    mp.spawn(gpu_pcg_slab_worker, args=(world, free_port(), dim, 1, 3, c, 2, 0), nprocs=world, join=True)
