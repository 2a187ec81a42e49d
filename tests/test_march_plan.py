"""March plans of the K-sweep march (`jk3_plan`, mg_jacobik3d.hip.h; "fuse_k_plan"): per (tile, wave) the longest run of planes
whose class bytes are all the level's main class (steps inside it are form 0) and the longest run whose class bytes do not
change from plane to plane (form 1); the steps of the march inside a run load no classes, keep no class ring and decide
nothing.  Everything here is bits against bits: plan on, plan off ("fuse_k_plan" 0: the instructions of the march without
plans) and one sweep per launch must agree exactly.

Which grids reach which path (64 x 32 tiles store WI = 64 - 2K columns and HY = 34 - 2K lines; a wave loads 64 consecutive
columns of two lines): a wave has a run of the first kind only if none of its 128 cells is on or next to the boundary, which
needs a tile column strictly inside the grid -- three tile columns, 2 WI + K + 1 < nx: 121^3 is the smallest grid of the
generator's sizes (8c + 1) that has one for K = 3, 4 and 5.  On 17^3 .. 105^3 every wave sees the x boundary and all runs are
of the second kind: on a Poisson level the classes of a grid line are the same in the planes 2 .. n - 3, so a wave's run
is [2, n - 2) at most -- 13 planes on 17^3, where with K = 5 and one segment the steps [max(2, 1, z0 - K), min(15 - K,
17 - K - 1)) = [2, 10) are planned: entering and leaving lie eight steps apart, and with four segments (planes 0-4, 5-9, 10-14,
15-16) the segments have 3, 8, 5 and 0 planned steps.  What a handle reports (`mg_march_plan`) is compared with a NumPy
restatement of the plan that reads the classes from the host matrix (poisson.lexicographic_level: rows equal bit for bit are one
class, the most frequent is the main one) through the tile geometry written out again below.

GPU tests: bit-identity for K = 3, 4, 5 on shapes 7 and 8, grids 17^3, 41^3, 57^3, 65^3, 105^3 and 121^3, one to four plane
segments and a tail of short segments; a generated diffusion level whose kappa jumps across a plane normal to z and one
normal to x (runs that end in the middle of the grid, at the interface, and resume behind it as ordinary steps); a refresh
of that hierarchy with the interfaces elsewhere (the plan must go with the classes); two captured V(5,5) cycles.  CPU: the new
kernel and the march kernels that read plans stay within 128 VGPRs with nothing spilled."""
import functools
import os
import re

import numpy as np
import pytest

from tests.test_march_one_barrier import LIB, LLVM, _MARCH, _SINGLE, _kernel_notes

HI = 3      # finest level of synthetic(3, HI - 2, HI, c): 8 c + 1 nodes per axis
_GRIDS = [2, 5, 7, 8, 13, 15]       # 17, 41, 57, 65, 105, 121
_EXTRAS = [dict(fuse_k_segments=1), dict(fuse_k_segments=2), dict(fuse_k_segments=3), dict(fuse_k_segments=4), dict(fuse_k_tail=4)]
OMEGA = 2.0 / 3.0


# ---- the plan, restated on the host ------------------------------------------------------------------------------------------
def _row_classes(A, n1):
    """(class id per row, id of the most frequent class): rows whose seven entries are equal bit for bit share a class."""
    n = A.shape[0]
    d = np.zeros((n, 7))
    for i, o in enumerate((-n1 * n1, -n1, -1, 0, 1, n1, n1 * n1)):
        diag = A.diagonal(o)
        if o >= 0:
            d[:n - o, i] = diag
        else:
            d[-o:, i] = diag
    keys = np.ascontiguousarray(d).view(np.dtype((np.void, 56))).ravel()
    _, inv, counts = np.unique(keys, return_inverse=True, return_counts=True)
    return inv.reshape(-1).astype(np.int64), int(np.argmax(counts))


@functools.lru_cache(maxsize=None)
def _poisson_classes(c):
    from multigrid_dolfinx_amd import poisson
    n1 = 8 * c + 1
    return _row_classes(poisson.lexicographic_level(8 * c, 3, keep_zeros=False).A, n1)


def _longest(starts, ends):
    """The longest of the runs [starts[i], ends[i]), the first of equally long ones; (0, 0) without any."""
    if len(starts) == 0:
        return 0, 0
    i = int(np.argmax(ends - starts))
    return int(starts[i]), int(ends[i])


def _host_plan(cls, main, n1, K, runs=None):
    """(waves, planes, const_waves, const_planes) as mg_march_plan counts them, for the 64 x 32 tiles of K sweeps per pass on a
    whole n1^3 level: a wave's cells are the columns tx0 + min(lane, nx + 1 - tx0) of the lines ty0 + 2 wave + {0, 1} clamped to
    [-2, ny + 1], as offsets into the plane in ROW space (rows outside the level: no class).  `runs`, a list: every wave's
    (p0, p1, q0, q1) is appended."""
    nx = ny = nz = n1
    P = nx * ny
    WI, HY = 64 - 2 * K, 34 - 2 * K
    pad = 2 * P
    padded = np.full(P * nz + 2 * pad, -1, dtype=np.int64)
    padded[pad:pad + P * nz] = cls
    out = [0, 0, 0, 0]
    for tiy in range(-(-ny // HY)):
        for tix in range(-(-nx // WI)):
            tx0, ty0 = tix * WI - K, tiy * HY - (K - 1)
            col = tx0 + np.minimum(np.arange(64), nx + 1 - tx0)
            for wave in range(16):
                lines = np.clip(ty0 + 2 * wave + np.arange(2), -2, ny + 1)
                off = (lines[:, None] * nx + col[None, :]).ravel()
                got = padded[np.arange(nz)[:, None] * P + off[None, :] + pad]
                allmain = np.r_[False, (got == main).all(axis=1), False]
                edge = np.flatnonzero(allmain[1:] != allmain[:-1])
                p0, p1 = _longest(edge[0::2], edge[1::2])
                fresh = np.flatnonzero(np.r_[True, (got[1:] != got[:-1]).any(axis=1)])     # planes that start a run
                q0, q1 = _longest(fresh, np.r_[fresh[1:], nz])
                if runs is not None:
                    runs.append((p0, p1, q0, q1))
                if p1 > p0:
                    out[0] += 1
                    out[1] += p1 - p0
                if q1 > q0 and (q0, q1) != (p0, p1):
                    out[2] += 1
                    out[3] += q1 - q0
    return tuple(out)


def test_host_plan_of_a_poisson_level_by_hand():
    """17^3, K = 5: one tile, every wave sees the x boundary -- no run of the first kind.  The classes of a grid line are those
    of the plane before in the planes 3 .. 14: a run of 13 planes, [2, 15), for the waves 2 .. 9 (tile lines -4 .. 27, two per
    wave: theirs are the grid lines 0 .. 15).  In ROW space a line below 0 is a line of the plane before and a line above 16
    one of the next plane: the waves 0 and 1 (lines clamped to -2, and -2, -1) have [3, 16), the waves 11 .. 15 (both lines
    clamped to 18) have [1, 14), and wave 10 (lines 16 and 17) only what [2, 15) and [1, 14) share, 12 planes."""
    cls, main = _poisson_classes(2)
    waves, planes, cwaves, cplanes = _host_plan(cls, main, 17, 5)
    assert (waves, planes) == (0, 0) and cwaves == 16
    assert cplanes == 15 * 13 + 12


@functools.lru_cache(maxsize=None)
def _expected_plan(c, k):
    cls, main = _poisson_classes(c)
    return _host_plan(cls, main, 8 * c + 1, k)


# ---- Poisson levels ----------------------------------------------------------------------------------------------------------
def _vectors(m, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(m ** 3), rng.standard_normal(m ** 3)


def _smoothed(c, nw, k, tuning):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    with DeviceHierarchy.synthetic(3, HI - 2, HI, c=c, mu1=2, mu2=2, **tuning) as dev:
        v, f = _vectors(8 * c + 1, 2000 + c)
        dev.set_vector(HI, "v", v)
        dev.set_vector(HI, "f", f)
        dev.reset_smoother_launches()
        before = dev.march_plan(HI, k)
        dev.smooth(HI, nw)
        return dev.get_vector(HI, "v"), dev.smoother_launches(HI), before, dev.march_plan(HI, k)


@functools.lru_cache(maxsize=None)
def _single_sweeps(c, nw):
    """nw sweeps, one per launch (computed once per grid and sweep count; read-only)."""
    got = _smoothed(c, nw, 5, _SINGLE)[0]
    got.setflags(write=False)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("c", _GRIDS, ids=[str(8 * c + 1) for c in _GRIDS])
@pytest.mark.parametrize("k", [3, 4, 5])
@pytest.mark.parametrize("shape", [8, 7])
def test_planned_march_is_bit_identical(shape, k, c):
    """Two passes of K sweeps with the plan, without it and as single sweeps, for 1 .. 4 plane segments and a tail of short
    ones; the handle reports the plan of the host restatement -- runs of some kind on every grid from 41^3 on, runs of the
    first kind from 121^3 on -- and nothing before the first launch or with "fuse_k_plan" 0."""
    nw = 2 * k
    n1 = 8 * c + 1
    want_plan = _expected_plan(c, k)
    assert (want_plan[1] > 0) == (n1 >= 121), want_plan
    if n1 >= 41:
        assert want_plan[1] + want_plan[3] > 0, want_plan
    for extra in _EXTRAS:
        tuning = dict(_MARCH, fuse_k=k, fuse_k_shape=shape, fuse_k_min_side=16, **extra)
        on, ran, before, plan = _smoothed(c, nw, k, tuning)
        off, ran_off, _, plan_off = _smoothed(c, nw, k, dict(tuning, fuse_k_plan=0))
        print(n1, k, shape, extra, "plan:", plan, "host:", want_plan)
        assert set(ran) == {"ksweep"} and ran["ksweep"][:2] == (2, nw) and ran_off == ran, (ran, ran_off)
        assert before == (0, 0, 0, 0) and plan_off == (0, 0, 0, 0), (before, plan_off)
        assert plan == want_plan, (extra, plan, want_plan)
        assert np.array_equal(on, off), extra
        assert np.array_equal(_single_sweeps(c, nw), on), extra


# ---- a diffusion level whose classes change in the middle of the grid ----------------------------------------------------------
def _kappa(N, zi, xi):
    """4 in the cells with z >= zi and x >= xi, 1 elsewhere ([z, y, x] cells; every entry of the matrix exact): an interface
    plane normal to z and one normal to x, and 52 distinct rows -- two half-spaces that cross have 76, and a level with more
    than 64 classes leaves the 64 x 32 tiles for shape 1, which takes no plan."""
    k = np.ones((N, N, N))
    k[zi:, :, xi:] = 4.0
    return k.reshape(-1)


@functools.lru_cache(maxsize=None)
def _diffusion_plan(N, zi, xi, K):
    from multigrid_dolfinx_amd import poisson
    cls, main = _row_classes(poisson.diffusion_level(N, 3, _kappa(N, zi, xi), keep_zeros=False).A, N + 1)
    assert cls.max() + 1 == 52
    runs = []
    return _host_plan(cls, main, N + 1, K, runs), runs


def _diffusion_handle(N, kappa, k, shape, **tuning):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    h = DeviceHierarchy(3, 0, 1, c=N // 2, **dict(_MARCH, fuse_k=k, fuse_k_shape=shape, fuse_k_min_side=16, **tuning))
    h.set_params(2, 2, OMEGA)
    h.gen_diffusion_hierarchy(kappa, top_level=1)
    return h


def _diffusion_smoothed(h, N, nw, seed):
    v, f = _vectors(N + 1, seed)
    h.set_vector(1, "v", v)
    h.set_vector(1, "f", f)
    h.reset_smoother_launches()
    h.smooth(1, nw)
    return h.get_vector(1, "v"), h.smoother_launches(1)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [40, 64], ids=["41", "65"])
@pytest.mark.parametrize("k,shape,seg", [(5, 8, 1), (5, 8, 3), (4, 7, 2), (3, 8, 1), (3, 7, 4)])
def test_runs_that_end_at_an_interface(k, shape, seg, N):
    """A stored variable-coefficient diffusion level (mg_gen_diffusion_hierarchy, all faces Dirichlet) takes the class march at
    41^3 and 65^3 (`ksweep` in mg_smoother_launches).  kappa jumps across the node plane z = zi (where x >= xi) and across
    x = xi (where z >= zi); every wave of these grids that holds rows off the boundary loads whole grid lines, so it does not
    keep its classes through the planes zi - 1 .. zi + 1: its run ends at the interface, in the middle of the grid, and the
    segment leaves its planned steps there and goes on with ordinary ones.  The plan is the host restatement's, in which more
    than half of the waves have such a run (the others hold boundary rows only, identity rows in every plane)."""
    zi, xi = N // 2 + 2, N // 2 - 3
    nw = 2 * k
    got = {}
    for plan in (1, 0):
        with _diffusion_handle(N, _kappa(N, zi, xi), k, shape, fuse_k_segments=seg, fuse_k_plan=plan) as h:
            got[plan] = _diffusion_smoothed(h, N, nw, 77) + (h.march_plan(1, k),)
    (on, ran, plan), (off, ran_off, plan_off) = got[1], got[0]
    print(N, k, shape, seg, "plan:", plan)
    assert set(ran) == {"ksweep"} and ran == ran_off and ran["ksweep"][:2] == (2, nw), (ran, ran_off)
    assert plan_off == (0, 0, 0, 0)
    waves, planes, cwaves, cplanes = plan
    want_plan, runs = _diffusion_plan(N, zi, xi, k)
    assert plan == want_plan, (plan, want_plan)
    at_interface = [r for r in runs if zi - 1 <= r[3] <= zi + 1 and r[3] - r[2] > k + 1]
    assert waves + cwaves == len(runs) and 2 * len(at_interface) > len(runs), (len(at_interface), len(runs))
    assert np.array_equal(on, off)


@pytest.mark.gpu
def test_refresh_drops_the_plan():
    """The plan describes the classes it was built from: mg_refresh_diffusion_hierarchy with a kappa whose interfaces lie
    elsewhere rebuilds the classes, and the next march must run on a plan of the new ones -- the result of a fresh handle
    without plans."""
    N, k, shape = 40, 5, 8
    first, second = _kappa(N, 22, 17), _kappa(N, 9, 30)
    with _diffusion_handle(N, first, k, shape) as h:
        _diffusion_smoothed(h, N, 2 * k, 5)
        plan_first = h.march_plan(1, k)
        h.refresh_diffusion_hierarchy(second, top_level=1)
        assert h.march_plan(1, k) == (0, 0, 0, 0)
        got, ran = _diffusion_smoothed(h, N, 2 * k, 6)
        plan_second = h.march_plan(1, k)
    with _diffusion_handle(N, second, k, shape, fuse_k_plan=0) as fresh:
        want, ran_fresh = _diffusion_smoothed(fresh, N, 2 * k, 6)
    with _diffusion_handle(N, second, k, shape) as planned:
        _diffusion_smoothed(planned, N, 2 * k, 6)
        plan_fresh = planned.march_plan(1, k)
    print("plans:", plan_first, plan_second, plan_fresh)
    assert set(ran) == {"ksweep"} and ran == ran_fresh
    assert plan_first[3] > 0 and plan_second == plan_fresh and plan_second != plan_first
    assert np.array_equal(got, want)


# ---- captured cycles -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_captured_cycles_use_a_plan_built_before_the_capture():
    """Two V(5,5) cycles on 17^3 .. 65^3, captured with the plan against eager without: mg_prepare_cycle builds the plans (an
    allocation and a synchronisation, neither possible inside a capture), the captured launches read them."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    tuning = dict(_MARCH, fuse_k=5, fuse_k_min_side=16)
    f = np.random.default_rng(9).standard_normal(65 ** 3)
    got = {}
    for graph, plan in ((1, 1), (0, 0)):
        with DeviceHierarchy.synthetic(3, HI - 2, HI, c=8, mu1=5, mu2=5, omega=OMEGA, graph=graph, fuse_k_plan=plan, **tuning) as dev:
            dev.set_vector(HI, "f", f)
            dev.zero_vector(HI, "v")
            if plan:
                assert dev.march_plan(HI, 5) == (0, 0, 0, 0)
                dev.prepare_cycle(HI)
                built = dev.march_plan(HI, 5)
                assert built == _expected_plan(8, 5) and built[3] > 0, built
            dev.reset_smoother_launches()
            res = dev.vcycle(HI, 2, residuals=True)
            got[graph] = (dev.get_vector(HI, "v"), res, dev.smoother_launches(HI), dev.counters())
            assert dev.march_plan(HI, 5) == (built if plan else (0, 0, 0, 0))
    (v1, r1, ran1, n1), (v0, r0, ran0, n0) = got[1], got[0]
    assert "ksweep" in ran1 and "ksweep" in ran0, (ran1, ran0)
    assert n1["graphs_cached"] >= 1 and n0["graphs_cached"] == 0, (n1, n0)
    assert np.array_equal(v1, v0) and np.array_equal(r1, r0)


# ---- registers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"), reason="needs the built library and ROCm's LLVM tools")
def test_plan_kernels_fit_the_register_budget():
    """jk3_plan for K = 3, 4, 5 and every march kernel of the 64 x 32 tiles that reads a plan (shapes 7 and 8, not the escape
    variant): present in the gfx950 code object, at most 128 VGPRs (sixteen waves per workgroup), nothing spilled, no scratch."""
    notes = _kernel_notes()
    want = [f"void mgk::jk3_plan<{k}, 16, 2>(mgk::JK3PlanArgs)" for k in (3, 4, 5)]
    for k in (3, 4, 5):
        want += [f"void mgk::{kind}<{k}, 16, 2, 4, 256>(mgk::JK3Args)"
                 for kind in ("sdia_jacobikc_b1", "sdia_jacobikc_finest_b1", "sdia_jacobikc", "sdia_jacobikc_finest")]
    have = sorted(n for n in notes if "jacobikc" in n or "jk3_plan" in n)
    for name in want:
        assert name in notes, (name, have)
    planned = [n for n in have if re.search(r"sdia_jacobikc(_finest)?(_b1)?<[345], 16, 2, ", n) or "jk3_plan" in n]
    assert set(want) <= set(planned)
    for name in planned:
        vgpr, spilled, scratch = notes[name]
        assert vgpr <= 128 and spilled == 0 and scratch == 0, (name, notes[name])
