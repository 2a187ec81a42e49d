"""Tile shape 9 of the K-sweep march (`sdia_jacobikc_rim`, mg_jacobik3d.hip.h): shape 8 on 64 x 36 tiles whose first and last
wave own the four rim lines (caps 1, 2, 3, 4 and 4, 3, 2, 1) and whose fourteen waves between them own two full-cap lines each --
28 result lines per tile instead of 24, every wave ten line-levels per step, five sweeps per pass on whole levels.

The tile: cell (0, 0) at the grid position (tix * 54 - 5, tiy * 28 - 4); wave 0 has the tile lines 0 .. 3, wave w = 1 .. 14 the
lines 2 w + 2 and 2 w + 3, wave 15 the lines 32 .. 35; the lines 4 .. 31 are stored.  Which grids reach what (8c + 1 nodes):
17^3 one tile whose lines from 21 on (all of wave 15's among them) lie beyond the grid; 25^3 fewer lines than a tile stores; 33^3
= 28 + 5; 57^3 = 2 * 28 + 1, the last tile row holds one grid line; 65^3; 121^3, the smallest generated grid with a tile column
strictly inside, so that steps of the first straight-line form exist.  One and three plane segments and a tail of short ones,
with and without the march plan: together all three forms of a step in all three kinds of wave, and segments that start at
plane 0, in the middle of the level and in a tail.

CPU: both kernels are in the built library within 128 VGPRs with nothing spilled and no scratch; the plan of the new line map,
restated in NumPy, by hand on 17^3.  GPU: bit-identity with one sweep per launch; the plan a handle reports against the
restatement; V(50,50) against the oracle on 129^3; captured cycles against eager ones; a level with no-flux faces; slabs (which
run shape 8 when a handle asks for 9); four sweeps per pass (shape 7 then); and which shape "fuse_k_shape" -1 picks by the
level's rows ("fuse_k_rim_min_rows")."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_march_one_barrier import LIB, LLVM, _MARCH, _SINGLE, _kernel_notes
from tests.test_march_plan import _longest, _poisson_classes

HI = 3      # finest level of synthetic(3, HI - 2, HI, c): 8 c + 1 nodes per axis
K = 5
_RIM = dict(_MARCH, fuse_k=K, fuse_k_shape=9, fuse_k_min_side=16)
_GRIDS = [2, 3, 4, 7, 8, 15]        # 17, 25, 33, 57, 65, 121
_EXTRAS = [dict(fuse_k_segments=1), dict(fuse_k_segments=3), dict(fuse_k_tail=4)]
OMEGA = 2.0 / 3.0


# ---- registers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"), reason="needs the built library and ROCm's LLVM tools")
def test_rim_kernels_fit_the_register_budget():
    notes = _kernel_notes()
    for kind in ("sdia_jacobikc_rim", "sdia_jacobikc_finest_rim"):
        name = f"void mgk::{kind}<{K}, 64>(mgk::JK3Args)"
        assert name in notes, (name, sorted(n for n in notes if "jacobikc" in n))
        vgpr, spilled, scratch = notes[name]
        print(name, notes[name])
        assert vgpr <= 128 and spilled == 0 and scratch == 0, (name, notes[name])
    name = f"void mgk::jk3_plan_rim<{K}>(mgk::JK3PlanArgs)"
    assert name in notes and notes[name][0] <= 128 and notes[name][1:] == (0, 0), (name, notes.get(name))


# ---- the plan of the new line map, restated on the host ---------------------------------------------------------------------------
def _wave_lines(wave):
    """Tile lines of a wave (jk3_rim_map<5>)."""
    if wave == 0:
        return np.arange(0, 4)
    if wave == 15:
        return np.arange(32, 36)
    return 4 + 2 * (wave - 1) + np.arange(2)


def _host_plan_rim(cls, main, n1, runs=None):
    """tests/test_march_plan.py's _host_plan for the 64 x 36 tiles of shape 9 (K = 5): 54 columns and 28 lines stored per tile,
    a wave's cells are the columns tx0 + min(lane, nx + 1 - tx0) of the lines ty0 + _wave_lines(wave) clamped to [-2, ny + 1]."""
    nx = ny = nz = n1
    P = nx * ny
    WI, HY = 64 - 2 * K, 28
    pad = 2 * P
    padded = np.full(P * nz + 2 * pad, -1, dtype=np.int64)
    padded[pad:pad + P * nz] = cls
    out = [0, 0, 0, 0]
    for tiy in range(-(-ny // HY)):
        for tix in range(-(-nx // WI)):
            tx0, ty0 = tix * WI - K, tiy * HY - (K - 1)
            col = tx0 + np.minimum(np.arange(64), nx + 1 - tx0)
            for wave in range(16):
                lines = np.clip(ty0 + _wave_lines(wave), -2, ny + 1)
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


def test_line_map_covers_the_tile_once():
    lines = np.concatenate([_wave_lines(w) for w in range(16)])
    assert np.array_equal(lines, np.arange(36))
    caps = np.minimum(np.minimum(lines + 1, 36 - lines), K)
    per_wave = [int(caps[np.isin(lines, _wave_lines(w))].sum()) for w in range(16)]
    assert per_wave == [10] * 16                        # every wave: ten line-levels per step
    assert np.array_equal(np.flatnonzero(caps == K), np.arange(4, 32))      # the stored lines: 28


def test_host_plan_of_a_poisson_level_by_hand():
    """17^3: one tile, ty0 = -4, every wave sees the x boundary -- no run of the first kind.  As in tests/test_march_plan.py the
    classes of a grid line repeat in the planes 3 .. 14: [2, 15), 13 planes, for the waves 1 .. 8 (tile lines 4 .. 19, the grid
    lines 0 .. 15).  In ROW space a line below 0 is a line of the plane before and a line above 16 one of the plane after: wave
    0 (tile lines 0 .. 3, the grid lines -4 .. -1, clamped to -2, -2, -2, -1) has [3, 16); the waves 10 .. 15 (grid lines 18 and
    up, all clamped to 18) have [1, 14); wave 9 (grid lines 16 and 17) has what [2, 15) and [1, 14) share, 12 planes."""
    cls, main = _poisson_classes(2)
    runs = []
    waves, planes, cwaves, cplanes = _host_plan_rim(cls, main, 17, runs)
    assert (waves, planes) == (0, 0) and cwaves == 16
    assert [r[2:] for r in runs] == [(3, 16)] + [(2, 15)] * 8 + [(2, 14)] + [(1, 14)] * 6
    assert cplanes == 15 * 13 + 12


@functools.lru_cache(maxsize=None)
def _expected_plan(c):
    cls, main = _poisson_classes(c)
    return _host_plan_rim(cls, main, 8 * c + 1)


# ---- bit-identity on Poisson levels ---------------------------------------------------------------------------------------------
def _smoothed(c, nw, tuning, k=K):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    with DeviceHierarchy.synthetic(3, HI - 2, HI, c=c, mu1=2, mu2=2, **tuning) as dev:
        rng = np.random.default_rng(3000 + c)
        m = 8 * c + 1
        dev.set_vector(HI, "v", rng.standard_normal(m ** 3))
        dev.set_vector(HI, "f", rng.standard_normal(m ** 3))
        dev.reset_smoother_launches()
        dev.smooth(HI, nw)
        return dev.get_vector(HI, "v"), dev.smoother_launches(HI), dev.march_plan(HI, k)


@pytest.mark.gpu
@pytest.mark.parametrize("c", _GRIDS, ids=[str(8 * c + 1) for c in _GRIDS])
def test_rim_waves_are_bit_identical_to_single_sweeps(c):
    """Two passes of five sweeps in shape 9 against ten single sweeps, for one and three plane segments and a tail of short ones,
    with the march plan and without; with it the handle reports the plan of the new line map (on 57^3 and 121^3 the issue's
    plan check; on every grid what tells shape 9's launches from shape 8's)."""
    nw = 2 * K
    want, ran_single, _ = _smoothed(c, nw, _SINGLE)
    assert "ksweep" not in ran_single and np.all(np.isfinite(want)), ran_single
    want_plan = _expected_plan(c)
    assert (want_plan[1] > 0) == (c == 15), want_plan
    for extra in _EXTRAS:
        for plan in (1, 0):
            got, ran, reported = _smoothed(c, nw, dict(_RIM, fuse_k_plan=plan, **extra))
            print(8 * c + 1, extra, "plan", plan, reported, "host:", want_plan, ran)
            assert set(ran) == {"ksweep"} and ran["ksweep"][:2] == (2, nw), (extra, plan, ran)
            assert reported == (want_plan if plan else (0, 0, 0, 0)), (extra, plan, reported, want_plan)
            diff = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
            assert np.array_equal(got, want), (extra, plan, "rows that differ:", diff.size, "the first:", diff[:8])


@pytest.mark.gpu
def test_shape9_below_five_sweeps_is_shape7():
    """A handle that asks for shape 9 with four sweeps per pass gets shape 7: the same bits, and shape 7's plan."""
    c, nw = 7, 8
    want, _, _ = _smoothed(c, nw, _SINGLE)
    got = {shape: _smoothed(c, nw, dict(_RIM, fuse_k=4, fuse_k_shape=shape), k=4) for shape in (9, 7)}
    assert got[9][1] == got[7][1] and set(got[9][1]) == {"ksweep"}, (got[9][1], got[7][1])
    assert got[9][2] == got[7][2] and sum(got[9][2]) > 0, (got[9][2], got[7][2])
    assert np.array_equal(got[9][0], want)


@pytest.mark.gpu
def test_default_shape_by_level_size():
    """"fuse_k_shape" -1: five sweeps per pass take shape 9 on whole levels of at least "fuse_k_rim_min_rows" rows (2^26 by
    default: 25^3 keeps shape 8) -- told apart by the plan the handle reports: shape 8's tiles store 24 lines, so 25^3 has two
    tile rows (32 waves) there and one (16 waves) in shape 9."""
    from tests.test_march_plan import _expected_plan as _expected_plan_shape8
    c, nw = 3, 2 * K
    assert _expected_plan(c)[2] == 16 and _expected_plan_shape8(c, K)[2] == 32
    want, _, _ = _smoothed(c, nw, _SINGLE)
    by_k = dict(_RIM, fuse_k_shape=-1)
    for tuning, plan in ((by_k, _expected_plan_shape8(c, K)), (dict(by_k, fuse_k_rim_min_rows=0), _expected_plan(c)),
                         (dict(by_k, fuse_k_rim_min_rows=25 ** 3), _expected_plan(c)), (dict(by_k, fuse_k_rim_min_rows=25 ** 3 + 1), _expected_plan_shape8(c, K))):
        got, ran, reported = _smoothed(c, nw, tuning)
        assert set(ran) == {"ksweep"} and reported == plan, (tuning, ran, reported, plan)
        assert np.array_equal(got, want)


# ---- the oracle, captured cycles, no-flux faces, slabs ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_shape9_against_the_oracle_at_129():
    """The reference's V(50,50) on the 129^3 hierarchy with five sweeps per pass in shape 9 on every level."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    from tests.helpers import rel_l2
    from tests.test_gpu_parity import TOL_ITER, _n128_oracle
    want, res_want = _n128_oracle()
    with DeviceHierarchy.synthetic(3, 2, 4, c=8, mu1=50, mu2=50, **dict(_MARCH, fuse_k_shape=9, fuse_k_small_rows=1 << 22)) as dev:
        dev.zero_vector(4, "v")
        res = dev.vcycle(4, 1, residuals=True)
        got = dev.get_vector(4, "v")
        counts = dev.smoother_launches(4)
        plan = dev.march_plan(4, K)
    assert {p: (n, s) for p, (n, s, _) in counts.items()} == {"ksweep": (20, 100)}, counts
    assert plan[1] > 0 and plan[3] > 0, plan
    print("rel l2", rel_l2(got, want), "residual", res[0], res_want)
    assert rel_l2(got, want) <= TOL_ITER
    assert abs(res[0] - res_want) <= TOL_ITER * res_want


@pytest.mark.gpu
def test_captured_cycles_equal_eager_ones():
    """Two V(5,5) cycles on 17^3 .. 65^3 in shape 9, captured (mg_prepare_cycle builds the plans before the capture) against
    eager: the iterate and the residual history byte for byte."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    f = np.random.default_rng(9).standard_normal(65 ** 3)
    got = {}
    for graph in (1, 0):
        with DeviceHierarchy.synthetic(3, HI - 2, HI, c=8, mu1=5, mu2=5, omega=OMEGA, graph=graph, **_RIM) as dev:
            dev.set_vector(HI, "f", f)
            dev.zero_vector(HI, "v")
            if graph:
                assert dev.march_plan(HI, K) == (0, 0, 0, 0)
                dev.prepare_cycle(HI)
                assert dev.march_plan(HI, K) == _expected_plan(8)
            dev.reset_smoother_launches()
            res = dev.vcycle(HI, 2, residuals=True)
            got[graph] = (dev.get_vector(HI, "v"), res, dev.smoother_launches(HI), dev.counters())
            assert dev.march_plan(HI, K) == _expected_plan(8)
    (v1, r1, ran1, n1), (v0, r0, ran0, n0) = got[1], got[0]
    assert set(ran1) == {"ksweep"} and set(ran0) == {"ksweep"}, (ran1, ran0)     # (a replayed cycle's launches are counted once)
    assert n1["graphs_cached"] >= 1 and n0["graphs_cached"] == 0, (n1, n0)
    assert v1.tobytes() == v0.tobytes() and np.asarray(r1).tobytes() == np.asarray(r0).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("faces", [21])
def test_level_with_no_flux_faces(faces):
    """A generated diffusion level of 65^3 nodes (`jump` kappa) whose x+, y+ and z+ faces carry no flux -- free rows with real
    couplings on the grid boundary, as in tests/test_neumann_smoother_paths.py -- in shape 9 against one sweep per launch, on the
    finest level of a handle and on one that is not."""
    from tests.test_neumann_smoother_paths import REFERENCE, _handle, _kappa, _smooths
    N, sweeps = 64, (5, 10)
    kappa = _kappa("jump", N)
    rng = np.random.default_rng(1000 * faces + N)
    v, f = rng.standard_normal((N + 1) ** 3), rng.standard_normal((N + 1) ** 3)
    with _handle(N, faces, kappa, REFERENCE, True, reference=True) as h:
        want = _smooths(h, v, f, sweeps)
    for nw, (x, ran) in want.items():
        assert ran == {"slice": (nw, nw, 0)} and np.all(np.isfinite(x)), (nw, ran)
    for finest in (True, False):
        for seg in (1, 3):
            with _handle(N, faces, kappa, dict(fuse_block=0, fuse_k=K, fuse_k_shape=9, fuse_k_segments=seg), finest) as h:
                assert 2 <= h.level_info(1)["row_classes"] <= 64
                got = _smooths(h, v, f, sweeps)
                plan = h.march_plan(1, K)
            for nw, (x, ran) in got.items():
                assert ran == {"ksweep": (nw // K, nw, 0)}, (finest, seg, nw, ran)
                assert np.array_equal(x, want[nw][0]), (finest, seg, nw, np.flatnonzero(x.reshape(-1) != want[nw][0].reshape(-1))[:8])
            assert plan[1] + plan[3] > 0, plan


@pytest.mark.gpu
def test_shape9_on_slabs_runs_shape8_and_matches_single_handle():
    """Slabs keep shape 8: the two-rank stand-in worker of tests/test_march_one_barrier.py with "fuse_k_shape" 9 in its tune
    string still matches the single-handle run bit for bit, through the K-sweep slab path."""
    here = os.path.dirname(os.path.abspath(__file__))
    lib = os.path.join(here, "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(here, "fake_rccl")], check=True)
    tune = "halo_depth=5,fuse_k=5,fuse_k_shape=9,fuse_min_rows=0,fuse_k_slab_min_rows=0,fuse_k_slab_min_sweeps=2"
    env = dict(os.environ, MG_RCCL_LIBRARY=lib, MG_TEST_TUNE=tune, MG_TEST_EXPECT_KSLAB="1")
    out = subprocess.run([sys.executable, os.path.join(here, "fake_rccl_worker.py"), "2", "3", "2", "4", "8", "5", "0", "1"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "OK" in out.stdout
