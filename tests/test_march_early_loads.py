"""Tile shape 9 of the K-sweep march with the next plane's loads issued early (`sdia_jacobikc_rim_early`, mg_jacobik3d.hip.h;
"fuse_k_load_early" 1 on levels of at least "fuse_k_load_early_min_rows" rows): f and, off plan, the classes go out in front
of the step's barrier, x of all the wave's lines behind the first piece of phase B.  No value that is computed changes:
everything here is bits against bits.

CPU: the variant is in the built library within 128 VGPRs with nothing spilled and no scratch, next to the two kernels of the
parent placement.  GPU: out-of-range values of both keys are refused and change nothing; two passes of five sweeps against ten
single sweeps with the variant on (row threshold 0), with one and three plane segments and a tail of short ones, with the
march plan and without, on 17^3 (one tile, lines beyond the grid, the plane clamp at both ends of every segment), 33^3 and
57^3 (a last tile row of one grid line) and 121^3 (steps of the straight-line form and planned steps without class loads);
"fuse_k_load_early" 0 under the same threshold for the parent placement; captured cycles against eager ones with the variant
on every level."""
import functools
import os

import numpy as np
import pytest

from tests.test_march_one_barrier import LIB, LLVM, _SINGLE, _kernel_notes
from tests.test_march_rim_waves import HI, K, OMEGA, _EXTRAS, _RIM, _expected_plan, _smoothed

_VARIANTS = {"early": dict(fuse_k_load_early=1, fuse_k_load_early_min_rows=0), "parent": dict(fuse_k_load_early=0, fuse_k_load_early_min_rows=0)}
_GRIDS = [2, 4, 7, 15]      # 17, 33, 57, 121


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"), reason="needs the built library and ROCm's LLVM tools")
def test_load_variants_fit_the_register_budget():
    notes = _kernel_notes()
    names = [f"void mgk::{kind}<{K}, 64>(mgk::JK3Args)" for kind in ("sdia_jacobikc_rim", "sdia_jacobikc_finest_rim")]
    names += [f"void mgk::{kind}_early<{K}, 64>(mgk::JK3Args)" for kind in ("sdia_jacobikc_rim", "sdia_jacobikc_finest_rim")]
    have = sorted(n for n in notes if "jacobikc" in n and "rim" in n)
    assert have == sorted(names), have          # these and no others
    for name in names:
        vgpr, spilled, scratch = notes[name]
        print(name, notes[name])
        assert vgpr <= 128 and spilled == 0 and scratch == 0, (name, notes[name])


@functools.lru_cache(maxsize=None)
def _single(c):
    want, ran, _ = _smoothed(c, 2 * K, _SINGLE)
    assert "ksweep" not in ran and np.all(np.isfinite(want)), ran
    want.setflags(write=False)
    return want


@pytest.mark.gpu
def test_bad_values_are_refused():
    from multigrid_dolfinx_amd._capi import MgError
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    c = 2
    with DeviceHierarchy.synthetic(3, HI - 2, HI, c=c, mu1=2, mu2=2, **dict(_RIM, **_VARIANTS["early"])) as dev:
        for bad in (-1, 2, 9):
            with pytest.raises(MgError, match="fuse_k_load_early must be 0 or 1"):
                dev.set_tuning("fuse_k_load_early", bad)
        with pytest.raises(MgError, match="fuse_k_load_early_min_rows must be >= 0"):
            dev.set_tuning("fuse_k_load_early_min_rows", -1)
        rng = np.random.default_rng(3000 + c)       # (_smoothed's vectors: the refused values changed nothing, the handle works)
        dev.set_vector(HI, "v", rng.standard_normal(17 ** 3))
        dev.set_vector(HI, "f", rng.standard_normal(17 ** 3))
        dev.reset_smoother_launches()
        dev.smooth(HI, 2 * K)
        assert set(dev.smoother_launches(HI)) == {"ksweep"}
        assert np.array_equal(dev.get_vector(HI, "v"), _single(c))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(_VARIANTS))
@pytest.mark.parametrize("c", _GRIDS, ids=[str(8 * c + 1) for c in _GRIDS])
def test_load_variants_are_bit_identical_to_single_sweeps(c, variant):
    nw = 2 * K
    want = _single(c)
    want_plan = _expected_plan(c)
    assert (want_plan[1] > 0) == (c == 15), want_plan       # 121^3: planned steps of the straight-line form
    for extra in _EXTRAS:
        for plan in (1, 0):
            got, ran, reported = _smoothed(c, nw, dict(_RIM, fuse_k_plan=plan, **_VARIANTS[variant], **extra))
            assert set(ran) == {"ksweep"} and ran["ksweep"][:2] == (2, nw), (extra, plan, ran)
            assert reported == (want_plan if plan else (0, 0, 0, 0)), (extra, plan, reported, want_plan)
            diff = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
            assert np.array_equal(got, want), (variant, extra, plan, "rows that differ:", diff.size, "the first:", diff[:8])


@pytest.mark.gpu
def test_captured_cycles_equal_eager_ones_with_early_loads():
    """Two V(5,5) cycles on 17^3 .. 65^3 in shape 9 with the default "fuse_k_load_early" and the row threshold at 0, so that
    every level takes the variant, captured against eager: the iterate and the residual history byte for byte."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    f = np.random.default_rng(9).standard_normal(65 ** 3)
    got = {}
    for graph in (1, 0):
        with DeviceHierarchy.synthetic(3, HI - 2, HI, c=8, mu1=5, mu2=5, omega=OMEGA, graph=graph, fuse_k_load_early_min_rows=0, **_RIM) as dev:
            dev.set_vector(HI, "f", f)
            dev.zero_vector(HI, "v")
            if graph:
                dev.prepare_cycle(HI)
            dev.reset_smoother_launches()
            res = dev.vcycle(HI, 2, residuals=True)
            got[graph] = (dev.get_vector(HI, "v"), res, dev.smoother_launches(HI), dev.counters())
            assert dev.march_plan(HI, K) == _expected_plan(8)
    (v1, r1, ran1, n1), (v0, r0, ran0, n0) = got[1], got[0]
    assert set(ran1) == {"ksweep"} and set(ran0) == {"ksweep"}, (ran1, ran0)
    assert n1["graphs_cached"] >= 1 and n0["graphs_cached"] == 0, (n1, n0)
    assert v1.tobytes() == v0.tobytes() and np.asarray(r1).tobytes() == np.asarray(r0).tobytes()
