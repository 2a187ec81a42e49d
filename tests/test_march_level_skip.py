"""Level caps of the K-sweep march (`jk3_caps`, mg_jacobik3d.hip.h): on the 64 x 32 tiles of tile shapes 7 and 8 a line of
the tile takes part in the levels 1 .. min(ey + 1, EY - ey, K) only, and the waves that own such lines skip the levels above.

GPU: the march against one sweep per launch, bit for bit, on the grids where a cap can go wrong and that the other suites
(41^3 .. 129^3) do not have: one tile whose top lines lie beyond the grid (17^3), and grids whose last tile row holds exactly
one grid line (a tile stores HY = EY - 2K + 2 = 24, 26, 28 lines for K = 5, 4, 3) -- each with segments that start at the
level's first plane, in its middle and in a tail of short segments -- and on slabs, where a segment starts inside a
neighbour's halo planes.  CPU: every instantiation of the two shapes the dispatcher can launch stays within the register
budget of a 1024-thread workgroup (four waves per SIMD: at most 128 VGPRs), with nothing spilled and no scratch."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.test_march_one_barrier import LIB, LLVM, _MARCH, _SINGLE, _kernel_notes

HI = 3      # finest level of synthetic(3, HI - 2, HI, c): 8 c + 1 nodes per axis

# (K, c): 17^3 for every K; K = 5: 25^3, 49^3, 73^3 (1, 2, 3 tile rows of 24 lines and one line); K = 4: 105^3 (4 x 26 + 1);
# K = 3: 57^3 (2 x 28 + 1)
_CASES = [(3, 2), (4, 2), (5, 2), (5, 3), (5, 6), (5, 9), (4, 13), (3, 7)]
_EXTRAS = [dict(fuse_k_segments=1), dict(fuse_k_segments=3), dict(fuse_k_tail=4)]


def _vectors(c):
    m = 8 * c + 1
    rng = np.random.default_rng(1000 + c)
    return rng.standard_normal(m ** 3), rng.standard_normal(m ** 3)


def _smoothed(c, nw, tuning):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    with DeviceHierarchy.synthetic(3, HI - 2, HI, c=c, mu1=2, mu2=2, **tuning) as dev:
        assert dev.elements(HI) + 1 == 8 * c + 1
        v, f = _vectors(c)
        dev.set_vector(HI, "v", v)
        dev.set_vector(HI, "f", f)
        dev.reset_smoother_launches()
        dev.smooth(HI, nw)
        return dev.get_vector(HI, "v"), dev.smoother_launches(HI)


@functools.lru_cache(maxsize=None)
def _single_sweeps(c, nw):
    """nw sweeps, one per launch (computed once per grid and sweep count; read-only)."""
    got, _ = _smoothed(c, nw, _SINGLE)
    got.setflags(write=False)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("extra", _EXTRAS, ids=["s1", "s3", "tail"])
@pytest.mark.parametrize("k,c", _CASES, ids=[f"k{k}-{8 * c + 1}" for k, c in _CASES])
@pytest.mark.parametrize("shape", [8, 7])
def test_capped_march_is_bit_identical_to_single_sweeps(shape, k, c, extra):
    nw = 2 * k
    # ("fuse_k_min_side": the march on grids narrower than the 32 x 32 planes it otherwise asks for)
    got, ran = _smoothed(c, nw, dict(_MARCH, fuse_k=k, fuse_k_shape=shape, fuse_k_min_side=16, **extra))
    assert set(ran) == {"ksweep"} and ran["ksweep"][:2] == (2, nw), ran
    assert np.array_equal(_single_sweeps(c, nw), got)


@pytest.mark.gpu
def test_capped_march_on_slabs_matches_single_handle():
    """Shape 8, five sweeps per pass on two slabs with five halo planes (ranks as threads over the in-process RCCL stand-in):
    a rank's segments start inside its neighbour's planes; bit-identical to the single-handle run."""
    here = os.path.dirname(os.path.abspath(__file__))
    lib = os.path.join(here, "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(here, "fake_rccl")], check=True)
    tune = "halo_depth=5,fuse_k=5,fuse_k_shape=8,fuse_min_rows=0,fuse_k_slab_min_rows=0,fuse_k_slab_min_sweeps=2"
    env = dict(os.environ, MG_RCCL_LIBRARY=lib, MG_TEST_TUNE=tune, MG_TEST_EXPECT_KSLAB="1")
    out = subprocess.run([sys.executable, os.path.join(here, "fake_rccl_worker.py"), "2", "3", "2", "4", "8", "5", "0", "1"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "OK" in out.stdout


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"), reason="needs the built library and ROCm's LLVM tools")
def test_march_kernels_of_shapes_7_and_8_fit_the_register_budget():
    notes = _kernel_notes()
    want = []
    for k in (3, 4, 5):
        want += [f"void mgk::{kind}<{k}, 16, 2, 4, 256>(mgk::JK3Args)"
                 for kind in ("sdia_jacobikc_b1", "sdia_jacobikc_finest_b1", "sdia_jacobikc", "sdia_jacobikc_finest", "sdia_jacobikc_escape")]
    march = sorted(n for n in notes if "jacobikc" in n)
    for name in want:
        assert name in notes, (name, march)
    # ... and whatever else of the two shapes the library holds
    both = [n for n in march if re.search(r"sdia_jacobikc\w*<[345], 16, 2, ", n)]
    assert set(want) <= set(both)
    for name in both:
        vgpr, spilled, scratch = notes[name]
        assert vgpr <= 128 and spilled == 0 and scratch == 0, (name, notes[name])
