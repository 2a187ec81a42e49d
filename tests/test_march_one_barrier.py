"""Tile shape 8 of the K-sweep march (`sdia_jacobikc_b1`, mg_jacobik3d.hip.h): one barrier per step -- level 0 in registers,
the images of levels 1 .. K-1 double-buffered by the parity of the step.

CPU: the built library holds the kernels for K = 3, 4, 5 within the register budget of a 1024-thread workgroup (four waves per
SIMD: at most 128 VGPRs), with nothing spilled.  GPU: bit-identical to one sweep per launch on tile-unaligned grids, with one
to four plane segments and a tail of short ones, on slabs, against the oracle on 129^3 and at the headline size against
shape 7."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "multigrid_dolfinx_amd", "libmg_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"

# one sweep per launch on every level
_SINGLE = dict(fuse_k=0, fuse_sweeps=0, fuse_block=0, fuse_small=0)
# the march on every level, whatever its size
_MARCH = dict(fuse_min_rows=0, march_min_rows=0, fuse_k_min_rows=0, fuse_k4_min_rows=0, fuse_k5_min_rows=0,
              fuse_k_small_rows=0, fuse_block=0, fuse_small=0, fuse_k_shape=8)


def _kernel_notes():
    """{demangled kernel name: (vgpr, spilled vgpr, scratch bytes)} from the gfx950 code object's notes."""
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(LIB, local)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", local], cwd=tmp, check=True, capture_output=True)
        co = next(os.path.join(tmp, f) for f in os.listdir(tmp) if "gfx950" in f)
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    rows = []
    for block in notes.split("- .agpr_count:")[1:]:
        val = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
        rows.append((re.search(r"\.name:\s+(\S+)", block).group(1),
                     (val("vgpr_count"), val("vgpr_spill_count"), val("private_segment_fixed_size"))))
    names = subprocess.run(["c++filt"] + [r[0] for r in rows], capture_output=True, text=True, check=True).stdout.split("\n")
    return {dn: res for (_, res), dn in zip(rows, names)}


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"), reason="needs the built library and ROCm's LLVM tools")
def test_shape8_kernels_fit_the_register_budget():
    notes = _kernel_notes()
    for k in (3, 4, 5):
        for kind in ("sdia_jacobikc_b1", "sdia_jacobikc_finest_b1"):
            name = f"void mgk::{kind}<{k}, 16, 2, 4, 256>(mgk::JK3Args)"
            assert name in notes, (name, sorted(n for n in notes if "jacobikc" in n))
            vgpr, spilled, scratch = notes[name]
            assert vgpr <= 128 and spilled == 0 and scratch == 0, (name, notes[name])


def _random_level(dev, level, seed):
    m = dev.elements(level) + 1
    rng = np.random.default_rng(seed)
    return rng.standard_normal(m ** 3), rng.standard_normal(m ** 3)


# c, finest level: 41^3, 57^3, 65^3 (c = 4: tiles of 54 x 24 cells leave a partial tile in x and y on all of them), 129^3
_GRIDS = [(5, 3), (7, 3), (4, 4), (8, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("c,hi", _GRIDS, ids=["41", "57", "65", "129"])
@pytest.mark.parametrize("k,extra", [(3, {}), (4, dict(fuse_k_segments=2)), (5, dict(fuse_k_segments=3)), (5, dict(fuse_k_segments=1)),
                                     (4, dict(fuse_k_segments=4)), (3, dict(fuse_k_tail=4)), (5, dict(fuse_k_tail=4))],
                         ids=["k3", "k4s2", "k5s3", "k5s1", "k4s4", "k3tail", "k5tail"])
def test_shape8_is_bit_identical_to_single_sweeps(c, hi, k, extra):
    """K sweeps per pass in shape 8 against one sweep per launch: every tile of the plane (interior tiles, those on the x
    and y boundaries -- the three forms of a step --) and the first and last planes of every segment."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    nw = 2 * k
    got = {}
    for name, kw in (("single", _SINGLE), ("march", dict(_MARCH, fuse_k=k, **extra))):
        with DeviceHierarchy.synthetic(3, hi - 2, hi, c=c, mu1=2, mu2=2, **kw) as dev:
            v, f = _random_level(dev, hi, 11 * c + hi)
            dev.set_vector(hi, "v", v)
            dev.set_vector(hi, "f", f)
            dev.reset_smoother_launches()
            dev.smooth(hi, nw)
            got[name] = dev.get_vector(hi, "v")
            ran = dev.smoother_launches(hi)
        if name == "march":
            assert set(ran) == {"ksweep"} and ran["ksweep"][:2] == (2, nw), ran
            if extra.get("fuse_k_tail") and (c, hi) != (5, 3):      # (41^3: two tiles, no last round to cut short)
                assert ran["ksweep"][2] > 0, ran
    assert np.array_equal(got["single"], got["march"])


@pytest.mark.gpu
def test_shape8_against_the_oracle_at_129():
    """The reference's V(50,50) on the 129^3 hierarchy with five sweeps per pass in shape 8 on every level."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    from tests.helpers import rel_l2
    from tests.test_gpu_parity import TOL_ITER, _n128_oracle
    want, res_want = _n128_oracle()
    with DeviceHierarchy.synthetic(3, 2, 4, c=8, mu1=50, mu2=50, **dict(_MARCH, fuse_k_small_rows=1 << 22)) as dev:
        dev.zero_vector(4, "v")
        res = dev.vcycle(4, 1, residuals=True)
        got = dev.get_vector(4, "v")
        counts = dev.smoother_launches(4)
    assert {p: (n, s) for p, (n, s, _) in counts.items()} == {"ksweep": (20, 100)}, counts
    assert rel_l2(got, want) <= TOL_ITER
    assert abs(res[0] - res_want) <= TOL_ITER * res_want


@pytest.mark.gpu
@pytest.mark.parametrize("world,mu,depth,fuse_k", [(2, 5, 5, 5), (3, 9, 4, 4)])
def test_shape8_on_slabs_matches_single_handle(world, mu, depth, fuse_k):
    """Shape 8 on slabs (plane ranges beyond the owned ones, two plane ranges per launch), ranks as threads over the
    in-process RCCL stand-in: bit-identical to the single-handle run."""
    here = os.path.dirname(os.path.abspath(__file__))
    lib = os.path.join(here, "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(here, "fake_rccl")], check=True)
    tune = f"halo_depth={depth},fuse_k={fuse_k},fuse_k_shape=8,fuse_min_rows=0,fuse_k_slab_min_rows=0,fuse_k_slab_min_sweeps=2"
    env = dict(os.environ, MG_RCCL_LIBRARY=lib, MG_TEST_TUNE=tune, MG_TEST_EXPECT_KSLAB="1")
    out = subprocess.run([sys.executable, os.path.join(here, "fake_rccl_worker.py"), str(world), "3", "2", "4", "8", str(mu), "0", "1"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "OK" in out.stdout


@pytest.mark.gpu
def test_headline_size_shape8_matches_shape7():
    """C4's hierarchy (1025^3, 6 levels) with V(7,7): the default (shape 8 for the five-sweep passes on 1025^3 and 513^3)
    against shape 7 -- equal residual norms, the same exact fingerprint of the finest iterate."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    from tests.test_gpu_parity import _fingerprint
    norms, prints = [], []
    for kw in (dict(), dict(fuse_k_shape=7)):
        with DeviceHierarchy.synthetic(3, 2, 7, c=8, mu1=7, mu2=7, **kw) as dev:
            dev.zero_vector(7, "v")
            res = dev.vcycle(7, 1, residuals=True)
            counts = dev.smoother_launches(7)
            v = dev.get_vector(7, "v")
        assert counts["ksweep"][:2] == (2, 10), counts
        norms.append(float(res[0]))
        prints.append(_fingerprint(v))
        del v
    assert norms[0] == norms[1], norms
    for a, b in zip(*prints):
        assert np.array_equal(a, b)
