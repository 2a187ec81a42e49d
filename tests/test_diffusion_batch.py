"""Batched diffusion solves: one march of kappa for several right-hand sides (mg_apply_batch, mg_pcg_batch, DiffusionSolver.solve_many).

CPU: the header, the binding and the library agree on the new entries; the code object holds the fused march for NV = 2, 3, 4 in
every mode, with nothing spilled, no scratch and its LDS within a CU's 160 KiB.
GPU: every double and every partial sum of the fused launches has the bits of the one-vector kernel on that vector alone; every
lane of mg_pcg_batch has the solution, the history and the iteration count of a single mg_pcg; solve_many has the bits of B calls
of solve, and its gradients those of the ascending-lane sums."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from multigrid_dolfinx_amd import _capi
from tests.diffusion_reaction_workers import reaction_sigma
from tests.diffusion_robin_workers import robin_alpha
from tests.diffusion_workers import lognormal_kappa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "multigrid_dolfinx_amd", "libmg_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
ENTRIES = ("mg_apply_batch", "mg_pcg_batch", "mg_batch_info", "mg_release_batch")
# the fused march's tile and images (mg_diffusion_mf.hip.h): NV sets of four x images, three kappa images, NV x 8 partial sums
MF_XS, MF_KS = 66 * 10, 65 * 9
CU_LDS = 160 * 1024


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_batch_entries():
    header = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _capi.load()
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _capi.SIGNATURES and getattr(lib, name).argtypes == _capi.SIGNATURES[name], name
    assert re.search(r"#define\s+MG_BATCH_MAX\s+32\b", code) and _capi.MG_BATCH_MAX == 32
    ops = re.search(r"enum mg_batch_op \{([^}]*)\}", code).group(1)
    assert dict((n, int(v)) for n, v in re.findall(r"MG_BATCH_([A-Z]+)\s*=\s*(\d+)", ops)) == {"JACOBI": 0, "RESIDUAL": 1, "SPMV": 2}
    assert (_capi.MG_BATCH_JACOBI, _capi.MG_BATCH_RESIDUAL, _capi.MG_BATCH_SPMV) == (0, 1, 2)
    # the pointer arrays and the counts, as the header declares them
    assert _capi.SIGNATURES["mg_pcg_batch"] == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p,
                                                C.c_void_p]
    assert _capi.SIGNATURES["mg_apply_batch"] == [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4


def _kernel_notes():
    """{demangled kernel name: (spilled vgpr, scratch bytes, LDS bytes, vgpr)} from the gfx950 code object's notes (read as
    tests/test_march_one_barrier.py reads them)."""
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
                     (val("vgpr_spill_count"), val("private_segment_fixed_size"), val("group_segment_fixed_size"), val("vgpr_count"))))
    names = subprocess.run(["c++filt"] + [r[0] for r in rows], capture_output=True, text=True, check=True).stdout.split("\n")
    return {dn: res for (_, res), dn in zip(rows, names)}


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"), reason="needs the built library and ROCm's LLVM tools")
def test_fused_march_kernels_are_in_the_code_object_within_their_resources():
    """NV = 2, 3, 4 x (Jacobi, residual, SpMV, SpMV with the dot) x (default faces, a face set) x (with, without the nodal diagonal):
    no spilled VGPR, no scratch, and exactly the LDS of NV sets of x images, one set of kappa images and the partial sums."""
    notes = _kernel_notes()
    found = {}
    for name, res in notes.items():
        m = re.match(r"void mgk::diffusion_mf_batch<(\d+), (\d+), (true|false), (true|false), (true|false)>\(mgk::MfBatchArgs<(\d+)>\)", name)
        if m:
            assert m.group(1) == m.group(6)
            found.setdefault(int(m.group(1)), {})[m.groups()[1:5]] = res
    assert sorted(found) == [2, 3, 4], sorted(found)
    for nv, kernels in found.items():
        assert len(kernels) == 16, (nv, sorted(kernels))
        assert len({k[0] for k in kernels}) == 3 and {k[1:] for k in kernels if k[1] == "true"} and {k[2] for k in kernels} == {"true", "false"}
        for key, (spilled, scratch, group, vgpr) in kernels.items():
            images = 8 * (nv * 4 * MF_XS + 3 * MF_KS)
            sums = 8 * nv * 8 + 64 if key[1] == "true" else 0       # (the partial sums and their alignment: with the dot only)
            print(nv, key, "vgpr", vgpr, "lds", group)
            assert spilled == 0 and scratch == 0, (nv, key, spilled, scratch)
            assert images <= group <= images + sums and group <= CU_LDS, (nv, key, group, images)


# ---- GPU: the kernel by itself --------------------------------------------------------------------------------------------------
KERNEL_N = (8, 36, 72)      # 9^3 nodes: part of one 64 x 8 tile; 37^3: the y tiles, two z segments; 73^3: past the tile edge in x, four segments
LANES = 7                   # groups of 4 + 3; its prefixes give 4 + 1 and the odd NVs
# (face set, reaction field, Robin face)
VARIANTS = {"default": (63, False, None), "sigma": (63, True, None), "faces18": (18, False, None), "faces18_sigma": (18, True, None),
            "faces1": (1, False, None), "faces1_sigma": (1, True, None), "faces18_robin": (18, False, 32)}       # (z+ = 32: a no-flux face of the set 18)


def _device_array(h, host):
    from multigrid_dolfinx_amd.hierarchy import _DeviceArray
    host = np.ascontiguousarray(host, dtype=np.float64).reshape(-1)
    return _DeviceArray(h._lib, h.device, host.size, host)


class _Lanes:
    """Device copies of a list of host vectors, freed on exit."""

    def __init__(self, h, hosts):
        self.arrays = [_device_array(h, x) for x in hosts]
        self.ptrs = [a.ptr.value for a in self.arrays]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for a in self.arrays:
            a.free()

    def download(self):
        return [a.download() for a in self.arrays]


def _level_handle(N, variant, matrix_free, **tuning):
    """Level 1 of a two-level handle generated from a log-normal kappa, stored or matrix-free, in the variant's setting."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    faces, react, robin = VARIANTS[variant]
    h = DeviceHierarchy(3, 0, 1, c=N // 2, **tuning)
    h.set_diffusion_faces(faces)
    if react:
        h.set_diffusion_reaction(reaction_sigma(N))
    if robin:
        h.set_diffusion_robin(robin, robin_alpha(N, robin))
    h.gen_diffusion_level(1, lognormal_kappa(N, 3, seed=3), matrix_free=matrix_free)
    h.set_params(2, 2, 2.0 / 3.0)
    assert h.level_matrix_free(1) == matrix_free
    return h


def _single_vector_results(h, xs, fs):
    """Per lane, with the handle's own one-vector calls: (Jacobi sweep, residual, A x, x . A x)."""
    out = []
    for x, f in zip(xs, fs):
        h.set_vector(1, "v", x)
        h.set_vector(1, "f", f)
        h.residual(1)
        r = h.get_vector(1, "r").reshape(-1)
        h.smooth(1, 1)
        j = h.get_vector(1, "v").reshape(-1)
        h.set_vector(1, "v", x)
        dot = h.quadratic_form(1, "v")          # the SpMV with its dot product: A x in "r"
        out.append((j, r, h.get_vector(1, "r").reshape(-1), dot))
    return out


def _check_apply(h, xs, fs, want, nb, label):
    n = xs[0].size
    with _Lanes(h, xs[:nb]) as X, _Lanes(h, fs[:nb]) as F, _Lanes(h, [np.full(n, np.nan)] * nb) as O:
        for k, op in enumerate(("jacobi", "residual", "spmv")):
            dots = h.apply_batch(op, X.ptrs, None if op == "spmv" else F.ptrs, O.ptrs, level=1, dots=op == "spmv")
            for b, got in enumerate(O.download()):
                assert got.tobytes() == want[b][k].tobytes(), (label, op, nb, b, np.flatnonzero(got != want[b][k])[:5])
            if op == "spmv":
                assert dots.tobytes() == np.array([w[3] for w in want[:nb]]).tobytes(), (label, nb, dots, [w[3] for w in want[:nb]])
        h.apply_batch("spmv", X.ptrs, None, O.ptrs, level=1)       # ... and the SpMV without the dot product
        for b, got in enumerate(O.download()):
            assert got.tobytes() == want[b][2].tobytes(), (label, "spmv, no dots", nb, b)
        for b, (x, f) in enumerate(zip(X.download(), F.download())):       # the inputs are only read
            assert x.tobytes() == xs[b].tobytes() and f.tobytes() == fs[b].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("N", KERNEL_N)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_fused_march_has_the_bits_of_the_one_vector_kernel(variant, N):
    """mg_apply_batch on a matrix-free level, nb in {2, 3, 4, 5, 7} (groups of 2, 3, 4, 4 + 1, 4 + 3) and "mf_batch" 0 and 2: the
    three operations and the dots, byte for byte the handle's own mg_smooth(level, 1), mg_residual and the SpMV with its dot
    product (mg_quadratic_form: A x in MG_VEC_R, the partial sums reduced in the same order)."""
    rng = np.random.default_rng(100 + N)
    with _level_handle(N, variant, True) as h:
        n = h.n_dofs(1)
        xs = [rng.standard_normal(n) for _ in range(LANES)]
        fs = [rng.standard_normal(n) for _ in range(LANES)]
        want = _single_vector_results(h, xs, fs)
        assert h.batch_info() == {"lanes": 0, "bytes": 0}
        for nb, launches in ((2, 1), (3, 1), (4, 1), (5, 2), (7, 2)):
            h.reset_smoother_launches()
            _check_apply(h, xs, fs, want, nb, variant)
            assert h.smoother_launches(1) == {"matrix_free": (launches, nb, 0)}     # one Jacobi call: a launch per group, a sweep per lane
        for mf_batch, nb, launches in ((0, 3, 3), (1, 2, 2), (2, 5, 3)):
            h.set_tuning("mf_batch", mf_batch)
            h.reset_smoother_launches()
            _check_apply(h, xs, fs, want, nb, (variant, "mf_batch", mf_batch))
            assert h.smoother_launches(1) == {"matrix_free": (launches, nb, 0)}
        assert h.batch_info()["lanes"] == LANES - 1


@pytest.mark.gpu
def test_fused_march_in_the_chunked_workgroup_order():
    """161^3 nodes: 3 x 21 tiles in at least nine z segments, 567 work items or more -- at 512 the plan hands the workgroups to the
    XCDs in chunks of 16 (`ch` = 16), the order every smaller shape here does not take.  Four lanes in one launch, the three
    operations and the dots to the byte of the one-vector calls."""
    N = 160
    rng = np.random.default_rng(N)
    with _level_handle(N, "faces18_sigma", True) as h:
        n = h.n_dofs(1)
        xs = [rng.standard_normal(n) for _ in range(4)]
        fs = [rng.standard_normal(n) for _ in range(4)]
        want = _single_vector_results(h, xs, fs)
        h.reset_smoother_launches()
        _check_apply(h, xs, fs, want, 4, "ch16")
        assert h.smoother_launches(1) == {"matrix_free": (1, 4, 0)}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "faces18_sigma"])
def test_apply_batch_on_a_stored_level_loops_over_the_lanes(variant):
    """The same calls on a stored level run the one-vector kernels once per lane: the bytes of the single calls."""
    N = 36
    rng = np.random.default_rng(7)
    with _level_handle(N, variant, False, row_classes=0, fuse_sweeps=0) as h:
        n = h.n_dofs(1)
        xs = [rng.standard_normal(n) for _ in range(3)]
        fs = [rng.standard_normal(n) for _ in range(3)]
        want = _single_vector_results(h, xs, fs)
        h.reset_smoother_launches()
        _check_apply(h, xs, fs, want, 3, variant)
        assert h.smoother_launches(1) == {"slice": (3, 3, 0)}


# ---- GPU: mg_pcg_batch ----------------------------------------------------------------------------------------------------------
def _hierarchy(N, nlev, smoother="jacobi", faces=63, **tuning):
    """A generated diffusion hierarchy with every level above the coarsest matrix-free, the P1 transfers, V(2,2)."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    top = nlev - 1
    h = DeviceHierarchy(3, 0, top, c=N >> top, **tuning)
    h.set_prolongation("p1")
    h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose", smoother=smoother)
    h.set_diffusion_faces(faces)
    h.gen_diffusion_hierarchy(lognormal_kappa(N, 3, seed=5), matrix_free_min_rows=0)
    assert all(h.level_matrix_free(l) for l in range(1, top + 1)) and not h.level_matrix_free(0)
    return h


def _right_hand_sides(N):
    """Five lanes of very different difficulty: a smooth mode, white noise, zero, a point source, and noise again (which the test
    starts next to its solution)."""
    m = N + 1
    rng = np.random.default_rng(N)
    t = np.linspace(0.0, 1.0, m)
    smooth = np.einsum("i,j,k->ijk", np.sin(np.pi * t), np.sin(np.pi * t), np.sin(np.pi * t)).reshape(-1)
    noise = rng.standard_normal(m ** 3)
    point = np.zeros(m ** 3)
    point[(m // 3) * m * m + (m // 2) * m + m // 4] = 1.0e3
    return [smooth, noise, np.zeros(m ** 3), point, noise.copy()]


def _single_solves(h, top, fs, x0s, rtol, max_iter):
    """The call sequence of the contract, lane by lane: (x, history)."""
    out = []
    n = fs[0].size
    for f, x0 in zip(fs, x0s):
        with _Lanes(h, [f, x0]) as D:
            h.set_vector_device(top, "f", D.ptrs[0])
            h.set_vector_device(top, "v", D.ptrs[1])
            hist = h.pcg(rtol, max_iter, top)
            h.get_vector_device(top, "v", D.ptrs[1])
            out.append((D.arrays[1].download(), hist))
        assert out[-1][0].size == n
    return out


def _plain_pcg(h, top, f, rtol, max_iter):
    h.set_vector(top, "f", f)
    h.zero_vector(top, "v")
    hist = h.pcg(rtol, max_iter, top)
    return hist.tobytes(), h.get_vector(top, "v").tobytes(), h.get_vector(top, "r").tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("N,nlev,smoother,faces", [(32, 4, "jacobi", 63), (64, 6, "jacobi", 63), (32, 4, "chebyshev", 63), (32, 4, "jacobi", 18)],
                         ids=["n32", "n64", "n32-chebyshev", "n32-faces18"])
def test_pcg_batch_lanes_have_the_bits_of_single_solves(N, nlev, smoother, faces):
    """nb = 5, lanes that stop at different iterations (one at 0): x, the history and the iteration count of every lane, byte for
    byte those of the single mg_pcg sequence on a second handle; afterwards a plain mg_pcg on the batch handle equals that of
    the handle that never ran a batch, and the lanes' bytes are what memory_bytes grew by and what release_batch returns."""
    top, rtol, max_iter = nlev - 1, 1e-9, 40
    fs = _right_hand_sides(N)
    with _hierarchy(N, nlev, smoother, faces) as ref, _hierarchy(N, nlev, smoother, faces) as h:
        x0s = [np.zeros_like(f) for f in fs]
        first = _single_solves(ref, top, fs[1:2], x0s[1:2], rtol, max_iter)[0]
        x0s[4] = first[0] * (1.0 + 1.0e-5)                # next to the solution: a few iterations
        want = _single_solves(ref, top, fs, x0s, rtol, max_iter)
        its = [len(hist) for _, hist in want]
        print("iterations per lane:", its)
        assert its[2] == 0 and len(set(its)) >= 3 and max(its) < max_iter, its
        plain_ref = _plain_pcg(ref, top, fs[1], rtol, max_iter)
        assert _plain_pcg(h, top, fs[1], rtol, max_iter) == plain_ref        # (so that lane 0's work vectors exist on both)
        before = h.memory_bytes()
        assert before == ref.memory_bytes() and h.batch_info() == {"lanes": 0, "bytes": 0}
        for mf_batch in (4, 2, 0):
            h.set_tuning("mf_batch", mf_batch)
            with _Lanes(h, fs) as F, _Lanes(h, x0s) as X:
                hists = h.pcg_batch(F.ptrs, X.ptrs, rtol, max_iter, top)
                got = X.download()
                for b, f in enumerate(F.download()):
                    assert f.tobytes() == fs[b].tobytes()
            for b in range(len(fs)):
                assert hists[b].tobytes() == want[b][1].tobytes(), (mf_batch, b, hists[b], want[b][1])
                assert got[b].tobytes() == want[b][0].tobytes(), (mf_batch, b)
        h.set_tuning("mf_batch", 4)
        info = h.batch_info()
        assert info["lanes"] == 4 and info["bytes"] > 0 and h.memory_bytes() == before + info["bytes"], (info, before, h.memory_bytes())
        # a smaller batch reuses the lanes; a plain solve is what it is on a handle that never ran a batch
        with _Lanes(h, fs[:2]) as F, _Lanes(h, x0s[:2]) as X:
            hists = h.pcg_batch(F.ptrs, X.ptrs, rtol, max_iter, top)
            assert [x.tobytes() for x in X.download()] == [w[0].tobytes() for w in want[:2]]
        assert h.batch_info() == info
        assert _plain_pcg(h, top, fs[1], rtol, max_iter) == plain_ref
        h.release_batch()
        assert h.batch_info() == {"lanes": 0, "bytes": 0} and h.memory_bytes() == before
        assert _plain_pcg(h, top, fs[1], rtol, max_iter) == plain_ref


@pytest.mark.gpu
def test_pcg_batch_counts_a_fused_launch_once_with_a_sweep_per_lane():
    """rtol = 0: every lane runs exactly max_iter iterations, so all lanes are active in every cycle.  With nb <= "mf_batch" every
    smoother launch of a matrix-free level carries nb sweeps; with "mf_batch" 0 every launch is one sweep."""
    N, nlev, nb = 32, 4, 3
    fs = _right_hand_sides(N)[:2] + [np.ones((N + 1) ** 3)]
    counts = {}
    for mf_batch in (4, 0):
        with _hierarchy(N, nlev, mf_batch=mf_batch) as h, _Lanes(h, fs) as F, _Lanes(h, [np.zeros_like(f) for f in fs]) as X:
            h.reset_smoother_launches()
            hists = h.pcg_batch(F.ptrs, X.ptrs, 0.0, 2, nlev - 1)
            assert [len(x) for x in hists] == [2] * nb
            counts[mf_batch] = [h.smoother_launches(l) for l in range(1, nlev)]
    for per_level in counts[4]:
        launches, sweeps, _ = per_level["matrix_free"]
        assert set(per_level) == {"matrix_free"} and launches > 0 and sweeps == nb * launches, per_level
    for per_level, fused in zip(counts[0], counts[4]):
        launches, sweeps, _ = per_level["matrix_free"]
        assert sweeps == launches == fused["matrix_free"][1], (per_level, fused)


@pytest.mark.gpu
def test_lanes_survive_a_refresh_and_go_with_a_level_of_another_size():
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N, nlev = 16, 3
    fs = _right_hand_sides(N)[:3]
    with _hierarchy(N, nlev) as h:
        with _Lanes(h, fs) as F, _Lanes(h, [np.zeros_like(f) for f in fs]) as X:
            h.pcg_batch(F.ptrs, X.ptrs, 1e-8, 20, nlev - 1)
        info = h.batch_info()
        assert info["lanes"] == 2
        h.refresh_diffusion_hierarchy(lognormal_kappa(N, 3, seed=6))
        assert h.batch_info() == info
        h.gen_diffusion_hierarchy(lognormal_kappa(N, 3, seed=6), matrix_free_min_rows=0)       # the same sizes again: kept
        assert h.batch_info() == info
    with DeviceHierarchy(3, 0, 1, c=8) as h:
        h.gen_diffusion_level(1, lognormal_kappa(16, 3, seed=1), matrix_free=True)
        n = h.n_dofs(1)
        with _Lanes(h, [np.ones(n)] * 2) as X, _Lanes(h, [np.zeros(n)] * 2) as O:
            h.apply_batch("spmv", X.ptrs, None, O.ptrs, level=1)
        assert h.batch_info()["lanes"] == 1
        h.gen_diffusion_level(0, lognormal_kappa(8, 3, seed=1))        # another level: level 1's lanes stay
        assert h.batch_info()["lanes"] == 1
        # level 1 set again with ANOTHER size (33^3 nodes instead of 17^3; the library takes any N = N0 * 2^level): the lanes go,
        # and the handle holds what a handle holds that generated that level and never ran a batch
        k32 = lognormal_kappa(32, 3, seed=1)
        _capi.check(h._lib.mg_gen_diffusion_level_mf(h._h, 1, 32, _capi.ptr(k32)))
        assert h.batch_info() == {"lanes": 0, "bytes": 0}
        with DeviceHierarchy(3, 0, 1, c=8) as fresh:       # the same history without the batch call
            fresh.gen_diffusion_level(1, lognormal_kappa(16, 3, seed=1), matrix_free=True)
            fresh.gen_diffusion_level(0, lognormal_kappa(8, 3, seed=1))
            _capi.check(fresh._lib.mg_gen_diffusion_level_mf(fresh._h, 1, 32, _capi.ptr(k32)))
            assert h.memory_bytes() == fresh.memory_bytes()
            n = 33 ** 3
            with _Lanes(h, [np.ones(n)] * 2) as X, _Lanes(h, [np.zeros(n)] * 2) as O:       # ... and batches again at the new size
                h.apply_batch("spmv", X.ptrs, None, O.ptrs, level=1)
                got = O.download()
            assert h.batch_info()["lanes"] == 1
            with _Lanes(fresh, [np.ones(n)]) as V:          # (by pointer: the Python handle still counts 17^3 nodes)
                fresh.set_vector_device(1, "v", V.ptrs[0])
                fresh.quadratic_form(1, "v")
                fresh.get_vector_device(1, "r", V.ptrs[0])
                want = V.download()[0]
            assert got[0].tobytes() == got[1].tobytes() == want.tobytes() and np.abs(want).max() > 0.0


def _refused(call, text):
    with pytest.raises(_capi.MgError) as e:
        call()
    assert text in str(e.value), (text, str(e.value))


@pytest.mark.gpu
def test_batch_refusals_leave_the_handle_as_it_was():
    """Every refusal by name, before anything is launched or allocated: memory_bytes, the lanes and a following mg_pcg unchanged."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N, nlev = 16, 3
    top = nlev - 1
    fs = _right_hand_sides(N)[:2]
    with _hierarchy(N, nlev) as h:
        n = h.n_dofs(top)
        plain = _plain_pcg(h, top, fs[1], 1e-8, 20)
        before = h.memory_bytes()
        host = np.zeros(n)
        with _Lanes(h, fs) as F, _Lanes(h, [np.zeros(n)] * 2) as X, _Lanes(h, [np.zeros(2 * n)]) as W:
            pcg = lambda f, x, level=top: h.pcg_batch(f, x, 1e-8, 20, level)
            calls = [
                (lambda: pcg([], []), "is outside 1..32"),
                (lambda: pcg([F.ptrs[0]] * 33, [X.ptrs[0]] * 33), "is outside 1..32"),
                (lambda: pcg([F.ptrs[0], 0], X.ptrs), "null pointer (f_dev[1])"),
                (lambda: pcg(F.ptrs, [0, X.ptrs[1]]), "null pointer (x_dev[0])"),
                (lambda: pcg(F.ptrs, [X.ptrs[0], host.ctypes.data]), "x_dev[1] is not device memory"),
                (lambda: pcg(F.ptrs, [X.ptrs[0], X.ptrs[0]]), "x_dev[0] overlaps x_dev[1]"),
                (lambda: pcg(F.ptrs, [W.ptrs[0], W.ptrs[0] + 8 * (n - 1)]), "x_dev[0] overlaps x_dev[1]"),
                (lambda: pcg(F.ptrs, [X.ptrs[0], F.ptrs[0]]), "x_dev[1] overlaps f_dev[0]"),
                (lambda: pcg(F.ptrs, X.ptrs, 0), "level 0 is the coarsest level"),
                (lambda: h.apply_batch("jacobi", X.ptrs, F.ptrs, X.ptrs, level=top), "out_dev[0] overlaps x_dev[0]"),
                (lambda: h.apply_batch("residual", X.ptrs, F.ptrs, [W.ptrs[0], W.ptrs[0] + 8]), "out_dev[0] overlaps out_dev[1]"),
                (lambda: h.apply_batch("spmv", [X.ptrs[0], 0], None, [W.ptrs[0], W.ptrs[0] + 8 * n]), "null pointer (x_dev[1])"),
            ]
            for call, text in calls:
                _refused(call, text)
                assert h.memory_bytes() == before and h.batch_info() == {"lanes": 0, "bytes": 0}, text
            _refused(lambda: h._lib.mg_pcg_batch(h._h, top, 2, None, None, 1e-8, 20, None, None) and _capi.check(1), "null pointer array")
            # a Gauss-Seidel smoother with a matrix-free level in the cycle; transfers the face set does not allow
            h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose", smoother="rbgs")
            _refused(lambda: pcg(F.ptrs, X.ptrs), "Gauss-Seidel smoothers (RBGS, MCGS) need stored rows")
            _refused(lambda: h.apply_batch("jacobi", X.ptrs, F.ptrs, [W.ptrs[0], W.ptrs[0] + 8 * n], level=top), "the handle's smoother is another one")
            h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
            assert h.memory_bytes() == before and h.batch_info() == {"lanes": 0, "bytes": 0}
        assert _plain_pcg(h, top, fs[1], 1e-8, 20) == plain
    with _hierarchy(N, nlev, faces=18) as h:
        h.set_params(2, 2, 2.0 / 3.0, restriction="full_weighting")
        before = h.memory_bytes()
        with _Lanes(h, fs) as F, _Lanes(h, [np.zeros_like(f) for f in fs]) as X:
            _refused(lambda: h.pcg_batch(F.ptrs, X.ptrs, 1e-8, 20, top), "need the P1 transfers")
        assert h.memory_bytes() == before
    nothing = lambda *args: None
    with DeviceHierarchy(3, 0, 1, c=4) as slab:                             # a slab handle
        slab.set_comm_callbacks(0, 2, nothing, nothing, nothing)
        with _Lanes(slab, [np.zeros(9 ** 3)] * 2) as F, _Lanes(slab, [np.zeros(9 ** 3)] * 2) as X:
            _refused(lambda: slab.pcg_batch(F.ptrs, X.ptrs, 1e-8, 5, 1), "needs a whole (not slab) handle")
            _refused(lambda: slab.apply_batch("spmv", F.ptrs, None, X.ptrs, level=1), "needs a whole (not slab) handle")
    with DeviceHierarchy(3, 0, 0, c=16) as flat:                            # a flat level
        from multigrid_dolfinx_amd import poisson
        flat.set_flat_level(poisson.lexicographic_level(4, 2).A)
        before = flat.memory_bytes()
        with _Lanes(flat, [np.zeros(125)] * 2) as F, _Lanes(flat, [np.zeros(125)] * 2) as X:
            _refused(lambda: flat.apply_batch("spmv", F.ptrs, None, X.ptrs, level=0), "is flat (no grid)")
            _refused(lambda: flat.pcg_batch(F.ptrs, X.ptrs, 1e-8, 5, 0), "is flat (no grid)")
        assert flat.memory_bytes() == before
    with DeviceHierarchy.synthetic(2, 2, 3, c=8, mu1=2, mu2=2) as h:       # a 2-D handle
        n = h.n_dofs(3)
        with _Lanes(h, [np.zeros(n)] * 2) as F, _Lanes(h, [np.zeros(n)] * 2) as X:
            _refused(lambda: h.pcg_batch(F.ptrs, X.ptrs, 1e-8, 5, 3), "3-D only (this handle is 2-D)")
            _refused(lambda: h.apply_batch("spmv", F.ptrs, None, X.ptrs, level=3), "3-D only (this handle is 2-D)")


# ---- GPU: DiffusionSolver.solve_many (torch in a worker process, as the other diffusion tests run it) -----------------------------
def _torch_first(worker, *args):
    code = "import torch, sys; sys.path.insert(0, %r); import tests.diffusion_batch_workers as w; w.%s(%s)" % (
        ROOT, worker, ", ".join(repr(a) for a in args))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    print(out.stdout)
    return out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("N,nlev", [(16, 3), (32, 4)])
def test_solve_many_forward_and_gradients_against_single_solves(N, nlev):
    """U[b], grad_F byte for byte those of solve(kappa, F[b]); grad_kappa, grad_sigma, grad_alpha (no g) byte for byte the
    ascending-lane sums of the single solves' gradients; with g (shared and per lane) within the reassociation bound."""
    assert "gradients ok" in _torch_first("gradients_worker", N, nlev)


@pytest.mark.gpu
@pytest.mark.parametrize("N,nlev", [(16, 3), (32, 4)])
def test_solve_many_hessian_vector_product_is_four_batched_solves(N, nlev):
    assert "hvp ok" in _torch_first("hvp_worker", N, nlev)


@pytest.mark.gpu
@pytest.mark.parametrize("N,nlev", [(16, 3), (32, 4)])
def test_solve_many_bookkeeping(N, nlev):
    """NotConverged names the lanes; same_operator=True performs no generation; warm starts; close() releases the lanes."""
    assert "bookkeeping ok" in _torch_first("bookkeeping_worker", N, nlev)
