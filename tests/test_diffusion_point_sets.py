"""Located point sets (mg_points_create, _destroy, _info, mg_points_sample, _load, _gradient, _gradient_t; "Located point
sets" in mg_diffusion_points.hip.h): a set that is checked, located and sorted once serves S, S^T, G and G^T for any number of
lanes per call, every lane with the bytes of the host restatements in poisson.py AND of the one-field entries
mg_diffusion_point_*; poisson.diffusion_point_runs restates the order and the runs a set keeps; DiffusionSolver.locate and the
`_many` forms through autograd."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from multigrid_dolfinx_amd import poisson
from tests.diffusion_points_workers import special_points
from tests.diffusion_workers import lognormal_kappa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sample", "load", "gradient", "gradient_t")
LANES = 9


# ---- host ------------------------------------------------------------------------------------------------------------------
def _crowd(N=5, M=1000):
    """The 1000 points in one cell of tests/test_diffusion_points.py::test_a_node_sums_its_points_in_ascending_order."""
    rng = np.random.default_rng(4)
    return (np.array([2.0, 4.0, 0.0]) + rng.random((M, 3))) / N


@pytest.mark.parametrize("N, pts", [(5, _crowd()), (8, special_points(8, seed=8))], ids=["N5-one-cell", "N8-special"])
def test_runs_are_the_stable_order_by_node(N, pts):
    """`diffusion_point_runs`: slot_order is a permutation of 0 .. 4 M - 1 along which the nodes do not decrease and, inside a
    run, the slots ascend; run_node is strictly ascending and is np.unique of the nodes; adding lam * w along each run front to
    back onto +0.0 gives `diffusion_point_load` to the byte."""
    M = pts.shape[0]
    nodes, lam, _ = poisson.diffusion_point_locate(N, pts)
    order, start, run_node = poisson.diffusion_point_runs(N, pts)
    assert order.dtype == np.int64 and np.array_equal(np.sort(order), np.arange(4 * M))
    along = nodes.reshape(-1)[order]
    assert np.all(np.diff(along) >= 0)
    R = run_node.size
    assert start.shape == (R + 1,) and start[0] == 0 and start[-1] == 4 * M and np.all(np.diff(start) > 0)
    assert np.all(np.diff(run_node) > 0) and np.array_equal(run_node, np.unique(nodes))
    w = np.random.default_rng(2).standard_normal(M)
    contrib = (lam * w[:, None]).reshape(-1)
    out = np.zeros((N + 1) ** 3)
    for r in range(R):
        run = order[start[r]:start[r + 1]]
        assert np.all(np.diff(run) > 0) and np.all(along[start[r]:start[r + 1]] == run_node[r])
        acc = 0.0
        for s in run:
            acc = acc + contrib[s]
        out[run_node[r]] = acc
    assert out.tobytes() == poisson.diffusion_point_load(N, pts, w).tobytes()
    if N == 5:
        assert R == 8 and np.diff(start).max() == M         # every point of the crowd touches the cell's two diagonal corners


def test_capi_names_the_seven_entries():
    """Header and binding agree on the seven new names (the library's side: tests/test_capi_symbols)."""
    from multigrid_dolfinx_amd import _capi
    header = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    assert "int mg_points_create(mg_handle h, int level, int64_t M, const double* pts_dev, mg_points_handle* ps);" in header
    assert "int mg_points_destroy(mg_handle h, mg_points_handle ps);" in header
    assert "int mg_points_info(mg_handle h, mg_points_handle ps, int* level, int* N, int64_t* M, int64_t* runs, int64_t* longest_run, int64_t* bytes);" in header
    assert len(_capi.SIGNATURES["mg_points_create"]) == 5 and len(_capi.SIGNATURES["mg_points_destroy"]) == 2
    assert len(_capi.SIGNATURES["mg_points_info"]) == 8
    for k in NAMES:
        name = "mg_points_" + k
        assert "int %s(mg_handle h, mg_points_handle ps, int nb, const double* const* " % name in header
        assert len(_capi.SIGNATURES[name]) == 5
    lib = _capi.load()
    for name in ("create", "destroy", "info") + NAMES:
        assert getattr(lib, "mg_points_" + name) is not None


# ---- device ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _set_case(N, M=None):
    """The points (`special_points`, or the first M of them), LANES lanes of different random data per operand, and the host
    restatement of every lane and entry."""
    rng = np.random.default_rng(700 + N)
    pts = special_points(N, seed=N)
    if M is not None:
        pts = np.ascontiguousarray(pts[:M])
    M = pts.shape[0]
    n = (N + 1) ** 3
    ins = {"sample": rng.standard_normal((LANES, n)), "load": rng.standard_normal((LANES, M)), "gradient_t": rng.standard_normal((LANES, 3 * M))}
    ins["gradient"] = ins["sample"]
    host = {"sample": poisson.diffusion_point_sample, "load": poisson.diffusion_point_load,
            "gradient": lambda N, pts, x: poisson.diffusion_point_gradient(N, pts, x).reshape(-1),
            "gradient_t": lambda N, pts, p: poisson.diffusion_point_gradient_t(N, pts, p.reshape(-1, 3))}
    want = {k: np.stack([host[k](N, pts, ins[k][b]) for b in range(LANES)]) for k in NAMES}
    for a in (pts, *ins.values(), *want.values()):
        a.setflags(write=False)
    return pts, ins, want


def _check_set(h, level, N, label, M=None, nbs=(1, 3, 4, 5, 9)):
    """All four set entries for nb lanes (a full group of four, a tail of one, more than two groups), every lane against the
    host restatement and against the one-field entry on the same handle; two lanes sharing an input; each transpose twice."""
    pts, ins, want = _set_case(N, M)
    M = pts.shape[0]
    assert h.elements(level) == N
    single = {k: getattr(h, "diffusion_point_" + k) for k in NAMES}
    singles = {k: [single[k](level, M, pts, ins[k][b]) for b in range(max(nbs))] for k in NAMES}
    for k in NAMES:
        for b in range(max(nbs)):
            assert singles[k][b].tobytes() == want[k][b].tobytes(), (label, k, b, "the one-field entry")
    with h.points(level, pts) as ps:
        many = {k: getattr(ps, k + "_many") for k in NAMES}
        for k in NAMES:
            for nb in nbs:
                got = many[k]([ins[k][b] for b in range(nb)])
                assert got.shape == want[k][:nb].shape
                for b in range(nb):
                    bad = np.flatnonzero(got[b] != want[k][b])
                    assert got[b].tobytes() == want[k][b].tobytes(), (label, k, nb, b, bad[:5], bad.size)
                    assert got[b].tobytes() == singles[k][b].tobytes(), (label, k, nb, b, "differs from the one-field entry")
                if k in ("load", "gradient_t"):
                    again = many[k]([ins[k][b] for b in range(nb)])
                    assert again.tobytes() == got.tobytes(), (label, k, nb, "a second call gave other bytes")
            # two lanes share an input: lanes (0, 1, 0), the first array uploaded once and its pointer passed twice
            a0, a1 = ins[k][0], ins[k][1]
            got = many[k]([a0, a1, a0])
            for lane, b in enumerate((0, 1, 0)):
                assert got[lane].tobytes() == want[k][b].tobytes(), (label, k, "shared input", lane)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [8, 36, 72])
def test_set_entries_match_the_restatements_and_the_single_entries_to_the_bit(N):
    """The top level at N = 8, 36 and 72 as a grid-only, a stored and a matrix-free level (the construction of
    test_diffusion_points.py::test_kernels_match_the_host_restatements_to_the_bit), `special_points`, nb in {1, 3, 4, 5, 9}
    with different random data per lane."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.set_level_grid(1)
        _check_set(h, 1, N, "grid-only")
    for matrix_free in (False, True):
        with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
            h.gen_diffusion_level(1, lognormal_kappa(N, 3, seed=1), matrix_free=matrix_free)
            assert h.level_matrix_free(1) == matrix_free
            _check_set(h, 1, N, "matrix-free" if matrix_free else "stored")


@pytest.mark.gpu
def test_a_set_of_one_point():
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 8
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.set_level_grid(1)
        _check_set(h, 1, N, "M = 1", M=1)
        with h.points(1, _set_case(N, 1)[0]) as ps:
            info = ps.info
            assert info["M"] == 1 and info["runs"] == 4 and info["longest_run"] == 1


@pytest.mark.gpu
def test_sets_on_the_level_below_the_top():
    """A hierarchy with N = 36 on top, generated stored and matrix-free: sets on the level below it (N = 18) and on the top."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 36
    for min_rows in (None, 0):
        with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
            h.gen_diffusion_hierarchy(lognormal_kappa(N, 3, seed=1), matrix_free_min_rows=min_rows)
            _check_set(h, 0, N // 2, "generated, below the top", nbs=(1, 5))
            _check_set(h, 1, N, "generated, the top", nbs=(5,))


def _pcg_bytes(h, top, f):
    h.set_vector(top, "f", f)
    h.zero_vector(top, "v")
    hist = h.pcg(rtol=1e-10, max_iter=60, level=top)
    return hist.tobytes(), h.get_vector(top, "v").tobytes()


@pytest.mark.gpu
def test_info_memory_and_what_a_set_leaves_alone():
    """`runs` and `longest_run` are those of `diffusion_point_runs`; `mg_memory_bytes` rises by `bytes` on creation and comes
    back on destroy; two sets live side by side; creating, using and destroying a set moves neither `mg_counters` nor
    `mg_smoother_launches`, and the `mg_pcg` after it has the bytes of a handle that never made a set."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 16
    kappa = lognormal_kappa(N, 3, seed=2)
    f = np.random.default_rng(21).standard_normal((N + 1) ** 3)
    pts_a, pts_b = special_points(N, seed=5), _crowd(N=N, M=300)
    x = np.random.default_rng(22).standard_normal((3, (N + 1) ** 3))
    with DeviceHierarchy(3, 0, 1, c=N // 2) as plain:
        plain.gen_diffusion_hierarchy(kappa)
        want = _pcg_bytes(plain, 1, f)
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.gen_diffusion_hierarchy(kappa)
        before = h.memory_bytes()
        counters = h.counters()
        launches = [h.smoother_launches(l) for l in (0, 1)]
        a = h.points(1, pts_a)
        info = a.info
        order, start, run_node = poisson.diffusion_point_runs(N, pts_a)
        assert info["level"] == 1 and info["N"] == N and info["M"] == pts_a.shape[0]
        assert info["runs"] == run_node.size and info["longest_run"] == int(np.diff(start).max())
        assert info["bytes"] > 0 and h.memory_bytes() == before + info["bytes"]
        b = h.points(0, pts_b)
        info_b = b.info
        _, start_b, nodes_b = poisson.diffusion_point_runs(N // 2, pts_b)
        assert info_b["level"] == 0 and info_b["N"] == N // 2 and info_b["runs"] == nodes_b.size
        assert info_b["longest_run"] == int(np.diff(start_b).max())
        assert h.memory_bytes() == before + info["bytes"] + info_b["bytes"]
        got = a.sample_many(x)
        for lane in range(3):
            assert got[lane].tobytes() == poisson.diffusion_point_sample(N, pts_a, x[lane]).tobytes()
        w = np.random.default_rng(23).standard_normal((2, 300))
        got = b.load_many(w)
        for lane in range(2):
            assert got[lane].tobytes() == poisson.diffusion_point_load(N // 2, pts_b, w[lane]).tobytes()
        a.close()
        assert h.memory_bytes() == before + info_b["bytes"]
        assert b.gradient_many(x[:1, :(N // 2 + 1) ** 3].copy()).shape == (1, 3 * 300)     # the other set lives on
        b.close()
        b.close()                                       # a second close does nothing
        assert h.memory_bytes() == before
        assert h.counters() == counters
        assert [h.smoother_launches(l) for l in (0, 1)] == launches
        assert _pcg_bytes(h, 1, f) == want


def _device_array(h, n, host=None):
    from multigrid_dolfinx_amd.hierarchy import _DeviceArray
    return _DeviceArray(h._lib, h.device, n, host)


@pytest.mark.gpu
def test_refusals_name_their_cause_and_their_entry():
    from multigrid_dolfinx_amd import _capi
    from multigrid_dolfinx_amd._capi import MG_BATCH_MAX, MgError
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N, M = 12, 40
    n = (N + 1) ** 3
    rng = np.random.default_rng(8)
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        lib = h._lib
        h.gen_diffusion_level(1, np.ones(N ** 3), matrix_free=True)
        good = rng.random((M, 3))
        bad = good.copy()
        bad[31, 1], bad[17, 2], bad[23, 0] = 1.0 + 2.0 ** -52, np.nan, -0.25
        xs = rng.standard_normal((2, n))
        bufs = [_device_array(h, 3 * M, good.reshape(-1)), _device_array(h, 3 * M, bad.reshape(-1)), _device_array(h, n, xs[0]),
                _device_array(h, n, xs[1]), _device_array(h, n), _device_array(h, n)]
        try:
            pts, pts_bad, x0, x1, o0, o1 = (d.ptr.value for d in bufs)
            host = np.zeros(n).ctypes.data
            memory = h.memory_bytes()

            def create(handle, level, count, p, out=True):
                ps = C.c_void_p()
                _capi.check(lib.mg_points_create(handle, level, C.c_int64(count), C.c_void_p(p), C.byref(ps) if out else None))
                return ps

            # ---- creation: what the one-field entries refuse, under this entry's name
            for args, text in (((None, 1, M, pts), "null handle"), ((h._h, 5, M, pts), "level 5 out of range"),
                               ((h._h, 0, M, pts), "level 0 has not been set"), ((h._h, 1, 0, pts), "M = 0"),
                               ((h._h, 1, -3, pts), "M = -3"), ((h._h, 1, 2 ** 31 + 1, pts), "more than 2\\^31"),
                               ((h._h, 1, M, 0), "null pointer"), ((h._h, 1, M, host), "pts is not device memory")):
                with pytest.raises(MgError, match="mg_points_create: .*" + text):
                    create(*args)
            with pytest.raises(MgError, match="mg_points_create: null pointer"):
                create(h._h, 1, M, pts, out=False)
            # 1 + 2^-52 at point 31, a NaN at 17, -0.25 at 23: the lowest index is named and no set is made
            ps = C.c_void_p(1)
            assert lib.mg_points_create(h._h, 1, C.c_int64(M), C.c_void_p(pts_bad), C.byref(ps)) != 0
            assert "mg_points_create: a point must lie in the unit cube" in lib.mg_last_error().decode()
            assert ": point 17 is" in lib.mg_last_error().decode() and not ps.value
            with pytest.raises(MgError, match="mg_points_create: a point must lie in the unit cube.*: point 17 is"):
                h.points(1, bad)
            assert h.memory_bytes() == memory
            with DeviceHierarchy(2, 0, 1, c=16) as h2:
                h2.gen_poisson_level(1)
                with pytest.raises(MgError, match="mg_points_create: .*2-D"):
                    create(h2._h, 1, M, pts)
            with DeviceHierarchy(3, 0, 1, c=16) as hs:
                nothing = lambda *args: None
                hs.set_comm_callbacks(0, 2, nothing, nothing, nothing, replicate_below=0)
                with pytest.raises(MgError, match="mg_points_create needs a whole .*slab"):
                    create(hs._h, 1, M, pts)
            with DeviceHierarchy(3, 0, 0, c=16) as hf:
                hf.set_flat_level(poisson.lexicographic_level(4, 2).A)
                with pytest.raises(MgError, match="mg_points_create: .*flat"):
                    create(hf._h, 0, M, pts)

            # ---- the four batched entries
            want = poisson.diffusion_point_sample(N, good, xs[0])
            P = h.points(1, good)
            good_call = lambda: P.sample_many([xs[0]])[0].tobytes() == want.tobytes()
            assert good_call()
            ptrs = DeviceHierarchy._ptr_array
            for k in NAMES:
                name = "mg_points_" + k
                fn = getattr(lib, name)
                call = lambda nb, ins, outs, ps=None, handle=None: _capi.check(fn(handle or h._h, ps or P.handle, nb, ins, outs))
                # (in and out are n doubles each, at least as long as any operand of the four entries at M = 40)
                for nb in (0, MG_BATCH_MAX + 1):
                    with pytest.raises(MgError, match=name + ": nb = %d is outside 1..%d" % (nb, MG_BATCH_MAX)):
                        call(nb, ptrs([x0] * max(nb, 1)), ptrs([o0] * max(nb, 1)))
                for ins, outs in ((None, ptrs([o0])), (ptrs([x0]), None)):
                    with pytest.raises(MgError, match=name + ": null pointer array"):
                        call(1, ins, outs)
                for ins, outs in (([x0, 0], [o0, o1]), ([x0, x1], [o0, 0])):
                    with pytest.raises(MgError, match=name + r": null pointer \(.*\[1\]\)"):
                        call(2, ptrs(ins), ptrs(outs))
                for ins, outs in (([host, x1], [o0, o1]), ([x0, x1], [o0, host])):
                    with pytest.raises(MgError, match=name + r": .*\[[01]\] is not device memory"):
                        call(2, ptrs(ins), ptrs(outs))
                with pytest.raises(MgError, match=name + r": out\[0\] overlaps [xwp]\[1\]"):
                    call(2, ptrs([x0, o0 + 8]), ptrs([o0, o1]))
                with pytest.raises(MgError, match=name + r": out\[0\] overlaps out\[1\]"):
                    call(2, ptrs([x0, x1]), ptrs([o0, o0]))
                with pytest.raises(MgError, match=name + ": null point set"):
                    _capi.check(fn(h._h, None, 1, ptrs([x0]), ptrs([o0])))
                with pytest.raises(MgError, match=name + ": null handle"):
                    _capi.check(fn(None, P.handle, 1, ptrs([x0]), ptrs([o0])))
                assert good_call(), name

            # ---- a set on another handle; a set after its destruction
            with DeviceHierarchy(3, 0, 1, c=N // 2) as other:
                other.set_level_grid(1)
                for k in NAMES:
                    with pytest.raises(MgError, match="mg_points_%s: this is no live point set of this handle" % k):
                        _capi.check(getattr(lib, "mg_points_" + k)(other._h, P.handle, 1, ptrs([x0]), ptrs([o0])))
                with pytest.raises(MgError, match="mg_points_destroy: this is no live point set of this handle"):
                    _capi.check(lib.mg_points_destroy(other._h, P.handle))
                with pytest.raises(MgError, match="mg_points_info: this is no live point set of this handle"):
                    _capi.check(lib.mg_points_info(other._h, P.handle, None, None, None, None, None, None))
            assert good_call()
            dead = C.c_void_p(P.handle.value)
            P.close()
            for k in NAMES:
                with pytest.raises(MgError, match="mg_points_%s: this is no live point set of this handle" % k):
                    _capi.check(getattr(lib, "mg_points_" + k)(h._h, dead, 1, ptrs([x0]), ptrs([o0])))
            with pytest.raises(MgError, match="mg_points_destroy: this is no live point set of this handle"):
                _capi.check(lib.mg_points_destroy(h._h, dead))
            with pytest.raises(MgError, match="this point set has been closed"):
                P.sample_many([xs[0]])
            assert h.memory_bytes() == memory
            P = h.points(1, good)
            assert good_call()

            # ---- the level set again with another N: the set says where it was located
            with DeviceHierarchy(3, 0, 1, c=N // 2) as hg:
                hg.set_level_grid(1)
                Q = hg.points(1, good)
                assert Q.sample_many([xs[0]])[0].tobytes() == want.tobytes()
                hg.c = N                                # the same handle, its level 1 now with N = 24
                hg.set_level_grid(1)
                assert hg.elements(1) == 2 * N
                for k in NAMES:
                    with pytest.raises(MgError, match="mg_points_%s: level 1 has been set again with N = %d; this set was located on N = %d"
                                       % (k, 2 * N, N)):
                        _capi.check(getattr(lib, "mg_points_" + k)(hg._h, Q.handle, 1, ptrs([x0]), ptrs([o0])))
                Q.close()
                n2 = (2 * N + 1) ** 3
                x2 = rng.standard_normal(n2)
                with hg.points(1, good) as Q2:          # a new set on the new level works
                    assert Q2.sample_many([x2])[0].tobytes() == poisson.diffusion_point_sample(2 * N, good, x2).tobytes()
            assert good_call()
            P.close()
        finally:
            for d in bufs:
                d.free()


# ---- DiffusionSolver: in a process of its own that imports torch FIRST (see tests/test_diffusion_points.py) -------------------
def _torch_first(worker):
    code = "import torch, sys; sys.path.insert(0, %r); import tests.diffusion_point_sets_workers as w; w.%s()" % (ROOT, worker)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.gpu
def test_batched_point_functions_pass_gradcheck_and_gradgradcheck():
    """gradcheck and gradgradcheck at torch's default tolerances on `sample_many`, `point_load_many` and
    `sample_gradient_many`, in the fields and -- through a `LocatedPoints` made from a tensor that requires grad -- in the
    positions; `sample(u, P)` is `torch.equal` to `sample(u, X)` (`gradcheck_worker`)."""
    assert "gradcheck ok" in _torch_first("gradcheck_worker")


@pytest.mark.gpu
def test_a_survey_equals_the_loop_of_single_calls():
    """N = 8, three sources and 12 off-grid receivers: `solve_many` on `point_load_many` and `sample_many` of it against three
    `solve`, `point_load` and `sample` calls, dJ/dkappa against the loop's, the stale-set refusal and the solver's counters
    (`survey_worker`)."""
    assert "survey ok" in _torch_first("survey_worker")
