"""kappa handed over from device memory (mg_gen_diffusion_hierarchy_device, kappa_ingest of mg_diffusion_kappa.hip.h), diffusion
hierarchies refreshed in place (mg_refresh_diffusion_hierarchy), and torch_diffusion.DiffusionSolver on a device kappa.
Everything is compared as bytes with what the host hand-off and a fresh generation give."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.diffusion_workers import lognormal_kappa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _handle(dim, N, nlev, **tuning):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    top = nlev - 1
    assert N % (1 << top) == 0
    h = DeviceHierarchy(dim, 0, top, c=N >> top, **tuning)
    h.set_prolongation("p1")
    h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
    return h


def _device_array(h, host):
    """float64 on the handle's device without torch (which must not be imported after libmg_hip.so is loaded)."""
    from multigrid_dolfinx_amd.hierarchy import _DeviceArray
    host = np.ascontiguousarray(host, dtype=np.float64).reshape(-1)
    return _DeviceArray(h._lib, h.device, host.size, host)


def _rhs(h, top):
    """MG_VEC_F of every level as generated (a cycle overwrites the coarse ones with restricted residuals)."""
    return [h.get_vector(l, "f").tobytes() for l in range(top + 1)]


def _cycle(h, top, ncycles=1):
    """The iterate after V(2,2) cycles from zero on the top level's own right-hand side."""
    h.zero_vector(top, "v")
    h.vcycle(top, ncycles)
    return h.get_vector(top, "v").tobytes()


# ---- 1. device hand-off = host hand-off -------------------------------------------------------------------------------------
# 3-D 4 / 2 levels: a coarse level of 2^3 cells, less than a wave; 36 / 3: 36 -> 18 -> 9, an odd coarse N and partial waves;
# 130 / 2: 65 coarse cells per line; 2-D 24 / 3: the 2-D path.  3-D with all levels stored and with every level above level 0
# matrix-free (the top level then gets its copy from kappa_ingest), 2-D stored.
_SHAPES = [(3, 4, 2, None), (3, 4, 2, 0), (3, 36, 3, None), (3, 36, 3, 0), (3, 130, 2, None), (3, 130, 2, 0), (2, 24, 3, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("averaging", ["arithmetic", "harmonic"])
@pytest.mark.parametrize("dim,N,nlev,min_rows", _SHAPES)
def test_device_handoff_equals_host_handoff_to_the_bit(dim, N, nlev, min_rows, averaging):
    """A handle generated from a host kappa and one generated from the same kappa in device memory: level_info and
    level_matrix_free of every level, mg_memory_bytes, F of every level, the residual of one random V and the iterate after
    one V(2,2) cycle with P1 transfers, all as bytes.  Both handles coarsen with kappa_ingest, so this pins the two ways
    the walk over the levels owns its source (an upload it may give away, a borrowed buffer it copies) against each other;
    the coarsening itself is pinned against poisson.coarsen_kappa by
    tests/test_diffusion.py::test_device_hierarchy_entry_equals_per_level_calls_from_every_source.  The caller's buffer
    comes back unchanged and no whole-vector copy is counted across the call."""
    top = nlev - 1
    kappa = lognormal_kappa(N, dim, seed=11)
    V = np.random.default_rng(N).standard_normal((N + 1) ** dim)

    def snapshot(h):
        out = {"info": [(h.level_info(l), h.level_matrix_free(l), h.level_kappa_bytes(l)) for l in range(nlev)],
               "memory": h.memory_bytes(), "F": _rhs(h, top)}
        h.set_vector(top, "v", V)
        h.residual(top)
        out["residual"] = h.get_vector(top, "r").tobytes()
        out["cycle"] = _cycle(h, top)
        return out

    with _handle(dim, N, nlev) as host, _handle(dim, N, nlev) as dev:
        host.gen_diffusion_hierarchy(kappa, averaging, matrix_free_min_rows=min_rows)
        buf = _device_array(dev, kappa)
        try:
            before = dev.counters()
            dev.gen_diffusion_hierarchy(buf.ptr.value, averaging, matrix_free_min_rows=min_rows)
            assert dev.counters() == before
            assert buf.download().tobytes() == kappa.tobytes()
        finally:
            buf.free()          # (matrix-free levels keep their own copy: the caller's buffer may go)
        want, got = snapshot(host), snapshot(dev)
        assert [m for _, m, _ in got["info"]] == [False] + [min_rows is not None] * top
        for key in want:
            assert got[key] == want[key], key


# ---- 2. refresh = fresh generation ------------------------------------------------------------------------------------------
def _exercise(h, top, f):
    """The calls of the refresh test on a handle that has just got its kappa: F of every level; two Jacobi V-cycles (a graph
    is captured and replayed); the Chebyshev interval of every level above level 0 and one Chebyshev cycle; one mg_pcg."""
    out = {"F": _rhs(h, top)}
    h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
    out["jacobi"] = _cycle(h, top, 2)
    out["graphs"] = h.counters()["graphs_cached"]
    h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose", smoother="chebyshev")
    out["bounds"] = [h.chebyshev_bounds(l) for l in range(1, top + 1)]
    out["chebyshev"] = _cycle(h, top)
    h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
    h.zero_vector(top, "v")
    h.set_vector(top, "f", f)
    out["pcg"] = h.pcg(rtol=1e-8, max_iter=50, level=top).tobytes()
    out["x"] = h.get_vector(top, "v").tobytes()
    out["memory"] = h.memory_bytes()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("min_rows", [0, None])
def test_refresh_equals_fresh_generation(min_rows):
    """N = 36, three levels, matrix-free above level 0 and all stored.  Handle A: generated from kappa_1 on the device, cycled
    (`_exercise`: cached graph, Chebyshev intervals, mg_pcg work vectors), refreshed with kappa_2 (another seed), cycled again.
    Handle B: generated from kappa_2 (host hand-off), cycled once.  F of every level, the Chebyshev intervals, the Jacobi and
    the Chebyshev iterate, the mg_pcg history and iterate and mg_memory_bytes agree as bytes; then A is refreshed with kappa_1
    again and agrees with its own first results: nothing of kappa_2 lingers.

    mg_memory_bytes before and after the refresh is compared at the same point of the call sequence (after `_exercise`): the
    refresh has to drop level 0's factorisation and the stored levels' lazily built parts, which the next cycle builds again,
    so directly after the refresh the figure is lower by those (asserted: never higher) until their next use."""
    N, nlev, top = 36, 3, 2
    k1, k2 = lognormal_kappa(N, 3, seed=21), lognormal_kappa(N, 3, seed=22)
    f = np.random.default_rng(7).standard_normal((N + 1) ** 3)
    with _handle(3, N, nlev) as A, _handle(3, N, nlev) as B:
        buf = _device_array(A, k1)
        try:
            A.gen_diffusion_hierarchy(buf.ptr.value, matrix_free_min_rows=min_rows)
        finally:
            buf.free()
        split = [A.level_matrix_free(l) for l in range(nlev)]
        assert split == [False] + [min_rows is not None] * top
        first = _exercise(A, top, f)
        assert first["graphs"] > 0
        kappa_bytes = [A.level_kappa_bytes(l) for l in range(nlev)]
        buf = _device_array(A, k2)
        try:
            A.refresh_diffusion_hierarchy(buf.ptr.value)        # by address ...
            assert buf.download().tobytes() == k2.tobytes()
        finally:
            buf.free()
        assert A.counters()["graphs_cached"] == 0
        assert A.memory_bytes() <= first["memory"]
        assert [A.level_matrix_free(l) for l in range(nlev)] == split
        assert [A.level_kappa_bytes(l) for l in range(nlev)] == kappa_bytes
        second = _exercise(A, top, f)
        B.gen_diffusion_hierarchy(k2, matrix_free_min_rows=min_rows)
        fresh = _exercise(B, top, f)
        assert first["F"] != fresh["F"] and first["jacobi"] != fresh["jacobi"] and first["bounds"] != fresh["bounds"]
        for key in set(fresh) - {"graphs"}:
            assert second[key] == fresh[key], key
        assert second["memory"] == first["memory"]
        A.refresh_diffusion_hierarchy(k1)                       # ... and from a NumPy array
        again = _exercise(A, top, f)
        for key in set(first) - {"graphs"}:
            assert again[key] == first[key], key


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_name_their_cause_and_leave_the_handle_as_it_was():
    from multigrid_dolfinx_amd._capi import MgError, check
    N, nlev, top = 16, 2, 1
    kappa = lognormal_kappa(N, 3, seed=31)
    cell = (5 * N + 7) * N + 3
    with _handle(3, N, nlev) as h, _handle(3, N, nlev) as other:
        h.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=0)
        want = _cycle(h, top)
        memory = h.memory_bytes()
        good = _device_array(h, kappa)
        held = [good]
        try:
            p = good.ptr.value
            host = kappa.copy()
            calls = [("not device memory", lambda: h.gen_diffusion_hierarchy(host.ctypes.data, matrix_free_min_rows=0)),
                     ("not device memory", lambda: h.refresh_diffusion_hierarchy(host.ctypes.data)),
                     ("null pointer", lambda: h.gen_diffusion_hierarchy(0, matrix_free_min_rows=0)),
                     ("null pointer", lambda: h.refresh_diffusion_hierarchy(0))]
            for text, call in calls:
                with pytest.raises(MgError, match=text):
                    call()
                assert _cycle(h, top) == want, text
            for bad in (-1.0, np.nan):
                k = kappa.copy()
                k[cell] = bad
                with pytest.raises(MgError, match=rf"cell \(3, 7, 5\) = index {cell} ") as by_host:
                    other.gen_diffusion_hierarchy(k)
                d = _device_array(h, k)
                held.append(d)
                for call in (lambda: h.gen_diffusion_hierarchy(d.ptr.value, matrix_free_min_rows=0),
                             lambda: h.gen_diffusion_hierarchy(d.ptr.value), lambda: h.refresh_diffusion_hierarchy(d.ptr.value)):
                    with pytest.raises(MgError) as by_device:
                        call()
                    assert str(by_device.value) == str(by_host.value)
                    assert _cycle(h, top) == want, bad
                assert d.download().tobytes() == k.tobytes()
            for text, call in (("averaging", lambda: h._lib.mg_refresh_diffusion_hierarchy(h._h, top, good.ptr, 7)),
                               ("averaging", lambda: h._lib.mg_gen_diffusion_hierarchy_device(h._h, top, N, good.ptr, 7, -1)),
                               ("N0 \\* 2\\^1", lambda: h._lib.mg_gen_diffusion_hierarchy_device(h._h, top, N + 1, good.ptr, 0, -1))):
                with pytest.raises(MgError, match=text):
                    check(call())
                assert _cycle(h, top) == want, text
            assert h.memory_bytes() == memory
            # levels that no diffusion hierarchy call generated
            with _handle(3, N, nlev) as hp:
                for l in range(nlev):
                    hp.gen_poisson_level(l)
                was = _cycle(hp, top)
                with pytest.raises(MgError, match="level 1 was not generated by a diffusion hierarchy call"):
                    hp.refresh_diffusion_hierarchy(p)
                assert _cycle(hp, top) == was
            with _handle(3, N, nlev) as hs:
                hs.gen_diffusion_hierarchy(kappa)
                hs.gen_diffusion_level(top, kappa)          # the top level once more, singly
                was = _cycle(hs, top)
                with pytest.raises(MgError, match="level 1 was not generated by a diffusion hierarchy call"):
                    hs.refresh_diffusion_hierarchy(p)
                assert _cycle(hs, top) == was
            with _handle(3, N, nlev) as hn:
                with pytest.raises(MgError, match="level 1 has not been set"):
                    hn.refresh_diffusion_hierarchy(p)
            with _handle(3, N, nlev) as slab:
                nothing = lambda *a: None
                slab.set_comm_callbacks(0, 2, nothing, nothing, nothing, replicate_below=0)
                for call in (lambda: slab.gen_diffusion_hierarchy(p), lambda: slab.gen_diffusion_hierarchy(p, matrix_free_min_rows=0),
                             lambda: slab.refresh_diffusion_hierarchy(p)):
                    with pytest.raises(MgError, match="slab"):
                        call()
            with _handle(2, N, nlev) as two_d:
                k2d = _device_array(two_d, lognormal_kappa(N, 2, seed=32))
                held.append(k2d)
                two_d.gen_diffusion_hierarchy(k2d.ptr.value)
                was = _cycle(two_d, top)
                with pytest.raises(MgError, match="2-D"):
                    two_d.gen_diffusion_hierarchy(k2d.ptr.value, matrix_free_min_rows=0)
                assert _cycle(two_d, top) == was
                two_d.refresh_diffusion_hierarchy(k2d.ptr.value)     # (2-D hierarchies are stored, and refresh like any)
                assert _cycle(two_d, top) == was
            # after all of it the first handle still takes a good kappa
            h.refresh_diffusion_hierarchy(p)
            assert _cycle(h, top) == want
        finally:
            for d in held:
                d.free()


# ---- 4. timing name ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_timing_name_runs_the_kernel_and_leaves_the_level_alone():
    from multigrid_dolfinx_amd._capi import MgError
    N, nlev, top = 36, 3, 2
    with _handle(3, N, nlev) as h:
        h.gen_diffusion_hierarchy(lognormal_kappa(N, 3, seed=41), matrix_free_min_rows=(N // 2 + 1) ** 3 + 1)
        assert [h.level_matrix_free(l) for l in range(nlev)] == [False, False, True]
        want, memory = _cycle(h, top), h.memory_bytes()
        assert h.time_kernel("kappa_ingest", top, reps=2) > 0.0
        assert _cycle(h, top) == want and h.memory_bytes() == memory
        with pytest.raises(MgError, match="not a matrix-free diffusion level"):
            h.time_kernel("kappa_ingest", 1, reps=2)
        assert _cycle(h, top) == want


# ---- 5. DiffusionSolver on a device kappa: in a process of its own that imports torch FIRST (tests/test_diffusion_adjoint.py) ---
def _torch_first(worker):
    code = "import torch, sys; sys.path.insert(0, %r); import tests.diffusion_device_kappa_workers as w; w.%s()" % (ROOT, worker)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.gpu
def test_solver_generates_from_the_device_then_refreshes():
    """N = 16, two levels, kappa on the device: "device", then "refresh"; both solves' gradients against the host adjoint
    within GRADIENT_LIMIT of tests/diffusion_adjoint_workers.py; the refreshed solve's u has the bytes of a fresh solver's
    (`device_kappa_worker`)."""
    assert "device kappa ok" in _torch_first("device_kappa_worker")


@pytest.mark.gpu
def test_backward_after_a_later_forward_is_the_gradient_of_its_own_kappa():
    """(`stale_backward_worker`)"""
    assert "stale backward ok" in _torch_first("stale_backward_worker")


@pytest.mark.gpu
def test_a_cpu_kappa_still_takes_the_host_path():
    """(`cpu_kappa_worker`)"""
    assert "cpu kappa ok" in _torch_first("cpu_kappa_worker")


@pytest.mark.gpu
def test_warm_start_needs_no_more_iterations():
    """N = 32, three levels, kappa_2 = kappa_1 (1 + 0.01 eta): the warm forward solve of kappa_2 takes no more iterations than
    the cold one and both meet rtol (`warm_start_worker`, which prints both counts)."""
    assert "warm start ok" in _torch_first("warm_start_worker")
