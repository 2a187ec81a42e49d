"""Variable-coefficient diffusion levels, -div(kappa grad u) with one kappa per cell, generated on the device
(mg_gen_diffusion_level / mg_gen_diffusion_hierarchy) and restated on the host (poisson.diffusion_level / coarsen_kappa).

On the Kuhn mesh the rows keep the Poisson level's five- / seven-point shape: kappa == 1 must give the generated Poisson
level bit for bit, any kappa the host restatement's bits, and the 1:1000 jump the independent assembly of
tests/cheb_reference.py."""
import numpy as np
import pytest
import scipy.sparse as sp

from multigrid_dolfinx_amd import poisson
from tests import cheb_reference as ref
from tests.diffusion_workers import jump_kappa, kappa_levels, lognormal_kappa


def _same_csr(A, B):
    return (np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and A.data.tobytes() == B.data.tobytes())


# ---- host restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N", [(2, 16), (2, 33), (3, 8), (3, 12)])
@pytest.mark.parametrize("keep_zeros", [True, False])
def test_unit_kappa_is_the_poisson_level(dim, N, keep_zeros):
    want = poisson.lexicographic_level(N, dim, keep_zeros=keep_zeros)
    got = poisson.diffusion_level(N, dim, np.ones(N ** dim), keep_zeros=keep_zeros)
    assert _same_csr(got.A, want.A)
    assert got.b.tobytes() == want.b.tobytes()


@pytest.mark.parametrize("dim,N", [(2, 32), (3, 8), (3, 16)])
def test_jump_agrees_with_independent_assembly(dim, N):
    got = poisson.diffusion_level(N, dim, jump_kappa(N, dim), keep_zeros=False).A
    want = ref.kuhn_diffusion(N, dim)
    assert abs(got - want).max() <= 1e-14 * abs(want).max()
    assert got.nnz == want.nnz


@pytest.mark.parametrize("dim,N", [(2, 32), (3, 12)])
def test_lognormal_rows_are_symmetric_axis_stencils(dim, N):
    A = poisson.diffusion_level(N, dim, lognormal_kappa(N, dim, seed=1), keep_zeros=False).A
    assert _same_csr(A, A.T.tocsr().sorted_indices())
    assert np.diff(A.indptr).max() == (5 if dim == 2 else 7)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("averaging", ["arithmetic", "harmonic"])
def test_coarsen_kappa_on_constant_and_planar_fields(dim, averaging):
    N = 16
    for value in (1.0, 3.0):
        got = poisson.coarsen_kappa(np.full(N ** dim, value), dim, averaging)
        assert np.array_equal(got, np.full((N // 2) ** dim, value))
    jump = jump_kappa(N, dim, jump=1024.0)
    assert np.array_equal(poisson.coarsen_kappa(jump, dim, averaging), jump_kappa(N // 2, dim, jump=1024.0))
    got = poisson.coarsen_kappa(jump_kappa(N, dim), dim, averaging)
    want = jump_kappa(N // 2, dim)
    if averaging == "arithmetic":
        assert np.array_equal(got, want)
    else:
        assert np.max(np.abs(got - want) / want) <= 4e-16


def test_coarsen_kappa_order_is_pinned():
    k = lognormal_kappa(8, 3, seed=2).reshape(8, 8, 8)
    kids = [k[c::2, b::2, a::2] for c in (0, 1) for b in (0, 1) for a in (0, 1)]
    s = kids[0]
    for x in kids[1:]:
        s = s + x
    assert poisson.coarsen_kappa(k, 3).tobytes() == (s * 0.125).reshape(-1).tobytes()


def test_bad_kappa_is_refused_on_the_host():
    for bad in (0.0, -1.0, np.nan, np.inf):
        k = np.ones(64)
        k[5] = bad
        with pytest.raises(ValueError):
            poisson.diffusion_level(8, 2, k)


# ---- device ----------------------------------------------------------------------------------------------------------
_INFO = ("n_global", "nnz_stored", "nnz_nonzero", "ell_width", "offset_codes", "symmetric_diagonals", "row_classes")


def _storage(h, l):
    """level_storage, with distinct_rows above 255 reported as 256: past that the row dictionary's count is wherever its
    concurrent inserts stopped, not a property of the matrix."""
    out = h.level_storage(l)
    out["distinct_rows"] = min(out["distinct_rows"], 256)
    return out


def _outputs(h, l, v, f, sweeps=3):
    """F as generated, then residual and smoother output for (v, f)."""
    out = [h.get_vector(l, "f")]
    h.set_vector(l, "v", v)
    h.set_vector(l, "f", f)
    h.residual(l)
    out.append(h.get_vector(l, "r"))
    h.smooth(l, sweeps)
    out.append(h.get_vector(l, "v"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dim,N", [(2, 64), (2, 2048), (3, 32), (3, 256)])
@pytest.mark.parametrize("prune", [True, False])
def test_device_unit_kappa_is_the_generated_poisson_level(dim, N, prune):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    with DeviceHierarchy(dim, 0, 1, c=N // 2) as d, DeviceHierarchy(dim, 0, 1, c=N // 2) as p:
        d.set_params(2, 2, 2.0 / 3.0)
        p.set_params(2, 2, 2.0 / 3.0)
        d.gen_diffusion_level(1, np.ones(N ** dim), prune_zeros=prune)
        p.gen_poisson_level(1, prune_zeros=prune)
        assert d.level_info(1) == p.level_info(1)
        assert _storage(d, 1) == _storage(p, 1)
        rng = np.random.default_rng(3)
        v, f = rng.standard_normal(d.n_dofs(1)), rng.standard_normal(d.n_dofs(1))
        for a, b in zip(_outputs(d, 1, v, f), _outputs(p, 1, v, f)):
            assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("dim,c,nlev", [(2, 8, 4), (2, 8, 8), (3, 4, 4), (3, 4, 6)])     # 65^2, 1025^2, 33^3, 129^3
@pytest.mark.parametrize("field", ["lognormal", "jump"])
def test_device_level_equals_host_restatement(dim, c, nlev, field):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    top = nlev - 1
    N = c << top
    kappa = lognormal_kappa(N, dim, seed=7) if field == "lognormal" else jump_kappa(N, dim)
    ks = kappa_levels(kappa, dim, nlev)
    host = [poisson.diffusion_level(c << l, dim, ks[l]) for l in range(nlev)]
    with DeviceHierarchy(dim, 0, top, c=c) as d, DeviceHierarchy(dim, 0, top, c=c) as s:
        for l in range(nlev):
            d.gen_diffusion_level(l, ks[l])
            s.set_level(l, host[l].A, prune_zeros=True)
        for h in (d, s):
            h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
            h.set_prolongation("p1")
        assert {k: d.level_info(top)[k] for k in _INFO} == {k: s.level_info(top)[k] for k in _INFO}
        sd = _storage(d, top)
        assert sd == _storage(s, top)
        assert sd["symmetric"] == 1 and sd["max_pair_ulps"] == 0
        assert d.get_vector(top, "f").tobytes() == host[top].b.tobytes()
        rng = np.random.default_rng(11)
        v = rng.standard_normal(d.n_dofs(top))
        f = host[top].b.reshape(-1)
        a, b = _outputs(d, top, v, f), _outputs(s, top, v, f)
        for x, y in zip(a[1:], b[1:]):
            assert x.tobytes() == y.tobytes()
        r = f - host[top].A @ v
        assert np.linalg.norm(a[1].reshape(-1) - r) <= 1e-14 * np.linalg.norm(r)
        cyc = []
        for h in (d, s):
            h.zero_vector(top, "v")
            h.set_vector(top, "f", f)
            h.vcycle(top, 2)
            cyc.append(h.get_vector(top, "v"))
        assert cyc[0].tobytes() == cyc[1].tobytes()


@pytest.mark.gpu
def test_device_jump_hierarchy_runs_the_poisson_paths_at_257():
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    lo, hi, c = 0, 5, 8
    with DeviceHierarchy.synthetic_diffusion(3, lo, hi, jump_kappa(c << hi, 3), c=c, mu1=50, mu2=50) as d, \
            DeviceHierarchy.synthetic(3, lo, hi, c=c, mu1=50, mu2=50) as p:
        p.set_params(50, 50, 2.0 / 3.0, restriction="p1_transpose")
        p.set_prolongation("p1")
        for l in range(lo, hi + 1):
            if p.level_info(l)["row_classes"] > 0:
                assert d.level_info(l)["row_classes"] > 0, l
            assert d.level_storage(l)["escape_rows"] == 0, l
        launches = []
        for h in (d, p):
            h.zero_vector(hi, "v")
            h.set_vector(hi, "f", np.ones(h.n_dofs(hi)))
            h.prepare_cycle(hi)
            h.reset_smoother_launches()
            h.vcycle(hi, 1)
            launches.append({l: h.smoother_launches(l) for l in range(lo + 1, hi + 1)})
        assert launches[0] == launches[1]
        assert "ksweep" in launches[0][hi], launches[0][hi]


@pytest.mark.gpu
@pytest.mark.parametrize("dim,c,nlev", [(2, 8, 5), (3, 4, 4)])
@pytest.mark.parametrize("averaging", ["arithmetic", "harmonic"])
def test_device_hierarchy_entry_equals_per_level_calls(dim, c, nlev, averaging):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    top = nlev - 1
    kappa = lognormal_kappa(c << top, dim, seed=3)
    ks = kappa_levels(kappa, dim, nlev, averaging)
    with DeviceHierarchy(dim, 0, top, c=c) as e, DeviceHierarchy(dim, 0, top, c=c) as p:
        e.gen_diffusion_hierarchy(kappa, averaging)
        for l in range(nlev):
            p.gen_diffusion_level(l, ks[l])
        rng = np.random.default_rng(2)
        for l in range(nlev):
            assert e.level_info(l) == p.level_info(l), l
            assert _storage(e, l) == _storage(p, l), l
            assert e.get_vector(l, "f").tobytes() == p.get_vector(l, "f").tobytes(), l
            v = rng.standard_normal(e.n_dofs(l))
            r = []
            for h in (e, p):
                h.set_vector(l, "v", v)
                h.residual(l)
                r.append(h.get_vector(l, "r"))
            assert r[0].tobytes() == r[1].tobytes(), l


def _level_snapshots(h, nlev):
    """What the hierarchy entries and the per-level calls must agree on, per level: level_info, the stored / matrix-free
    split, level_storage of a stored level (a matrix-free level has no stored rows to report on), F and the residual of a
    seeded random vector as bytes."""
    out = []
    for l in range(nlev):
        mf = h.level_matrix_free(l)
        h.set_vector(l, "v", np.random.default_rng(20 + l).standard_normal(h.n_dofs(l)))
        f = h.get_vector(l, "f").tobytes()
        h.residual(l)
        out.append({"info": h.level_info(l), "matrix_free": mf, "kappa_bytes": h.level_kappa_bytes(l),
                    "storage": None if mf else _storage(h, l), "f": f, "residual": h.get_vector(l, "r").tobytes()})
    return out


@pytest.fixture(scope="module")
def per_level_reference():
    """Per-level mg_gen_diffusion_level[_mf] calls fed by NumPy's poisson.coarsen_kappa, as `_level_snapshots`: computed once
    per (dim, N, nlev, matrix_free, averaging) and shared by the three sources."""
    made = {}

    def reference(dim, N, nlev, matrix_free, averaging):
        key = (dim, N, nlev, matrix_free, averaging)
        if key not in made:
            from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
            ks = kappa_levels(lognormal_kappa(N, dim, seed=3), dim, nlev, averaging)
            with DeviceHierarchy(dim, 0, nlev - 1, c=N >> (nlev - 1)) as p:
                for l in range(nlev):
                    p.gen_diffusion_level(l, ks[l], matrix_free=matrix_free and l > 0)
                made[key] = _level_snapshots(p, nlev)
        return made[key]
    return reference


# 3-D 4 / 2 levels: a coarse field of 2^3 cells, less than a wave; 36 / 3: 36 -> 18 -> 9, an odd coarse N and partial waves;
# 2-D 24 / 3: the 2-D path.  3-D with all levels stored and with every level above level 0 matrix-free, 2-D stored.
@pytest.mark.gpu
@pytest.mark.parametrize("source", ["host", "device", "device_unaligned"])
@pytest.mark.parametrize("averaging", ["arithmetic", "harmonic"])
@pytest.mark.parametrize("dim,N,nlev,matrix_free", [(3, 4, 2, False), (3, 4, 2, True), (3, 36, 3, False), (3, 36, 3, True),
                                                    (2, 24, 3, False)])
def test_device_hierarchy_entry_equals_per_level_calls_from_every_source(per_level_reference, dim, N, nlev, matrix_free,
                                                                        averaging, source):
    """The device's coarsening (kappa_ingest) against NumPy's, whoever owns the top level's kappa: a host array (uploaded;
    a matrix-free top level takes the upload over), a device address (borrowed; a matrix-free top level gets its copy from
    the coarsening pass) and a device address 8 bytes into a buffer one double longer, which is not 16-byte aligned and
    takes the kernel's path of 8-byte accesses.  Every level agrees with the per-level calls (`_level_snapshots`), and a
    borrowed buffer comes back unchanged."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy, _DeviceArray
    kappa = lognormal_kappa(N, dim, seed=3)
    min_rows = 0 if matrix_free else None
    with DeviceHierarchy(dim, 0, nlev - 1, c=N >> (nlev - 1)) as e:
        if source == "host":
            e.gen_diffusion_hierarchy(kappa, averaging, matrix_free_min_rows=min_rows)
        else:
            shift = 1 if source == "device_unaligned" else 0
            padded = np.concatenate([np.full(shift, -1.0), kappa])
            buf = _DeviceArray(e._lib, e.device, padded.size, padded)
            try:
                address = buf.ptr.value + 8 * shift
                assert address % 16 == 8 * shift
                e.gen_diffusion_hierarchy(address, averaging, matrix_free_min_rows=min_rows)
                assert buf.download().tobytes() == padded.tobytes()
            finally:
                buf.free()
        got, want = _level_snapshots(e, nlev), per_level_reference(dim, N, nlev, matrix_free, averaging)
        assert [s["matrix_free"] for s in got] == [False] + [matrix_free] * (nlev - 1)
        for l in range(nlev):
            for key in want[l]:
                assert got[l][key] == want[l][key], (l, key)


@pytest.mark.gpu
def test_device_chebyshev_estimates_on_the_3d_jump_hierarchy():
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    dim, c, nlev = 3, 4, 4
    kappa = jump_kappa(c << (nlev - 1), dim)
    ks = kappa_levels(kappa, dim, nlev)
    with DeviceHierarchy.synthetic_diffusion(dim, 0, nlev - 1, kappa, c=c, smoother="chebyshev") as h:
        for l in range(1, nlev):
            b = h.chebyshev_bounds(l)
            want = ref.lanczos_lmax(poisson.diffusion_level(c << l, dim, ks[l], keep_zeros=False).A, 10)
            assert abs(b["lmax_estimate"] - want) <= 1e-10 * want, (l, b, want)


def _histories(dim, c, nlev, kappa, smoother, f):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    with DeviceHierarchy.synthetic_diffusion(dim, 0, nlev - 1, kappa, c=c, smoother=smoother) as h:
        top = nlev - 1
        h.zero_vector(top, "v")
        h.set_vector(top, "f", f)
        hv = h.vcycle(top, 12, residuals=True)
        h.zero_vector(top, "v")
        hp = h.pcg(rtol=1e-10, max_iter=80)
    return hv, hp


def _close(got, want):
    keep = want >= 1e-4 * want[0]
    assert np.all(np.abs(got[keep] - want[keep]) <= 1e-10 * want[keep]), (got, want)
    assert np.all(np.abs(got - want) <= 1e-12 * want[0]), (got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,c,nlev", [(2, 4, 5), (3, 4, 4)])                # 65^2 and 33^3
@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
def test_device_cycle_and_pcg_match_numpy_on_the_jump(dim, c, nlev, smoother):
    kappa = jump_kappa(c << (nlev - 1), dim)
    ks = kappa_levels(kappa, dim, nlev)
    As = [poisson.diffusion_level(c << l, dim, ks[l], keep_zeros=False).A for l in range(nlev)]
    f = np.random.default_rng(4).standard_normal(As[-1].shape[0])
    hv, hp = _histories(dim, c, nlev, kappa, smoother, f)
    cyc = ref.Cycle(As, dim, c, smoother=smoother)
    want_v, want_p = cyc.history(f, 12), cyc.pcg(f, 1e-10, 80)
    _close(hv, want_v)
    assert len(hp) == len(want_p)
    _close(hp, want_p)


@pytest.mark.gpu
def test_device_pcg_on_a_lognormal_field_at_129():
    dim, c = 3, 4
    small = lognormal_kappa(c << 3, dim, seed=8)
    ks = kappa_levels(small, dim, 4)
    As = [poisson.diffusion_level(c << l, dim, ks[l], keep_zeros=False).A for l in range(4)]
    f = np.random.default_rng(4).standard_normal(As[-1].shape[0])
    bound = 2 * len(ref.Cycle(As, dim, c, smoother="jacobi").pcg(f, 1e-10, 200))
    kappa = lognormal_kappa(c << 5, dim, seed=8)
    f = np.random.default_rng(4).standard_normal(((c << 5) + 1) ** dim)
    _, hp = _histories(dim, c, 6, kappa, "jacobi", f)
    assert hp[-1] <= 1e-10 * np.linalg.norm(f) and len(hp) <= bound, (len(hp), bound, hp[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("world,dim,c", [(2, 3, 4), (3, 2, 8)])
def test_device_slabs_bit_identical_to_single_handle(world, dim, c):
    import torch.multiprocessing as mp
    from tests.dist_helpers import free_port
    from tests.diffusion_workers import gpu_diffusion_slab_worker
    mp.spawn(gpu_diffusion_slab_worker, args=(world, free_port(), dim, 1, 3, c, 2), nprocs=world, join=True)


@pytest.mark.gpu
def test_device_refusals_leave_the_handle_usable():
    from multigrid_dolfinx_amd._capi import MgError, load
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    dim, c = 3, 4
    kappa = jump_kappa(c << 2, dim)
    with DeviceHierarchy.synthetic_diffusion(dim, 0, 2, kappa, c=c) as h:
        f = np.random.default_rng(1).standard_normal(h.n_dofs(2))
        h.zero_vector(2, "v")
        h.set_vector(2, "f", f)
        want = h.vcycle(2, 2, residuals=True)
        mem = h.memory_bytes()
        bad = kappa.copy()
        bad[(3 * 16 + 2) * 16 + 1] = -2.0
        bad[-1] = np.nan
        with pytest.raises(MgError, match=r"cell \(1, 2, 3\)"):
            h.gen_diffusion_level(2, bad)
        with pytest.raises(MgError, match=r"cell \(1, 2, 3\)"):
            h.gen_diffusion_hierarchy(bad)
        lib = load()
        with pytest.raises(MgError, match="null kappa"):
            from multigrid_dolfinx_amd._capi import check
            check(lib.mg_gen_diffusion_level(h._h, 2, 16, None, 1))
        with pytest.raises(MgError):
            check(lib.mg_gen_diffusion_level(h._h, 2, 17, kappa.ctypes.data, 1))            # not N0 * 2^level
        with pytest.raises(MgError, match="even"):
            check(lib.mg_gen_diffusion_hierarchy(h._h, 2, 18, kappa.ctypes.data, 0))        # N1 = 9 is odd
        assert h.memory_bytes() == mem
        h.zero_vector(2, "v")
        h.set_vector(2, "f", f)
        assert h.vcycle(2, 2, residuals=True).tobytes() == want.tobytes()


@pytest.mark.gpu
def test_device_memory_equals_the_poisson_level():
    """kappa is freed on return: a unit-kappa level holds exactly the generated Poisson level's device memory."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    with DeviceHierarchy(3, 0, 1, c=32) as d, DeviceHierarchy(3, 0, 1, c=32) as p:
        d.gen_diffusion_level(1, np.ones(64 ** 3))
        p.gen_poisson_level(1)
        assert d.memory_bytes() == p.memory_bytes() > 0
