"""P1 natural-embedding transfers (mg_set_prolongation_p1, MG_RESTRICT_P1_TRANSPOSE) and Galerkin coarse levels
(mg_galerkin_level / mg_galerkin_hierarchy).  No reference counterpart: the reference injects and interpolates bilinearly.

CPU: the binding, the tables against an explicit SciPy P, the contraction of the NumPy cycle, P^T A P against the
rediscretised levels.  GPU: the kernels against the table path and the NumPy reference, slabs, Galerkin levels, convergence.
"""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from multigrid_dolfinx_amd import _capi, poisson
from tests import p1_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_binding_and_library():
    text = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    assert re.search(r"MG_RESTRICT_P1_TRANSPOSE\s*=\s*3", text)
    for name in ("mg_set_prolongation_p1", "mg_galerkin_level", "mg_galerkin_hierarchy"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _capi.SIGNATURES, name
        assert getattr(_capi.load(), name) is not None
    assert _capi.MG_RESTRICT_P1_TRANSPOSE == 3
    from multigrid_dolfinx_amd import hierarchy, multigrid
    assert hierarchy._RESTRICT["p1_transpose"] == 3
    assert "prolongation" in multigrid._options


def _oracle_pair(dim, c, seed):
    bag = poisson.make_hierarchy(dim, 0, 1, c=c, seed=seed)
    gi = {l: L.grid_index for l, L in bag.levels.items()}
    return bag, gi, ref.p1_oracle(bag, gi, dim)


@pytest.mark.parametrize("dim,c", [(2, 8), (3, 4)])
@pytest.mark.parametrize("seed", [None, 3])
def test_tables_equal_explicit_scipy_p(dim, c, seed):
    bag, gi, orc = _oracle_pair(dim, c, seed)
    rng = np.random.default_rng(11)
    nc, nf = (c + 1) ** dim, (2 * c + 1) ** dim
    vc = rng.standard_normal((nc, 1))
    rf = rng.standard_normal((nf, 1))
    P = ref.prolongation(c, dim)
    R = ref.restriction(c, dim)
    # explicit operators act in grid numbering; the caller's numbering is permuted at the edges, as the library does
    node_c, node_f = gi[0], gi[1]
    want_p = np.empty((nf, 1))
    want_p[:, 0] = (P @ vc[np.argsort(node_c), 0])[node_f]
    want_r = np.empty((nc, 1))
    want_r[:, 0] = (R @ rf[np.argsort(node_f), 0])[node_c]
    got_p = orc.interpolate_table(vc, 0, orc.prolongation_table)
    got_r = orc.restrict_table(rf, 1, orc.restriction_table)
    assert np.array_equal(got_p, want_p)
    assert np.array_equal(got_r, want_r)
    # R is the transpose of P on the interior block
    fi, ci = ref.interior(2 * c, dim), ref.interior(c, dim)
    assert (abs(sp.csr_matrix(R[ci][:, fi]) - sp.csr_matrix(P[fi][:, ci]).T)).max() == 0


@pytest.mark.parametrize("dim,lo,hi,c,bound", [(2, 0, 4, 8, 0.25), (3, 0, 3, 4, 0.40)])
def test_numpy_cycle_contraction(dim, lo, hi, c, bound):
    """V(2,2), Jacobi 2/3, from zero: P1 + P^T contracts at least bound per cycle; the reference transfers do not."""
    bag = poisson.make_hierarchy(dim, lo, hi, c=c, mu1=2, mu2=2)
    gi = {l: L.grid_index for l, L in bag.levels.items()}
    orc = ref.p1_oracle(bag, gi, dim)
    rho_p1 = ref.contraction(ref.residual_history(orc, hi, 12, "table"))
    assert rho_p1 <= bound, rho_p1
    from oracle.mg_oracle import Oracle
    plain = Oracle(poisson.make_hierarchy(dim, lo, hi, c=c, mu1=2, mu2=2), gi, dim=dim)
    for restriction in ("direct", "full_weighting"):
        rho = ref.contraction(ref.residual_history(plain, hi, 12, restriction))
        assert rho >= 0.85, (restriction, rho)


@pytest.mark.parametrize("dim,N", [(2, 32), (3, 16)])
def test_galerkin_equals_rediscretised_level(dim, N):
    A = poisson.make_level(N, dim).A
    G = ref.galerkin(A, N, dim)
    Ac = poisson.make_level(N // 2, dim).A.copy()
    Ac.eliminate_zeros()
    Ac.sort_indices()
    assert np.array_equal(G.indptr, Ac.indptr)
    assert np.array_equal(G.indices, Ac.indices)
    assert np.array_equal(G.data, Ac.data)


# ---- GPU -------------------------------------------------------------------------------------------------------------
def _grid_hierarchy(dim, c, lo=0, hi=1, **tuning):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    return DeviceHierarchy.synthetic(dim, lo, hi, c=c, mu1=2, mu2=2, **tuning)


def _set_tables(h, dim):
    cnt, off, w = (np.ascontiguousarray(x) for x in poisson.p1_prolongation_table(dim))
    _capi.check(h._lib.mg_set_prolongation_table(h._h, _capi.ptr(cnt.astype(np.int32)), _capi.ptr(off.astype(np.int32)),
                                                 _capi.ptr(w)))
    rc, ro, rw = poisson.p1_restriction_table(dim)
    rc, ro, rw = rc.astype(np.int32), np.ascontiguousarray(ro, dtype=np.int32), np.ascontiguousarray(rw)
    _capi.check(h._lib.mg_set_restriction_table(h._h, int(ro.shape[1]), _capi.ptr(rc), _capi.ptr(ro), _capi.ptr(rw)))


@pytest.mark.gpu
@pytest.mark.parametrize("dim,c", [(2, 8), (2, 64), (3, 4), (3, 64), (3, 128)])
def test_kernels_bit_identical_to_table_path_and_numpy(dim, c):
    """Up to 257^3: the new kernels, the table path fed p1_*_table and the explicit SciPy P / P^T agree bit for bit;
    add = 0 writes ERR only, add = 1 writes ERR and V += ERR."""
    rng = np.random.default_rng(c + dim)
    nc, nf = (c + 1) ** dim, (2 * c + 1) ** dim
    vc, v0, rf = rng.standard_normal(nc), rng.standard_normal(nf), rng.standard_normal(nf)
    want_p = ref.prolongation(c, dim) @ vc
    want_r = ref.restriction(c, dim) @ rf
    out = {}
    for path in ("kernel", "table"):
        with _grid_hierarchy(dim, c) as h:
            h.set_params(2, 2, 2.0 / 3.0, keep_err=True, restriction="p1_transpose" if path == "kernel" else "table")
            if path == "kernel":
                h.set_prolongation("p1")
            else:
                _set_tables(h, dim)
            h.set_vector(0, "v", vc)
            h.set_vector(1, "v", v0)
            h.prolong(1, add=False)
            e0, v_after0 = h.get_vector(1, "err")[:, 0], h.get_vector(1, "v")[:, 0]
            h.set_vector(1, "err", np.full(nf, 7.0))
            h.prolong(1, add=True)
            e1, v1 = h.get_vector(1, "err")[:, 0], h.get_vector(1, "v")[:, 0]
            h.set_vector(1, "r", rf)
            h.restrict(1, "p1_transpose" if path == "kernel" else "table")
            out[path] = (e0, v_after0, e1, v1, h.get_vector(0, "f")[:, 0])
    e0, va0, e1, v1, fc = out["kernel"]
    assert np.array_equal(e0, want_p)
    assert np.array_equal(va0, v0)                     # add = 0 leaves V alone
    assert np.array_equal(e1, want_p)
    assert np.array_equal(v1, v0 + want_p)
    assert np.array_equal(fc, want_r)
    for a, b in zip(out["kernel"], out["table"]):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_table_and_p1_prolongation_exclude_each_other():
    dim, c = 3, 4
    rng = np.random.default_rng(5)
    vc = rng.standard_normal((c + 1) ** dim)
    with _grid_hierarchy(dim, c) as h:
        h.set_prolongation("p2")                       # a table ...
        h.set_prolongation("p1")                       # ... cleared by the P1 embedding
        h.set_vector(0, "v", vc)
        h.prolong(1, add=False)
        assert np.array_equal(h.get_vector(1, "err")[:, 0], ref.prolongation(c, dim) @ vc)
        _set_tables(h, dim)                            # ... and the P1 embedding cleared by a table (here: the same operator)
        h.prolong(1, add=False)
        assert np.array_equal(h.get_vector(1, "err")[:, 0], ref.prolongation(c, dim) @ vc)
        h.set_prolongation("q1")
        h.prolong(1, add=False)
        assert not np.array_equal(h.get_vector(1, "err")[:, 0], ref.prolongation(c, dim) @ vc)


@pytest.mark.gpu
@pytest.mark.parametrize("tuning", [{}, {"offset_codes": 0}])
def test_other_mesh_orientation_is_refused(tuning):
    """A 2-D level assembled on squares cut along (1, -1) (the x-mirror of poisson's mesh, its zero couplings kept) fails
    the Kuhn-pattern check of both transfers with a clear error: from the offset table / symmetric diagonals, and with
    offset_codes=0 from the device scan of the int32 columns."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    c = 8
    mats = {}
    for l, N in ((0, c), (1, 2 * c)):
        A = poisson.make_level(N, 2).A.tocoo()
        n1 = N + 1
        mirror = lambda g: (N - g % n1) + n1 * (g // n1)
        B = sp.csr_matrix((A.data, (mirror(A.row), mirror(A.col))), shape=A.shape)
        B.sort_indices()
        mats[l] = B
    with DeviceHierarchy(2, 0, 1, c=c, **tuning) as h:
        for l in (0, 1):
            h.set_level(l, mats[l], prune_zeros=False)
        assert h.level_info(1)["offset_codes"] == 0 if tuning else h.level_info(1)["symmetric_diagonals"] > 0
        h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
        h.set_prolongation("p1")
        with pytest.raises(_capi.MgError, match="Kuhn pattern"):
            h.prolong(1, add=False)
        with pytest.raises(_capi.MgError, match="Kuhn pattern"):
            h.restrict(1, "p1_transpose")


@pytest.mark.gpu
@pytest.mark.parametrize("dim,lo,hi,c", [(2, 0, 4, 8), (3, 0, 3, 4)])
def test_device_cycle_matches_numpy_reference(dim, lo, hi, c):
    """V(2,2) residual histories with P1 + P^T: device against the NumPy cycle, <= 1e-10 relative while the residual is above
    1e-4 of the first one.  Below that the smoother's round-off (the device streams v + w D^-1 (f - A v), the oracle the split
    form) is a constant ~1e-15 absolute floor: every cycle is held to 1e-12 of the first residual."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    bag = poisson.make_hierarchy(dim, lo, hi, c=c, mu1=2, mu2=2)
    gi = {l: L.grid_index for l, L in bag.levels.items()}
    want = ref.residual_history(ref.p1_oracle(bag, gi, dim), hi, 12, "table")
    with DeviceHierarchy.from_bag(bag, dim=dim, grid_index=gi) as h:
        h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
        h.set_prolongation("p1")
        h.set_vector(hi, "v", np.zeros_like(bag.b_dict[hi]))
        h.set_vector(hi, "f", bag.b_dict[hi])
        got = h.vcycle(hi, 12, residuals=True)
    big = want >= 1e-4 * want[0]
    assert big.sum() >= 5
    assert np.max(np.abs(got - want)[big] / want[big]) <= 1e-10, (got, want)
    assert np.max(np.abs(got - want)) <= 1e-12 * want[0], (got, want)
    assert ref.contraction(got) <= (0.25 if dim == 2 else 0.40)


@pytest.mark.gpu
@pytest.mark.parametrize("world,dim,c", [(2, 3, 4), (3, 2, 8)])
def test_slabs_bit_identical_to_single_handle(world, dim, c):
    """P1 + P^T on 2 and 3 slabs through the host-staged stand-in transport: transfers bit-identical to the single handle."""
    import torch.multiprocessing as mp
    from tests.dist_helpers import free_port
    from tests.p1_workers import gpu_p1_slab_worker
    mp.spawn(gpu_p1_slab_worker, args=(world, free_port(), dim, 1, 3, c, 2), nprocs=world, join=True)
