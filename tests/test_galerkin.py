"""Galerkin coarse levels on the device (mg_galerkin_level / mg_galerkin_hierarchy) with the P1 natural embedding.

On the synthetic Poisson levels P^T A P IS the rediscretised coarse matrix, bit for bit (dyadic entries): the Galerkin
levels must then get the generated levels' storage and residuals exactly.  On rows unlike each other they are checked
against SciPy's P^T A P.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from multigrid_dolfinx_amd import poisson
from tests import p1_reference as ref

pytestmark = pytest.mark.gpu

_INFO = ("n_global", "nnz_stored", "nnz_nonzero", "ell_width", "offset_codes", "symmetric_diagonals", "row_classes")


def _compare_with_generated(dim, lo, hi, c, check_residual=True):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    with DeviceHierarchy.galerkin_from_matrix(dim, lo, hi, c=c) as g, \
            DeviceHierarchy.synthetic(dim, lo, hi, c=c, mu1=2, mu2=2) as s:
        for l in range(lo, hi):
            gi, si = g.level_info(l), s.level_info(l)
            assert {k: gi[k] for k in _INFO} == {k: si[k] for k in _INFO}, (l, gi, si)
            if not check_residual:
                continue
            rng = np.random.default_rng(100 + l)
            v, f = rng.standard_normal(g.n_dofs(l)), rng.standard_normal(g.n_dofs(l))
            out = []
            for h in (g, s):
                h.set_vector(l, "v", v)
                h.set_vector(l, "f", f)
                h.residual(l)
                out.append(h.get_vector(l, "r"))
            assert np.array_equal(out[0], out[1]), l


@pytest.mark.parametrize("dim,lo,hi,c", [(2, 1, 3, 8), (3, 0, 3, 4), (3, 2, 5, 8)])
def test_galerkin_levels_equal_generated_levels(dim, lo, hi, c):
    """C1 (2-D 65^2, 3 levels), a small 3-D hierarchy and 257^3 -> 33^3: storage and residuals as the generated levels."""
    _compare_with_generated(dim, lo, hi, c)


def test_galerkin_1025_to_513():
    """Once at full size: 1025^3 -> 513^3 gets the generated 513^3 level's storage and residual."""
    _compare_with_generated(3, 7, 8, 4)


def _jump_matrix(N, dim, seed):
    """A fine matrix whose rows are unlike each other: poisson's level plus a reaction term on the diagonal with a jump
    (ten times larger in the half x > 1/2) and a random part."""
    L = poisson.make_level(N, dim)
    n1 = N + 1
    idx = np.arange(n1 ** dim)
    inner = ref.interior(N, dim)
    rng = np.random.default_rng(seed)
    react = np.where(idx % n1 > N // 2, 10.0, 1.0) * (1.0 + rng.random(idx.size)) * L.h ** dim
    A = (L.A + sp.diags(np.where(inner, react, 0.0))).tocsr()
    A.sort_indices()
    return A


@pytest.mark.parametrize("dim,lo,hi,c", [(2, 0, 3, 8), (3, 0, 3, 4)])
@pytest.mark.parametrize("tuning", [{}, {"symmetric_storage": 0}, {"offset_codes": 0}])
def test_galerkin_rows_unlike_each_other(dim, lo, hi, c, tuning):
    """Every storage format of the fine level: mg_residual on each Galerkin level against SciPy's P^T A P applied to the same
    vector (<= 1e-14 relative), and two calls bit-identical."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    Nf = c * 2 ** hi
    A = _jump_matrix(Nf, dim, seed=7)
    mats = {hi: A}
    for l in range(hi, lo, -1):
        mats[l - 1] = ref.galerkin(mats[l], c * 2 ** l, dim)
    runs = []
    for _ in range(2):
        with DeviceHierarchy.galerkin_from_matrix(dim, lo, hi, A=A, c=c, **tuning) as h:
            res = {}
            for l in range(lo, hi):
                rng = np.random.default_rng(200 + l)
                v = rng.standard_normal(h.n_dofs(l))
                h.set_vector(l, "v", v)
                h.zero_vector(l, "f")
                h.residual(l)
                got = -h.get_vector(l, "r")[:, 0]
                want = mats[l] @ v
                assert np.linalg.norm(got - want) <= 1e-14 * np.linalg.norm(want), (l, np.linalg.norm(got - want))
                res[l] = got
            runs.append(res)
    for l in runs[0]:
        assert np.array_equal(runs[0][l], runs[1][l]), l


def test_galerkin_errors():
    """Level 0, a grid-only level and a fine level whose stencil is not the Kuhn pattern are refused; the coarse level is
    left as it was.  (An odd elements_per_dim cannot reach mg_galerkin_level: level l >= 1 has N = N0 * 2^l.  Slabs:
    tests/p1_workers.py.)"""
    from multigrid_dolfinx_amd import _capi
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    with DeviceHierarchy.synthetic(2, 0, 1, c=8) as h:
        with pytest.raises(_capi.MgError, match="level must be >= 1"):
            h.galerkin_level(0)
        before = h.level_info(0)
        h.set_level_grid(1)
        with pytest.raises(_capi.MgError, match="no matrix"):
            h.galerkin_level(1)
        assert h.level_info(0) == before
    with DeviceHierarchy(2, 0, 1, c=8) as h:
        A = poisson.make_level(16, 2).A.tocoo()
        mirror = lambda g: (16 - g % 17) + 17 * (g // 17)
        B = sp.csr_matrix((A.data, (mirror(A.row), mirror(A.col))), shape=A.shape)
        h.gen_poisson_level(0)
        h.set_level(1, B, prune_zeros=False)
        with pytest.raises(_capi.MgError, match="Kuhn pattern"):
            h.galerkin_level(1)


def test_pcg_on_galerkin_levels_beats_reference_transfers_at_c3():
    """C3 (3-D 257^3, 4 levels) V(2,2): mg_pcg with P1 + P^T on Galerkin levels reaches 1e-10 in fewer iterations than the
    160 DESIGN.md records for the reference transfers."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    with DeviceHierarchy.galerkin_from_matrix(3, 2, 5, c=8) as h, DeviceHierarchy.synthetic(3, 2, 5, c=8) as s:
        f = s.get_vector(5, "f")
        h.set_vector(5, "f", f)
        h.zero_vector(5, "v")
        hist = h.pcg(rtol=1e-10, max_iter=400)
        bn = np.linalg.norm(f)
        print(f"C3 V(2,2) P1 + P^T on Galerkin levels: {len(hist)} PCG iterations to 1e-10")
        assert hist[-1] <= 1e-10 * bn
        assert h.norm2(5, "r") <= 2e-10 * bn
        assert len(hist) < 160, len(hist)
