"""Matrix-free diffusion levels (mg_gen_diffusion_level_mf / mg_gen_diffusion_hierarchy_mf, mg_diffusion_mf.hip.h): the
level keeps kappa and no matrix, and every kernel rebuilds the row it needs.  The row is defined by the stored level, so
everything here compares with a second handle that stores the same level: to the bit, except for mg_pcg, whose p.q
partial sums are per workgroup and therefore round differently."""
import struct
from fractions import Fraction

import numpy as np
import pytest

from tests.diffusion_workers import jump_kappa, lognormal_kappa

# the stored handle's one-step kernel whose summation order diffusion_mf restates is sdia_apply (path "slice"):
# "row_classes" 0 keeps the class kernels (sweep1c, block, small, K-sweep) off, "fuse_sweeps" 0 the pair pass
STORED_ONE_STEP = {"row_classes": 0, "fuse_sweeps": 0}


# ---- host: the division by six ------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fma(a, b, c) with one rounding (exact rational arithmetic; float() of a Fraction rounds to nearest even)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _div6(t):
    """mf_div6 of mg_diffusion_mf.hip.h, operation for operation."""
    if not (2.0 ** -900 <= t <= 2.0 ** 900):
        return t / 6.0
    c = float.fromhex("0x1.5555555555555p-3")
    q = t * c
    r = _fma(-q, 6.0, t)
    return _fma(r, c, q)


def test_division_by_six_shortcut_is_correctly_rounded():
    """q = t c, r = fma(-q, 6, t), q' = fma(r, c, q) with c = RN(1/6) against t / 6.0: 10^6 random mantissas across the
    exponents of the fast range, the edges of that range, powers of two and their neighbours, multiples of six and their
    neighbours, and the values next to the subnormals and to overflow (which take the division)."""
    assert float.fromhex("0x1.5555555555555p-3") == 1.0 / 6.0
    rng = np.random.default_rng(0)
    m = rng.integers(1 << 52, 1 << 53, size=1_000_000).astype(np.float64)
    e = rng.integers(-899, 900, size=m.size)
    cases = np.ldexp(m, e - 52).tolist()
    edge = []
    for p in list(range(-1074, -1000, 3)) + list(range(-905, -895)) + list(range(-60, 61)) + list(range(895, 905)) + [1020, 1023]:
        x = 2.0 ** p
        for y in (x, np.nextafter(x, 0.0), np.nextafter(x, np.inf), 3.0 * x, 6.0 * x if p < 1020 else x,
                  np.nextafter(6.0 * x if p < 1020 else x, 0.0), np.nextafter(6.0 * x if p < 1020 else x, np.inf)):
            edge.append(float(y))
    edge += [np.finfo(np.float64).tiny, np.nextafter(np.finfo(np.float64).tiny, 1.0), np.finfo(np.float64).max, 5e-324]
    bad = [(t, _div6(t), t / 6.0) for t in cases + edge if struct.pack("<d", _div6(t)) != struct.pack("<d", t / 6.0)]
    assert not bad, bad[:5]


# ---- device ----------------------------------------------------------------------------------------------------------------
def _kappa(field, N):
    if field == "ones":
        return np.ones(N ** 3)
    return jump_kappa(N, 3) if field == "jump" else lognormal_kappa(N, 3, seed=1)


def _same(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [32, 48, 256])
@pytest.mark.parametrize("field", ["ones", "jump", "lognormal"])
def test_bits_against_the_stored_level(N, field):
    """F as generated, residual, one and three Jacobi sweeps, Chebyshev polynomials of degree two and four with caller-set
    bounds: the bytes of the stored level's one-step kernel (sdia_apply, `slice`), and the launch counts say which ran."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    kappa = _kappa(field, N)
    with DeviceHierarchy(3, 0, 1, c=N // 2, **STORED_ONE_STEP) as s, DeviceHierarchy(3, 0, 1, c=N // 2) as m:
        s.gen_diffusion_level(1, kappa)
        m.gen_diffusion_level(1, kappa, matrix_free=True)
        assert m.level_matrix_free(1) and not s.level_matrix_free(1)
        assert s.level_info(1)["nnz_nonzero"] == m.level_info(1)["nnz_nonzero"]
        assert _same(s.get_vector(1, "f"), m.get_vector(1, "f"))
        rng = np.random.default_rng(11)
        v, f = rng.standard_normal(s.n_dofs(1)), rng.standard_normal(s.n_dofs(1))
        for smoother, sweeps in (("jacobi", (1, 3)), ("chebyshev", (2, 4))):
            for h in (s, m):
                h.set_params(2, 2, 2.0 / 3.0, smoother=smoother)
                h.set_chebyshev_bounds(1, 0.25, 2.125)
                h.reset_smoother_launches()
            for nw in sweeps:
                got = []
                for h in (s, m):
                    h.set_vector(1, "v", v)
                    h.set_vector(1, "f", f)
                    h.residual(1)
                    r = h.get_vector(1, "r")
                    h.set_vector(1, "v", v)
                    h.smooth(1, nw)
                    got.append((r, h.get_vector(1, "v")))
                assert np.all(np.isfinite(got[0][1]))
                assert _same(got[0][0], got[1][0]), (smoother, nw, "residual")
                diff = np.flatnonzero(got[0][1] != got[1][1])
                assert _same(got[0][1], got[1][1]), (smoother, nw, diff[:5], diff.size)
            total = sum(sweeps)
            assert s.smoother_launches(1) == {"slice": (total, total, 0)}
            assert m.smoother_launches(1) == {"matrix_free": (total, total, 0)}


def _hierarchy_pair(kappa, averaging, min_rows, **tuning):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    s = DeviceHierarchy(3, 0, 3, c=16, **tuning)
    m = DeviceHierarchy(3, 0, 3, c=16, **tuning)
    s.gen_diffusion_hierarchy(kappa, averaging)
    m.gen_diffusion_hierarchy(kappa, averaging, matrix_free_min_rows=min_rows)
    for h in (s, m):
        h.set_prolongation("p1")
    return s, m


_MIN_ROWS = 200_000         # 129^3 and 65^3 rows are matrix-free, 33^3 and 17^3 stored


@pytest.mark.gpu
@pytest.mark.parametrize("averaging", ["arithmetic", "harmonic"])
@pytest.mark.parametrize("graph", [0, 1])
def test_cycles_are_bit_identical(averaging, graph):
    """Three V(2,2) cycles at N = 128, four levels, log-normal kappa, the two finest levels matrix-free: residual norms
    and iterate to the bit, Jacobi and Chebyshev (caller-set and estimated bounds), eager and captured.  The stored
    hierarchy runs its default paths (block pass on the middle levels), which are bit-identical to single sweeps."""
    N = 128
    kappa = lognormal_kappa(N, 3, seed=1)
    s, m = _hierarchy_pair(kappa, averaging, _MIN_ROWS, graph=graph)
    with s, m:
        assert [m.level_matrix_free(l) for l in range(4)] == [False, False, True, True]
        assert [s.level_matrix_free(l) for l in range(4)] == [False] * 4
        f = np.random.default_rng(5).standard_normal(s.n_dofs(3))
        for smoother, bounds in (("jacobi", None), ("chebyshev", (0.3, 2.2)), ("chebyshev", None)):
            got = []
            for h in (s, m):
                h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose", smoother=smoother)
                for l in range(1, 4):
                    h.set_chebyshev_bounds(l, *(bounds or (0.0, 0.0)))
                h.reset_smoother_launches()
                h.zero_vector(3, "v")
                h.set_vector(3, "f", f)
                res = h.vcycle(3, 3, residuals=True)
                got.append((res, h.get_vector(3, "v")))
            if smoother == "chebyshev" and bounds is None:
                # the estimate's dot products are dot_device's, whatever the matrix format: the same interval to the bit
                for l in range(1, 4):
                    assert s.chebyshev_bounds(l) == m.chebyshev_bounds(l), l
            assert _same(got[0][0], got[1][0]), (smoother, bounds, got[0][0], got[1][0])
            assert _same(got[0][1], got[1][1]), (smoother, bounds)
            assert got[0][0][-1] < got[0][0][0]
            for l in (2, 3):
                assert set(m.smoother_launches(l)) == {"matrix_free"}, m.smoother_launches(l)
                assert "matrix_free" not in s.smoother_launches(l)
            assert "matrix_free" not in m.smoother_launches(1)


@pytest.mark.gpu
@pytest.mark.parametrize("averaging", ["arithmetic", "harmonic"])
def test_pcg_on_a_matrix_free_hierarchy(averaging):
    """mg_pcg: repeatable to the bit on the matrix-free handle (two calls, graph 0 and 1), within one iteration of the
    stored run, and its iterate solves the STORED system: ||f - A x|| <= 10 rtol ||f|| at rtol = 1e-8 (the factor ten
    caps the drift between the recurrence and the true residual; the stored handle's own iterate passes the same check
    first)."""
    N = 128
    rtol = 1e-8
    kappa = lognormal_kappa(N, 3, seed=1)
    s, m = _hierarchy_pair(kappa, averaging, _MIN_ROWS)
    with s, m:
        f = np.random.default_rng(6).standard_normal(s.n_dofs(3))
        fn = float(np.linalg.norm(f))

        def solve(h, graph):
            h.set_tuning("graph", graph)
            h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
            h.zero_vector(3, "v")
            h.set_vector(3, "f", f)
            hist = h.pcg(rtol=rtol, max_iter=100, level=3)
            return hist, h.get_vector(3, "v")

        def true_residual(x):
            s.set_vector(3, "v", x)
            s.set_vector(3, "f", f)
            s.residual(3)
            return s.norm2(3, "r")

        hs, xs = solve(s, 1)
        assert hs[-1] <= rtol * fn
        assert true_residual(xs) <= 10 * rtol * fn
        runs = [solve(m, 1), solve(m, 1), solve(m, 0)]
        for hist, x in runs[1:]:
            assert _same(hist, runs[0][0]) and _same(x, runs[0][1])
        hm, xm = runs[0]
        print("pcg iterations stored / matrix-free:", len(hs), len(hm), "true residuals / ||f||:",
              true_residual(xs) / fn, true_residual(xm) / fn)
        assert abs(len(hm) - len(hs)) <= 1
        assert hm[-1] <= rtol * fn
        assert true_residual(xm) <= 10 * rtol * fn


@pytest.mark.gpu
def test_storage_is_kappa_and_no_matrix():
    """A matrix-free 257^3 level holds at least 24 B per row less than the stored one: 32 B of symmetric diagonals gone,
    8 B of kappa kept."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 256
    kappa = lognormal_kappa(N, 3, seed=1)
    with DeviceHierarchy(3, 0, 1, c=N // 2) as s:
        s.gen_diffusion_level(1, kappa)
        stored = s.memory_bytes()
        assert s.level_kappa_bytes(1) == 0
    with DeviceHierarchy(3, 0, 1, c=N // 2) as m:
        m.gen_diffusion_level(1, kappa, matrix_free=True)
        free = m.memory_bytes()
        rows = m.n_dofs(1)
        assert m.level_kappa_bytes(1) == 8 * N ** 3
    assert stored - free >= 24 * rows, (stored, free, rows)


@pytest.mark.gpu
def test_min_rows_decides_which_levels_are_matrix_free():
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    kappa = lognormal_kappa(64, 3, seed=2)
    rows = [(8 * 2 ** l + 1) ** 3 for l in range(4)]
    for min_rows, want in ((0, [False, True, True, True]), (rows[2], [False, False, True, True]),
                           (rows[3] + 1, [False] * 4)):
        with DeviceHierarchy(3, 0, 3, c=8) as h:
            h.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=min_rows)
            assert [h.level_matrix_free(l) for l in range(4)] == want, min_rows


@pytest.mark.gpu
def test_refusals_name_their_cause():
    from multigrid_dolfinx_amd._capi import MgError
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    with DeviceHierarchy(2, 0, 1, c=16) as h:
        with pytest.raises(MgError, match="2-D"):
            h.gen_diffusion_level(1, np.ones(32 ** 2), matrix_free=True)
        with pytest.raises(MgError, match="2-D"):
            h.gen_diffusion_hierarchy(np.ones(32 ** 2), matrix_free_min_rows=0)
    with DeviceHierarchy(3, 0, 1, c=16) as h:
        nothing = lambda *a: None
        h.set_comm_callbacks(0, 2, nothing, nothing, nothing, replicate_below=0)
        with pytest.raises(MgError, match="slab"):
            h.gen_diffusion_level(1, np.ones(32 ** 3), matrix_free=True)
        with pytest.raises(MgError, match="slab"):
            h.gen_diffusion_hierarchy(np.ones(32 ** 3), matrix_free_min_rows=0)
    with DeviceHierarchy(3, 0, 1, c=16) as h:
        h.gen_diffusion_level(1, lognormal_kappa(32, 3, seed=3), matrix_free=True)
        with pytest.raises(MgError, match="matrix-free"):
            h.galerkin_level(1)
        for smoother in ("rbgs", "mcgs"):
            h.set_params(2, 2, 1.0, smoother=smoother)
            with pytest.raises(MgError, match="matrix-free"):
                h.smooth(1, 1)
        with pytest.raises(ValueError):
            h.gen_diffusion_level(1, np.ones(32 ** 3), prune_zeros=False, matrix_free=True)
        # the coarsest level is always stored: the direct solve factorises it
        with pytest.raises(MgError, match="level 0.*direct solve"):
            h.gen_diffusion_level(0, np.ones(16 ** 3), matrix_free=True)
        # the level is still usable
        h.set_params(2, 2, 2.0 / 3.0)
        h.smooth(1, 1)
        assert h.smoother_launches(1) == {"matrix_free": (1, 1, 0)}


@pytest.mark.gpu
@pytest.mark.parametrize("smoother", ["rbgs", "mcgs"])
def test_gauss_seidel_cycles_are_refused_before_anything_runs(smoother):
    """With a matrix-free level in the cycle, V-cycles, the prepared cycle and mg_pcg under a Gauss-Seidel smoother are
    refused by name (before the colouring check, which reads stored rows); the handle then cycles with Jacobi."""
    from multigrid_dolfinx_amd._capi import MgError
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    kappa = lognormal_kappa(32, 3, seed=4)
    with DeviceHierarchy(3, 0, 2, c=8) as h:
        h.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=0)
        assert [h.level_matrix_free(l) for l in range(3)] == [False, True, True]
        h.set_prolongation("p1")
        h.set_params(2, 2, 1.0, restriction="p1_transpose", smoother=smoother)
        f = np.random.default_rng(8).standard_normal(h.n_dofs(2))
        h.zero_vector(2, "v")
        h.set_vector(2, "f", f)
        for call in (lambda: h.vcycle(2, 1), lambda: h.prepare_cycle(2), lambda: h.pcg(rtol=1e-8, max_iter=5, level=2),
                     lambda: h.vcycle(1, 1)):
            with pytest.raises(MgError, match="matrix-free"):
                call()
        assert h.get_vector(2, "v").tobytes() == np.zeros(h.n_dofs(2)).tobytes()
        h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
        res = h.vcycle(2, 2, residuals=True)
        assert res[1] < res[0]


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [0.0, -1.0, np.nan, np.inf])
def test_bad_kappa_is_refused_with_its_cell(bad):
    from multigrid_dolfinx_amd._capi import MgError
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 32
    k = np.ones(N ** 3)
    cell = (5 * N + 7) * N + 3
    k[cell] = bad
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        with pytest.raises(MgError, match=rf"cell \(3, 7, 5\) = index {cell} ") as mf:
            h.gen_diffusion_level(1, k, matrix_free=True)
        with pytest.raises(MgError) as stored:
            h.gen_diffusion_level(1, k)
        assert str(mf.value) == str(stored.value)
        with pytest.raises(MgError, match=rf"index {cell} "):
            h.gen_diffusion_hierarchy(k, matrix_free_min_rows=0)
