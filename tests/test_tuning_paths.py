"""The `mg_set_tuning` keys that select code no other test runs: every accepted key must be set by some test, and every value
this module sets must give the bits of one sweep per launch (include/mg_hip.h promises "bit-identical" for all of them).

Reference of every GPU test: the handle with "fuse_sweeps", "fuse_small", "fuse_block", "fuse_k" 0 (`_SINGLE` of
tests/test_march_one_barrier.py, `REFERENCE` of tests/test_neumann_smoother_paths.py -- checked there against the oracle and
np.longdouble), built once per grid; on slabs the single handle.  Everything is np.array_equal, and mg_smoother_launches names
the path that ran.

  fuse_wi, fuse_even   width of a tile column of the pair pass (jacobi2_plan): 41^3 with columns of 8 cells (six columns,
                       narrower than a wave), 13 (last column two cells), 40 (last column one cell), 41, 3 (clamped to 8), 1000
                       (clamped to 124) and 0; 129^3 with "fuse_even" (65 + 64), 64 (last column one cell) and 65; the
                       class-coded pass in shapes 1 and 0, the plain pass ("fuse_plain" 2 and 1, the latter ignores the width),
                       on a Poisson level and a diffusion level whose x faces hold real rows
  fuse_xcd_chunk       1, 3, 32, 512: pair pass, K-sweep march with and without a tail of short segments, one-sweep plane march
  cls_blocks_per_cu    1, 3, 64: residual, Jacobi sweep (finest and middle level) and x^T A x at 65^3 and 129^3
  lds_pad              0, 32768, 65536, 153600 on levels of at least 100000 slices without row classes; 153601 refused
  fuse_k_nt_store, fuse_k_small_tiles   the K-sweep march with the switch on
  fuse_k_shape         1, 4, 7, 8, 9, -1 accepted; the retired shapes 0, 2, 3, 5, 6 refused; the retired keys unknown
  slab_pair_form       0 and 1 with the overlap on, two and three ranks over the in-process RCCL stand-in
  pcg_chunk            1, 5, 16, 64: iteration count, relative residual and solution of the coarsest-level PCG
  gen_odd_rows         what the generator perturbs, against the header's contract"""
import functools
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.test_march_one_barrier import _MARCH, _SINGLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
OMEGA = 2.0 / 3.0
LV = 3                      # the level the Poisson grids live on: 8 c + 1 nodes per axis
EPS = np.finfo(np.float64).eps

# the pair pass on every level: no K-sweep march, no block pass, no one-launch smoother
_PAIR = dict(fuse_k=0, fuse_block=0, fuse_small=0, fuse_min_rows=0)

# keys no test sets, each with the test that reaches it another way
EXEMPT = {
    "require_diagonal": "set to 0 by the shim's jacobiRelaxation on operands that belong to no initialised problem (multigrid.py): "
                        "tests/test_gpu_parity.py::test_jacobi_relaxation_standalone_operands",
}


# ---- host: the inventory ---------------------------------------------------------------------------------------------------------
def test_every_tuning_key_is_set_by_some_test():
    """Every key of mg_set_tuning's `k == "..."` chain (enumerated as tests/test_capi_symbols.py does) occurs in the text of
    tests/*.py -- this test's own source left out, so that neither it nor EXEMPT can satisfy it -- or is listed in EXEMPT with
    the test that reaches it.  A key added without a test fails here."""
    src = open(os.path.join(ROOT, "multigrid_dolfinx_amd", "csrc", "mg_capi.hip")).read()
    body = src[src.index("int mg_set_tuning("):]
    body = body[:body.index("\nnamespace {")]
    accepted = set(re.findall(r'k == "([a-z_0-9]+)"', body))
    assert len(accepted) >= 73, len(accepted)
    text = ""
    for name in sorted(os.listdir(HERE)):
        if name.endswith(".py"):
            text += open(os.path.join(HERE, name)).read()
    mine = inspect.getsource(test_every_tuning_key_is_set_by_some_test)
    assert mine in text
    text = text.replace(mine, "")
    text = re.sub(r"(?ms)^EXEMPT = \{.*?^\}", "", text)
    unset = sorted(k for k in accepted if not re.search(r"\b" + k + r"\b", text))
    assert set(EXEMPT) <= accepted, sorted(set(EXEMPT) - accepted)
    assert unset == sorted(EXEMPT), (sorted(set(unset) - set(EXEMPT)), sorted(set(EXEMPT) - set(unset)))


# ---- Poisson levels ---------------------------------------------------------------------------------------------------------------
def _poisson(c, tuning, middle=False):
    """Levels LV - 1 and LV of the generator's Poisson hierarchy (8 c + 1 nodes per axis on LV), LV the finest level of the
    handle or, with `middle`, below a level that is never set."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    h = DeviceHierarchy(3, LV - 1, LV + 1 if middle else LV, c=c, **tuning)
    h.gen_poisson_level(LV - 1)
    h.gen_poisson_level(LV)
    h.set_params(2, 2, OMEGA)
    return h


@functools.lru_cache(maxsize=None)
def _vectors(n1, seed=0):
    rng = np.random.default_rng(4000 + 7 * n1 + seed)
    v, f = rng.standard_normal(n1 ** 3), rng.standard_normal(n1 ** 3)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def _smooth(h, level, nw, v, f):
    h.set_vector(level, "v", v)
    h.set_vector(level, "f", f)
    h.reset_smoother_launches()
    h.smooth(level, nw)
    return h.get_vector(level, "v"), h.smoother_launches(level)


def _residual(h, level, v, f):
    h.set_vector(level, "v", v)
    h.set_vector(level, "f", f)
    h.residual(level)
    return h.get_vector(level, "r")


@functools.lru_cache(maxsize=None)
def _single_sweeps(c, nw):
    """nw sweeps, one per launch, from _vectors(8 c + 1): the same bits on the finest and on a middle level (once per grid and
    sweep count; read-only)."""
    v, f = _vectors(8 * c + 1)
    got = []
    for middle in (False, True):
        with _poisson(c, _SINGLE, middle) as h:
            x, ran = _smooth(h, LV, nw, v, f)
        assert ran == {"slice": (nw, nw, 0)}, ran
        got.append(x)
    assert np.all(np.isfinite(got[0])) and np.array_equal(got[0], got[1])
    got[0].setflags(write=False)
    return got[0]


@functools.lru_cache(maxsize=None)
def _single_residual(c):
    v, f = _vectors(8 * c + 1)
    with _poisson(c, _SINGLE) as h:
        r = _residual(h, LV, v, f)
    assert np.all(np.isfinite(r)) and np.any(r != 0.0)
    r.setflags(write=False)
    return r


def _pair_counts(nw, pair, single="slice"):
    """mg_smoother_launches of nw sweeps taken as pairs and a single one"""
    want = {pair: (nw // 2, 2 * (nw // 2), 0)}
    if nw % 2:
        want[single] = (1, 1, 0)
    return want


# (what the variant sets, the pair path it must take); widths come from `fuse_wi` / `fuse_even` on top
_PAIR_KERNELS = [(dict(), "pair_class"), (dict(fuse_shape=0), "pair_class"),
                 (dict(fuse_classes=0, fuse_plain_shape=0), "pair_plain")]
_WIDTHS_41 = [8, 13, 40, 41, 3, 1000, 0]


def _differ(a, b):
    return "rows that differ: %d, the first: %s" % (np.count_nonzero(a != b), np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:8])


# ---- 2. column widths of the pair pass ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wi", _WIDTHS_41)
def test_pair_pass_column_widths_on_41(wi):
    """41^3 Poisson: 2, 3 and 6 sweeps as pairs with tile columns of `wi` cells -- the class-coded pass in "fuse_shape" 1 and 0
    and the plain pass of the stored rows, on the finest level of a handle and on a middle one, with the default plane
    segments and three -- against one sweep per launch."""
    c = 5
    v, f = _vectors(41)
    for kernel, path in _PAIR_KERNELS:
        for extra in (dict(), dict(fuse_segments=3)) if wi in (13, 40) else (dict(),):
            for middle in (False, True):
                tuning = dict(_PAIR, fuse_wi=wi, **kernel, **extra)
                with _poisson(c, tuning, middle) as h:
                    assert 2 <= h.level_info(LV)["row_classes"] <= 64
                    for nw in (2, 3, 6):
                        got, ran = _smooth(h, LV, nw, v, f)
                        assert ran == _pair_counts(nw, path), (tuning, middle, nw, ran)
                        assert np.array_equal(got, _single_sweeps(c, nw)), (tuning, middle, nw, _differ(got, _single_sweeps(c, nw)))


@pytest.mark.gpu
def test_round_one_plain_pass_ignores_the_width():
    """"fuse_classes" 0, "fuse_plain" 1 (sdia_jacobi2): jacobi2_plan gives that pass its own columns of 126 cells and no `wi`;
    "fuse_wi" and "fuse_even" change nothing."""
    c = 5
    v, f = _vectors(41)
    for knob in (dict(), dict(fuse_wi=8), dict(fuse_wi=13), dict(fuse_even=1)):
        tuning = dict(_PAIR, fuse_classes=0, fuse_plain=1, **knob)
        with _poisson(c, tuning) as h:
            for nw in (2, 3, 6):
                got, ran = _smooth(h, LV, nw, v, f)
                assert ran == _pair_counts(nw, "pair_plain"), (tuning, nw, ran)
                assert np.array_equal(got, _single_sweeps(c, nw)), (tuning, nw, _differ(got, _single_sweeps(c, nw)))


@pytest.mark.gpu
@pytest.mark.parametrize("knob", [dict(fuse_even=1), dict(fuse_wi=64), dict(fuse_wi=65)], ids=["even", "wi64", "wi65"])
def test_pair_pass_column_widths_on_129(knob):
    """129^3: "fuse_even" 1 (two columns of 65 and 64 cells), columns of 64 (three, the last one cell) and of 65."""
    c = 16
    v, f = _vectors(129)
    for kernel, path in _PAIR_KERNELS:
        tuning = dict(_PAIR, **kernel, **knob)
        with _poisson(c, tuning) as h:
            for nw in (2, 3):
                got, ran = _smooth(h, LV, nw, v, f)
                assert ran == _pair_counts(nw, path), (tuning, nw, ran)
                assert np.array_equal(got, _single_sweeps(c, nw)), (tuning, nw, _differ(got, _single_sweeps(c, nw)))


_DIFFUSION_N, _DIFFUSION_FACES, _DIFFUSION_SWEEPS = 40, 18, (2, 3, 6)


@functools.lru_cache(maxsize=None)
def _diffusion_inputs():
    from tests.diffusion_workers import jump_kappa
    n = (_DIFFUSION_N + 1) ** 3
    rng = np.random.default_rng(418)
    return jump_kappa(_DIFFUSION_N, 3), rng.standard_normal(n), rng.standard_normal(n)


@functools.lru_cache(maxsize=None)
def _diffusion_single_sweeps():
    from tests.test_neumann_smoother_paths import REFERENCE, _handle, _smooths
    kappa, v, f = _diffusion_inputs()
    with _handle(_DIFFUSION_N, _DIFFUSION_FACES, kappa, REFERENCE, reference=True) as h:
        got = _smooths(h, v, f, _DIFFUSION_SWEEPS)
    for nw, (x, ran) in got.items():
        assert ran == {"slice": (nw, nw, 0)} and np.all(np.isfinite(x)), (nw, ran)
        x.setflags(write=False)
    return {nw: x for nw, (x, _) in got.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("wi", _WIDTHS_41)
def test_pair_pass_column_widths_on_a_level_with_free_x_faces(wi):
    """A generated diffusion level of 40^3 cells, kappa jumping at x = 1/2, face set 18 (x-, x+, z- free): the rows at i = 0 and
    i = 40 are relaxed, so a last column of one cell (`wi` 40, 8) holds rows that matter."""
    from tests.test_neumann_smoother_paths import _handle, _smooths
    kappa, v, f = _diffusion_inputs()
    want = _diffusion_single_sweeps()
    for kernel, path in _PAIR_KERNELS:
        for finest in (True, False):
            tuning = dict(_PAIR, fuse_wi=wi, **kernel)
            with _handle(_DIFFUSION_N, _DIFFUSION_FACES, kappa, tuning, finest) as h:       # (every size threshold 0: a single sweep marches)
                assert 2 <= h.level_info(1)["row_classes"] <= 64
                got = _smooths(h, v, f, _DIFFUSION_SWEEPS)
            for nw, (x, ran) in got.items():
                assert ran == _pair_counts(nw, path, "sweep1c"), (tuning, finest, nw, ran)
                assert np.array_equal(x, want[nw]), (tuning, finest, nw, _differ(x, want[nw]))


# ---- 3. the order in which workgroups take tiles ------------------------------------------------------------------------------------
_CHUNKS = [1, 3, 32, 512]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", _CHUNKS)
def test_tile_order_of_the_pair_pass(chunk):
    """41^3, three plane segments: 6 work items (one column, two tile rows), 36 with columns of 8 cells -- never a multiple of
    8 x chunk, so the grid has workgroups without a tile and the last group of chunks is partly filled."""
    c = 5
    v, f = _vectors(41)
    for kernel, path in _PAIR_KERNELS:
        for width in (dict(), dict(fuse_wi=8)):
            tuning = dict(_PAIR, fuse_segments=3, fuse_xcd_chunk=chunk, **kernel, **width)
            with _poisson(c, tuning) as h:
                for nw in (2, 3):
                    got, ran = _smooth(h, LV, nw, v, f)
                    assert ran == _pair_counts(nw, path), (tuning, nw, ran)
                    assert np.array_equal(got, _single_sweeps(c, nw)), (tuning, nw, _differ(got, _single_sweeps(c, nw)))


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", _CHUNKS)
def test_tile_order_of_the_k_sweep_march(chunk):
    """57^3 (six tiles of 54 x 24 cells for five sweeps): three plane segments (18 work items); a tail of short segments, whose
    items come after those of the whole segments in the permuted order; four sweeps per pass in shape 7."""
    c = 7
    v, f = _vectors(57)
    for k, extra, tail in ((5, dict(fuse_k_shape=8, fuse_k_segments=3), False), (5, dict(fuse_k_shape=8, fuse_k_tail=4), True),
                           (4, dict(fuse_k_shape=7), False)):
        tuning = dict(_MARCH, fuse_k=k, fuse_xcd_chunk=chunk, **extra)
        with _poisson(c, tuning) as h:
            got, ran = _smooth(h, LV, 2 * k, v, f)
        assert set(ran) == {"ksweep"} and ran["ksweep"][:2] == (2, 2 * k), (tuning, ran)
        if tail:
            assert ran["ksweep"][2] > 0, (tuning, ran)
        assert np.array_equal(got, _single_sweeps(c, 2 * k)), (tuning, _differ(got, _single_sweeps(c, 2 * k)))


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", _CHUNKS)
def test_tile_order_of_the_one_sweep_march(chunk):
    """65^3 with "march_min_rows" 0: the residual and one Jacobi sweep as a plane march (sdia_sweep1c)."""
    c = 8
    v, f = _vectors(65)
    tuning = dict(_SINGLE, march_min_rows=0, fuse_xcd_chunk=chunk)
    for middle in (False, True):
        with _poisson(c, tuning, middle) as h:
            r = _residual(h, LV, v, f)
            got, ran = _smooth(h, LV, 1, v, f)
        assert ran == {"sweep1c": (1, 1, 0)}, (tuning, ran)
        assert np.array_equal(r, _single_residual(c)), (tuning, middle, _differ(r, _single_residual(c)))
        assert np.array_equal(got, _single_sweeps(c, 1)), (tuning, middle, _differ(got, _single_sweeps(c, 1)))


# ---- 4. persistent blocks of the one-sweep class kernels ----------------------------------------------------------------------------
_CLASS_SLICES = dict(_SINGLE, march_sweeps=0)        # sdia_cls_apply / sdia_cls_jacobi_finest, not the plane march


@functools.lru_cache(maxsize=None)
def _stored_row_results(c):
    """(residual, one sweep, x^T A x) of the level's stored rows ("class_sweeps" 0)"""
    v, f = _vectors(8 * c + 1)
    with _poisson(c, dict(_CLASS_SLICES, class_sweeps=0)) as h:
        r = _residual(h, LV, v, f)
        x, ran = _smooth(h, LV, 1, v, f)
        h.set_vector(LV, "v", v)
        q = h.quadratic_form(LV, "v")
    assert ran == {"slice": (1, 1, 0)}, ran
    assert np.isfinite(q) and q > 0.0
    return r, x, q


@pytest.mark.gpu
@pytest.mark.parametrize("c", [8, 16], ids=["65", "129"])
@pytest.mark.parametrize("blocks", [1, 3, 64])
def test_persistent_class_kernels(blocks, c):
    """sdia_cls_apply and sdia_cls_jacobi_finest with 1, 3 and 64 persistent blocks per CU: 65^3 has 537 virtual blocks of four
    128-row slices and 129^3 4193 -- more than the 256 blocks of "cls_blocks_per_cu" 1 and fewer than the 16384 of 64, so
    blocks that loop over several groups and blocks that take one both run.  The residual, one Jacobi sweep on a
    middle and on the finest level and x^T A x have the bits of the stored rows; the dot-product form keeps one group per
    block whatever the key says (launch_ell: `if (!dot) grid = min(grid, resident)`), so its bits do not move either."""
    v, f = _vectors(8 * c + 1)
    want_r, want_x, want_q = _stored_row_results(c)
    assert np.array_equal(want_x, _single_sweeps(c, 1)) and np.array_equal(want_r, _single_residual(c))
    for middle in (True, False):
        with _poisson(c, dict(_CLASS_SLICES, cls_blocks_per_cu=blocks), middle) as h:
            assert 2 <= h.level_info(LV)["row_classes"] <= 64
            r = _residual(h, LV, v, f)
            x, ran = _smooth(h, LV, 1, v, f)
            h.set_vector(LV, "v", v)
            q = h.quadratic_form(LV, "v")
        assert ran == {"slice": (1, 1, 0)}, ran
        assert np.array_equal(r, want_r), (middle, _differ(r, want_r))
        assert np.array_equal(x, want_x), (middle, _differ(x, want_x))
        assert q == want_q, (middle, q, want_q)


# ---- 5. lds_pad -----------------------------------------------------------------------------------------------------------------------
LDS_PAD_MAX = 150 * 1024


@pytest.mark.gpu
@pytest.mark.parametrize("c,rows_per_lane", [(24, 1), (30, 2)], ids=["193-r1", "241-r2"])
def test_lds_pad_on_a_level_of_100000_slices(c, rows_per_lane):
    """The pad is dynamic LDS of sdia_apply / sdia_jacobi_finest on levels of at least 100000 slices that run without row
    classes: 193^3 is the smallest generator grid with that many slices of 64 rows ("rows_per_lane" 1), 241^3 the smallest with
    slices of 128 (the default).  A residual and two single sweeps, on the finest and on a middle level, with 0, the default,
    64 KiB and the largest pad accepted (above 48 KiB the launch sets the kernel's dynamic-LDS attribute first) have the bits
    of pad 0; a pad outside the range is refused by name and the handle goes on working."""
    from multigrid_dolfinx_amd._capi import MgError
    n1 = 8 * c + 1
    assert n1 ** 3 // (64 * rows_per_lane) >= 100000 > (n1 - 8) ** 3 // (64 * rows_per_lane)
    v, f = _vectors(n1)
    want = None
    for middle in (False, True):
        with _poisson(c, dict(_SINGLE, row_classes=0, rows_per_lane=rows_per_lane), middle) as h:
            assert h.level_info(LV)["row_classes"] == 0
            for pad in (0, 32768, 65536, LDS_PAD_MAX):
                h.set_tuning("lds_pad", pad)
                r = _residual(h, LV, v, f)
                x, ran = _smooth(h, LV, 2, v, f)
                assert ran == {"slice": (2, 2, 0)}, (pad, ran)
                if want is None:
                    assert np.all(np.isfinite(x)) and np.any(r != 0.0)
                    want = (r, x)
                assert np.array_equal(r, want[0]), (pad, middle, _differ(r, want[0]))
                assert np.array_equal(x, want[1]), (pad, middle, _differ(x, want[1]))
            for bad in (LDS_PAD_MAX + 1, 160 * 1024, -1):
                with pytest.raises(MgError, match="lds_pad must be in 0..%d" % LDS_PAD_MAX):
                    h.set_tuning("lds_pad", bad)
            x, ran = _smooth(h, LV, 2, v, f)                 # (the refused values changed nothing: still the largest pad)
            assert ran == {"slice": (2, 2, 0)} and np.array_equal(x, want[1])


@pytest.mark.gpu
def test_lds_pad_changes_nothing_on_a_small_level():
    """65^3 has 4291 slices: no pad whatever the key says."""
    c = 8
    v, f = _vectors(65)
    with _poisson(c, dict(_SINGLE, row_classes=0, lds_pad=LDS_PAD_MAX)) as h:
        assert h.level_info(LV)["row_classes"] == 0
        r = _residual(h, LV, v, f)
        x, ran = _smooth(h, LV, 2, v, f)
    assert ran == {"slice": (2, 2, 0)}, ran
    assert np.array_equal(r, _single_residual(c)) and np.array_equal(x, _single_sweeps(c, 2))


# ---- 6. experiment switches of the K-sweep march --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", [7, 15], ids=["57", "121"])
@pytest.mark.parametrize("k", [3, 4, 5])
@pytest.mark.parametrize("shape", [7, 8])
def test_march_with_nontemporal_stores(shape, k, c):
    """"fuse_k_nt_store" 1: two passes of K sweeps whose results are stored past the caches -- the bits of the same march with
    ordinary stores and of single sweeps."""
    v, f = _vectors(8 * c + 1)
    got = {}
    for nt in (1, 0):
        tuning = dict(_MARCH, fuse_k=k, fuse_k_shape=shape, fuse_k_nt_store=nt)
        with _poisson(c, tuning) as h:
            got[nt], ran = _smooth(h, LV, 2 * k, v, f)
        assert set(ran) == {"ksweep"} and ran["ksweep"][:2] == (2, 2 * k), (tuning, ran)
    assert np.array_equal(got[1], got[0]), _differ(got[1], got[0])
    assert np.array_equal(got[1], _single_sweeps(c, 2 * k)), _differ(got[1], _single_sweeps(c, 2 * k))


@pytest.mark.gpu
@pytest.mark.parametrize("c", [7, 13], ids=["57", "105"])
@pytest.mark.parametrize("k", [3, 4, 5])
def test_march_with_small_tiles(k, c):
    """"fuse_k_small_tiles" 1 with "fuse_k_shape" 1: planes with fewer 64 x 48 tiles than the GPU has CUs (57^3: 4, 105^3: 6 or 9)
    take the 64 x 24 tiles of shape 4 for three and four sweeps per pass; five sweeps keep shape 1.  The bits of the march
    with the switch off and of single sweeps."""
    v, f = _vectors(8 * c + 1)
    got = {}
    for small in (1, 0):
        tuning = dict(_MARCH, fuse_k=k, fuse_k_shape=1, fuse_k_small_tiles=small)
        with _poisson(c, tuning) as h:
            got[small], ran = _smooth(h, LV, 2 * k, v, f)
        assert set(ran) == {"ksweep"} and ran["ksweep"][:2] == (2, 2 * k), (tuning, ran)
    assert np.array_equal(got[1], got[0]), _differ(got[1], got[0])
    assert np.array_equal(got[1], _single_sweeps(c, 2 * k)), _differ(got[1], _single_sweeps(c, 2 * k))


@pytest.mark.gpu
def test_retired_march_shapes_and_knobs_are_refused():
    """The tile shapes 0, 2, 3, 5 and 6 of the K-sweep march and the keys "fuse_k_dpp" and "fuse_k_pf" were retired: the shapes
    are refused by that word, the keys are unknown, the shapes that exist are accepted, and the handle goes on working with
    the last accepted value.  One handle at 17^3; no kernel runs."""
    from multigrid_dolfinx_amd._capi import MgError
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    with DeviceHierarchy.synthetic(3, 1, 3, c=2) as h:
        for shape in (1, 4, 7, 8, 9, -1):
            h.set_tuning("fuse_k_shape", shape)
        for shape in (0, 2, 3, 5, 6):
            with pytest.raises(MgError, match="fuse_k_shape.*0, 2, 3, 5 and 6 were retired"):
                h.set_tuning("fuse_k_shape", shape)
        for shape in (-2, 10):
            with pytest.raises(MgError, match="fuse_k_shape must be 1, 4, 7, 8 or 9, or -1"):
                h.set_tuning("fuse_k_shape", shape)
        for key in ("fuse_k_dpp", "fuse_k_pf"):
            for value in (0, 1, 2):
                with pytest.raises(MgError, match="unknown tuning key " + key):
                    h.set_tuning(key, value)
        h.set_tuning("fuse_k_shape", 7)


# ---- 7. overlapped pair sweeps on slabs -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("form", [1, 0])
def test_overlapped_pair_sweeps_on_slabs(form, world):
    """129^3, 65^3 and 33^3 on two and three slabs, four plane segments per slab, the overlap on from the first row
    ("overlap_min_rows" 0), ranks as threads over the in-process RCCL stand-in: "slab_pair_form" 1 (the boundary segments of
    the pass first, then the interior segments beside the boundary chain) and 0 (one launch of the pass beside a chain that
    relaxes the boundary planes itself).  Both count three launches per pair -- the sequential form, two -- and give the
    single handle's bits (tests/fake_rccl_worker.py)."""
    lib = os.path.join(HERE, "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(HERE, "fake_rccl")], check=True)
    tune = "fuse_min_rows=0,fuse_segments=4,overlap_min_rows=0,slab_pair_form=%d" % form
    env = dict(os.environ, MG_RCCL_LIBRARY=lib, MG_TEST_TUNE=tune, MG_TEST_EXPECT_PAIR_LAUNCHES="3")
    out = subprocess.run([sys.executable, os.path.join(HERE, "fake_rccl_worker.py"), str(world), "3", "2", "4", "8", "2", "0", "1"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "OK" in out.stdout


# ---- 8. iterations enqueued between convergence checks of the coarsest-level PCG ---------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", [8, 16], ids=["9", "17"])
def test_pcg_chunk_does_not_change_the_coarse_solve(c):
    """mg_coarse_solve with "coarse_direct" 0 on a 9^3 (17^3) coarsest level and a random right-hand side: the device's `done`
    flag turns the iterations enqueued past convergence into no-ops, so the iteration count, the relative residual and the
    solution do not depend on the chunk -- nor on "pcg_predict", from which the second call of a handle starts."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    n = (c + 1) ** 3
    b = np.random.default_rng(80 + c).standard_normal(n)
    runs = {}
    for chunk in (1, 5, 16, 64):
        with DeviceHierarchy.synthetic(3, 0, 1, c=c, mu1=2, mu2=2, coarse_direct=0, pcg_chunk=chunk) as h:
            assert h.level_info(0)["n_global"] == n
            out = []
            for call in range(2):
                h.set_vector(0, "f", b)
                h.zero_vector(0, "v")
                iters, rel = h.coarse_solve()
                out.append((iters, rel, h.get_vector(0, "v")))
            runs[chunk] = out
    iters, rel, x = runs[16][0]
    print("coarsest level %d^3: %d iterations, relative residual %.3e" % (c + 1, iters, rel))
    assert iters > 16 and iters % 16 and 0.0 < rel <= 1e-14 and np.all(np.isfinite(x)), (iters, rel)
    for chunk, out in runs.items():
        for call, (i, r, y) in enumerate(out):
            assert (i, r) == (iters, rel), (chunk, call, i, r, iters, rel)
            assert np.array_equal(y, x), (chunk, call, _differ(y, x))


# ---- 9. the generator's odd rows --------------------------------------------------------------------------------------------------------
_ODD_C = 8                  # 65^3


def _integer_vector(n, seed):
    """Non-zero integers of magnitude 1 .. 8 with random signs: every entry of the generated levels is an integer multiple of
    2^-26 below 2^-2 (h = 2^-6, the diagonal 6 h (2^20 + m) / 2^20), so every product and every partial sum of A x is exact
    in float64 and (A' - A) x is the exact difference."""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 9, n) * rng.choice([-1, 1], n)).astype(np.float64)


def _generated_apply(odd, xs):
    """A x for each x of xs with the level generated under "gen_odd_rows" = odd, as plain stored rows ("row_escape" 0: more than
    255 distinct rows leave a level without classes): F = 0, the residual, negated.  Also the level's row classes."""
    out = []
    with _poisson(_ODD_C, dict(_SINGLE, row_escape=0, gen_odd_rows=odd)) as h:
        classes = h.level_info(LV)["row_classes"]
        for x in xs:
            h.zero_vector(LV, "f")
            h.set_vector(LV, "v", x)
            h.residual(LV)
            out.append(-h.get_vector(LV, "r").reshape(-1))
    return out, classes


@pytest.mark.gpu
def test_gen_odd_rows_perturbs_the_diagonal_of_one_interior_row_in_a_hundred():
    """include/mg_hip.h: "gen_odd_rows" gives this many of 10000 interior rows, picked by a hash of their grid index, a reaction
    term of their own on the diagonal, diag (1 + r) with 0 <= r < 1 -- rows unlike any other.  65^3 generated with 0 and with
    100, applied to two vectors of non-zero integers (all arithmetic exact, see _integer_vector), d = (A_100 - A_0) x:
      * d is exactly 0 on the Dirichlet rows;
      * delta_i = d_i / x_i is the same from both vectors to 8 eps |diag| (the change is on the diagonal only) and lies in
        [0, diag), diag = 6 h;
      * at least 99 % of the non-zero delta are distinct;
      * the number k of odd rows among the n = 63^3 interior ones is within six binomial standard deviations of n / 100,
        |k - n / 100| <= 6 sqrt(0.01 x 0.99 n) = 299;
      * a second handle gives the same bits; with 10000 every interior row is changed."""
    n1 = 8 * _ODD_C + 1
    n = n1 ** 3
    xs = [_integer_vector(n, 91), _integer_vector(n, 92)]
    (a0, b0), classes0 = _generated_apply(0, xs)
    (a1, b1), classes1 = _generated_apply(100, xs)
    (a2, b2), _ = _generated_apply(100, xs)
    (a3,), _ = _generated_apply(10000, xs[:1])
    assert 2 <= classes0 <= 64 and classes1 == 0, (classes0, classes1)
    assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
    idx = np.arange(n)
    i, j, k = idx % n1, (idx // n1) % n1, idx // (n1 * n1)
    interior = (i > 0) & (i < n1 - 1) & (j > 0) & (j < n1 - 1) & (k > 0) & (k < n1 - 1)
    diag = 6.0 / (n1 - 1)
    da, db = (a1 - a0) / xs[0], (b1 - b0) / xs[1]
    assert np.all(da[~interior] == 0.0) and np.all(db[~interior] == 0.0)
    assert np.all(np.abs(da - db) <= 8 * EPS * diag), float(np.abs(da - db).max())
    assert np.all(da >= 0.0) and np.all(da < diag), (float(da.min()), float(da.max()))
    odd = da[da != 0.0]
    count, nint = odd.size, int(interior.sum())
    distinct = np.unique(odd).size
    print("odd rows: %d of %d interior rows (%.4f %%), %d distinct values" % (count, nint, 100.0 * count / nint, distinct))
    assert nint == 63 ** 3
    assert abs(count - nint / 100) <= 6 * np.sqrt(nint * 0.01 * 0.99), (count, nint / 100)
    assert distinct >= 0.99 * count, (distinct, count)
    dall = (a3 - a0) / xs[0]
    assert np.all(dall[~interior] == 0.0) and np.all(dall[interior] > 0.0) and np.all(dall < diag)
    assert np.array_equal(dall[da != 0.0], odd)                 # (the rows picked at 100 keep their term at 10000)


@pytest.mark.gpu
def test_generated_odd_rows_take_the_escape_march():
    """What bench.py's `value_with_odd_rows` measures: the same level with "row_escape" 1 keeps its 255 classes (65^3 has
    2^16 rows and more, the size from which build_row_classes_q admits escape rows), runs the escape variant of the K-sweep
    march and gives the bits of single sweeps on the stored rows."""
    c, nw = _ODD_C, 5
    v, f = _vectors(8 * c + 1)
    with _poisson(c, dict(_SINGLE, row_escape=0, gen_odd_rows=100)) as h:
        want, ran = _smooth(h, LV, nw, v, f)
    assert ran == {"slice": (nw, nw, 0)}, ran
    for middle in (False, True):
        with _poisson(c, dict(_MARCH, fuse_k=5, row_escape=1, gen_odd_rows=100), middle) as h:
            info, st = h.level_info(LV), h.level_storage(LV)
            assert info["row_classes"] == 255 and st["distinct_rows"] > 255 and 2000 < st["escape_rows"] < 3100, (info, st)
            got, ran = _smooth(h, LV, nw, v, f)
        assert set(ran) == {"ksweep_escape"} and ran["ksweep_escape"][:2] == (1, nw), ran
        assert np.all(np.isfinite(want)) and np.array_equal(got, want), (middle, _differ(got, want))
