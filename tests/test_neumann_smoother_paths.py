"""The multi-sweep smoother passes on levels generated with a face set (mg_set_diffusion_faces): nodes on the no-flux faces are
free rows with real couplings along the face, so the grid-boundary rows that every other bit-identity test sees as identity rows
are relaxed here.  What the passes lean on at the boundary -- the row-space wrap of the marches, the clamped cells of a tile, the
block pass's rim and its zero cells outside the grid, the step forms chosen from the class bytes of the ring planes, the escape
pool -- is checked by comparing every pass with single sweeps on such levels, bit for bit.

Inputs.  FACE_SETS: those of tests/diffusion_neumann_workers.py (1, 32, 12, 18, 63) and 21 (x-, y-, z- Dirichlet: the three "+"
faces and the corner (N, N, N) free) and 42 (the "+" faces Dirichlet: rows at i = 0, j = 0, k = 0 free, where row r - 1 of a
march is the live last node of the previous grid line).  Fields: `ones`; `jump` (jump_kappa); `lognormal` (every row distinct);
`patch` (ones with an 8 x 8 x 8 block of log-normal cells in the corner at (N, N, N): a few hundred rows unlike any other, on
free faces under the sets 21, 1 and 12).  Sizes: 9^3 and 17^3 (the one-launch smoother of small levels), 41^3 (the plane marches
need 32 x 32 planes; a partial tile in x and in y), 65^3 (a second tile column, several blocks of the block pass).

CPU, the premise (`test_levels_have_the_rows_the_paths_need`): for every face set and N = 16, 40 the host restatement has at most
64 distinct 7-entry rows for `ones` and `jump` (counted: 28 and 46 for all seven sets and both sizes) and more than 255 for
`patch` (539 to 756) and `lognormal` (thousands), the seven diagonals hold every entry of A, no entry couples a node to the last
node of the previous grid line or plane, and the `patch` rows that differ from the `ones` level include rows on a free face for
the sets 21, 1 and 12.  So `ones` and `jump` take the class-coded paths, `lognormal` the
plain ones and `patch` the escape pool.

One sweep (`test_one_sweep_against_long_double`): every set, field and N = 16, 40 against x + (omega / d)(f - sum_j a_j x_j)
evaluated in np.longdouble from the seven diagonals of poisson.diffusion_level(...).A.  Per row
    |got_i - want_i| <= 16 eps (|x_i| + (omega / |d_i|)(|f_i| + sum_j |a_ij x_j|)):
seven fused multiply-adds, one subtraction, one reciprocal, two products and one add are twelve roundings, each at most eps / 2
of a partial magnitude no larger than that sum (6 eps; 16 eps leaves room for the second-order terms and for the reference's own
rounding, 2^-64 per operation).  The plain float64 NumPy evaluation stays inside the same bound for these inputs (checked on the
CPU, `test_float64_evaluation_is_inside_the_one_sweep_bound`).  Which kernel: a default-tuned handle runs `slice` on every one
of these levels -- the one-sweep plane march (`sweep1c`) needs 32 x 32 planes and "march_min_rows" rows (4194304 by default) --,
as class-coded slices where the level has classes; at N = 40 a second handle with "march_min_rows" 0 runs `sweep1c` for `ones`
and `jump` and `slice` for `lognormal` and `patch`, by the launch counts.

Multi-sweep passes (`test_passes_are_bit_identical_to_single_sweeps`, `test_small_level_smoother_...`, `test_escape_rows_...`):
the reference handle runs one sweep per launch ("fuse_sweeps", "fuse_small", "fuse_block", "fuse_k" 0); every variant handle has
its size thresholds at 0 and runs nw = 2, 3, 5, 6, 9 sweeps from the same random v and f; np.array_equal with the reference, and
mg_smoother_launches says that the pass the variant pins ran and that the sweeps add up to nw (`_paths`, the rules of
tests/test_gpu_parity.py's `_paths_3d` with the block pass's default size window and the one-sweep march added).  Variants:
  default tuning                                    block (41^3 and 65^3 lie in its window); small at 9^3 and 17^3
  fuse_block 0                                      ksweep, five sweeps per pass in shape 8
  fuse_block 0, fuse_k 0 (and fuse_segments 3)      pair_class
  fuse_block 0, fuse_classes 0 (and on `lognormal`, with the plain tile shapes)   pair_plain
  fuse_block 0, fuse_sweeps 0                       sweep1c against the reference's slices
  fuse_k 3, 4, 5 x fuse_k_shape 8, 7 x fuse_k_segments 1, 3; fuse_k_tail 4 / 5; fuse_k 4 in fuse_k_shape 1     ksweep
  fuse_block 2 x fuse_block_k 2, 3, 4 x fuse_block_ez 11, 19                                     block
  `patch`, row_escape on                            ksweep_escape, the level keeping its 255 classes
each on the finest level of its handle and on a level that is not the finest (the marches have a kernel for either).  The full
list runs on the sets 21, 42 and 18 at 41^3 and 65^3, a short list (default, one K-sweep, one block) on the others at 41^3; the
small-level smoother, Jacobi and Chebyshev with caller-set bounds, on every set.

Whole cycles (`test_cycles_equal_single_sweep_cycles`): 65^3, four levels, P1 transfers, V(2,2) and V(3,2), sets 21, 42, 12,
`ones` and `jump`: three cycles of a default-tuned handle (block on 65^3 and 33^3, small on 17^3) and of the single-sweep handle,
eager and captured -- the iterate and the residual history byte for byte.  The solve (`test_pcg_on_class_levels_against_spsolve`):
mg_pcg at rtol 1e-10, `jump`, N = 32, four levels, sets 1 and 18, within cond(A) rtol of the sparse direct solve."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from multigrid_dolfinx_amd import poisson
from tests.diffusion_neumann_workers import FACE_SETS as NEUMANN_FACE_SETS, free_mask
from tests.diffusion_workers import jump_kappa, lognormal_kappa

EPS = np.finfo(np.float64).eps
OMEGA = 2.0 / 3.0

FACE_SETS = NEUMANN_FACE_SETS + (21, 42)
FULL_SETS = (21, 42, 18)                            # the whole variant list
SHORT_SETS = tuple(s for s in FACE_SETS if s not in FULL_SETS)
PATCH_ON_FREE_FACES = (21, 1, 12)
FIELDS = ("ones", "jump", "lognormal", "patch")
CLASS_FIELDS = ("ones", "jump")
SMALL_N, MARCH_N, BLOCK_N = (8, 16), 40, 64
SWEEPS = (2, 3, 5, 6, 9)

# one sweep per launch
REFERENCE = dict(fuse_sweeps=0, fuse_small=0, fuse_block=0, fuse_k=0)
# every pass whatever the level's size
THRESHOLDS = ("fuse_min_rows", "fuse_k_min_rows", "fuse_k4_min_rows", "fuse_k5_min_rows", "fuse_k_small_rows", "march_min_rows")

_NO_BLOCK = dict(fuse_block=0)
SHORT_VARIANTS = [dict(), dict(_NO_BLOCK), dict(fuse_block=2, fuse_block_k=3, fuse_block_ez=11)]
FULL_VARIANTS = SHORT_VARIANTS + [
    dict(_NO_BLOCK, fuse_k=0), dict(_NO_BLOCK, fuse_k=0, fuse_segments=3), dict(_NO_BLOCK, fuse_classes=0), dict(_NO_BLOCK, fuse_sweeps=0),
] + [dict(_NO_BLOCK, fuse_k=k, fuse_k_shape=shape, fuse_k_segments=seg) for k in (3, 4, 5) for shape in (8, 7) for seg in (1, 3)] + [
    dict(_NO_BLOCK, fuse_k=5, fuse_k_shape=8, fuse_k_tail=4), dict(_NO_BLOCK, fuse_k=4, fuse_k_shape=7, fuse_k_tail=5),
    dict(_NO_BLOCK, fuse_k=4, fuse_k_shape=1),
    dict(fuse_block=2), dict(fuse_block=2, fuse_block_k=2, fuse_block_ez=11), dict(fuse_block=2, fuse_block_k=4, fuse_block_ez=11),
    dict(fuse_block=2, fuse_block_k=2, fuse_block_ez=19), dict(fuse_block=2, fuse_block_k=3, fuse_block_ez=19),
    dict(fuse_block=2, fuse_block_k=4, fuse_block_ez=19)]
PLAIN_VARIANTS = [dict(), dict(fuse_classes=0), dict(fuse_classes=0, fuse_plain_shape=1), dict(fuse_classes=0, fuse_plain_shape=2, fuse_segments=3),
                  dict(fuse_classes=0, fuse_plain=1), dict(fuse_classes=0, fuse_segments=5, fuse_nontemporal=1)]
ESCAPE_VARIANTS = [dict(), dict(fuse_k=3), dict(fuse_k=4, fuse_k_segments=3)]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kappa(field, N):
    if field == "ones":
        return np.ones(N ** 3)
    if field == "jump":
        return jump_kappa(N, 3)
    if field == "lognormal":
        return lognormal_kappa(N, 3, seed=3)
    k = np.ones((N, N, N))                              # [z, y, x] cells
    w = min(8, N)
    k[N - w:, N - w:, N - w:] = lognormal_kappa(w, 3, seed=3).reshape(w, w, w)
    return k.reshape(-1)


def _offsets(N):
    n1 = N + 1
    return (-n1 * n1, -n1, -1, 0, 1, n1, n1 * n1)       # the order in which the kernels sum a row


@functools.lru_cache(maxsize=4)
def _diagonals(N, faces, field):
    """(7, n): entry a[r, r + offset] of the host restatement per row, zero where the column is outside the matrix -- and, as the
    level stores it, where row r + offset is no grid neighbour (the last node of the previous grid line for offset -1 at i = 0);
    checked to hold every entry of A."""
    A = poisson.diffusion_level(N, 3, _kappa(field, N), dirichlet_faces=faces).A.tocsr()
    n = A.shape[0]
    rows = np.zeros((7, n))
    for t, off in enumerate(_offsets(N)):
        d = A.diagonal(off)
        rows[t, max(0, -off):max(0, -off) + d.size] = d
    back = sp.diags([rows[t, max(0, -off):n - max(0, off)] for t, off in enumerate(_offsets(N))], _offsets(N), shape=(n, n), format="csr")
    assert (back != A).nnz == 0
    return rows


def _neighbours(N, x, dtype):
    """(7, n): x[r + offset] per row in ROW space (zero outside the vector): what a march reads, wrap included."""
    n1 = N + 1
    P = n1 * n1
    xp = np.concatenate([np.zeros(P, dtype=dtype), np.asarray(x, dtype=dtype), np.zeros(P, dtype=dtype)])
    return np.stack([xp[P + off:P + off + x.size] for off in _offsets(N)])


def _sweep(N, rows, x, f, dtype):
    """One weighted-Jacobi sweep from the seven diagonals in `dtype`, and the per-row magnitude the bound is taken on."""
    a, xs = rows.astype(dtype), _neighbours(N, x, dtype)
    x, f, d = np.asarray(x, dtype=dtype), np.asarray(f, dtype=dtype), a[3]
    acc = np.zeros(x.size, dtype=dtype)
    for t in range(7):
        acc = acc + a[t] * xs[t]
    out = x + (dtype(OMEGA) * (dtype(1.0) / d)) * (f - acc)
    size = np.abs(x) + (OMEGA / np.abs(d)) * (np.abs(f) + np.abs(a * xs).sum(axis=0))
    return out, size.astype(np.float64)


def _one_sweep_inputs(N):
    rng = np.random.default_rng(100 + N)
    n = (N + 1) ** 3
    return rng.standard_normal(n), rng.standard_normal(n)


def _one_sweep_reference(N, faces, field):
    """(longdouble result, 16 eps x the per-row magnitude) of one sweep on _one_sweep_inputs(N)."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is no wider than float64 here: no high-precision reference"
    v, f = _one_sweep_inputs(N)
    want, size = _sweep(N, _diagonals(N, faces, field), v, f, np.longdouble)
    return want, 16 * EPS * size


# ---- host: the premise ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, MARCH_N])
@pytest.mark.parametrize("faces", FACE_SETS)
def test_levels_have_the_rows_the_paths_need(faces, N):
    n1 = N + 1
    count = {}
    for field in FIELDS:
        rows = _diagonals(N, faces, field)
        count[field] = np.unique(rows.T, axis=0).shape[0]
    print("faces", faces, "N", N, "distinct rows", count)
    assert count["ones"] <= 64 and count["jump"] <= 64, count
    assert count["patch"] > 255 and count["lognormal"] > 255, count
    free = free_mask(N, faces)
    # free rows on the grid boundary exist for every set but 63, with couplings along the face
    idx = np.arange(n1 ** 3)
    i, j, k = idx % n1, (idx // n1) % n1, idx // (n1 * n1)
    on_boundary = (i == 0) | (i == N) | (j == 0) | (j == N) | (k == 0) | (k == N)
    ones = _diagonals(N, faces, "ones")
    live = free & on_boundary
    assert live.any() == (faces != 63)
    assert np.all((ones[:3, live] != 0.0).sum(axis=0) + (ones[4:, live] != 0.0).sum(axis=0) >= 3)
    # the row-space wrap: no entry couples a node to the last node of the previous grid line or plane (what the marches and
    # the block pass's admission rely on)
    for rows in (ones, _diagonals(N, faces, "lognormal")):
        assert not rows[2, i == 0].any() and not rows[4, i == N].any()
        assert not rows[1, j == 0].any() and not rows[5, j == N].any()
        assert not rows[0, k == 0].any() and not rows[6, k == N].any()
    if faces == 42:
        assert live[i == 0].any() and live[j == 0].any() and live[k == 0].any()
    if not faces & 3:                                   # x- and x+ free: row r - 1 of a free node at i = 0 is a free node too
        assert live[(idx - 1)[(i == 0) & (idx > 0) & live]].any()
    odd = np.any(_diagonals(N, faces, "patch") != ones, axis=0)
    assert 255 < odd.sum() <= 9 ** 3
    if faces in PATCH_ON_FREE_FACES:
        assert (odd & live).sum() >= 81, (odd & live).sum()


@pytest.mark.parametrize("N", [16, MARCH_N])
@pytest.mark.parametrize("faces", FACE_SETS)
def test_float64_evaluation_is_inside_the_one_sweep_bound(faces, N):
    """The bound of the one-sweep test is wide enough for a correct float64 evaluation (and the reference is no float64 one)."""
    v, f = _one_sweep_inputs(N)
    for field in FIELDS:
        want, bound = _one_sweep_reference(N, faces, field)
        got, _ = _sweep(N, _diagonals(N, faces, field), v, f, np.float64)
        err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
        assert err.max() > 0.0
        print("faces", faces, field, "N", N, "largest error / bound %.3f" % (err / bound).max())
        assert np.all(err <= bound)


# ---- device -----------------------------------------------------------------------------------------------------------------------
def _fits_one_cu(n_side):
    """small_level_ok's size test (3-D): at most 16384 rows, and x, the result and the class table in 150 KiB of LDS"""
    rows, pad = n_side ** 3, n_side ** 2
    return rows <= 16384 and 256 * 8 * 8 + 2 * (rows + 2 * pad) * 8 <= 150 * 1024


def _paths(kw, n_side, nw, classes):
    """The smoother paths a variant may take on a whole 3-D level of n_side^3 rows with every size threshold at zero -- the rules
    of tests/test_gpu_parity.py's _paths_3d, with the block pass's default window of 2^15 <= rows < 2^23, the one-sweep march
    (a single sweep is `sweep1c` on a level with classes and 32 x 32 planes, else `slice`) and levels without classes --, and the
    one among them that must run (None: any of them)."""
    rows = n_side ** 3
    cls = bool(classes and kw.get("fuse_classes", 1))
    single = "sweep1c" if classes and n_side >= 32 else "slice"
    if nw >= 2 and cls and kw.get("fuse_small", 1) and _fits_one_cu(n_side):
        return {"small"}, "small"
    block = kw.get("fuse_block", 1)
    if nw >= 2 and cls and n_side >= 8 and (block >= 2 or (block == 1 and (1 << 15) <= rows < (1 << 23))):
        return {"block", single}, "block"
    if n_side < 32 or not kw.get("fuse_sweeps", 1) or nw < 2:                  # (the pair and K-sweep passes: 32 x 32 planes)
        return {single}, single
    pair = "pair_class" if cls else "pair_plain"
    if cls and kw.get("fuse_k", 5) >= 3 and nw >= 3 and not (kw.get("fuse_k", 5) == 3 and nw == 4):
        return {"ksweep", pair}, "ksweep"                                       # (no single sweep is left over: 5 = 3 + 2)
    return {pair, single}, pair


def _handle(N, faces, kappa, tuning, finest=True, reference=False, **make):
    """A handle whose level 1 is the level of N^3 cells generated with the face set, the finest of two levels or the middle one
    of three (the third never set)."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    h = DeviceHierarchy(3, 0, 1 if finest else 2, c=N // 2, **make)
    if not reference:
        for key in THRESHOLDS:
            h.set_tuning(key, 0)
    for key, value in tuning.items():
        h.set_tuning(key, value)
    h.set_diffusion_faces(faces)
    h.set_params(2, 2, OMEGA)
    h.gen_diffusion_hierarchy(kappa, top_level=1)
    assert h.diffusion_faces() == faces and h.level_info(1)["n_global"] == (N + 1) ** 3
    return h


def _smooths(h, v, f, sweeps=SWEEPS):
    out = {}
    for nw in sweeps:
        h.set_vector(1, "v", v)
        h.set_vector(1, "f", f)
        h.reset_smoother_launches()
        h.smooth(1, nw)
        out[nw] = (h.get_vector(1, "v"), h.smoother_launches(1))
    return out


def _reference_smooths(N, faces, kappa, v, f, **make):
    """One sweep per launch on the finest and on a middle level: slices only, the same bits on both."""
    want = None
    for finest in (True, False):
        with _handle(N, faces, kappa, REFERENCE, finest, reference=True, **make) as h:
            got = _smooths(h, v, f)
        for nw, (x, ran) in got.items():
            assert ran == {"slice": (nw, nw, 0)}, (nw, ran)
            assert np.all(np.isfinite(x))
            assert want is None or np.array_equal(x, want[nw][0]), nw
        want = want or got
    return {nw: x for nw, (x, _) in want.items()}


def _check(kw, got, want, allowed_must, where):
    for nw, (x, ran) in got.items():
        allowed, must = allowed_must(nw)
        assert sum(s for _, s, _ in ran.values()) == nw, (where, kw, nw, ran)
        assert set(ran) <= allowed and (must is None or must in ran), (where, kw, nw, ran)
        diff = np.flatnonzero(x.reshape(-1) != want[nw].reshape(-1))
        assert np.array_equal(x, want[nw]), (where, kw, nw, ran, "rows that differ:", diff.size, "the first:", diff[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("N", [16, MARCH_N])
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("faces", FACE_SETS)
def test_one_sweep_against_long_double(faces, field, N):
    """One weighted-Jacobi sweep of a generated level against the np.longdouble restatement, per row within 16 eps (|x_i| +
    (omega / |d_i|)(|f_i| + sum_j |a_ij x_j|)) -- twelve roundings of at most eps / 2 of that magnitude each; the float64 NumPy
    evaluation stays inside the same bound (test_float64_evaluation_is_inside_the_one_sweep_bound).  A default-tuned handle
    runs `slice` at these sizes (class-coded where the level has classes: the one-sweep plane march needs 32 x 32 planes and
    "march_min_rows" = 2^22 rows); at N = 40 a handle with "march_min_rows" 0 runs `sweep1c` for `ones` and `jump`."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    want, bound = _one_sweep_reference(N, faces, field)
    v, f = _one_sweep_inputs(N)
    classes = field in CLASS_FIELDS
    runs = [(dict(), "slice")]
    if N >= 32:
        runs.append((dict(march_min_rows=0), "sweep1c" if classes else "slice"))
    for tuning, path in runs:
        with DeviceHierarchy(3, 0, 1, c=N // 2, **tuning) as h:
            h.set_diffusion_faces(faces)
            h.set_params(2, 2, OMEGA)
            h.gen_diffusion_level(1, _kappa(field, N))
            info = h.level_info(1)
            assert (2 <= info["row_classes"] <= 64) if classes else info["row_classes"] in (0, 255), info
            h.set_vector(1, "v", v)
            h.set_vector(1, "f", f)
            h.reset_smoother_launches()
            h.smooth(1, 1)
            got = h.get_vector(1, "v").reshape(-1)
            ran = h.smoother_launches(1)
        assert ran == {path: (1, 1, 0)}, (tuning, ran)
        err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
        worst = int(np.argmax(err / bound))
        print("faces", faces, field, "N", N, path, "largest error / bound %.3f at row %d" % ((err / bound)[worst], worst))
        assert np.all(err <= bound), (tuning, worst, err[worst], bound[worst])


def _march_cases():
    cases = []
    for faces in FACE_SETS:
        full = faces in FULL_SETS
        for field in CLASS_FIELDS:
            for N in (MARCH_N, BLOCK_N) if full else (MARCH_N,):
                cases.append((faces, field, N))
        if full:
            cases.append((faces, "lognormal", MARCH_N))
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("faces,field,N", _march_cases())
def test_passes_are_bit_identical_to_single_sweeps(faces, field, N):
    """The block pass, the K-sweep march, the class-coded and plain pair passes and the one-sweep march against one sweep per
    launch on a level whose free boundary rows are relaxed (the module docstring lists the variants and what each pins): the
    same bits for 2, 3, 5, 6 and 9 sweeps, on the finest level of a handle and on one that is not; the launch counts name the
    pass that ran and add up to the sweeps asked for."""
    kappa = _kappa(field, N)
    classes = field in CLASS_FIELDS
    rng = np.random.default_rng(1000 * faces + N)
    n = (N + 1) ** 3
    v, f = rng.standard_normal(n), rng.standard_normal(n)
    want = _reference_smooths(N, faces, kappa, v, f)
    variants = PLAIN_VARIANTS if not classes else FULL_VARIANTS if faces in FULL_SETS else SHORT_VARIANTS
    seen = set()
    for kw in variants:
        for finest in (True, False):
            with _handle(N, faces, kappa, kw, finest) as h:
                info = h.level_info(1)
                assert info["symmetric_diagonals"] == 4, info
                assert (2 <= info["row_classes"] <= 64) if classes else info["row_classes"] == 0, info
                got = _smooths(h, v, f)
            _check(kw, got, want, lambda nw: _paths(kw, N + 1, nw, classes), (faces, field, N, "finest" if finest else "middle"))
            seen |= set().union(*(set(ran) for _, ran in got.values()))
    if not classes:
        assert seen == {"pair_plain", "slice"}, seen
    elif faces in FULL_SETS:
        assert seen == {"block", "ksweep", "pair_class", "pair_plain", "sweep1c"}, seen
    else:
        assert seen == {"block", "ksweep", "pair_class"}, seen


@pytest.mark.gpu
@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
@pytest.mark.parametrize("N", SMALL_N)
@pytest.mark.parametrize("faces", FACE_SETS)
def test_small_level_smoother_is_bit_identical_to_single_sweeps(faces, N, smoother):
    """9^3 and 17^3 levels with a face set: all sweeps (all Chebyshev steps, caller-set bounds) of a call in one launch of one
    workgroup against one per launch, `ones` and `jump`."""
    rng = np.random.default_rng(10 * faces + N)
    n = (N + 1) ** 3
    v, f = rng.standard_normal(n), rng.standard_normal(n)
    for field in CLASS_FIELDS:
        out = []
        for kw, reference in ((REFERENCE, True), (dict(), False)):
            with _handle(N, faces, _kappa(field, N), kw, reference=reference) as h:
                assert 2 <= h.level_info(1)["row_classes"] <= 64
                h.set_params(2, 2, OMEGA, smoother=smoother)
                h.set_chebyshev_bounds(1, 0.33, 2.05)
                out.append(_smooths(h, v, f))
        for nw in SWEEPS:
            (a, ra), (b, rb) = out[0][nw], out[1][nw]
            assert ra == {"slice": (nw, nw, 0)} and rb == {"small": (1, nw, 0)}, (field, nw, ra, rb)
            assert np.all(np.isfinite(a))
            assert np.array_equal(a, b), (field, nw, np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("faces,N", [(s, MARCH_N) for s in FACE_SETS] + [(21, BLOCK_N), (42, BLOCK_N)])
def test_escape_rows_on_free_faces_keep_the_class_path(faces, N):
    """`patch`: more than 255 distinct rows, a few hundred of them unlike any other and (sets 21, 1, 12) on free faces.  With
    "row_escape" the level keeps its 255 classes, the odd rows come from the stored matrix through the march's pool, and the
    escape variant of the K-sweep march runs -- the bits of single sweeps on the stored rows ("row_escape" 0)."""
    kappa = _kappa("patch", N)
    rng = np.random.default_rng(2000 * faces + N)
    n = (N + 1) ** 3
    v, f = rng.standard_normal(n), rng.standard_normal(n)
    want = _reference_smooths(N, faces, kappa, v, f, row_escape=0)
    for kw in ESCAPE_VARIANTS:
        for finest in (True, False):
            with _handle(N, faces, kappa, kw, finest, row_escape=1) as h:
                info, st = h.level_info(1), h.level_storage(1)
                assert info["symmetric_diagonals"] == 4 and st["distinct_rows"] > 255, (info, st)
                assert info["row_classes"] == 255 and 0 < st["escape_rows"] <= 9 ** 3 + 64, (info, st)
                got = _smooths(h, v, f)

            def allowed_must(nw):
                return {"ksweep_escape", "pair_plain", "slice"}, "ksweep_escape" if nw >= 3 else "pair_plain"
            _check(kw, got, want, allowed_must, (faces, N, "finest" if finest else "middle"))


# ---- whole cycles and the solve ---------------------------------------------------------------------------------------------------
def _cycle_handle(N, top, faces, kappa, mu, tuning):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    h = DeviceHierarchy(3, 0, top, c=N >> top, **tuning)
    h.set_diffusion_faces(faces)
    h.set_params(mu[0], mu[1], OMEGA, restriction="p1_transpose")
    h.set_prolongation("p1")
    h.gen_diffusion_hierarchy(kappa)
    return h


def _first_differing_vector(N, top, faces, kappa, mu):
    """Where a default-tuned cycle leaves the single-sweep one: both handles in lockstep, eager, one operation of the first
    cycle's descent at a time, every vector of the level compared after each -- (level, operation, vector, first row)."""
    with _cycle_handle(N, top, faces, kappa, mu, dict(graph=0)) as a, _cycle_handle(N, top, faces, kappa, mu, dict(REFERENCE, graph=0)) as b:
        for h in (a, b):
            h.zero_vector(top, "v")
        for level in range(top, 0, -1):
            for name, op in (("smooth", lambda h: h.smooth(level, mu[0])), ("residual", lambda h: h.residual(level)),
                             ("restrict", lambda h: (h.restrict(level, "p1_transpose"), h.zero_vector(level - 1, "v")))):
                for h in (a, b):
                    op(h)
                for l, which in ((level, "v"), (level, "r"), (level - 1, "f")):
                    x, y = a.get_vector(l, which).reshape(-1), b.get_vector(l, which).reshape(-1)
                    if not np.array_equal(x, y):
                        return level, name, (l, which), int(np.flatnonzero(x != y)[0])
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("field", CLASS_FIELDS)
@pytest.mark.parametrize("faces", [21, 42, 12])
def test_cycles_equal_single_sweep_cycles(faces, field):
    """Three V(2,2) and V(3,2) cycles on 65^3 .. 9^3 with the P1 transfers: a default-tuned handle (the block pass on 65^3 and
    33^3, the small-level smoother on 17^3) against one sweep per launch, eager and captured.  Only the smoother differs and
    every pass claims bit identity: the iterate and the residual history are equal byte for byte."""
    N, top = BLOCK_N, 3
    kappa = _kappa(field, N)
    for mu in ((2, 2), (3, 2)):
        runs = {}
        for name, tuning in (("single", REFERENCE), ("default", dict())):
            for graph in (0, 1):
                with _cycle_handle(N, top, faces, kappa, mu, dict(tuning, graph=graph)) as h:
                    h.zero_vector(top, "v")
                    h.reset_smoother_launches()
                    hist = h.vcycle(top, 3, residuals=True)
                    runs[name, graph] = (hist.copy(), h.get_vector(top, "v"), [h.smoother_launches(l) for l in range(top + 1)],
                                         h.counters())
        for (name, graph), (hist, x, ran, counters) in runs.items():
            assert np.all(np.isfinite(x)) and hist[2] < hist[0], (name, graph, hist)
            assert graph or counters["graph_replays"] == 0, (name, graph, counters)
            if name == "single":
                assert all(set(r) <= {"slice"} for r in ran), ran
            else:
                assert "block" in ran[3] and "block" in ran[2] and set(ran[1]) == {"small"}, ran
        print("faces", faces, field, "V(%d,%d)" % mu, "residuals", runs["single", 0][0])
        want = runs["single", 0]
        for key, got in runs.items():
            same = got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
            assert same, (key, mu, got[0], want[0], "first differing vector (level, operation, vector, row):",
                          _first_differing_vector(N, top, faces, kappa, mu))


@functools.lru_cache(maxsize=None)
def _host_solution(N, faces, field):
    """tests/test_diffusion_neumann.py's _host_solution for the fields of this module: (A^-1 b, cond(A)) of the restated level
    from one SuperLU factorisation, which also serves Lanczos as the shift-invert operator for lambda_min; lambda_max by
    Lanczos on A.  The level is symmetric positive definite, identity rows included."""
    host = poisson.diffusion_level(N, 3, _kappa(field, N), dirichlet_faces=faces)
    A = host.A.tocsc()
    A.eliminate_zeros()
    lu = spl.splu(A, permc_spec="MMD_AT_PLUS_A")
    lo = spl.eigsh(A, k=1, sigma=0.0, which="LM", return_eigenvectors=False, OPinv=spl.LinearOperator(A.shape, matvec=lu.solve))[0]
    hi = spl.eigsh(A, k=1, which="LA", return_eigenvectors=False)[0]
    return host.b.copy(), lu.solve(host.b.reshape(-1)), float(hi / lo)


@pytest.mark.gpu
@pytest.mark.parametrize("faces", [1, 18])
def test_pcg_on_class_levels_against_spsolve(faces):
    """mg_pcg on a default-tuned hierarchy of `jump` levels (row classes on every level: tests/test_diffusion_neumann.py's solve
    has log-normal kappa, which has none), N = 32, four levels: rtol 1e-10 within 200 iterations, and the solution within
    cond(A) rtol of the sparse direct solve of the restated level in relative l2 -- a relative residual rtol bounds the relative
    error by cond(A) rtol --, cond computed on the host for this level.  The iteration count is printed."""
    N, top, rtol = 32, 3, 1e-10
    b, want, cond = _host_solution(N, faces, "jump")
    with _cycle_handle(N, top, faces, _kappa("jump", N), (2, 2), dict()) as h:
        assert all(2 <= h.level_info(l)["row_classes"] <= 64 for l in range(1, top + 1))
        assert h.get_vector(top, "f").tobytes() == b.tobytes()
        h.zero_vector(top, "v")
        h.reset_smoother_launches()
        hist = h.pcg(rtol=rtol, max_iter=200, level=top)
        x = h.get_vector(top, "v").reshape(-1)
        ran = [h.smoother_launches(l) for l in range(top + 1)]
    assert len(hist) < 200 and hist[-1] <= rtol * np.linalg.norm(b)
    assert "block" in ran[3] and set(ran[2]) == {"small"}, ran
    err = np.linalg.norm(x - want) / np.linalg.norm(want)
    print("faces", faces, "jump N", N, "iterations", len(hist), "cond %.3e" % cond, "rel l2 error %.3e" % err)
    assert err <= cond * rtol
