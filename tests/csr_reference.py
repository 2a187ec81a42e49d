"""Host restatement of what a CSR hand-off means, for tests/test_csr_handoff.py (test infrastructure, no GPU).

Everything here works from the raw triplet `(indptr, indices, data)` exactly as it is stored -- unsorted columns, explicit
zeros and duplicate entries included -- with SciPy's semantics (duplicates sum) and computes in `np.longdouble`:

  residual(A, v, f)            r = f - A v
  jacobi(A, v, f, w)           v + w D^-1 (f - A v), D the summed diagonal
  sweeps(A, v, f, w, n)        n such sweeps

Each also returns the per-row rounding bound a correct fp64 evaluation, in ANY order of summation and with or without
fused multiply-adds, stays within.  With eps = 2^-52 = twice the unit roundoff u, k_i the entries of row i that take part
(the stored ones; the non-zero ones if the hand-off prunes zeros) and S_i = |f_i| + sum_j |a_ij| |v_j|:

  residual   k_i products, k_i - 1 additions and one subtraction put at most k_i + 1 roundings on any term, so the error
             is at most ((1 + u)^(k_i + 1) - 1) S_i <= (k_i + 2) u S_i.  The bound is (k_i + 2) eps S_i, twice that.
  one sweep  delta_i = w dinv_i r_i adds three roundings (dinv_i = fl(1 / d_i) and two products): (k_i + 4) u |w dinv_i| S_i
             <= (k_i + 2) eps |w dinv_i| S_i for every k_i >= 0, and for k_i >= 1 a spare u |w dinv_i| S_i >= u |delta_i|.
             The last addition rounds by u |v_i + delta_i| <= u |v_i| + u |delta_i|.  The bound is the residual's bound times
             |w dinv_i|, plus 2 eps |v_i|.
  n sweeps   E_0 = 0, E_(t+1) = (one-sweep bound at the reference's own iterate v_t) + E_t + |w dinv| (|A| E_t): the error
             already there passes through the same sweep.

The transformers turn a canonical matrix into another CSR of the SAME matrix (SciPy matrices whose raw arrays are left
exactly as built: nothing here calls a SciPy method that would sort or sum them).
"""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
EPS = np.finfo(np.float64).eps


# ---- raw-triplet arithmetic ---------------------------------------------------------------------------------------
def _rows_of(A):
    return np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr))


def _row_sums(indptr, terms, n):
    """sum of `terms` over each row's stored entries (rows without entries: 0)."""
    out = np.zeros(n, dtype=terms.dtype)
    starts = np.asarray(indptr[:-1], dtype=np.int64)
    full = np.diff(indptr) > 0
    if full.any():
        out[full] = np.add.reduceat(terms, starts[full])
    return out


class Operator:
    """The raw triplet of `A` in longdouble, with what the bounds need.  `prune`: the hand-off drops stored zeros."""

    def __init__(self, A, prune=True):
        self.n = A.shape[0]
        self.indptr = np.asarray(A.indptr, dtype=np.int64)
        self.indices = np.asarray(A.indices, dtype=np.int64)
        self.data = np.asarray(A.data, dtype=LD)
        self.rows = _rows_of(A)
        kept = (A.data != 0.0) if prune else np.ones(A.data.size, dtype=bool)
        self.k = _row_sums(self.indptr, kept.astype(np.int64), self.n)
        self.diag = _row_sums(self.indptr, np.where(self.indices == self.rows, self.data, LD(0)), self.n)

    def matvec(self, x):
        return _row_sums(self.indptr, self.data * np.asarray(x, dtype=LD).ravel()[self.indices], self.n)

    def absmatvec(self, x):
        return _row_sums(self.indptr, np.abs(self.data) * np.abs(np.asarray(x, dtype=LD).ravel())[self.indices], self.n)

    def residual(self, v, f):
        v, f = np.asarray(v, dtype=LD).ravel(), np.asarray(f, dtype=LD).ravel()
        r = f - self.matvec(v)
        bound = (self.k + 2) * LD(EPS) * (np.abs(f) + self.absmatvec(v))
        return r, bound

    def jacobi(self, v, f, w):
        v = np.asarray(v, dtype=LD).ravel()
        r, rb = self.residual(v, f)
        scale = LD(w) / self.diag
        return v + scale * r, np.abs(scale) * rb + 2 * LD(EPS) * np.abs(v)

    def sweeps(self, v, f, w, n):
        """The iterate after each of n sweeps and the accumulated bound of each."""
        v = np.asarray(v, dtype=LD).ravel()
        scale = np.abs(LD(w) / self.diag)
        E = np.zeros(self.n, dtype=LD)
        iterates, bounds = [], []
        for _ in range(n):
            nxt, b = self.jacobi(v, f, w)
            E = b + E + scale * self.absmatvec(E)
            v = nxt
            iterates.append(v)
            bounds.append(E)
        return iterates, bounds


def residual(A, v, f, prune=True):
    return Operator(A, prune).residual(v, f)


def jacobi(A, v, f, w, prune=True):
    return Operator(A, prune).jacobi(v, f, w)


def sweeps(A, v, f, w, n, prune=True):
    return Operator(A, prune).sweeps(v, f, w, n)


# ---- SciPy matrices with raw arrays of our choosing -----------------------------------------------------------------
def raw_csr(data, indices, indptr, shape):
    """A csr_matrix holding exactly these arrays (SciPy's constructor would unify the index types)."""
    B = sp.csr_matrix(shape, dtype=np.float64)
    B.data = np.ascontiguousarray(data, dtype=np.float64)
    B.indices = np.ascontiguousarray(indices)
    B.indptr = np.ascontiguousarray(indptr)
    return B


def canonical(B):
    """A fresh SciPy copy of B in canonical form: duplicates summed, zeros dropped, columns sorted."""
    C = sp.csr_matrix((B.data.copy(), B.indices.astype(np.int64), B.indptr.astype(np.int64)), shape=B.shape)
    C.sum_duplicates()
    C.eliminate_zeros()
    return C


def same_matrix(B, A):
    """True if the raw arrays of B describe the matrix A, entry for entry and bit for bit."""
    D = canonical(B) - canonical(A)
    return D.nnz == 0 or abs(D).max() == 0.0


def kept_entries(B, prune):
    """SciPy's count of the entries a hand-off keeps."""
    return int(np.count_nonzero(B.data)) if prune else int(B.data.size)


def _reordered(A, order):
    return raw_csr(A.data[order], A.indices[order], A.indptr.copy(), A.shape)


def shuffle_columns(A, seed):
    """A random order within every row."""
    rng = np.random.default_rng(seed)
    return _reordered(A, np.lexsort((rng.random(A.data.size), _rows_of(A))))


def reverse_columns(A):
    return _reordered(A, np.lexsort((-np.arange(A.data.size), _rows_of(A))))


def with_int64_indptr(A):
    return raw_csr(A.data.copy(), A.indices.copy(), A.indptr.astype(np.int64), A.shape)


def _merged(A, rows_new, cols_new, vals_new, keys_new):
    """A with extra entries; an entry's key orders it among its row's stored entries, whose keys are their positions."""
    rows = np.concatenate([_rows_of(A), rows_new])
    keys = np.concatenate([np.arange(A.data.size, dtype=np.float64), keys_new])
    order = np.lexsort((keys, rows))
    indptr = np.zeros(A.shape[0] + 1, dtype=A.indptr.dtype)
    np.cumsum(np.bincount(rows, minlength=A.shape[0]), out=indptr[1:])
    return raw_csr(np.concatenate([A.data, vals_new])[order],
                   np.concatenate([A.indices, cols_new.astype(A.indices.dtype)])[order], indptr, A.shape)


def with_explicit_zeros(A, seed, in_reach=True, plane=None, fresh=True):
    """Extra stored 0.0 and -0.0 entries at random places of random rows: on offsets (column - row) that other rows use
    and, with `fresh`, on up to three offsets no row uses.  `in_reach`: every extra entry lies within `plane` of its row
    (one grid plane of a lexicographic level, which is as far as a slab's halo reaches)."""
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    rows = _rows_of(A)
    used = np.unique(A.indices.astype(np.int64) - rows)
    reach = int(plane) if in_reach else n - 1
    if in_reach and plane is None:
        raise ValueError("in_reach needs the size of a grid plane")
    stored = rows * n + A.indices.astype(np.int64)
    free = np.setdiff1d(np.arange(-reach, reach + 1), used)
    new_offsets = rng.choice(free, size=min(3, free.size), replace=False) if fresh else np.zeros(0, dtype=np.int64)
    picks = []
    for offsets, count in ((used[np.abs(used) <= reach], max(4, n // 8)), (new_offsets, max(3, n // 16))):
        if offsets.size == 0:
            continue
        r_all = np.repeat(np.arange(n, dtype=np.int64), offsets.size)
        c_all = r_all + np.tile(offsets.astype(np.int64), n)
        ok = (c_all >= 0) & (c_all < n)
        open_places = np.setdiff1d(r_all[ok] * n + c_all[ok], stored)
        picks.append(rng.choice(open_places, size=min(count, open_places.size), replace=False))
    picks = np.concatenate(picks) if picks else np.zeros(0, dtype=np.int64)
    if picks.size == 0:
        raise ValueError("no free position for an explicit zero")
    r_new, c_new = picks // n, picks % n
    v_new = np.where(np.arange(r_new.size) % 2 == 0, 0.0, -0.0)
    keys = rng.uniform(A.indptr[r_new] - 0.5, A.indptr[r_new + 1] - 0.5)
    return _merged(A, r_new, c_new, v_new, keys)


def split_entries(A, which):
    """Duplicates whose halves sum exactly: the chosen entries v become v/2 where they stand and v/2 at the end of their
    row.  `which`: "diagonal" (every diagonal entry), "offdiagonal" (every non-zero off-diagonal entry, so both halves of
    each symmetric pair) or "single" (one off-diagonal entry of the middle row)."""
    rows = _rows_of(A)
    on_diag = A.indices == rows
    if which == "diagonal":
        mask = on_diag & (A.data != 0.0)
    elif which == "offdiagonal":
        mask = ~on_diag & (A.data != 0.0)
    elif which == "single":
        cand = np.flatnonzero(~on_diag & (A.data != 0.0) & (rows >= A.shape[0] // 2))
        mask = np.zeros(A.data.size, dtype=bool)
        mask[cand[0]] = True
    else:
        raise ValueError(which)
    half = A.data[mask] / 2.0
    assert np.array_equal(half + half, A.data[mask])
    halved = raw_csr(np.where(mask, A.data / 2.0, A.data), A.indices.copy(), A.indptr.copy(), A.shape)
    return _merged(halved, rows[mask], A.indices[mask].astype(np.int64), half, A.indptr[rows[mask] + 1] - 0.5)


def first_duplicate(B):
    """(row, column) of the first repeated entry in stored order (what a one-pass check meets first), or None."""
    for r in range(B.shape[0]):
        seen = set()
        for c in B.indices[B.indptr[r]:B.indptr[r + 1]].tolist():
            if c in seen:
                return r, c
            seen.add(c)
    return None


def permute_dofs(A, numbering):
    """A lexicographic matrix in the DoF numbering `numbering[node] = dof`, every row's entries kept in their stored
    order (poisson.renumber sorts them).  Returns the matrix and `grid_index[dof] = node`."""
    n = A.shape[0]
    numbering = np.asarray(numbering, dtype=np.int64)
    grid_index = np.empty(n, dtype=np.int64)
    grid_index[numbering] = np.arange(n, dtype=np.int64)
    counts = np.diff(A.indptr)[grid_index]
    indptr = np.zeros(n + 1, dtype=A.indptr.dtype)
    np.cumsum(counts, out=indptr[1:])
    src = np.repeat(A.indptr[:-1][grid_index].astype(np.int64) - indptr[:-1].astype(np.int64), counts) + np.arange(A.data.size)
    return raw_csr(A.data[src], numbering[A.indices[src]].astype(A.indices.dtype), indptr, A.shape), grid_index


def scale_rows(A, s):
    """diag(s) A with the pattern of A (stored zeros stay stored)."""
    return raw_csr(A.data * np.asarray(s)[_rows_of(A)], A.indices.copy(), A.indptr.copy(), A.shape)
