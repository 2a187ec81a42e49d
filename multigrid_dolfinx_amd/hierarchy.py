"""Device-resident multigrid hierarchy: a thin object wrapper over the C ABI.

The reference keeps its hierarchy in sixteen module globals (`multigrid.py:10-45`);
here it is one explicit handle per hierarchy.  All arithmetic happens in
`libmg_hip.so`; this module only marshals NumPy / SciPy buffers across ctypes.
Levels are addressed by the reference's integer level keys
(`coarsest_level .. finest_level`, `N_l = c * 2**l`).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import scipy.sparse as sp

from . import _capi
from ._capi import (MG_RESTRICT_FULL_WEIGHTING, MG_RESTRICT_INJECTION, MG_VEC_ERR, MG_VEC_F, MG_VEC_R,
                    MG_VEC_V, check, load, ptr)
from . import poisson
from .poisson import face_set, grid_index_from_coords

__all__ = ["DeviceHierarchy", "PointSet", "jacobi_split", "csr_check"]

# lower_ratio of the Chebyshev interval by default (include/mg_hip.h, mg_set_chebyshev)
CHEB_LOWER_RATIO = 6.0

_VEC = {"v": MG_VEC_V, "f": MG_VEC_F, "r": MG_VEC_R, "err": MG_VEC_ERR}
_RESTRICT = {"direct": MG_RESTRICT_INJECTION, "injection": MG_RESTRICT_INJECTION,
             "full_weighting": MG_RESTRICT_FULL_WEIGHTING, "table": _capi.MG_RESTRICT_TABLE,
             "p1_transpose": _capi.MG_RESTRICT_P1_TRANSPOSE}
_NODE_SETS = {"interior": _capi.MG_NODES_INTERIOR, "all": _capi.MG_NODES_ALL}


def _csr_arrays(A):
    if not sp.isspmatrix_csr(A):
        raise TypeError("the stiffness matrix must be a scipy.sparse.csr_matrix (Multigrid_prototype.py:96)")
    if np.iscomplexobj(A.data):
        raise TypeError("complex scalars are not supported (real fp64 only)")
    data = np.ascontiguousarray(A.data, dtype=np.float64)
    indices = np.asarray(A.indices)
    if indices.dtype != np.int32 and indices.size:
        # (a 64-bit-index PETSc build delivers int64: narrowing must not wrap)
        lo, hi = int(indices.min()), int(indices.max())
        if lo < np.iinfo(np.int32).min or hi > np.iinfo(np.int32).max:
            raise ValueError(f"column indices {lo}..{hi} do not fit the library's int32 column indices")
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    if A.indptr.dtype == np.int64:
        indptr, is64 = np.ascontiguousarray(A.indptr), 1
    else:
        indptr, is64 = np.ascontiguousarray(A.indptr, dtype=np.int32), 0
    return indptr, is64, indices, data


def csr_check(A, allow_duplicates=False):
    """The structural check every CSR hand-off starts with (`mg_csr_check`; host only, no device needed): raises
    `MgError` naming the cause -- row pointers that do not start at 0, decrease or do not end at nnz, a column index
    outside the matrix and, unless `allow_duplicates`, a (row, column) pair stored twice."""
    indptr, is64, indices, data = _csr_arrays(A)
    check(load().mg_csr_check(A.shape[0], A.shape[1], data.size, ptr(indptr), is64, ptr(indices),
                              1 if allow_duplicates else 0))


def jacobi_split(A, device=0):
    """`getJacobiMatrices` arithmetic on the GPU (`multigrid.py:48-56`).

    Returns `(DinvR csr, Dinv dia)` with the structure SciPy gives the reference:
    explicit zeros and the diagonal dropped, each row's entries in reversed order
    (`csr_matmat`), int32 indices, `has_sorted_indices == False`.
    """
    lib = load()
    indptr, is64, indices, data = _csr_arrays(A)
    n, nnz = A.shape[0], data.size
    dinv = np.empty(n)
    scaled = np.empty(nnz)
    keep = np.empty(nnz, dtype=np.uint8)
    check(lib.mg_jacobi_split(device, n, nnz, ptr(indptr), is64, ptr(indices), ptr(data), ptr(dinv),
                              ptr(scaled), ptr(keep)))
    keep = keep.astype(bool)
    rows = np.repeat(np.arange(n), np.diff(indptr))[keep]
    counts = np.bincount(rows, minlength=n)
    new_ptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(counts, out=new_ptr[1:])
    kept = int(new_ptr[-1])
    rank = np.arange(kept) - new_ptr[:-1][rows]
    dest = new_ptr[1:][rows] - 1 - rank                      # reversed inside every row
    out_idx = np.empty(kept, dtype=np.int32)
    out_val = np.empty(kept)
    out_idx[dest] = indices[keep]
    out_val[dest] = scaled[keep]
    R = sp.csr_matrix((out_val, out_idx, new_ptr), shape=A.shape)
    R.has_sorted_indices = False
    return R, sp.diags(dinv, 0)


class _DeviceArray:
    """A device buffer of float64 for `diffusion_dkappa` and `refresh_diffusion_hierarchy` fed NumPy arrays (tests): the HIP runtime is reached through
    libmg_hip.so, which links it, so nothing else has to be found or imported."""

    def __init__(self, lib, device: int, n: int, host: Optional[np.ndarray] = None):
        self._lib, self.n, self.ptr = lib, int(n), C.c_void_p()
        for name, args in (("hipSetDevice", [C.c_int]), ("hipMalloc", [C.POINTER(C.c_void_p), C.c_size_t]), ("hipFree", [C.c_void_p]),
                           ("hipMemcpy", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int])):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, C.c_int
        self._hip(lib.hipSetDevice(int(device)), "hipSetDevice")
        self._hip(lib.hipMalloc(C.byref(self.ptr), max(8, 8 * self.n)), "hipMalloc")
        if host is not None:
            self._hip(lib.hipMemcpy(self.ptr, ptr(host), 8 * self.n, 1), "hipMemcpy")     # hipMemcpyHostToDevice

    @staticmethod
    def _hip(status, what):
        if status != 0:
            raise _capi.MgError(f"{what} failed with HIP error {status}")

    def download(self) -> np.ndarray:
        out = np.empty(self.n)
        self._hip(self._lib.hipMemcpy(ptr(out), self.ptr, 8 * self.n, 2), "hipMemcpy")    # hipMemcpyDeviceToHost
        return out

    def free(self):
        if self.ptr:
            self._lib.hipFree(self.ptr)
            self.ptr = C.c_void_p()


class DeviceHierarchy:
    """One multigrid hierarchy resident on one MI355X (or one slab of it per rank)."""

    def __init__(self, dim: int, coarsest_level: int, finest_level: int, c: int = 8, device: int = 0,
                 rows_per_lane: Optional[int] = None, xcd_chunk: Optional[int] = None,
                 offset_codes: Optional[int] = None, strip_slices: Optional[int] = None,
                 nontemporal: Optional[int] = None, coarse_direct: Optional[int] = None,
                 symmetric_storage: Optional[int] = None, graph: Optional[int] = None,
                 lds_pad: Optional[int] = None, **more_tuning):
        self._lib = load()
        self.dim = dim
        self.c = c
        self.coarsest_level = coarsest_level
        self.finest_level = finest_level
        self.device = device
        self._h = C.c_void_p()
        check(self._lib.mg_create(finest_level - coarsest_level + 1, dim, device, C.byref(self._h)))
        self._keepalive = []
        if rows_per_lane is not None:
            self.set_tuning("rows_per_lane", rows_per_lane)
        if xcd_chunk is not None:
            self.set_tuning("xcd_chunk", xcd_chunk)
        if offset_codes is not None:
            self.set_tuning("offset_codes", offset_codes)
        if strip_slices is not None:
            self.set_tuning("strip_slices", strip_slices)
        if nontemporal is not None:
            self.set_tuning("nontemporal", nontemporal)
        if coarse_direct is not None:
            self.set_tuning("coarse_direct", coarse_direct)
        if symmetric_storage is not None:
            self.set_tuning("symmetric_storage", symmetric_storage)
        if graph is not None:
            self.set_tuning("graph", graph)
        if lds_pad is not None:
            self.set_tuning("lds_pad", lds_pad)
        for key, value in more_tuning.items():        # any other mg_set_tuning key (fuse_sweeps, fuse_segments ...)
            self.set_tuning(key, value)

    # ---- life cycle ---------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.mg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _idx(self, level: int) -> int:
        if level < self.coarsest_level or level > self.finest_level:
            raise KeyError(f"level {level} outside {self.coarsest_level}..{self.finest_level}")
        return level - self.coarsest_level

    def elements(self, level: int) -> int:
        return self.c * 2 ** level

    def n_dofs(self, level: int) -> int:
        if getattr(self, "_flat_n", None) is not None:
            return self._flat_n
        return (self.elements(level) + 1) ** self.dim

    def device_info(self) -> str:
        buf = C.create_string_buffer(256)
        check(self._lib.mg_device_info(self._h, buf, 256))
        return buf.value.decode()

    # ---- set-up ----------------------------------------------------------------------------
    def set_tuning(self, key: str, value: int):
        check(self._lib.mg_set_tuning(self._h, key.encode(), int(value)))

    def set_comm_rccl(self, rank: int, world: int, unique_id: bytes, replicate_below: int = 1 << 21):
        buf = C.create_string_buffer(unique_id, len(unique_id))
        check(self._lib.mg_set_comm(self._h, rank, world, buf, len(unique_id), int(replicate_below)))

    def set_comm_callbacks(self, rank: int, world: int, exchange, allreduce, allgatherv,
                           replicate_below: int = 1 << 21):
        """Host-staged transport (tests): three Python callables moving NumPy buffers."""
        def _ex(user, slo, shi, rlo, rhi, count):
            try:
                as_np = lambda p: None if not p else np.ctypeslib.as_array(p, shape=(count,))
                exchange(as_np(slo), as_np(shi), as_np(rlo), as_np(rhi))
                return 0
            except Exception:          # pragma: no cover - surfaced as an MgError by the library
                import traceback
                traceback.print_exc()
                return 1

        def _ar(user, buf, count):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(count,)))
                return 0
            except Exception:          # pragma: no cover
                import traceback
                traceback.print_exc()
                return 1

        def _ag(user, send, send_count, recv, counts):
            try:
                cnt = np.ctypeslib.as_array(counts, shape=(world,)).copy()
                allgatherv(np.ctypeslib.as_array(send, shape=(send_count,)),
                           np.ctypeslib.as_array(recv, shape=(int(cnt.sum()),)), cnt)
                return 0
            except Exception:          # pragma: no cover
                import traceback
                traceback.print_exc()
                return 1

        cbs = (_capi.EXCHANGE_FN(_ex), _capi.ALLREDUCE_FN(_ar), _capi.ALLGATHERV_FN(_ag))
        self._keepalive.append(cbs)
        check(self._lib.mg_set_comm_callbacks(self._h, rank, world, cbs[0], cbs[1], cbs[2], None,
                                              int(replicate_below)))

    def set_level(self, level: int, A, grid_index=None, prune_zeros: bool = True):
        """Hand over one level's stiffness CSR (`Multigrid_prototype.py:95-99`)."""
        indptr, is64, indices, data = _csr_arrays(A)
        n = A.shape[0]
        if n != self.n_dofs(level):
            raise ValueError(f"level {level}: matrix has {n} rows, expected {self.n_dofs(level)}")
        gi = None
        if grid_index is not None:
            gi = np.ascontiguousarray(grid_index, dtype=np.int64)
            if gi.size != n:
                raise ValueError("grid_index has the wrong length")
            if np.array_equal(gi, np.arange(n)):
                gi = None
        check(self._lib.mg_set_level_csr(self._h, self._idx(level), self.elements(level), n, data.size,
                                         ptr(indptr), is64, ptr(indices), ptr(data),
                                         ptr(gi) if gi is not None else None, 1 if prune_zeros else 0))

    def set_prolongation(self, kind: str = "q1"):
        """"q1": the reference's bilinear / trilinear interpolation (`Interpolation2D`); "p2": the natural embedding of
        the coarse P2 space (`poisson.p2_prolongation_table`), for hierarchies of P2 lattice levels; "p1": the natural
        embedding of the coarse P1 space on the simplicial mesh of `poisson` (`mg_set_prolongation_p1`; its transpose is
        `set_params(restriction="p1_transpose")`)."""
        if kind == "q1":
            check(self._lib.mg_set_prolongation_table(self._h, None, None, None))
            return
        if kind == "p1":
            check(self._lib.mg_set_prolongation_p1(self._h, 1))
            return
        if kind != "p2":
            raise ValueError("prolongation must be 'q1', 'p1' or 'p2'")
        from .poisson import p2_prolongation_table
        cnt, off, w = p2_prolongation_table(self.dim)
        cnt = np.ascontiguousarray(cnt, dtype=np.int32)
        off = np.ascontiguousarray(off, dtype=np.int32)
        w = np.ascontiguousarray(w, dtype=np.float64)
        check(self._lib.mg_set_prolongation_table(self._h, ptr(cnt), ptr(off), ptr(w)))
        # ... and its transpose, selected with set_params(restriction="table")
        from .poisson import p2_restriction_table
        rc, ro, rw = p2_restriction_table(self.dim)
        rc = np.ascontiguousarray(rc, dtype=np.int32)
        ro = np.ascontiguousarray(ro, dtype=np.int32)
        rw = np.ascontiguousarray(rw, dtype=np.float64)
        check(self._lib.mg_set_restriction_table(self._h, int(ro.shape[1]), ptr(rc), ptr(ro), ptr(rw)))

    def galerkin(self, top_level: Optional[int] = None):
        """Galerkin coarse levels (`mg_galerkin_hierarchy`): every level below `top_level` (default: the finest) becomes
        P^T A P of the level above it, with P the P1 natural embedding, computed on the device.  The coarse levels' vectors
        are lexicographic and start at zero; `fmg` on them needs `set_rhs_true` again."""
        top = self.finest_level if top_level is None else top_level
        check(self._lib.mg_galerkin_hierarchy(self._h, self._idx(top)))

    def galerkin_level(self, level: int):
        """Level - 1 := P^T A_level P (`mg_galerkin_level`)."""
        check(self._lib.mg_galerkin_level(self._h, self._idx(level)))

    @classmethod
    def galerkin_from_matrix(cls, dim: int, coarsest_level: int, finest_level: int, A=None, grid_index=None, c: int = 8,
                             mu1: int = 2, mu2: int = 2, omega: float = 2.0 / 3.0, smoother: str = "jacobi",
                             prune_zeros: bool = True, device: int = 0, **tuning):
        """A hierarchy from ONE finest matrix: `A` (SciPy CSR in the DoF numbering `grid_index`), or None for the device
        generator (`gen_poisson_level`), then Galerkin coarse levels with the P1 transfers selected."""
        h = cls(dim, coarsest_level, finest_level, c=c, device=device, **tuning)
        if A is None:
            h.gen_poisson_level(finest_level, prune_zeros=prune_zeros)
        else:
            h.set_level(finest_level, A, grid_index, prune_zeros=prune_zeros)
        h.galerkin(finest_level)
        h.set_params(mu1, mu2, omega, restriction="p1_transpose", smoother=smoother)
        h.set_prolongation("p1")
        return h

    def level_slab(self, level: int):
        """`(row0, n_local, halo_lo, halo_hi)`: the lexicographic nodes this rank owns on `level` and how many nodes
        below / above them it may couple to (before the level is set)."""
        v = [C.c_int64() for _ in range(4)]
        check(self._lib.mg_level_slab(self._h, self._idx(level), self.elements(level), *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def set_level_local(self, level: int, A_local, col_nodes, grid_index=None, prune_zeros: bool = True):
        """Per-rank hand-off (`mg_set_level_csr_local`): `A_local` holds this rank's owned rows, its columns are local
        ids and `col_nodes[id]` their global lexicographic nodes (the first `A_local.shape[0]` ids are the rows)."""
        indptr, is64, indices, data = _csr_arrays(A_local)
        cn = np.ascontiguousarray(col_nodes, dtype=np.int64)
        if cn.size != A_local.shape[1]:
            raise ValueError("col_nodes must name every local column")
        gi = None
        if grid_index is not None:
            gi = np.ascontiguousarray(grid_index, dtype=np.int64)
            if np.array_equal(gi, np.arange(gi.size)):
                gi = None
        check(self._lib.mg_set_level_csr_local(self._h, self._idx(level), self.elements(level), A_local.shape[0],
                                               A_local.shape[1], data.size, ptr(indptr), is64, ptr(indices), ptr(data),
                                               ptr(cn), ptr(gi) if gi is not None else None, 1 if prune_zeros else 0))

    def gen_poisson_level(self, level: int, prune_zeros: bool = True):
        """Device-side synthetic level (same tiles as `poisson.make_level` + `set_level`)."""
        check(self._lib.mg_gen_poisson_level(self._h, self._idx(level), self.elements(level),
                                             1 if prune_zeros else 0))

    def _kappa(self, level: int, kappa) -> np.ndarray:
        k = np.ascontiguousarray(np.asarray(kappa, dtype=np.float64).reshape(-1))
        if k.size != self.elements(level) ** self.dim:
            raise ValueError(f"level {level}: kappa has {k.size} entries, the level has {self.elements(level) ** self.dim} cells")
        return k

    def gen_diffusion_level(self, level: int, kappa, prune_zeros: bool = True, matrix_free: bool = False):
        """Device-side level of -div(kappa grad u), one kappa per cell (`mg_gen_diffusion_level`; the host restatement is
        `poisson.diffusion_level`).  On slabs every rank passes the whole kappa of the level.  `matrix_free=True`
        (`mg_gen_diffusion_level_mf`; 3-D, whole handles, pruned) keeps kappa instead of a matrix: same results bit for bit."""
        k = self._kappa(level, kappa)
        if matrix_free:
            if not prune_zeros:
                raise ValueError("matrix-free diffusion levels are pruned levels (prune_zeros=True)")
            check(self._lib.mg_gen_diffusion_level_mf(self._h, self._idx(level), self.elements(level), ptr(k)))
            return
        check(self._lib.mg_gen_diffusion_level(self._h, self._idx(level), self.elements(level), ptr(k),
                                               1 if prune_zeros else 0))

    def gen_diffusion_hierarchy(self, kappa, averaging: str = "arithmetic", top_level: Optional[int] = None,
                                matrix_free_min_rows: Optional[int] = None):
        """Levels top_level (default: the finest) .. coarsest from one kappa, coarsened on the device
        (`mg_gen_diffusion_hierarchy`, as `poisson.coarsen_kappa` does it); pruned; whole handles only.  With
        `matrix_free_min_rows` the levels above the coarsest with at least that many rows are matrix-free
        (`mg_gen_diffusion_hierarchy_mf`).  An integer `kappa` is the device address of the top level's cells (the
        convention of `diffusion_dkappa`): nothing is uploaded, the buffer is only read and the results are the same bit
        for bit (`mg_gen_diffusion_hierarchy_device`)."""
        top = self.finest_level if top_level is None else top_level
        avg = {"arithmetic": _capi.MG_KAPPA_ARITHMETIC, "harmonic": _capi.MG_KAPPA_HARMONIC}[averaging]
        if isinstance(kappa, (int, np.integer)):
            check(self._lib.mg_gen_diffusion_hierarchy_device(self._h, self._idx(top), self.elements(top), C.c_void_p(int(kappa)),
                                                              avg, -1 if matrix_free_min_rows is None else int(matrix_free_min_rows)))
            return
        k = self._kappa(top, kappa)
        if matrix_free_min_rows is not None:
            check(self._lib.mg_gen_diffusion_hierarchy_mf(self._h, self._idx(top), self.elements(top), ptr(k), avg,
                                                          int(matrix_free_min_rows)))
            return
        check(self._lib.mg_gen_diffusion_hierarchy(self._h, self._idx(top), self.elements(top), ptr(k), avg))

    def refresh_diffusion_hierarchy(self, kappa, averaging: str = "arithmetic", top_level: Optional[int] = None):
        """Another kappa for a hierarchy `gen_diffusion_hierarchy` generated, in place (`mg_refresh_diffusion_hierarchy`):
        the state a fresh generation with the same stored / matrix-free split leaves, bit for bit, without freeing or
        allocating anything for the matrix-free levels.  `kappa` is a device address or, for tests, a NumPy array, which
        is uploaded to a temporary device buffer first."""
        top = self.finest_level if top_level is None else top_level
        avg = {"arithmetic": _capi.MG_KAPPA_ARITHMETIC, "harmonic": _capi.MG_KAPPA_HARMONIC}[averaging]
        if isinstance(kappa, (int, np.integer)):
            check(self._lib.mg_refresh_diffusion_hierarchy(self._h, self._idx(top), C.c_void_p(int(kappa)), avg))
            return
        k = self._kappa(top, kappa)
        dev = _DeviceArray(self._lib, self.device, k.size, k)
        try:
            check(self._lib.mg_refresh_diffusion_hierarchy(self._h, self._idx(top), dev.ptr, avg))
        finally:
            dev.free()

    def set_diffusion_faces(self, dirichlet=("x-", "x+", "y-", "y+", "z-", "z+")):
        """The faces of the unit cube that carry a Dirichlet condition in the diffusion levels generated from now on
        (`mg_set_diffusion_faces`): names "x-" .. "z+" or the integer of `poisson.face_set`.  Nodes on the other faces are
        free nodes with the natural (no-flux) rows.  3-D, whole handles; all six faces is the default.  An integer goes to
        the library as it is, which refuses what is no face set."""
        faces = int(dirichlet) if isinstance(dirichlet, (int, np.integer)) else face_set(dirichlet)
        check(self._lib.mg_set_diffusion_faces(self._h, faces))

    def set_diffusion_insulated(self):
        """No Dirichlet node in the diffusion levels generated from now on (`mg_set_diffusion_insulated`): every node is a
        free node, `diffusion_faces` reports 0, Robin fields may sit on any face.  3-D, whole handles.  With a reaction or a
        Robin field the operator is regular and everything works as on any face set; with neither it is singular and `pcg`
        computes the projected solve u = Q A^+ Q^T f (mg_hip.h), while `pcg_batch`, `eigs`, `fmg` and the Chebyshev and
        Gauss-Seidel smoothers are refused.  `set_diffusion_faces` with a valid set leaves the state."""
        check(self._lib.mg_set_diffusion_insulated(self._h))

    def diffusion_nullspace(self, level: Optional[int] = None) -> bool:
        """True where solves from `level` run projected (`mg_diffusion_nullspace`): the levels up to it were generated on an
        insulated handle and none holds a reaction or Robin diagonal."""
        out = C.c_int(0)
        check(self._lib.mg_diffusion_nullspace(self._h, self._idx(self.finest_level if level is None else level), C.byref(out)))
        return bool(out.value)

    def remove_mean(self, x_ptr: int, n: int, w_ptr: Optional[int] = None) -> float:
        """x -= its mean, in place over `n` doubles of device memory at `x_ptr` (`mg_remove_mean`): (w.x) / (w.1) with the
        weights at `w_ptr`, (1.x) / n without.  Both 16-byte aligned.  Returns the mean removed; the same bits on every run."""
        out = C.c_double(0.0)
        check(self._lib.mg_remove_mean(self._h, C.c_void_p(x_ptr), C.c_void_p(w_ptr) if w_ptr else None, int(n), C.byref(out)))
        return float(out.value)

    def diffusion_faces(self) -> int:
        """The handle's face set as an integer (`mg_diffusion_faces`): x- = 1, x+ = 2, y- = 4, y+ = 8, z- = 16, z+ = 32."""
        faces = C.c_int(0)
        check(self._lib.mg_diffusion_faces(self._h, C.byref(faces)))
        return int(faces.value)

    def set_diffusion_reaction(self, sigma, N: Optional[int] = None):
        """The reaction field of the diffusion levels generated from now on (`mg_set_diffusion_reaction`): the operator
        A(kappa) + R(sigma) with the lumped diagonal of `poisson.reaction_diag`.  `sigma`: one finite value >= 0 per cell of
        the level it is meant for (the top level of a hierarchy call), as a NumPy array -- its size gives the cells per
        dimension unless `N` does -- or as an integer device address with `N=` (`mg_set_diffusion_reaction_device`).  The
        handle keeps its own copy.  None clears the field.  3-D, whole handles."""
        if sigma is None:
            check(self._lib.mg_set_diffusion_reaction(self._h, 0, None))
            return
        if isinstance(sigma, (int, np.integer)):
            if N is None:
                raise TypeError("a device address needs N=, the cells per dimension of the field")
            check(self._lib.mg_set_diffusion_reaction_device(self._h, int(N), C.c_void_p(int(sigma))))
            return
        s = np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).reshape(-1))
        n = int(round(s.size ** (1.0 / 3.0))) if N is None else int(N)
        if n ** 3 != s.size:
            raise ValueError(f"sigma has {s.size} entries, which is not {n}^3 cells")
        check(self._lib.mg_set_diffusion_reaction(self._h, n, ptr(s)))

    def diffusion_reaction(self):
        """(on, cells per dimension) of the handle's reaction field (`mg_diffusion_reaction`); (0, 0) without one."""
        on, n = C.c_int(0), C.c_int(0)
        check(self._lib.mg_diffusion_reaction(self._h, C.byref(on), C.byref(n)))
        return int(on.value), int(n.value)

    def level_reaction(self, level: int) -> bool:
        """True if the level was generated with a reaction diagonal (`mg_level_reaction`)."""
        on = C.c_int(0)
        check(self._lib.mg_level_reaction(self._h, self._idx(level), C.byref(on)))
        return bool(on.value)

    def set_diffusion_robin(self, face, alpha, N: Optional[int] = None):
        """The Robin field of one face for the diffusion levels generated from now on (`mg_set_diffusion_robin`): the
        condition kappa du/dn + alpha (u - u_ext) = 0 there, with the lumped diagonal of `poisson.robin_diag`.  `face`: a
        name ("z+") or one bit of the face set.  `alpha`: one finite value >= 0 per boundary face-cell of the level it is
        meant for (the top level of a hierarchy call), face-cell (ca, cb) at `cb * N + ca` with (a, b) the in-plane axes in
        ascending order, as a NumPy array -- its size gives the cells per dimension unless `N` does -- or as an integer
        device address with `N=` (`mg_set_diffusion_robin_device`).  The handle keeps its own copy.  None clears the face's
        field.  3-D, whole handles."""
        bit = poisson._one_face(face)
        if alpha is None:
            check(self._lib.mg_set_diffusion_robin(self._h, 0, bit, None))
            return
        if isinstance(alpha, (int, np.integer)):
            if N is None:
                raise TypeError("a device address needs N=, the cells per dimension of the field")
            check(self._lib.mg_set_diffusion_robin_device(self._h, int(N), bit, C.c_void_p(int(alpha))))
            return
        a = np.ascontiguousarray(np.asarray(alpha, dtype=np.float64).reshape(-1))
        n = int(round(a.size ** 0.5)) if N is None else int(N)
        if n * n != a.size:
            raise ValueError(f"alpha has {a.size} entries, which is not {n}^2 face-cells")
        check(self._lib.mg_set_diffusion_robin(self._h, n, bit, ptr(a)))

    def diffusion_robin(self):
        """(faces, cells per dimension) of the handle's Robin fields (`mg_diffusion_robin`): the bits of the faces that hold
        one; (0, 0) without any."""
        faces, n = C.c_int(0), C.c_int(0)
        check(self._lib.mg_diffusion_robin(self._h, C.byref(faces), C.byref(n)))
        return int(faces.value), int(n.value)

    def level_robin(self, level: int) -> int:
        """The faces whose Robin field the level was generated with, as bits (`mg_level_robin`); 0: none."""
        faces = C.c_int(0)
        check(self._lib.mg_level_robin(self._h, self._idx(level), C.byref(faces)))
        return int(faces.value)

    def level_matrix_free(self, level: int) -> bool:
        """True if the level keeps kappa instead of a matrix (`mg_level_matrix_free`)."""
        on = C.c_int(0)
        check(self._lib.mg_level_matrix_free(self._h, self._idx(level), C.byref(on), None))
        return bool(on.value)

    def level_kappa_bytes(self, level: int) -> int:
        """Device bytes of the kappa a matrix-free level keeps (8 per cell); 0 for a stored level."""
        nbytes = C.c_int64(0)
        check(self._lib.mg_level_matrix_free(self._h, self._idx(level), None, C.byref(nbytes)))
        return int(nbytes.value)

    @classmethod
    def synthetic_diffusion(cls, dim: int, coarsest_level: int, finest_level: int, kappa, c: int = 8,
                            coarse: str = "arithmetic", mu1: int = 2, mu2: int = 2, omega: float = 2.0 / 3.0,
                            smoother: str = "jacobi", prune_zeros: bool = True, device: int = 0, comm=None,
                            matrix_free_min_rows: Optional[int] = None, **tuning):
        """Hierarchy of -div(kappa grad u) levels from the finest level's kappa, with the P1 transfers (P and R = P^T).
        Coarse levels: `coarse="arithmetic"` / `"harmonic"` regenerate them from a coarsened kappa -- on one handle with
        `mg_gen_diffusion_hierarchy`, on slabs (`comm`) level by level with `poisson.coarsen_kappa` on the host --
        and `"galerkin"` takes P^T A P (whole handles only).  `matrix_free_min_rows`: regenerated levels with at least
        that many rows keep kappa instead of a matrix (whole handles, 3-D, pruned; `gen_diffusion_hierarchy`)."""
        from .poisson import coarsen_kappa
        if coarse not in ("arithmetic", "harmonic", "galerkin"):
            raise ValueError("coarse must be 'arithmetic', 'harmonic' or 'galerkin'")
        if coarse == "galerkin" and comm is not None:
            raise ValueError("Galerkin coarse levels need a whole handle, not slabs")
        if matrix_free_min_rows is not None and (coarse == "galerkin" or comm is not None or not prune_zeros):
            raise ValueError("matrix-free levels need regenerated, pruned coarse levels on a whole handle")
        h = cls(dim, coarsest_level, finest_level, c=c, device=device, **tuning)
        if comm is not None:
            comm(h)
        if coarse == "galerkin":
            h.gen_diffusion_level(finest_level, kappa, prune_zeros=prune_zeros)
            h.galerkin(finest_level)
        elif comm is not None or not prune_zeros:
            k = np.asarray(kappa, dtype=np.float64).reshape(-1)
            for level in range(finest_level, coarsest_level - 1, -1):
                h.gen_diffusion_level(level, k, prune_zeros=prune_zeros)
                if level > coarsest_level:
                    k = coarsen_kappa(k, dim, coarse)
        else:
            h.gen_diffusion_hierarchy(kappa, coarse, matrix_free_min_rows=matrix_free_min_rows)
        h.set_params(mu1, mu2, omega, restriction="p1_transpose", smoother=smoother)
        h.set_prolongation("p1")
        return h

    def gen_p2_level(self, level: int):
        """Device-side synthetic P2 level on the lattice with `elements(level)` steps per dimension (= twice the
        cells; BASELINE config 5), from the per-class interior stencils of `poisson.p2_stencils`."""
        from .poisson import p2_stencils
        if not hasattr(self, "_p2_tables"):
            self._p2_tables = p2_stencils(self.dim)
        count, offsets, values, load = self._p2_tables
        steps = self.elements(level)
        h = 2.0 / steps                                 # cell size
        vals = np.ascontiguousarray(values * h ** (self.dim - 2))
        ld = np.ascontiguousarray(load * h ** self.dim)
        cnt = np.ascontiguousarray(count, dtype=np.int32)
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        check(self._lib.mg_gen_lattice_level(self._h, self._idx(level), steps, int(cnt.max()), ptr(cnt), ptr(off),
                                             ptr(vals), ptr(ld)))

    @classmethod
    def synthetic_p2(cls, dim: int, coarsest_level: int, finest_level: int, c: int = 8, mu1: int = 2, mu2: int = 2,
                     omega: float = 1.0, smoother: str = "mcgs", device: int = 0, comm=None, transfers: str = "q1",
                     restriction: str = "direct", **tuning):
        """Whole P2 hierarchy from the device generator (lattices of c * 2^level steps per dimension); on slabs
        (`comm`) the tuning must carry halo_planes=2: P2 rows reach two lattice planes.  `transfers="p2"` +
        `restriction="table"`: the P2 prolongation and its transpose instead of the reference's bilinear table / injection."""
        h = cls(dim, coarsest_level, finest_level, c=c, device=device, **tuning)
        if comm is not None:
            comm(h)
        for level in range(coarsest_level, finest_level + 1):
            h.gen_p2_level(level)
        h.set_params(mu1, mu2, omega, smoother=smoother, restriction=restriction)
        if transfers == "p2":
            h.set_prolongation("p2")
        return h

    def set_params(self, mu1: int, mu2: int, omega: float, restriction: str = "direct",
                   coarse_rtol: float = 1e-14, coarse_maxit: int = 20000, keep_err: bool = False,
                   smoother: str = "jacobi"):
        sm = {"jacobi": _capi.MG_SMOOTH_JACOBI, "rbgs": _capi.MG_SMOOTH_RBGS, "mcgs": _capi.MG_SMOOTH_MCGS,
              "chebyshev": _capi.MG_SMOOTH_CHEBYSHEV}[smoother]
        check(self._lib.mg_set_params(self._h, int(mu1), int(mu2), float(omega), _RESTRICT[restriction],
                                      sm, float(coarse_rtol), int(coarse_maxit), 1 if keep_err else 0))

    def set_chebyshev(self, eig_steps: int = 10, lower_ratio: float = CHEB_LOWER_RATIO, upper_factor: float = 1.1):
        """Settings of the Chebyshev smoother (`smoother="chebyshev"`, `mg_set_chebyshev`): Lanczos steps of the estimate of
        lambda_max(D^-1 A) per level, and the interval [b / lower_ratio, b] with b = upper_factor * that estimate."""
        check(self._lib.mg_set_chebyshev(self._h, int(eig_steps), float(lower_ratio), float(upper_factor)))

    def set_chebyshev_bounds(self, level: int, lmin: float, lmax: float):
        """The Chebyshev interval [lmin, lmax] of one level instead of the estimate's (lmin <= 0: lmax / lower_ratio;
        lmax <= 0: back to the estimate)."""
        check(self._lib.mg_set_chebyshev_bounds(self._h, self._idx(level), float(lmin), float(lmax)))

    def chebyshev_bounds(self, level: int) -> dict:
        """{"lmin", "lmax"}: the interval the Chebyshev smoother uses on `level`; "lmax_estimate": the Lanczos estimate of
        lambda_max(D^-1 A) (0.0 if none has run).  Runs the estimate if it has not run yet."""
        lo, hi, est = C.c_double(), C.c_double(), C.c_double()
        check(self._lib.mg_chebyshev_bounds(self._h, self._idx(level), C.byref(lo), C.byref(hi), C.byref(est)))
        return {"lmin": lo.value, "lmax": hi.value, "lmax_estimate": est.value}

    def chebyshev_estimate_bytes(self) -> int:
        """Device bytes the last Chebyshev estimate held while it ran (freed afterwards)."""
        b = C.c_int64()
        check(self._lib.mg_chebyshev_estimate_bytes(self._h, C.byref(b)))
        return int(b.value)

    @classmethod
    def from_bag(cls, bag, dim: int = 2, grid_index: Optional[Dict[int, np.ndarray]] = None,
                 prune_zeros: bool = True, device: int = 0, keep_err: bool = True, **tuning):
        """Build from the reference's 16-field bag (`Multigrid_prototype.py:15-32`).

        The level link is taken from `grid_index[level]` if given, else recovered from
        the coordinate dictionaries `mesh_dof_list_dict` (`Multigrid_prototype.py:68-74`).
        """
        h = cls(dim, bag.coarsest_level, bag.finest_level, c=bag.coarsest_level_elements_per_dim,
                device=device, **tuning)
        for level in range(bag.coarsest_level, bag.finest_level + 1):
            A = bag.A_sp_dict[level][0]
            if grid_index is not None and level in grid_index:
                gi = grid_index[level]
            else:
                d = bag.mesh_dof_list_dict[level]
                n = A.shape[0]
                coords = np.array([d[j] for j in range(n)], dtype=np.float64)
                gi = grid_index_from_coords(coords, h.elements(level), dim)
            h.set_level(level, A, gi, prune_zeros=prune_zeros)
        h.set_params(bag.mu1, bag.mu2, bag.omega, keep_err=keep_err)
        return h

    @classmethod
    def synthetic(cls, dim: int, coarsest_level: int, finest_level: int, c: int = 8, mu1: int = 50,
                  mu2: int = 50, omega: float = 2.0 / 3.0, prune_zeros: bool = True, device: int = 0,
                  comm=None, **tuning):
        """Whole hierarchy from the device generator (bench and full-size tests)."""
        h = cls(dim, coarsest_level, finest_level, c=c, device=device, **tuning)
        if comm is not None:
            comm(h)
        for level in range(coarsest_level, finest_level + 1):
            h.gen_poisson_level(level, prune_zeros=prune_zeros)
        h.set_params(mu1, mu2, omega)
        return h

    # ---- queries -------------------------------------------------------------------------------
    def level_info(self, level: int) -> dict:
        vals = [C.c_int64() for _ in range(5)]
        w, rep, codes = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.mg_level_info(self._h, self._idx(level), *[C.byref(v) for v in vals], C.byref(w),
                                      C.byref(rep), C.byref(codes)))
        keys = ("n_global", "n_local", "row0", "nnz_stored", "nnz_nonzero")
        out = {k: int(v.value) for k, v in zip(keys, vals)}
        out["ell_width"] = int(w.value)
        out["replicated"] = bool(rep.value)
        out["offset_codes"] = max(0, int(codes.value))
        out["symmetric_diagonals"] = max(0, -int(codes.value))
        ncls = C.c_int()
        check(self._lib.mg_level_row_classes(self._h, self._idx(level), C.byref(ncls)))
        out["row_classes"] = int(ncls.value)
        return out

    def level_storage(self, level: int) -> dict:
        """How the level's matrix got its storage (`mg_level_storage`): `symmetric` 1 = bit for bit, 2 = within
        `ulps_used` units in the last place, 0 = not (then `first_asymmetric_row`, in lexicographic numbering, and
        `max_pair_ulps`, -1 for a pair with one half missing, say why), -1 = not tested; `distinct_rows` seen by the row
        dictionary (more than 255: no row classes, or -- `escape_rows` > 0 -- classes for the frequent rows and that many
        rows read from the stored matrix), -1 = not built."""
        sym, rows, used = C.c_int(), C.c_int(), C.c_int()
        first, spread, esc = C.c_int64(), C.c_int64(), C.c_int64()
        check(self._lib.mg_level_storage(self._h, self._idx(level), C.byref(sym), C.byref(first), C.byref(spread),
                                         C.byref(rows), C.byref(used), C.byref(esc)))
        return {"symmetric": int(sym.value), "first_asymmetric_row": int(first.value), "max_pair_ulps": int(spread.value),
                "distinct_rows": int(rows.value), "ulps_used": int(used.value), "escape_rows": int(esc.value)}

    def memory_bytes(self) -> int:
        b = C.c_int64()
        check(self._lib.mg_memory_bytes(self._h, C.byref(b)))
        return int(b.value)

    # ---- vectors ---------------------------------------------------------------------------------
    def set_vector(self, level: int, which: str, x):
        a = _capi.as_f64(x, self.n_dofs(level))
        check(self._lib.mg_set_vector(self._h, self._idx(level), _VEC[which], ptr(a)))

    def set_rhs_true(self, level: int, x):
        a = _capi.as_f64(x, self.n_dofs(level))
        check(self._lib.mg_set_rhs_true(self._h, self._idx(level), ptr(a)))

    def get_vector(self, level: int, which: str, gather: bool = False) -> np.ndarray:
        out = np.zeros(self.n_dofs(level))
        check(self._lib.mg_get_vector(self._h, self._idx(level), _VEC[which], ptr(out), 1 if gather else 0))
        return out.reshape(-1, 1)

    def set_vector_device(self, level: int, which: str, dev_ptr: int):
        """`set_vector` from device memory (`mg_set_vector_device`): `dev_ptr` is the integer address of `n_dofs(level)`
        float64 on this handle's device, in the caller's DoF numbering, and must be complete before the call (synchronise the
        stream that produced it).  Nothing crosses to the host."""
        check(self._lib.mg_set_vector_device(self._h, self._idx(level), _VEC[which], C.c_void_p(int(dev_ptr))))

    def get_vector_device(self, level: int, which: str, dev_ptr: int):
        """`get_vector` into device memory (`mg_get_vector_device`): writes `n_dofs(level)` float64 at the integer device
        address `dev_ptr`; the handle's stream has finished when this returns."""
        check(self._lib.mg_get_vector_device(self._h, self._idx(level), _VEC[which], C.c_void_p(int(dev_ptr))))

    @staticmethod
    def _node_sets(**sets):
        """The values of `enum mg_node_set` for "interior" / "all", or None where every set is "interior": the call the
        entries without node sets serve."""
        for what, name in sets.items():
            if name not in _NODE_SETS:
                raise ValueError(f"{what} must be 'interior' or 'all' (got {name!r})")
        values = [_NODE_SETS[name] for name in sets.values()]
        return values if any(values) else None

    def _sensitivity(self, entry, operands, n_out, out):
        """One sensitivity or cell gradient entry, `entry(*operand pointers, out pointer)`, on integer device addresses --
        `out` is then required and nothing is returned -- or, for tests, on NumPy arrays, which are uploaded, and the result
        (`n_out` values) comes back as a NumPy array (into `out` if given).  `operands`: (name, value, length, may be None)
        each; a None that may be one is passed as a null pointer.  An array given for two operands of one length (`a is b`)
        is uploaded once and its pointer passed twice."""
        is_address = lambda v: isinstance(v, (int, np.integer))
        given = [(name, v) for name, v, _, optional in operands if not (optional and v is None)]
        names = [name for name, _ in given]
        addresses = [is_address(v) for _, v in given]
        if all(addresses):
            if not is_address(out):
                raise TypeError(("with device addresses for " if len(names) > 1 else "with a device address for ") +
                                " and ".join(names) + ", out must be a device address too")
            check(entry(*[C.c_void_p(0 if v is None else int(v)) for _, v, _, _ in operands], C.c_void_p(int(out))))
            return None
        if any(addresses) or is_address(out):
            raise TypeError(", ".join(names) + " and out must be all device addresses or all NumPy arrays")
        held = {}
        try:
            for _, v, n, optional in operands:
                if not (optional and v is None) and (id(v), n) not in held:
                    held[id(v), n] = _DeviceArray(self._lib, self.device, n, _capi.as_f64(v, n))
            result = held["out"] = _DeviceArray(self._lib, self.device, n_out)
            check(entry(*[C.c_void_p(0) if optional and v is None else held[id(v), n].ptr for _, v, n, optional in operands],
                        result.ptr))
            got = result.download()
        finally:
            for d in held.values():
                d.free()
        if out is None:
            return got
        out.reshape(-1)[:] = got
        return out

    def diffusion_dkappa(self, level: int, a, b, out=None, a_nodes: str = "interior", b_nodes: str = "interior"):
        """d(a^T A(kappa) b) / d kappa for every cell of a 3-D grid level (`mg_diffusion_dkappa`; host restatement:
        `poisson.diffusion_dkappa`).  `a`, `b` (lexicographic nodal values, boundary entries count as 0) and `out`
        (`elements(level) ** 3` cells) are integer device addresses -- `out` is then required and nothing is returned --
        or, for tests, NumPy arrays, which are uploaded, and the result comes back as a NumPy array (into `out` if
        given).  `a is b` passes the same pointer twice.  `a_nodes`, `b_nodes`: "all" keeps the boundary entries of that
        vector (`mg_diffusion_dkappa_ex`: the derivative of (M_A a)^T A^ (M_B b) with the natural matrix A^); the defaults
        call `mg_diffusion_dkappa`."""
        sets = self._node_sets(a_nodes=a_nodes, b_nodes=b_nodes)
        if sets is None:
            entry = lambda pa, pb, po: self._lib.mg_diffusion_dkappa(self._h, self._idx(level), pa, pb, po)
        else:
            entry = lambda pa, pb, po: self._lib.mg_diffusion_dkappa_ex(self._h, self._idx(level), pa, sets[0], pb, sets[1], po)
        n = self.n_dofs(level)
        return self._sensitivity(entry, [("a", a, n, False), ("b", b, n, False)], self.elements(level) ** 3, out)

    def diffusion_apply_dkappa(self, level: int, dkappa, x, out=None, rows: str = "interior", cols: str = "interior"):
        """(dA/dkappa . dkappa) x on a 3-D grid level, the derivative of A(kappa) x in the direction `dkappa`
        (`mg_diffusion_apply_dkappa`; host restatement: `poisson.diffusion_apply_dkappa`).  `dkappa`
        (`elements(level) ** 3` cells, any sign), `x` and `out` (lexicographic nodal values; boundary rows of `out` are 0)
        are integer device addresses -- `out` is then required, must not overlap the inputs, and nothing is returned -- or,
        for tests, NumPy arrays, which are uploaded, and the result comes back as a NumPy array (into `out` if given).
        `rows`, `cols`: "all" keeps the boundary rows / the entries towards boundary columns of the natural matrix A^
        (`mg_diffusion_apply_dkappa_ex`: M_rows A^(dkappa) M_cols x); the defaults call `mg_diffusion_apply_dkappa`."""
        sets = self._node_sets(rows=rows, cols=cols)
        if sets is None:
            entry = lambda pk, px, po: self._lib.mg_diffusion_apply_dkappa(self._h, self._idx(level), pk, px, po)
        else:
            entry = lambda pk, px, po: self._lib.mg_diffusion_apply_dkappa_ex(self._h, self._idx(level), pk, px, sets[0], sets[1], po)
        n = self.n_dofs(level)
        return self._sensitivity(entry, [("dkappa", dkappa, self.elements(level) ** 3, False), ("x", x, n, False)], n, out)

    def diffusion_dsigma(self, level: int, a, b, out=None):
        """D_sigma(a, b): d(a^T R(sigma) b) / d sigma for every cell of a 3-D grid level (`mg_diffusion_dsigma`; host
        restatement: `poisson.diffusion_dsigma`, same bits).  `a`, `b` (lexicographic nodal values, entries on the Dirichlet
        nodes of the handle's face set count as 0) and `out` (`elements(level) ** 3` cells): device addresses or NumPy
        arrays, as in `diffusion_dkappa`."""
        entry = lambda pa, pb, po: self._lib.mg_diffusion_dsigma(self._h, self._idx(level), pa, pb, po)
        n = self.n_dofs(level)
        return self._sensitivity(entry, [("a", a, n, False), ("b", b, n, False)], self.elements(level) ** 3, out)

    def diffusion_apply_dsigma(self, level: int, dsigma, x, out=None):
        """T_sigma(dsigma, x) = R(dsigma) x on the free nodes of the handle's face set, 0 on its Dirichlet nodes
        (`mg_diffusion_apply_dsigma`; host restatement: `poisson.diffusion_apply_dsigma`, same bits).  `dsigma`
        (`elements(level) ** 3` cells, any sign), `x` and `out` (lexicographic nodal values): device addresses or NumPy
        arrays, as in `diffusion_apply_dkappa`."""
        entry = lambda ps, px, po: self._lib.mg_diffusion_apply_dsigma(self._h, self._idx(level), ps, px, po)
        n = self.n_dofs(level)
        return self._sensitivity(entry, [("dsigma", dsigma, self.elements(level) ** 3, False), ("x", x, n, False)], n, out)

    def diffusion_drobin(self, level: int, face, a, b, out=None):
        """D_alpha,F(a, b): d(a^T B(alpha) b) / d alpha for every boundary face-cell of `face` on a 3-D grid level
        (`mg_diffusion_drobin`; host restatement: `poisson.diffusion_drobin`, same bits).  `a`, `b` (lexicographic nodal
        values, entries on the Dirichlet nodes of the handle's face set count as 0) and `out` (`elements(level) ** 2`
        face-cells): device addresses or NumPy arrays, as in `diffusion_dsigma`."""
        bit = poisson._one_face(face)
        entry = lambda pa, pb, po: self._lib.mg_diffusion_drobin(self._h, self._idx(level), bit, pa, pb, po)
        n = self.n_dofs(level)
        return self._sensitivity(entry, [("a", a, n, False), ("b", b, n, False)], self.elements(level) ** 2, out)

    def diffusion_apply_drobin(self, level: int, face, dalpha, x, out=None):
        """T_alpha,F(dalpha, x) = b_F(dalpha) x on the free nodes of `face`, 0 on every other node
        (`mg_diffusion_apply_drobin`; host restatement: `poisson.diffusion_apply_drobin`, same bits).  `dalpha`
        (`elements(level) ** 2` face-cells, any sign), `x` and `out` (lexicographic nodal values): device addresses or NumPy
        arrays, as in `diffusion_apply_dsigma`."""
        bit = poisson._one_face(face)
        entry = lambda pw, px, po: self._lib.mg_diffusion_apply_drobin(self._h, self._idx(level), bit, pw, px, po)
        n = self.n_dofs(level)
        return self._sensitivity(entry, [("dalpha", dalpha, self.elements(level) ** 2, False), ("x", x, n, False)], n, out)

    def diffusion_cell_gradient(self, level: int, w, x, out=None):
        """F(w, x): the cell gradient of the nodal field `x` weighted by the cell field `w` on a 3-D grid level, 3 N^3 values with
        component d at d * N^3 + cell (`mg_diffusion_cell_gradient`; host restatement: `poisson.diffusion_cell_gradient`, same
        bits).  `w`: `elements(level) ** 3` cells of any sign, or None (the plain gradient); -F(kappa, u) is the cell average
        of the flux.  Device addresses or NumPy arrays, as in `diffusion_dkappa`."""
        entry = lambda pw, px, po: self._lib.mg_diffusion_cell_gradient(self._h, self._idx(level), pw, px, po)
        cells = self.elements(level) ** 3
        return self._sensitivity(entry, [("w", w, cells, True), ("x", x, self.n_dofs(level), False)], 3 * cells, out)

    def diffusion_cell_gradient_t(self, level: int, w, p, out=None):
        """F^T(w, p): the transpose of `diffusion_cell_gradient` in x, applied to the 3-component cell field `p` (3 N^3), nodal
        values (`mg_diffusion_cell_gradient_t`; host restatement: `poisson.diffusion_cell_gradient_t`, same bits).  `w` as in
        `diffusion_cell_gradient`.  Device addresses or NumPy arrays, as in `diffusion_dkappa`."""
        entry = lambda pw, pp, po: self._lib.mg_diffusion_cell_gradient_t(self._h, self._idx(level), pw, pp, po)
        cells = self.elements(level) ** 3
        return self._sensitivity(entry, [("w", w, cells, True), ("p", p, 3 * cells, False)], self.n_dofs(level), out)

    def diffusion_cell_gradient_dot(self, level: int, p, x, out=None):
        """C(p, x): per cell the product of the 3-component cell field `p` (3 N^3) with the cell gradient of the nodal field `x`,
        N^3 values (`mg_diffusion_cell_gradient_dot`; host restatement: `poisson.diffusion_cell_gradient_dot`, same bits).
        Device addresses or NumPy arrays, as in `diffusion_dkappa`."""
        entry = lambda pp, px, po: self._lib.mg_diffusion_cell_gradient_dot(self._h, self._idx(level), pp, px, po)
        cells = self.elements(level) ** 3
        return self._sensitivity(entry, [("p", p, 3 * cells, False), ("x", x, self.n_dofs(level), False)], cells, out)

    def _point_entry(self, fn, level: int, M: int):
        return lambda pp, pv, po: fn(self._h, self._idx(level), C.c_int64(int(M)), pp, pv, po)

    def diffusion_point_sample(self, level: int, M: int, pts, x, out=None):
        """S(x, pts): the P1 interpolant of the nodal field `x` of a 3-D grid level at the `M` points `pts` (M x 3, rows (x, y, z)
        in the unit cube), M values (`mg_diffusion_point_sample`; host restatement: `poisson.diffusion_point_sample`, same
        bits).  Device addresses or NumPy arrays, as in `diffusion_cell_gradient`."""
        entry = self._point_entry(self._lib.mg_diffusion_point_sample, level, M)
        return self._sensitivity(entry, [("pts", pts, 3 * M, False), ("x", x, self.n_dofs(level), False)], M, out)

    def diffusion_point_load(self, level: int, M: int, pts, w, out=None):
        """S^T(w, pts): the consistent point load of the weights `w` (M) at the points `pts`, nodal values, summed per node in
        ascending point index (`mg_diffusion_point_load`; host restatement: `poisson.diffusion_point_load`, same bits).
        Device addresses or NumPy arrays, as in `diffusion_cell_gradient`."""
        entry = self._point_entry(self._lib.mg_diffusion_point_load, level, M)
        return self._sensitivity(entry, [("pts", pts, 3 * M, False), ("w", w, M, False)], self.n_dofs(level), out)

    def diffusion_point_gradient(self, level: int, M: int, pts, x, out=None):
        """G(x, pts): the gradient of the nodal field `x` in the simplex that holds each point, M x 3 values
        (`mg_diffusion_point_gradient`; host restatement: `poisson.diffusion_point_gradient`, same bits).  Device addresses
        or NumPy arrays, as in `diffusion_cell_gradient`."""
        entry = self._point_entry(self._lib.mg_diffusion_point_gradient, level, M)
        return self._sensitivity(entry, [("pts", pts, 3 * M, False), ("x", x, self.n_dofs(level), False)], 3 * M, out)

    def diffusion_point_gradient_t(self, level: int, M: int, pts, p, out=None):
        """G^T(p, pts): the transpose of `diffusion_point_gradient` in x applied to `p` (M x 3), nodal values, summed per node in
        ascending point index (`mg_diffusion_point_gradient_t`; host restatement: `poisson.diffusion_point_gradient_t`, same
        bits).  Device addresses or NumPy arrays, as in `diffusion_cell_gradient`."""
        entry = self._point_entry(self._lib.mg_diffusion_point_gradient_t, level, M)
        return self._sensitivity(entry, [("pts", pts, 3 * M, False), ("p", p, 3 * M, False)], self.n_dofs(level), out)

    def points(self, level: int, pts) -> "PointSet":
        """A located point set on `level` (`mg_points_create`): `pts` is an (M, 3) NumPy array of rows (x, y, z) in the unit
        cube, or a pair (integer device address, M).  The points are copied, checked, located and sorted once; the returned
        `PointSet` then serves S, S^T, G and G^T for any number of fields per call.  Close it (or use it as a context manager);
        the handle frees what is left."""
        return PointSet(self, level, pts)

    def zero_vector(self, level: int, which: str = "v"):
        check(self._lib.mg_zero_vector(self._h, self._idx(level), _VEC[which]))

    def copy_vector(self, level: int, dst: str, src: str):
        check(self._lib.mg_copy_vector(self._h, self._idx(level), _VEC[dst], _VEC[src]))

    # ---- the hot path ------------------------------------------------------------------------------
    def smooth(self, level: int, nw: int):
        check(self._lib.mg_smooth(self._h, self._idx(level), int(nw)))

    def smooth_split(self, level: int, nw: int):
        """Sweeps in the reference's split-operand form (matrix = D^-1 R, "err" = diagonal of D^-1)."""
        check(self._lib.mg_smooth_split(self._h, self._idx(level), int(nw)))

    def residual(self, level: int):
        check(self._lib.mg_residual(self._h, self._idx(level)))

    def restrict(self, level: int, kind: str = "direct"):
        check(self._lib.mg_restrict(self._h, self._idx(level), _RESTRICT[kind]))

    def prolong(self, level: int, add: bool = True):
        check(self._lib.mg_prolong(self._h, self._idx(level), 1 if add else 0))

    def prepare_cycle(self, level):
        """Build now what the first V-cycle from `level` would build lazily (mg_prepare_cycle)."""
        check(self._lib.mg_prepare_cycle(self._h, self._idx(level)))

    def coarse_solve(self):
        it, rel = C.c_int(), C.c_double()
        check(self._lib.mg_coarse_solve(self._h, C.byref(it), C.byref(rel)))
        return int(it.value), float(rel.value)

    def vcycle(self, level: Optional[int] = None, ncycles: int = 1, residuals: bool = False):
        level = self.finest_level if level is None else level
        hist = np.zeros(max(1, ncycles)) if residuals else None
        check(self._lib.mg_vcycle(self._h, self._idx(level), int(ncycles), ptr(hist) if residuals else None))
        return hist[:ncycles] if residuals else None

    def norm2(self, level: int, which: str = "r") -> float:
        out = C.c_double()
        check(self._lib.mg_norm2(self._h, self._idx(level), _VEC[which], C.byref(out)))
        return float(out.value)

    def quadratic_form(self, level: int, which: str = "v") -> float:
        """x^T A x with the level's matrix (mass-matrix norms)."""
        out = C.c_double()
        check(self._lib.mg_quadratic_form(self._h, self._idx(level), _VEC[which], C.byref(out)))
        return float(out.value)

    def set_flat_space(self, n: int):
        """A single matrix-free level of n unknowns (vector norms)."""
        check(self._lib.mg_set_level_grid(self._h, 0, 0, int(n), None))
        self._flat_n = int(n)

    def fmg(self, mu0: int, tol: float = 0.0, max_cycles: int = 10000, top_level: Optional[int] = None,
            norm: str = "l2", errors: bool = False):
        """FMG on levels coarsest..top_level; returns the residual norm after every top-level cycle -- the l2 norm,
        or with norm="mass" the reference's L2(Omega) norm sqrt(r^T M r) (set_mass) -- and with `errors` also the
        norm of iterate - exact solution (set_exact) as a second array.  Everything stays on the device."""
        top = self.finest_level if top_level is None else top_level
        hist = np.zeros(max(mu0, max_cycles if tol > 0 else mu0, 1))
        ehist = np.zeros_like(hist) if errors else None
        done = C.c_int()
        check(self._lib.mg_fmg_ex(self._h, self._idx(top), int(mu0), float(tol), int(max_cycles),
                                  {"l2": _capi.MG_NORM_L2, "mass": _capi.MG_NORM_MASS}[norm], ptr(hist),
                                  ptr(ehist) if errors else None, C.byref(done)))
        if errors:
            return hist[:done.value].copy(), ehist[:done.value].copy()
        return hist[:done.value].copy()

    def pcg(self, rtol: float = 1e-11, max_iter: int = 200, level: Optional[int] = None) -> np.ndarray:
        """Flexible CG preconditioned by one V(mu1, mu2) cycle per iteration (`mg_pcg`), from "v" on A x = "f" of `level`
        (default: the finest) until ||r||_2 <= rtol ||f||_2 or `max_iter` iterations (rtol <= 0: exactly that many).
        Returns ||r_k||_2 of the recursion after every iteration; the iterate is in "v", "f" is unchanged and "r" holds
        f - A x.  After `fmg(mu0, tol=0)` it starts from the FMG iterate.
        On the singular levels of an insulated handle (`set_diffusion_insulated`, `diffusion_nullspace`) it computes the
        projected solve Q A^+ Q^T f: the tolerance is relative to Q^T f, which is what "f" holds afterwards, "v" has
        w.v = 0, and a Q^T f of zero returns Q v after no iteration."""
        level = self.finest_level if level is None else level
        hist = np.zeros(max(1, int(max_iter)))
        done = C.c_int()
        check(self._lib.mg_pcg(self._h, self._idx(level), float(rtol), int(max_iter), ptr(hist), C.byref(done)))
        return hist[:done.value].copy()

    # ---- batched solves: one operator, several right-hand sides ---------------------------------------
    @staticmethod
    def _ptr_array(ptrs, nb=None):
        """A host array of device addresses (None: a null array); with `nb`, its length is checked."""
        if ptrs is None:
            return None
        ptrs = [int(p) for p in ptrs]
        if nb is not None and len(ptrs) != nb:
            raise ValueError(f"{len(ptrs)} pointers for {nb} lanes")
        return (C.c_void_p * len(ptrs))(*ptrs)

    def apply_batch(self, op: str, x_ptrs, f_ptrs, out_ptrs, level: Optional[int] = None, dots: bool = False):
        """`mg_apply_batch`: for every lane b, out_b = one Jacobi sweep of x_b ("jacobi"), f_b - A x_b ("residual") or A x_b
        ("spmv"; `f_ptrs` may be None) on `level` (default: the finest), with the bits of the one-vector kernels.  The
        arguments are sequences of integer device addresses of `n_dofs(level)` float64 each, in the caller's DoF numbering.
        `dots=True` ("spmv" only) returns x_b . A x_b per lane as a NumPy array; otherwise None.  The handle's own "v", "f"
        and "r" are unspecified afterwards."""
        level = self.finest_level if level is None else level
        nb = len(x_ptrs)
        d = np.zeros(max(1, nb)) if dots else None
        check(self._lib.mg_apply_batch(self._h, self._idx(level), {"jacobi": _capi.MG_BATCH_JACOBI, "residual": _capi.MG_BATCH_RESIDUAL,
                                                                    "spmv": _capi.MG_BATCH_SPMV}[op], nb,
                                       self._ptr_array(x_ptrs), self._ptr_array(f_ptrs, nb), self._ptr_array(out_ptrs, nb),
                                       ptr(d) if dots else None))
        return d[:nb].copy() if dots else None

    def pcg_batch(self, f_ptrs, x_ptrs, rtol: float = 1e-11, max_iter: int = 200, level: Optional[int] = None):
        """`mg_pcg_batch`: `pcg` for several right-hand sides of one operator in lockstep.  `f_ptrs[b]` / `x_ptrs[b]` are integer
        device addresses of `n_dofs(level)` float64 (the right-hand side; the initial guess on entry and the solution on
        return).  Returns the list of the lanes' residual histories, each bit for bit what `set_vector_device("f")`,
        `set_vector_device("v")`, `pcg`, `get_vector_device("v")` give for that lane alone.  The handle's own "v", "f" and
        "r" are unspecified afterwards."""
        level = self.finest_level if level is None else level
        nb = len(f_ptrs)
        stride = max(1, int(max_iter))
        hist = np.zeros((max(1, nb), stride))
        done = (C.c_int * max(1, nb))()
        check(self._lib.mg_pcg_batch(self._h, self._idx(level), nb, self._ptr_array(f_ptrs), self._ptr_array(x_ptrs, nb),
                                     float(rtol), int(max_iter), ptr(hist), done))
        return [hist[b, :done[b]].copy() for b in range(nb)]

    def batch_info(self) -> dict:
        """Lanes held for batched solves beyond the handle's own vectors, and their device bytes (`mg_batch_info`)."""
        lanes, b = C.c_int(), C.c_int64()
        check(self._lib.mg_batch_info(self._h, C.byref(lanes), C.byref(b)))
        return {"lanes": int(lanes.value), "bytes": int(b.value)}

    def release_batch(self):
        """Frees the lanes of batched solves (`mg_release_batch`); the next batch call allocates them again."""
        check(self._lib.mg_release_batch(self._h))

    # ---- smallest eigenpairs of the level's operator against the lumped mass M(rho) --------------------
    def eigs(self, k: int, block: Optional[int] = None, rho=None, x_ptrs=None, warm: bool = False, rtol: float = 1e-8,
             max_iter: int = 100, level: Optional[int] = None) -> dict:
        """`mg_eigs`: the `k` smallest eigenpairs of K u = lambda M(rho) u on `level` (default: the finest) by LOBPCG with one
        V-cycle per vector and iteration as preconditioner, on a block of `block` vectors (default min(MG_EIGS_MAX, k + 2); the
        vectors beyond k are guards).  `rho`: None (rho = 1), an integer device address of N^3 float64, or an array of N^3 cell
        values (uploaded for the call).  `x_ptrs`: `block` integer device addresses of `n_dofs(level)` float64 in the caller's
        DoF numbering -- the start block with `warm=True`, the M-orthonormal Ritz vectors on return; None: buffers of the call,
        returned as the NumPy array "x" of shape (block, n_dofs).  Returns {"lambda", "resid", "iterations", "restarts"[, "x"]};
        reaching `max_iter` is not an error.  The handle's own "v", "f" and "r" are unspecified afterwards."""
        level = self.finest_level if level is None else level
        block = min(_capi.MG_EIGS_MAX, int(k) + 2) if block is None else int(block)
        held = []
        try:
            if rho is None or isinstance(rho, (int, np.integer)):
                rho_ptr = None if rho is None else C.c_void_p(int(rho))
            else:
                host = _capi.as_f64(rho)
                held.append(_DeviceArray(self._lib, self.device, host.size, host))
                rho_ptr = held[-1].ptr
            own = x_ptrs is None
            if own:
                if warm:
                    raise ValueError("a warm start needs x_ptrs")
                xs = [_DeviceArray(self._lib, self.device, self.n_dofs(level)) for _ in range(max(0, block))]
                held += xs
                x_ptrs = [a.ptr.value for a in xs]
            lam, res = np.zeros(max(1, block)), np.zeros(max(1, block))
            its, restarts = C.c_int(), C.c_int()
            check(self._lib.mg_eigs(self._h, self._idx(level), int(k), block, rho_ptr, self._ptr_array(x_ptrs), int(bool(warm)),
                                    float(rtol), int(max_iter), ptr(lam), ptr(res), C.byref(its), C.byref(restarts)))
            out = {"lambda": lam[:block].copy(), "resid": res[:block].copy(), "iterations": int(its.value),
                   "restarts": int(restarts.value)}
            if own:
                out["x"] = np.stack([a.download() for a in xs])
            return out
        finally:
            for a in held:
                a.free()

    def block_gram(self, a_ptrs, b_ptrs, d_ptr=None, level: Optional[int] = None) -> np.ndarray:
        """`mg_block_gram`: the matrix a_i . (d * b_j) of vectors of `level` (default: the finest) given as integer device
        addresses of `n_dofs(level)` float64, 16-byte aligned; `d_ptr`: a nodal weight or None.  Deterministic, and a pair has
        the same bits whatever the shape of the call; the same pointers on both sides give a symmetric matrix from its upper
        tiles."""
        level = self.finest_level if level is None else level
        na, nb = len(a_ptrs), len(b_ptrs)
        out = np.zeros((max(1, na), max(1, nb)))
        check(self._lib.mg_block_gram(self._h, self._idx(level), na, self._ptr_array(a_ptrs), nb, self._ptr_array(b_ptrs),
                                      None if d_ptr is None else C.c_void_p(int(d_ptr)), ptr(out)))
        return out[:na, :nb].copy()

    def block_combine(self, s_ptrs, coeff, out_ptrs, level: Optional[int] = None):
        """`mg_block_combine`: out_o = sum_i coeff[i, o] s_i on vectors of `level` given as integer device addresses; an output
        may be one of the inputs."""
        level = self.finest_level if level is None else level
        ns, no = len(s_ptrs), len(out_ptrs)
        c = np.ascontiguousarray(np.asarray(coeff, dtype=np.float64))
        if c.shape != (ns, no):
            raise ValueError(f"coeff has shape {c.shape}, expected {(ns, no)}")
        check(self._lib.mg_block_combine(self._h, self._idx(level), ns, self._ptr_array(s_ptrs), no, ptr(c), self._ptr_array(out_ptrs)))

    def eigs_info(self) -> dict:
        """The largest block `eigs` has work vectors for, and their device bytes (`mg_eigs_info`)."""
        blk, b = C.c_int(), C.c_int64()
        check(self._lib.mg_eigs_info(self._h, C.byref(blk), C.byref(b)))
        return {"block": int(blk.value), "bytes": int(b.value)}

    def release_eigs(self):
        """Frees the work vectors of `eigs` (`mg_release_eigs`); the next call allocates them again."""
        check(self._lib.mg_release_eigs(self._h))

    def set_mass(self, level: int, M):
        """The P1 mass matrix of `level` (SciPy CSR, the level's DoF numbering) for the L2(Omega) norms of fmg."""
        indptr, is64, indices, data = _csr_arrays(M)
        check(self._lib.mg_set_mass_csr(self._h, self._idx(level), M.shape[0], data.size, ptr(indptr), is64,
                                        ptr(indices), ptr(data)))

    def set_exact(self, level: int, u):
        """Nodal values of the exact solution on `level` (error history of fmg)."""
        a = _capi.as_f64(u, self.n_dofs(level))
        check(self._lib.mg_set_exact(self._h, self._idx(level), ptr(a)))

    def counters(self) -> dict:
        """Whole-vector host <-> device copies, replayed / cached V-cycle graphs so far (tests)."""
        up, down, rep = C.c_int64(), C.c_int64(), C.c_int64()
        cached = C.c_int()
        check(self._lib.mg_counters(self._h, C.byref(up), C.byref(down), C.byref(rep), C.byref(cached)))
        return {"uploads": int(up.value), "downloads": int(down.value), "graph_replays": int(rep.value),
                "graphs_cached": int(cached.value)}

    def smoother_launches(self, level: int) -> dict:
        """What the Jacobi smoother ran on `level` since the handle was made or last reset (`mg_smoother_launches`):
        {path: (launches, sweeps, tail_launches)} for the paths that ran, path names as in `_capi.SMOOTHER_PATHS`."""
        out = {}
        for i, name in enumerate(_capi.SMOOTHER_PATHS):
            n, s, t = C.c_int64(), C.c_int64(), C.c_int64()
            check(self._lib.mg_smoother_launches(self._h, self._idx(level), i, C.byref(n), C.byref(s), C.byref(t)))
            if n.value or s.value or t.value:
                out[name] = (int(n.value), int(s.value), int(t.value))
        return out

    def reset_smoother_launches(self):
        check(self._lib.mg_reset_smoother_launches(self._h))

    def march_plan(self, level: int, sweeps: int) -> tuple:
        """(waves, planes, const_waves, const_planes) of the march plan the K-sweep march of `sweeps` sweeps per pass uses
        on `level` (`mg_march_plan`): the (tile, wave) pairs with a run of main-class planes and the planes in those
        runs, and the same for the other runs of planes with unchanging classes; zeros where there is no plan."""
        out = [C.c_int64() for _ in range(4)]
        check(self._lib.mg_march_plan(self._h, self._idx(level), sweeps, *[C.byref(v) for v in out]))
        return tuple(int(v.value) for v in out)

    def set_level_grid(self, level: int, grid_index=None):
        """Geometry + numbering only (transfer operators without a matrix)."""
        n = self.n_dofs(level)
        gi = None
        if grid_index is not None:
            gi = np.ascontiguousarray(grid_index, dtype=np.int64)
            if gi.size != n:
                raise ValueError("grid_index has the wrong length")
            if np.array_equal(gi, np.arange(n)):
                gi = None
        check(self._lib.mg_set_level_grid(self._h, self._idx(level), self.elements(level), n,
                                          ptr(gi) if gi is not None else None))

    def set_flat_level(self, A, prune_zeros: bool = True):
        """A single level holding any square CSR matrix (stand-alone smoother / residual)."""
        indptr, is64, indices, data = _csr_arrays(A)
        check(self._lib.mg_set_level_csr(self._h, 0, 0, A.shape[0], data.size, ptr(indptr), is64, ptr(indices),
                                         ptr(data), None, 1 if prune_zeros else 0))
        self._flat_n = A.shape[0]

    def time_kernel(self, kernel: str, level: int, reps: int = 20) -> float:
        ms = C.c_double()
        check(self._lib.mg_time_kernel(self._h, kernel.encode(), self._idx(level), int(reps), C.byref(ms)))
        return float(ms.value)

    def sync(self):
        check(self._lib.mg_sync(self._h))


class PointSet:
    """A located point set of one `DeviceHierarchy` (`mg_points_create`; make it with `DeviceHierarchy.points`).  The four
    `*_many` methods take one operand per lane -- a sequence of integer device addresses together with `outs`, a sequence of
    as many device addresses, and return None; or, for tests, a sequence of NumPy arrays (a (B, ...) array will do), which
    are uploaded, an array that appears twice (`a is b`) once, and return a (B, ...) NumPy array.  Every lane has the bits of
    the matching `diffusion_point_*` call.  At most `MG_BATCH_MAX` lanes per call."""

    def __init__(self, hierarchy: DeviceHierarchy, level: int, pts):
        self._hier, self._lib, self.level = hierarchy, hierarchy._lib, level
        self._ps = C.c_void_p()
        idx = hierarchy._idx(level)
        if isinstance(pts, tuple) and len(pts) == 2 and isinstance(pts[0], (int, np.integer)):
            check(self._lib.mg_points_create(hierarchy._h, idx, C.c_int64(int(pts[1])), C.c_void_p(int(pts[0])), C.byref(self._ps)))
        else:
            P = np.ascontiguousarray(np.asarray(pts, dtype=np.float64))
            if P.ndim != 2 or P.shape[1] != 3:
                raise ValueError(f"points are an (M, 3) array (got shape {P.shape})")
            d = _DeviceArray(self._lib, hierarchy.device, P.size, P.reshape(-1))
            try:
                check(self._lib.mg_points_create(hierarchy._h, idx, C.c_int64(P.shape[0]), d.ptr, C.byref(self._ps)))
            finally:
                d.free()        # the set has its own copy
        self.M = self.info["M"]

    # ---- life cycle ---------------------------------------------------------------------
    def close(self):
        """`mg_points_destroy`; a second close, or one after the hierarchy was closed (which freed the set), does nothing."""
        if getattr(self, "_ps", None) is not None and self._ps and self._hier._h:
            ps, self._ps = self._ps, C.c_void_p()
            check(self._lib.mg_points_destroy(self._hier._h, ps))
        self._ps = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self) -> C.c_void_p:
        if not self._ps:
            raise _capi.MgError("this point set has been closed")
        return self._ps

    @property
    def info(self) -> dict:
        """`mg_points_info`: the level index inside the handle and its N at creation, M, the runs of equal node among the 4 M
        sorted slots, the slots in the longest run and the set's device bytes."""
        level, N = C.c_int(), C.c_int()
        M, runs, longest, b = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        check(self._lib.mg_points_info(self._hier._h, self.handle, C.byref(level), C.byref(N), C.byref(M), C.byref(runs),
                                       C.byref(longest), C.byref(b)))
        return {"level": int(level.value), "N": int(N.value), "M": int(M.value), "runs": int(runs.value),
                "longest_run": int(longest.value), "bytes": int(b.value)}

    # ---- the four operators ---------------------------------------------------------------
    def _many(self, fn, ins, outs, n_in: int, n_out: int):
        is_address = lambda v: isinstance(v, (int, np.integer))
        ins = list(ins)
        nb = len(ins)
        if nb and all(is_address(v) for v in ins):
            if outs is None or len(outs) != nb or not all(is_address(v) for v in outs):
                raise TypeError(f"with device addresses for the {nb} lanes, outs must be {nb} device addresses too")
            check(fn(self._hier._h, self.handle, nb, DeviceHierarchy._ptr_array(ins), DeviceHierarchy._ptr_array(outs)))
            return None
        if outs is not None or any(is_address(v) for v in ins):
            raise TypeError("the lanes and outs must be all device addresses, or NumPy arrays without outs")
        held, results = {}, []
        try:
            for v in ins:
                if id(v) not in held:
                    held[id(v)] = _DeviceArray(self._lib, self._hier.device, n_in, _capi.as_f64(v, n_in))
            results = [_DeviceArray(self._lib, self._hier.device, n_out) for _ in ins]
            check(fn(self._hier._h, self.handle, nb, DeviceHierarchy._ptr_array([held[id(v)].ptr.value for v in ins]),
                     DeviceHierarchy._ptr_array([r.ptr.value for r in results])))
            return np.stack([r.download() for r in results]) if results else np.zeros((0, n_out))
        finally:
            for d in list(held.values()) + results:
                d.free()

    def sample_many(self, xs, outs=None):
        """out_b = S(x_b), M values per lane (`mg_points_sample`)."""
        return self._many(self._lib.mg_points_sample, xs, outs, self._hier.n_dofs(self.level), self.M)

    def load_many(self, ws, outs=None):
        """out_b = S^T(w_b), the level's nodes per lane (`mg_points_load`)."""
        return self._many(self._lib.mg_points_load, ws, outs, self.M, self._hier.n_dofs(self.level))

    def gradient_many(self, xs, outs=None):
        """out_b = G(x_b), 3 M values per lane, row m = (d/dx, d/dy, d/dz) at point m (`mg_points_gradient`)."""
        return self._many(self._lib.mg_points_gradient, xs, outs, self._hier.n_dofs(self.level), 3 * self.M)

    def gradient_t_many(self, ps, outs=None):
        """out_b = G^T(p_b), the level's nodes per lane (`mg_points_gradient_t`)."""
        return self._many(self._lib.mg_points_gradient_t, ps, outs, 3 * self.M, self._hier.n_dofs(self.level))
