/*
 * mg_hip.h -- C ABI of the MI355X (gfx950) geometric-multigrid V-cycle library
 * (libmg_hip.so).
 *
 * This is the drop-in boundary for the hot path of nikhilTkur/Multigrid_dolfinx.
 * The reference has no FFI of its own: its boundary is the Python function surface
 * of multigrid.py.  Each entry point below names the reference interface it
 * replaces (file:line in the reference).  The only intended caller is the ctypes
 * shim multigrid_dolfinx_amd/_capi.py; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain C types, host pointers, caller owns every buffer it passes in;
 *   - every function returns 0 on success, non-zero on failure; the message is
 *     available from mg_last_error() (thread-local);
 *   - levels are numbered 0 (coarsest) .. n_levels-1 (finest); level l has
 *     N_l = N_0 * 2^l elements per dimension and (N_l+1)^dim unknowns
 *     (multigrid.py:247-248);
 *   - vectors crossing the boundary are fp64 in the CALLER's DoF numbering; the
 *     library keeps them in lexicographic grid numbering internally and permutes
 *     at this edge using the grid_index given to mg_set_level_csr;
 *   - one handle = one hierarchy on one GPU (or one slab of it, see mg_set_comm);
 *     calls on a handle are serialised on the handle's HIP stream; there is no
 *     global state in the library (the reference's module globals,
 *     multigrid.py:10-45, live in the Python shim only).
 */
#ifndef MG_HIP_H
#define MG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mg_context* mg_handle;

/* which per-level device vector an accessor refers to */
enum mg_vec {
    MG_VEC_V = 0,   /* iterate / correction v_h                                    */
    MG_VEC_F = 1,   /* right-hand side f_h (restricted residual on coarse levels)   */
    MG_VEC_R = 2,   /* residual r_h = f_h - A v_h of the last mg_residual / V-cycle */
    MG_VEC_ERR = 3  /* interpolated coarse correction err_h (multigrid.py:258-259),  */
                    /* kept only when mg_set_params(... keep_err = 1)                */
};

enum mg_restriction {
    MG_RESTRICT_INJECTION = 0,      /* Restriction2D_direct, multigrid.py:123-132 (the live path, :251-252) */
    MG_RESTRICT_FULL_WEIGHTING = 1, /* Restriction2D,        multigrid.py:135-198                            */
    MG_RESTRICT_TABLE = 2,          /* transpose of the table prolongation (mg_set_restriction_table); no reference */
    MG_RESTRICT_P1_TRANSPOSE = 3    /* R = P^T of the P1 natural embedding (mg_set_prolongation_p1); no reference */
};

enum mg_smoother {
    MG_SMOOTH_JACOBI = 0,           /* jacobiRelaxation, multigrid.py:223-228 */
    MG_SMOOTH_RBGS = 1,             /* red-black Gauss-Seidel / SOR with factor omega (no reference;
                                       BASELINE.json config 5): per sweep one in-place half sweep per
                                       colour, colour = parity of the lexicographic node index.  Needs
                                       pruned grid matrices (P1 stencils are then bipartite). */
    MG_SMOOTH_MCGS = 2,             /* nine-colour Gauss-Seidel / SOR for P2 rows (BASELINE.json config 5; no
                                       reference): the seven parity classes of the lattice's mid-points plus the
                                       vertices split red / black; one in-place launch per colour in ascending
                                       order.  Valid for pruned P2 and P1 grid matrices (checked per level). */
    MG_SMOOTH_CHEBYSHEV = 3         /* Chebyshev polynomial in D^-1 A (no reference; mg_set_chebyshev below): mu1 / mu2
                                       (nw of mg_smooth) are the polynomial's degree, each call a fresh polynomial from
                                       MG_VEC_V, one matrix application per degree.  omega is ignored. */
};

/* ---- life cycle ----------------------------------------------------------------
 * Replaces the module-global problem state set by initialize_problem
 * (multigrid.py:28-45) with an explicit handle. */
int mg_create(int n_levels, int dim, int device, mg_handle* out);
int mg_destroy(mg_handle h);
const char* mg_last_error(void);
/* "gfx950 <n_cus> CUs" style description of the device the handle runs on. */
int mg_device_info(mg_handle h, char* buf, size_t buflen);

/* ---- multi-GPU (no reference counterpart) -----------------------
 * One process per GPU.  Must be called before any level is set.  The finest
 * levels are split into contiguous slabs of grid planes (slowest axis), aligned so
 * that coarse plane K lives with fine plane 2K; levels with fewer than
 * `replicate_below` unknowns are replicated on every rank (no communication below
 * that size).  `nccl_unique_id` is the 128-byte RCCL id obtained on rank 0 with
 * mg_comm_unique_id and distributed by the caller (bench.py uses torch.distributed
 * for that rendezvous only).  Halo planes and scalar reductions then travel over
 * RCCL/xGMI. */
int mg_comm_unique_id(void* id_out, size_t id_bytes);
int mg_set_comm(mg_handle h, int rank, int world, const void* nccl_unique_id, size_t id_bytes,
                int64_t replicate_below);
/* Exercises every RCCL entry point the library uses (id, init, all-reduce, broadcast, grouped
 * send/recv, destroy) on a one-rank communicator of `device`; 0 = all results correct. */
int mg_comm_selftest(int device);
/* Host-staged transport for tests without RCCL peers: the library stages device
 * buffers through host memory and calls back into the caller (who moves the bytes,
 * e.g. over gloo).  exchange: send `count` doubles to rank-1 / rank+1 (NULL pointer
 * = no such neighbour) and receive as many from each.  allreduce: in-place sum of
 * `count` doubles over all ranks.  allgatherv: counts[r] doubles from every rank r
 * into recv (rank order). */
typedef int (*mg_exchange_fn)(void* user, const double* send_lo, const double* send_hi,
                              double* recv_lo, double* recv_hi, int64_t count);
typedef int (*mg_allreduce_fn)(void* user, double* inout, int64_t count);
typedef int (*mg_allgatherv_fn)(void* user, const double* send, int64_t send_count,
                                double* recv, const int64_t* counts);
int mg_set_comm_callbacks(mg_handle h, int rank, int world, mg_exchange_fn ex, mg_allreduce_fn ar,
                          mg_allgatherv_fn ag, void* user, int64_t replicate_below);

/* ---- hierarchy set-up --------------------------------------------------------------
 * mg_set_level_csr: hand over one level's stiffness matrix exactly as
 * scipy.sparse.csr_matrix((av, aj, ai)) holds it after PETSc getValuesCSR()
 * (Multigrid_prototype.py:95-99): fp64 values, int32 column indices, row pointers
 * int32 or int64 (indptr_is_64).  The contract for the three arrays: columns may
 * come in any order within a row, explicit zeros (0.0 and -0.0) may be stored
 * anywhere within reach of the row.  A row's kept entries are stored in ascending
 * grid column whatever order they came in, so all of these describe the same level,
 * with the same storage format, row classes and order of summation as the sorted,
 * zero-free form -- except that under prune_zeros = 0 a stored zero is an entry of
 * the pattern like any other: a zero on an offset no other row uses is a new
 * diagonal of the pattern and can change the format the level gets, and a row
 * with a kept zero is a row of its own in the stencil classes of a level without
 * symmetric diagonals (more classes, or none past 255).  Duplicate (row, column)
 * entries are REFUSED, not summed: sum them first (A.sum_duplicates()) -- a1 x + a2 x
 * and (a1 + a2) x round differently, and the compact formats keep one slot per
 * diagonal.  Structural errors -- indptr[0] != 0, a decreasing indptr,
 * indptr[n_rows] != nnz, a column index outside [0, n_rows) -- are refused too.
 * Both are found by mg_csr_check on the host before anything is freed, allocated,
 * uploaded or launched: a refused hand-off leaves the level as it was.  The same
 * holds for mg_set_level_csr_local (columns in [0, n_cols)), mg_set_mass_csr and
 * flat levels.  `grid_index[dof]` is the lexicographic node index
 * i + (N+1)(j + (N+1)k) of each DoF -- the integer form of the reference's
 * coordinate dictionaries (Multigrid_prototype.py:68-74); NULL means the DoFs are
 * already lexicographic.  The library renumbers once (P A P^T), optionally drops
 * explicit zeros (prune_zeros; the reference's own smoother matrix drops them too,
 * multigrid.py:52-55, App. A Q7) and stores sliced-ELL tiles.  This subsumes
 * getJacobiMatrices (multigrid.py:48-56): D^-1 is extracted here and the smoother
 * streams A itself (v + w D^-1 (f - A v)), so no second matrix is stored.
 * In slab mode every rank passes the full matrix (mg_set_level_csr_local takes the rank's rows only) and keeps its own planes. */
int mg_set_level_csr(mg_handle h, int level, int elements_per_dim, int64_t n_rows, int64_t nnz,
                     const void* indptr, int indptr_is_64, const int32_t* indices,
                     const double* data, const int64_t* grid_index, int prune_zeros);
/* The structural check every host CSR hand-off starts with; pure host code, usable without a device.  0 if
 * (indptr, indices) describe an n_rows x n_cols CSR pattern of nnz entries; otherwise 1 and mg_last_error names the cause
 * and, where there is one, the row and column in the caller's numbering: indptr[0] != 0, indptr[i + 1] < indptr[i],
 * indptr[n_rows] != nnz, a column index < 0 or >= n_cols and, unless allow_duplicates, a (row, column) pair stored twice
 * ("row r holds column c twice; sum duplicates before the hand-off (A.sum_duplicates())").  Two linear passes, no sorting:
 * the row pointers first, then the entries against an n_cols array of "last row that touched this column".
 * mg_jacobi_split calls it with allow_duplicates = 1 (duplicates sum there, as in SciPy), the level and mass hand-offs
 * with 0.  Device-built matrices (mg_galerkin_level) do not pass through it. */
int mg_csr_check(int64_t n_rows, int64_t n_cols, int64_t nnz, const void* indptr, int indptr_is_64,
                 const int32_t* indices, int allow_duplicates);
/* Per-rank hand-off for slabs: the rank passes ONLY the rows it owns (mg_level_slab says which: the lexicographic
 * nodes [row0, row0 + n_local) of the level, plus how many halo nodes it may couple to on either side), in a local
 * numbering like a distributed assembly has it (PETSc's owned + ghost layout behind getValuesCSR(),
 * Multigrid_prototype.py:95-96): row r of the CSR is local id r, column indices are local ids in [0, n_cols), and
 * col_nodes[id] names the global lexicographic node of every local id (ids < n_rows: the owned rows, in any order; the
 * rest: ghosts).  grid_index (n_global entries, or NULL for lexicographic) still maps the caller's GLOBAL DoF numbers to
 * nodes for the vector calls.  Replicated levels take the whole matrix this way too (n_rows = n_global).  Results are
 * those of the full-matrix hand-off bit for bit.  No reference counterpart (the reference is serial). */
int mg_level_slab(mg_handle h, int level, int elements_per_dim, int64_t* row0, int64_t* n_local, int64_t* halo_lo,
                  int64_t* halo_hi);
int mg_set_level_csr_local(mg_handle h, int level, int elements_per_dim, int64_t n_rows, int64_t n_cols, int64_t nnz,
                           const void* indptr, int indptr_is_64, const int32_t* indices, const double* data,
                           const int64_t* col_nodes, const int64_t* grid_index, int prune_zeros);
/* A level with grid geometry and numbering only (no matrix): enough for the transfer
 * operators, which the reference exposes as free functions taking two coordinate
 * dictionaries (Interpolation2D / Restriction2D(_direct), multigrid.py:59, :123, :135). */
int mg_set_level_grid(mg_handle h, int level, int elements_per_dim, int64_t n_rows,
                      const int64_t* grid_index);   /* elements_per_dim == 0: flat vector space */
/* Device-side synthetic generator (bench/tests; no reference counterpart): writes
 * the same tiles and right-hand side that poisson.make_level + mg_set_level_csr
 * would produce for the P1 Poisson problem of Multigrid_prototype.py:77-110
 * (lexicographic numbering), without a host CSR -- the only way to set up 1025^3
 * unknowns.  Also fills MG_VEC_F with the lifted right-hand side. */
int mg_gen_poisson_level(mg_handle h, int level, int elements_per_dim, int prune_zeros);
/* The same for elements whose unknowns fill a lattice with one row per parity class of the lattice point -- P2 on the
 * structured simplicial mesh, BASELINE.json config 5 (no reference counterpart: the reference is P1 only).  The
 * caller hands over, for each of the eight classes (i & 1) | (j & 1) << 1 | (k & 1) << 2, the interior stencil as
 * count[class] (offset, value) pairs -- offsets[class][t][3] = (di, dj, dk) in ascending column order, at most
 * 64 per class, values[class][t] for this level's mesh width -- and the load of the constant source; the device writes
 * the tiles with the reference's boundary treatment (identity rows, zeroed columns, lifted right-hand side,
 * Multigrid_prototype.py:77-108).  `lattice_steps` = lattice points per dimension - 1 (even).  Single GPU. */
int mg_gen_lattice_level(mg_handle h, int level, int lattice_steps, int width, const int* count, const int* offsets,
                         const double* values, const double* load);
/* Variable-coefficient diffusion level (no reference counterpart): the P1 matrix of -div(kappa grad u) on the Kuhn mesh of
 * mg_gen_poisson_level, with kappa one positive double per cell -- 3-D cube (ci, cj, ck) at (ck * N + cj) * N + ci, 2-D square
 * (ci, cy) at cy * N + ci, x fastest -- shared by all simplices of the cell.  Every simplex of that mesh has a right dihedral
 * angle at each non-axis edge, so the rows keep the five- / seven-point shape of the Poisson level: the axis edge between
 * node i and neighbour j gets a_ij = -(sum_c n_c kappa_c) h / 6 (3-D) or -(sum_c kappa_c) / 2 (2-D), c the cells holding the
 * edge in ascending index, n_c = 2 where the cell's corner at the edge has both other local coordinates equal, else 1; the
 * diagonal is the sum of the row's edge sums (ascending offset order), scaled the same way.  Boundary rows, zeroed columns
 * and the lifted right-hand side as mg_gen_poisson_level; kappa == 1 gives its level bit for bit.  a_ij and a_ji have the
 * same bits, so the level is bit-symmetric.  The level then gets the storage analysis, row classes and escape rows of any
 * level; "gen_odd_rows" does not apply.  `kappa` holds all N^dim cells of the level on the host; on slabs every rank passes
 * the whole array (as for mg_set_vector) and only the cell planes its owned rows read are uploaded.  A kappa that is not
 * positive and finite is refused, naming the first bad cell (found on the device), and the level is left as it was.  The
 * device copy of kappa is freed on return.  poisson.diffusion_level is the host restatement. */
int mg_gen_diffusion_level(mg_handle h, int level, int elements_per_dim, const double* kappa, int prune_zeros);
/* Levels top_level .. 0 from one kappa of the top level (elements_per_dim cells per dimension): each coarser level's kappa
 * is coarsened on the device from the level above -- the 2^dim children in ascending lexicographic order, summed one by
 * one, x 2^-dim (MG_KAPPA_ARITHMETIC) or 2^dim / sum of 1 / kappa (MG_KAPPA_HARMONIC); poisson.coarsen_kappa restates it --
 * and every level is generated as mg_gen_diffusion_level(..., prune_zeros = 1) would.  At most two kappa fields are on the
 * device at a time, none after return.  Needs a whole (not slab) handle and an even elements_per_dim on every level above
 * level 0; on slabs, call mg_gen_diffusion_level per level. */
enum mg_kappa_averaging {
    MG_KAPPA_ARITHMETIC = 0,
    MG_KAPPA_HARMONIC = 1
};
int mg_gen_diffusion_hierarchy(mg_handle h, int top_level, int elements_per_dim, const double* kappa_top, int averaging);
/* Matrix-free storage of the same level (opt-in; 3-D, whole handles, prune_zeros = 1): the level keeps the device kappa
 * (8 B per row) and its right-hand side and stores no matrix at all -- no ELL tiles, diagonals, row classes or 1 / diagonal.
 * Jacobi sweeps, residuals, the SpMV of mg_pcg and of the Chebyshev estimate and Chebyshev steps rebuild each row from the
 * eight cells around its node while they march through the planes (mg_diffusion_mf.hip.h, one step per launch, counted under
 * MG_PATH_MATRIX_FREE): 32 B per row and sweep instead of 56, 24 instead of 48 for the SpMV, 40 instead of 64 for a
 * Chebyshev step.  The row is defined by the level mg_gen_diffusion_level(..., 1) stores and every result has the bits that
 * level's one-step kernel gives (finite iterates; the p.q partial sums of the SpMV are per workgroup, so mg_pcg agrees to
 * rounding, not to bits).  Transfers run unfused (residual, then the transfer kernel).  Refused with an error: 2-D handles,
 * slab handles, level 0 (the coarsest level is factorised by the direct solve and read row by row by the coarse CG: it is
 * always stored), mg_galerkin_level of such a level (it reads stored rows), Gauss-Seidel smoothers with such a level in
 * the cycle (mg_smooth, mg_vcycle, mg_prepare_cycle, mg_fmg and mg_pcg refuse before anything is launched).  A bad kappa is
 * refused as mg_gen_diffusion_level refuses it. */
int mg_gen_diffusion_level_mf(mg_handle h, int level, int elements_per_dim, const double* kappa);
/* mg_gen_diffusion_hierarchy with matrix-free levels: levels above level 0 with at least min_rows rows keep their kappa
 * and no matrix; smaller levels and always level 0 (which the direct solve factorises) are stored as today. */
int mg_gen_diffusion_hierarchy_mf(mg_handle h, int top_level, int elements_per_dim, const double* kappa_top, int averaging,
                                  int64_t min_rows);
/* The same hierarchy from a kappa that is on the device already (opt-in): mg_gen_diffusion_hierarchy (mf_min_rows < 0) or
 * mg_gen_diffusion_hierarchy_mf (mf_min_rows >= 0, its min_rows), every result bit for bit the same.  kappa_dev: the
 * elements_per_dim^dim doubles of the top level in device memory of the handle's device, cell order as in
 * mg_gen_diffusion_level.  The caller's buffer is only read, never written and never taken over: a matrix-free top level
 * keeps its own copy, written by the pass that coarsens it (kappa_ingest, mg_diffusion_kappa.hip.h: the fine field read
 * once, the copy and the coarse field written, 17 B per fine cell in 3-D against 8 + 8 for a copy and 8 + 1 for a
 * coarsening pass of its own); the levels below take over the coarsened fields as in the host call.  Nothing of kappa crosses to the
 * host but the flag of the check and, in a refusal, the one bad value.  Runs on the handle's stream, which is synchronised
 * before return; the caller must have finished producing kappa (the contract of mg_set_vector_device).  Refused with an
 * error before any level is touched: a null pointer, a pointer that is not device memory of the handle's device, slab
 * handles, 2-D handles with mf_min_rows >= 0, an elements_per_dim that is not N0 * 2^top_level, an unknown averaging, and
 * a kappa that is not positive and finite, named by its first bad cell as mg_gen_diffusion_level names it.  As in the host
 * call only the top level's kappa is checked: the coarsened fields are not (averages of positive finite values can still
 * overflow). */
int mg_gen_diffusion_hierarchy_device(mg_handle h, int top_level, int elements_per_dim, const double* kappa_dev, int averaging,
                                      int64_t mf_min_rows);
/* Another kappa for levels top_level .. 0 of a hierarchy that one of the three diffusion hierarchy calls generated (the
 * handle remembers that per level, with the level's size; setting a level in any other way forgets it), without tearing it
 * down: afterwards the handle is in the state mg_gen_diffusion_hierarchy_device with this kappa and the same split into
 * stored and matrix-free levels leaves -- right-hand sides, MG_VEC_V and MG_VEC_R zeroed, every result of every later call
 * and mg_memory_bytes bit for bit.  Matrix-free levels keep their kappa buffer, their vectors and their mg_pcg work
 * vectors: nothing is freed or allocated for them, kappa is overwritten in place (the top level's by kappa_ingest, from the
 * caller's buffer; a matrix-free level below is the coarse field the pass above wrote) and MG_VEC_F and the true right-hand
 * side are recomputed.  Stored levels -- with min_rows set, the small ones -- are rebuilt from the device kappa by the
 * pipeline of mg_gen_diffusion_level.  What the old matrices fed does not survive: level 0's direct factorisation, every
 * captured V-cycle, and the Chebyshev estimate of every level (matrix-free ones included); all are rebuilt at next use, so
 * mg_memory_bytes is lower by the factorisation until then.  Intervals set by mg_set_chebyshev_bounds stay, as they do
 * across a generation.  kappa_dev, averaging, stream and synchronisation as in mg_gen_diffusion_hierarchy_device.
 * Refused by name, the handle left as it was (the old hierarchy stays fully usable): slab handles, a null pointer or one
 * that is not device memory of the handle's device, an unknown averaging, a level in top_level .. 0 that is not set or was
 * set from CSR, by mg_gen_poisson_level, by mg_galerkin_level or generated singly, and a kappa that is not positive and
 * finite -- found by a read-only pass over the caller's buffer before anything is written.  The coarsened fields are not
 * validated, as in the hierarchy calls. */
int mg_refresh_diffusion_hierarchy(mg_handle h, int top_level, const double* kappa_dev, int averaging);
/* No-flux (Neumann) faces for the generated diffusion levels (no reference counterpart).  dirichlet_faces is the set of the
 * faces of the unit cube that carry the Dirichlet condition, one bit per face (enum mg_face; the default, MG_FACES_ALL = 63,
 * is every call's behaviour before this entry existed, bit for bit and launch for launch).  A node on a face of the set is a
 * Dirichlet node: an identity row with the boundary data, its columns zeroed and lifted into the right-hand side.  Every
 * other node is a free node, the boundary nodes that lie only on faces outside the set included: such a node gets the
 * natural row of the P1 matrix -- the edge sums, the diagonal sum and the scaling of an interior row with a cell outside the
 * grid counting as +0.0 and no column outside the grid -- and the load f h^3 (T / 24), T the number of Kuhn simplices at the
 * node that lie inside the grid (24 inside).  That is the no-flux condition; a prescribed flux is a load added on those nodes
 * (mg_set_vector).  The level stays symmetric to the bit.
 * The set is handle state, read when levels are generated: mg_gen_diffusion_level[_mf], the three hierarchy calls, and
 * mg_refresh_diffusion_hierarchy, which refuses if it differs from the set the levels were generated with.  Each level
 * remembers its set: the matrix-free march, the P1-transpose restriction (a free coarse node on a no-flux face sums the
 * pattern without the offsets that leave the grid; a Dirichlet coarse node takes the coincident value) and mg_memory_bytes
 * follow it.  MG_NODES_INTERIOR of the sensitivity entries below means the free nodes of the handle's set.
 * Refused by name, the handle left as it was: 0 (no Dirichlet face: the operator would be singular), values outside 0..63,
 * and on 2-D handles and slab handles any value but 63.  A handle that is made a slab handle after a set other than 63 was
 * set is refused where the set is read: by the generating calls and the sensitivity entries.
 * With levels of another set than 63, three things are refused before anything is launched:
 *   - mg_vcycle, mg_prepare_cycle, mg_fmg and mg_pcg whose transfers are not the P1 prolongation (mg_set_prolongation_p1)
 *     with MG_RESTRICT_P1_TRANSPOSE, and single mg_restrict / mg_prolong calls of another kind on such levels;
 *   - the same calls over levels that were generated with different sets;
 *   - mg_galerkin_level. */
enum mg_face { MG_FACE_XLO = 1, MG_FACE_XHI = 2, MG_FACE_YLO = 4, MG_FACE_YHI = 8, MG_FACE_ZLO = 16, MG_FACE_ZHI = 32, MG_FACES_ALL = 63 };
int mg_set_diffusion_faces(mg_handle h, int dirichlet_faces);
/* *dirichlet_faces = the handle's face set */
int mg_diffusion_faces(mg_handle h, int* dirichlet_faces);
/* Insulated bodies: no Dirichlet node at all (no reference counterpart).  mg_set_diffusion_insulated puts the handle's face
 * set at "no Dirichlet node": mg_diffusion_faces then reports 0, every node of a level generated from now on is a free node
 * with the natural row, and Robin fields may sit on any of the six faces.  3-D whole handles only: 2-D and slab handles are
 * refused by name, the handle left as it was.  A later mg_set_diffusion_faces with a valid set leaves the state;
 * mg_set_diffusion_faces(h, 0) stays refused as before.  Everything a face set other than 63 refuses stays refused.
 * With every node free A(kappa) has zero row sums: its null space is the constants.  Two cases, by what the levels held
 * when they were generated:
 *   - regular: a reaction diagonal (mg_set_diffusion_reaction) or at least one Robin diagonal (mg_set_diffusion_robin)
 *     makes the operator regular, and every call works as on any face set; nothing is projected.  A field that is zero
 *     everywhere is the caller's mistake: the solve does not converge.
 *   - singular: neither.  Let w be the lumped mass of rho = 1 on the all-free grid (w_i = the integral of the hat
 *     function, reaction_diag of ones), s = w.1, Q = I - 1 w^T / s.  mg_pcg computes x = Q A^+ Q^T b, that is
 *         A x = b - w (1.b) / s,   w.x = 0:
 *     a uniform source density is taken off the load to make it compatible, and the solution has integral zero.
 *     mg_pcg turns the right-hand side into Q^T b once, makes every preconditioned residual mean-free (Euclidean
 *     weights) before it is used, returns Q x in MG_VEC_V and tests ||r|| <= rtol ||Q^T b||.  A projected right-hand side
 *     of zero gives Q x0 after zero iterations.  MG_VEC_F holds the projected load Q^T b after the call (not the caller's
 *     b), and MG_VEC_R = Q^T b - A x.  The coarsest level is factorised with node 0 pinned (identity row, column dropped),
 *     solved with a mean-free right-hand side and made mean-free: the pseudo-inverse for a consistent load, in the same
 *     launches as the regular solve and in a captured cycle; the coarse CG ("coarse_direct" 0) gets the same two
 *     projections.  mg_vcycle and mg_prepare_cycle work.  Refused by name in the singular case, before anything is
 *     launched: mg_pcg_batch, mg_eigs, mg_fmg, and cycles with the Chebyshev or a Gauss-Seidel smoother.
 * w lives with the handle (built at the first projected solve, counted in mg_memory_bytes, freed with the handle). */
int mg_set_diffusion_insulated(mg_handle h);
/* *singular = 1 where solves from `level` run projected: the levels 0 .. level were generated on an insulated handle and
 * none of them holds a reaction or Robin diagonal; else 0 */
int mg_diffusion_nullspace(mg_handle h, int level, int* singular);
/* x -= mean in place over n doubles of device memory, *mean = the mean removed: (w.x) / (w.1) with weights, (1.x) / n with
 * w_dev null.  x_dev and w_dev are 16-byte aligned.  Deterministic: per-workgroup partial sums in a fixed order over a grid
 * that depends on n only, folded by one block; no floating-point atomics, the same bits on every run. */
int mg_remove_mean(mg_handle h, double* x_dev, const double* w_dev, int64_t n, double* mean);
/* A lumped reaction term for the generated diffusion levels (no reference counterpart): the operator A(kappa) + R(sigma) of
 * -div(kappa grad u) + sigma u, R diagonal.  sigma is one double per cell of a 3-D grid of elements_per_dim^3 cells, in the cell
 * order of mg_gen_diffusion_level, finite and >= 0 (zero is allowed).  R of a cell field w is the row-sum lumped P1 mass of the
 * Kuhn mesh with the weights of the load:
 *     R(w)_i = ((sum over the 8 cells c around node i, in ascending index, of t_{c,i} w_c) / 24) * h^3,   h = 1 / N,
 * t = 6 where i is the cell's (0,0,0) or (1,1,1) corner, else 2; a cell outside the grid counts as +0.0 (w == 1: the load of
 * f == 1 on a free node).  A free row of a generated level gets diag = (the stiffness diagonal as before) + R(sigma)_i, one
 * more addition; Dirichlet rows stay identity rows; off-diagonals, the lifted right-hand side and the load do not change.
 * One implicit Euler step of du/dt - div(kappa grad u) = f is the solve with sigma = 1 / dt and the right-hand side
 * b + R(1 / dt) u_old.  Summation order: reaction_diag (mg_kernels.hip.h); poisson.reaction_diag and
 * poisson.diffusion_level(sigma=...) restate it bit for bit.
 * The field is handle state, like the face set: the handle keeps its own device copy (counted by mg_memory_bytes), and it is
 * read where levels are generated -- mg_gen_diffusion_level[_mf], the three hierarchy calls and
 * mg_refresh_diffusion_hierarchy.  A generating call whose elements_per_dim (the top level's, for a hierarchy) differs from the
 * field's is refused by name before any level is touched.  Coarse levels rediscretise with the arithmetic mean of the 2^3
 * children, whatever `averaging` says for kappa (mass is additive).  Each level remembers whether it was generated with a
 * reaction diagonal (mg_level_reaction); a matrix-free level keeps the nodal R(sigma), 8 bytes per row, and its march reads it
 * (40 bytes per row and sweep instead of 32).  mg_refresh_diffusion_hierarchy is refused if the handle has a field and the
 * levels were generated without one, or the reverse; the values may differ (a new dt, a new sigma iterate).  A handle that
 * never sets a field launches the kernels and allocates the bytes it did before these entries existed.
 * A null pointer clears the field.  The device variant takes its pointer under the contract of
 * mg_gen_diffusion_hierarchy_device (device memory of the handle's device, complete before the call; it is copied on the
 * handle's stream, which is synchronised before return).  Refused by name, the handle left as it was: 2-D handles, slab
 * handles (a handle made a slab handle after the field was set is refused at the generating calls), a non-positive
 * elements_per_dim, a device pointer to the host variant, a pointer that is not device memory of the handle's device to the
 * device variant, and a sigma that is negative or not finite, the first such cell named.  The face set 0 stays refused as
 * singular whatever sigma is. */
int mg_set_diffusion_reaction(mg_handle h, int elements_per_dim, const double* sigma_host);
int mg_set_diffusion_reaction_device(mg_handle h, int elements_per_dim, const double* sigma_dev);
/* *on = 1 if the handle holds a reaction field, *elements_per_dim = its cells per dimension (0, 0 otherwise) */
int mg_diffusion_reaction(mg_handle h, int* on, int* elements_per_dim);
/* *on = 1 if the level was generated with a reaction diagonal */
int mg_level_reaction(mg_handle h, int level, int* on);
/* Robin (convective) faces for the generated diffusion levels (no reference counterpart): on a face outside the Dirichlet
 * set the condition
 *     kappa du/dn + alpha (u - u_ext) = 0,   alpha >= 0 varying over the face,
 * instead of the no-flux condition (alpha == 0).  A field belongs to one face (`face`: exactly one bit of enum mg_face) and
 * holds elements_per_dim^2 doubles, one per boundary face-cell, finite and >= 0.  With (a, b) the two in-plane axes of the
 * face in ascending order -- x-faces: (y, z), y-faces: (x, z), z-faces: (x, y) -- face-cell (ca, cb) sits at cb * N + ca.
 * The Kuhn split cuts every boundary face-cell into two triangles along the diagonal from its in-plane (0,0) to its (1,1)
 * corner; the row-sum lumped P1 boundary mass gives each vertex of a triangle h^2 / 6.  For a free node i on a field face F
 *     b_F(alpha)_i = ((sum over the 4 face-cells q of F around i, in ascending index (db, da), of t_{q,i} alpha_q) / 6.0) * h^2,
 * t = 2 where i is the face-cell's in-plane (0,0) or (1,1) corner, else 1; a face-cell outside the face counts as +0.0; one
 * accumulator starts with the first product and takes the others one by one; h^2 = pow(h, 2) from the host.  B(alpha)_i is
 * the sum of b_F over the field faces that contain i in ascending face-bit order, the first term starting the accumulator,
 * and +0.0 on every node on no field face and on every Dirichlet node (alpha == 1 on a face: the face load of q == 1).
 * A free row of a generated level gets diag = (the stiffness diagonal as before) + d_i by one more addition, with
 * d_i = B(alpha)_i, or d_i = R(sigma)_i + B(alpha)_i, formed as that sum, where the handle also holds a reaction field.
 * Off-diagonals, identity rows, the lifted right-hand side and the load do not change; the ambient load
 * alpha u_ext int phi_i is mg_diffusion_apply_drobin(alpha, u_ext), which the caller adds to its right-hand side.
 * Summation order: robin_diag (mg_kernels.hip.h); poisson.robin_diag and poisson.diffusion_level(robin=...) restate it bit
 * for bit.
 * The fields are handle state, like the reaction field: the handle keeps its own device copies (counted by
 * mg_memory_bytes), and they are read where levels are generated -- mg_gen_diffusion_level[_mf], the three hierarchy calls
 * and mg_refresh_diffusion_hierarchy.  Coarse levels rediscretise with the arithmetic mean of the 2 x 2 children face-cells,
 * whatever `averaging` says for kappa (boundary mass is additive).  Each level remembers the faces it was generated with
 * (mg_level_robin); mg_level_reaction keeps meaning "generated with sigma".  A matrix-free level keeps the nodal
 * B(alpha), or R(sigma) + B(alpha), 8 bytes per row, and its march is that of the reaction term (40 bytes per row and sweep
 * instead of 32, also without a reaction field: a march that formed B from the face fields was measured slower).
 * A handle that never sets a field launches the kernels and allocates the bytes it did before these entries existed.
 * A null pointer clears the field of that face.  The device variant takes its pointer under the contract of
 * mg_set_diffusion_reaction_device.  Refused by name, the handle left as it was: 2-D handles, slab handles, a `face` that is
 * not exactly one bit, a non-positive elements_per_dim or one other than that of the fields held on other faces, a device
 * pointer to the host variant and the reverse, and an alpha that is negative or not finite, the first such face-cell named.
 * The generating calls refuse, before any level is touched, a field on a face of the handle's Dirichlet set and an
 * elements_per_dim other than the fields'; mg_refresh_diffusion_hierarchy refuses a set of field faces other than the
 * levels' (the values may differ).  The face set 0 stays refused as singular whatever alpha is. */
int mg_set_diffusion_robin(mg_handle h, int elements_per_dim, int face, const double* alpha_host);
int mg_set_diffusion_robin_device(mg_handle h, int elements_per_dim, int face, const double* alpha_dev);
/* *faces = the faces on which the handle holds a Robin field (bits of enum mg_face), *elements_per_dim = their face-cells per
 * dimension (0, 0 without a field) */
int mg_diffusion_robin(mg_handle h, int* faces, int* elements_per_dim);
/* *faces = the faces whose Robin field the level was generated with (0: none) */
int mg_level_robin(mg_handle h, int level, int* faces);
/* *on = 1 if the level is matrix-free, *kappa_bytes = the device bytes of its kappa (0 otherwise) */
int mg_level_matrix_free(mg_handle h, int level, int* on, int64_t* kappa_bytes);
/* Sensitivity of the diffusion operator to kappa (no reference counterpart): out_dev[c] = d(a^T A(kappa) b) / d kappa_c for the
 * N^3 cells c of a 3-D level, cell order as in mg_gen_diffusion_level.  A is linear in kappa, so neither kappa nor a matrix is read,
 * only the level's grid dimensions: any whole 3-D grid level will do, stored, matrix-free or grid-only.  With a~, b~ = a, b with
 * the boundary nodes taken as 0 (boundary rows are identity rows, interior rows have no boundary column),
 *     out[c] = (h / 6) * sum over the 12 axis edges e = (i, j) of cell c of n_{c,e} (a~_i - a~_j) (b~_i - b~_j),   h = 1 / N,
 * n_{c,e} = 2 where the cell's two other local coordinates at the edge are equal, else 1 (the weights of
 * mg_gen_diffusion_level).  Summation order: mg_diffusion_adj.hip.h; poisson.diffusion_dkappa restates it bit for bit.
 * a_dev, b_dev: device arrays of the level's n_global doubles in lexicographic node order (the numbering of generated
 * levels), possibly the same pointer; out_dev: N^3 doubles on the device.  Runs on the handle's stream, which is synchronised
 * before return (the caller must have finished producing a and b); nothing crosses to the host.  With u = A^-1 f and the
 * adjoint solve A lambda = dJ/du (A is symmetric: the same hierarchy, one more mg_pcg), dJ/dkappa = -out(lambda, u).
 * Refused with an error: 2-D handles, slab handles, flat levels, null pointers and pointers that are not device memory of the
 * handle's device. */
int mg_diffusion_dkappa(mg_handle h, int level, const double* a_dev, const double* b_dev, double* out_dev);
/* The tangent of the diffusion operator in a direction of kappa (no reference counterpart), the forward-mode half of what
 * mg_diffusion_dkappa is the reverse-mode half of: out_dev = (dA/dkappa . dkappa) x, the derivative of the product A(kappa) x of
 * mg_gen_diffusion_level's matrix along dkappa.  A is linear in kappa, so an interior row is the row the matrix-free march
 * rebuilds with kappa := dkappa (mg_diffusion_mf.hip.h: the same edge sums, (s / 6.0) * h, zero entries towards boundary
 * neighbours, the same fma order -- the bits of that SpMV where dkappa is a kappa), and a boundary row is +0.0: the identity
 * block does not depend on kappa.  a . out(w, x) = w . mg_diffusion_dkappa(a, x) for a with zero boundary entries.  Neither
 * the level's kappa nor a matrix is read: any whole 3-D grid level will do, stored, matrix-free or grid-only.
 * dkappa_dev: N^3 doubles in the cell order of mg_gen_diffusion_level, of any sign, zeros included (finiteness is the caller's
 * business, as for any vector); x_dev, out_dev: the level's n_global doubles in lexicographic node order.  All three are device
 * memory; runs on the handle's stream, which is synchronised before return (the caller must have finished producing dkappa
 * and x); nothing crosses to the host.  The tangent solve: du = A^-1 (df - out(dkappa, u)); poisson.diffusion_apply_dkappa
 * restates it in NumPy (no fma there: to a bound, not to the bit).
 * Refused with an error before anything is launched: 2-D handles, slab handles, flat levels, null pointers, pointers that
 * are not device memory of the handle's device, and an out_dev that overlaps x_dev or dkappa_dev (the march reads neighbours). */
int mg_diffusion_apply_dkappa(mg_handle h, int level, const double* dkappa_dev, const double* x_dev, double* out_dev);
/* The two operators above with the mask of each side chosen by the caller (no reference counterpart): what a lifted
 * inhomogeneous Dirichlet load -A_IB(kappa) g and its derivatives are written with.  A^(w) is the natural P1 stiffness matrix
 * of a cell field w on all (N + 1)^3 nodes of the Kuhn mesh, without boundary condition: an axis edge e of cell c carries
 * n_{c,e} w_c h / 6 (the weights of mg_gen_diffusion_level, whose matrix has the interior block of A^(kappa)).  M_set is the mask
 * that zeroes the boundary nodes (MG_NODES_INTERIOR) or the identity (MG_NODES_ALL):
 *     mg_diffusion_apply_dkappa_ex: out = T(w, x; rows, cols) = M_rows A^(w) M_cols x
 *     mg_diffusion_dkappa_ex:       out[c] = D(a, b; a_nodes, b_nodes)_c = d / d w_c (M_a a)^T A^(w) (M_b b)
 * (interior, interior) gives the bits of the two entries above.  A boundary row of T (rows = all) is the row of A^, summed as an
 * interior row is with a cell outside the grid counting as +0.0 and a neighbour outside it reading 0; with rows = interior it is
 * +0.0.  cols = interior zeroes every entry whose column is a boundary node, a boundary row's own diagonal included.  D applies
 * its masks where a node is loaded; one pointer may be passed as a and b with different sets.  They close under
 * differentiation: T with cotangent y gives w_bar = D(y, x; rows, cols) and x_bar = T(w, y; cols, rows); D with cotangent w gives
 * a_bar = T(w, b; a_nodes, b_nodes) and b_bar = T(w, a; b_nodes, a_nodes).  The lift of Dirichlet data g is
 * T(kappa, g_B; interior, all) with g_B = g on the boundary and 0 inside; poisson.diffusion_lift restates it.
 * Pointers, stream, synchronisation, cell and node order and the refusals are those of the two entries above; a node set
 * other than 0 or 1 is refused as well.  Nothing is launched by a refused call. */
enum mg_node_set { MG_NODES_INTERIOR = 0, MG_NODES_ALL = 1 };
int mg_diffusion_dkappa_ex(mg_handle h, int level, const double* a_dev, int a_nodes, const double* b_dev, int b_nodes, double* out_dev);
int mg_diffusion_apply_dkappa_ex(mg_handle h, int level, const double* dkappa_dev, const double* x_dev, int rows, int cols,
                                 double* out_dev);
/* The two sensitivity operators of the reaction term (no reference counterpart).  R is linear in sigma and diagonal:
 *     mg_diffusion_apply_dsigma: out_i = T_sigma(dsigma, x)_i = R(dsigma)_i x_i on the free nodes of the handle's face set,
 *                                +0.0 on its Dirichlet nodes; dsigma may have any sign;
 *     mg_diffusion_dsigma:       out_c = D_sigma(a, b)_c = (h^3 / 24) sum over the 8 corners i of cell c of t_{c,i} a~_i b~_i,
 *                                a~, b~ = a, b with the Dirichlet nodes taken as 0.
 * They are adjoint, a . T_sigma(w, x) = w . D_sigma(a, x), and close under differentiation: D_sigma with cotangent w gives
 * a_bar = T_sigma(w, b) and b_bar = T_sigma(w, a); T_sigma with cotangent y gives w_bar = D_sigma(y, x) and
 * x_bar = T_sigma(w, y).  With the adjoint solve (A + R) lambda = dJ/du, dJ/dsigma = -D_sigma(lambda, u).  Neither reads sigma
 * or a matrix: any whole 3-D grid level will do, as with mg_diffusion_dkappa.  Summation order: mg_diffusion_adj.hip.h;
 * poisson.diffusion_dsigma and poisson.diffusion_apply_dsigma restate them bit for bit (no fma in either).
 * Pointers, cell and node order, stream and synchronisation are those of mg_diffusion_dkappa / mg_diffusion_apply_dkappa.
 * Refused with an error before anything is launched: 2-D handles, slab handles, flat levels, null pointers, pointers that
 * are not device memory of the handle's device, and an out_dev that overlaps an input. */
int mg_diffusion_dsigma(mg_handle h, int level, const double* a_dev, const double* b_dev, double* out_dev);
int mg_diffusion_apply_dsigma(mg_handle h, int level, const double* dsigma_dev, const double* x_dev, double* out_dev);
/* The two sensitivity operators of the Robin term, per face F (no reference counterpart).  B is linear in alpha and diagonal:
 *     mg_diffusion_apply_drobin: out_i = T_alpha,F(dalpha, x)_i = b_F(dalpha)_i x_i on the free nodes of face F (those of the
 *                                handle's face set), +0.0 on every other node of the level; dalpha (N^2) may have any sign;
 *     mg_diffusion_drobin:       out_q = D_alpha,F(a, b)_q = (h^2 / 6) sum over the 4 corners i of face-cell q of
 *                                t_{q,i} a~_i b~_i, a~, b~ = a, b with the Dirichlet nodes taken as 0; out: N^2 face-cells.
 * They are adjoint, a . T(w, x) = w . D(a, x), and close under differentiation as D_sigma / T_sigma do.  With the adjoint solve
 * (A + R + B) lambda = dJ/du, dJ/dalpha_F = -D_alpha,F(lambda, u).  Neither reads alpha or a matrix.  Summation order:
 * mg_diffusion_adj.hip.h; poisson.diffusion_drobin and poisson.diffusion_apply_drobin restate them bit for bit (no fma in
 * either).  Pointers, node order, stream and synchronisation are those of mg_diffusion_dsigma / mg_diffusion_apply_dsigma.
 * Refused with an error before anything is launched: what those entries refuse, a `face` that is not exactly one bit, and a
 * face of the handle's Dirichlet set. */
int mg_diffusion_drobin(mg_handle h, int level, int face, const double* a_dev, const double* b_dev, double* out_dev);
int mg_diffusion_apply_drobin(mg_handle h, int level, int face, const double* dalpha_dev, const double* x_dev, double* out_dev);
/* Cell gradients and fluxes of a nodal field (no reference counterpart).  On a 3-D grid level with N^3 cells, h = 1 / N, cells
 * in kappa's order (ck * N + cj) * N + ci, nodes lexicographic, a 3-component cell field with component d in {x, y, z} at
 * d * N^3 + cell:
 *     mg_diffusion_cell_gradient:     out = F(w, x), 3 N^3: F_{d,c} = w_c G_d(x)_c with G(x)_c the mean of grad x_h over the six
 *                                     Kuhn simplices of cell c -- (N / 6) times the sum over the cell's four edges of axis d of
 *                                     n (x_upper - x_lower), n = 2, 1, 1, 2 as in mg_diffusion_dkappa.  w_dev null: F = G, no
 *                                     product.  No mask: x is the field itself, Dirichlet values included.  q = -F(kappa, u) is
 *                                     the exact cell average of -kappa grad u_h;
 *     mg_diffusion_cell_gradient_t:   out = F^T(w, p), nodes: the transpose of F in x, p a 3-component cell field;
 *     mg_diffusion_cell_gradient_dot: out = C(p, x), N^3: out_c = p_{x,c} G_x + p_{y,c} G_y + p_{z,c} G_z.
 * They are adjoint up to rounding, <p, F(w, x)> = <x, F^T(w, p)> = <w, C(p, x)>, and close under differentiation: F with
 * cotangent P gives w_bar = C(P, x), x_bar = F^T(w, P); F^T with cotangent y gives w_bar = C(p, y), p_bar = F(w, y); C with
 * cotangent z gives p_bar = F(z, x), x_bar = F^T(z, p).  None reads kappa or a matrix: any whole 3-D grid level will do, stored,
 * matrix-free or grid-only (mg_set_level_grid).  Summation order: mg_diffusion_flux.hip.h; poisson.diffusion_cell_gradient,
 * diffusion_cell_gradient_t and diffusion_cell_gradient_dot restate them bit for bit (no fma in any).  They run on the
 * handle's stream, which is synchronised before return; nothing crosses to the host and no handle memory is allocated.
 * Refused with an error before anything is launched: 2-D handles, slab handles, flat levels, null pointers other than w_dev,
 * pointers that are not device memory of the handle's device, and an out_dev that overlaps an input. */
int mg_diffusion_cell_gradient(mg_handle h, int level, const double* w_dev, const double* x_dev, double* out_dev);
int mg_diffusion_cell_gradient_t(mg_handle h, int level, const double* w_dev, const double* p_dev, double* out_dev);
int mg_diffusion_cell_gradient_dot(mg_handle h, int level, const double* p_dev, const double* x_dev, double* out_dev);
/* Point sources and point observations (no reference counterpart).  On a 3-D grid level with N cells per axis, nodes
 * lexicographic (k * n1 + j) * n1 + i with n1 = N + 1, pts_dev M x 3 doubles, row m = (x, y, z) of point m in [0, 1]^3.  Per
 * axis d: t = p_d * (double)N, c_d = min((int)floor(t), N - 1), xi_d = t - (double)c_d; pi sorts xi in descending order, stably
 * (a tie: the lower axis first).  The point lies in the Kuhn simplex of cell c with the vertices n0 = node(c), n1 = n0 +
 * stride(pi0), n2 = n1 + stride(pi1), n3 = n2 + stride(pi2) and the weights l0 = 1.0 - xi_pi0, l1 = xi_pi0 - xi_pi1, l2 = xi_pi1
 * - xi_pi2, l3 = xi_pi2:
 *     mg_diffusion_point_sample:     out = S(x), M: the P1 interpolant, out_m = ((l0 x[n0] + l1 x[n1]) + l2 x[n2]) + l3 x[n3].
 *                                    No mask: x is the field itself, Dirichlet values included;
 *     mg_diffusion_point_load:       out = S^T(w), nodes: the consistent point load sum_m w_m int delta(x - x_m) phi_i; point m
 *                                    contributes l_v w_m to node n_v;
 *     mg_diffusion_point_gradient:   out = G(x), M x 3: the gradient of the located simplex, component pi0 = (x[n1] - x[n0]) N,
 *                                    pi1 = (x[n2] - x[n1]) N, pi2 = (x[n3] - x[n2]) N;
 *     mg_diffusion_point_gradient_t: out = G^T(p), nodes, p M x 3: with P_a = p[m][pi_a] point m contributes (0.0 - P_0) N,
 *                                    (P_0 - P_1) N, (P_1 - P_2) N, P_2 N to n0 .. n3.
 * In both transposes a node starts at +0.0 and takes its contributions in ascending point index, an untouched node is +0.0, and
 * two calls give the same bits however many points share a node: no floating-point atomic, but a stable radix sort of the 4 M
 * (node, contribution) pairs by node and one thread per run (mg_diffusion_points.hip.h).  They are adjoint up to rounding,
 * <w, S(x)> = <x, S^T(w)>, <p, G(x)> = <x, G^T(p)>, and close under differentiation in the fields; d S(x)_m / d pts_m = G(x)_m
 * inside the located simplex (x_h kinks on simplex faces), G is piecewise constant in pts.  None reads kappa or a matrix: any
 * whole 3-D grid level will do, stored, matrix-free or grid-only (mg_set_level_grid).  poisson.diffusion_point_locate,
 * diffusion_point_sample, _load, _gradient and _gradient_t restate them bit for bit (no fma in any).  They run on the handle's
 * stream, which is synchronised before return; the temporaries of the transposes (128 M bytes and the sort's) are freed on
 * return and no handle memory, vector or counter is touched.  Refused with an error before anything is allocated or launched:
 * a null handle, 2-D handles, slab handles, flat and unset levels, M < 1 (and M > 2^31), null pointers, pointers that are not device memory of
 * the handle's device, and an out_dev that overlaps an input.  Refused after one checking kernel, with out_dev unwritten: a
 * coordinate that is not finite or lies outside [0, 1]; the message names the lowest offending point index. */
int mg_diffusion_point_sample(mg_handle h, int level, int64_t M, const double* pts_dev, const double* x_dev, double* out_dev);
int mg_diffusion_point_load(mg_handle h, int level, int64_t M, const double* pts_dev, const double* w_dev, double* out_dev);
int mg_diffusion_point_gradient(mg_handle h, int level, int64_t M, const double* pts_dev, const double* x_dev, double* out_dev);
int mg_diffusion_point_gradient_t(mg_handle h, int level, int64_t M, const double* pts_dev, const double* p_dev, double* out_dev);
/* Located point sets: the four point operators for one fixed set of points and any number of fields per call (no reference
 * counterpart).  A set is checked, located and sorted once; its calls launch no checking kernel, allocate nothing, sort nothing
 * and make no host round trip besides the final synchronisation.
 *   mg_points_create   copies the M points of pts_dev (the caller's array may be freed or overwritten afterwards), locates them
 *       on `level` with the rule above, orders the 4 M (node, slot = 4 m + v) pairs by node with the stable radix sort of the
 *       transposes, and keeps, in device memory that mg_memory_bytes counts: the points (24 M bytes), one 16-byte record per
 *       sorted slot (weight, point index, vertex and the two axes its gradient term reads: 64 M bytes) and the R runs of equal
 *       node (run_start[R + 1], run_node[R]: 16 R + 8 bytes).  Its temporaries are freed on return; no vector, level, counter,
 *       graph or lane of the handle is touched.  The set belongs to the handle: mg_destroy frees the sets that are left.
 *       Refused by name exactly as mg_diffusion_point_* refuse: before any allocation a null handle, 2-D and slab handles, flat
 *       and unset levels, M < 1 (and M > 2^31), null pointers and pointers that are not device memory of the handle's device;
 *       after the one checking kernel a coordinate that is not finite or outside [0, 1], the lowest offending point named,
 *       with no set made (*ps is null).
 *   mg_points_destroy  frees a set.  Every entry looks its set up in the handle's list before it reads anything of it: a set
 *       that is unknown, destroyed already or another handle's is refused by name, never dereferenced.
 *   mg_points_info     the level and its N at creation, M, the number of runs, the slots in the longest run and the set's
 *       device bytes; any output pointer may be null.
 *   mg_points_sample / _load / _gradient / _gradient_t   for every lane b < nb: out_b = S(x_b) (M doubles), S^T(w_b) (the
 *       level's nodes), G(x_b) (M x 3), G^T(p_b) (nodes).  Pointer arrays are HOST arrays of nb DEVICE pointers, as in
 *       mg_apply_batch.  For every b, out_b has bit for bit the bytes mg_diffusion_point_sample / _load / _gradient /
 *       _gradient_t write for the same points and operand -- for any nb, any mix of lanes, on every call.  In a transpose an
 *       untouched node is +0.0 and a node takes its contributions in ascending point index onto +0.0: one thread walks a run
 *       front to back for all lanes of a launch group (four lanes per launch, ascending).  No floating-point atomic, no fused
 *       product.  Two lanes may share an input pointer.  They run on the handle's stream, which is synchronised before return.
 *       Refused before anything is launched: nb outside 1..MG_BATCH_MAX, null arrays or pointers, a pointer that is not device
 *       memory of the handle's device, an output that overlaps another lane's output or any lane's input, and a level that is
 *       no longer set or has been set again with another N (the message says which N the set was located on). */
typedef struct mg_points* mg_points_handle;
int mg_points_create(mg_handle h, int level, int64_t M, const double* pts_dev, mg_points_handle* ps);
int mg_points_destroy(mg_handle h, mg_points_handle ps);
int mg_points_info(mg_handle h, mg_points_handle ps, int* level, int* N, int64_t* M, int64_t* runs, int64_t* longest_run, int64_t* bytes);
int mg_points_sample(mg_handle h, mg_points_handle ps, int nb, const double* const* x_dev, double* const* out_dev);
int mg_points_load(mg_handle h, mg_points_handle ps, int nb, const double* const* w_dev, double* const* out_dev);
int mg_points_gradient(mg_handle h, mg_points_handle ps, int nb, const double* const* x_dev, double* const* out_dev);
int mg_points_gradient_t(mg_handle h, mg_points_handle ps, int nb, const double* const* p_dev, double* const* out_dev);
/* getJacobiMatrices (multigrid.py:48-56) as a stand-alone set-up kernel, for callers that
 * want the reference's split operands back: for every stored entry a_ij of the CSR matrix
 * writes scaled[q] = a_ij / a_ii computed as (1/a_ii) * a_ij, keep[q] = 1 unless the entry
 * is the diagonal or an explicit zero (SciPy's CSR - DIA subtraction drops both, App. A Q7),
 * and dinv[i] = 1 / a_ii.  The caller compacts the kept entries (the Python shim does, in
 * SciPy's reversed per-row order) into D^-1 (A - D). */
int mg_jacobi_split(int device, int64_t n_rows, int64_t nnz, const void* indptr, int indptr_is_64,
                    const int32_t* indices, const double* data, double* dinv, double* scaled,
                    unsigned char* keep);
/* mu1/mu2/omega: Multigrid_prototype.py:43-46 via initialize_problem
 * (multigrid.py:38-41).  coarse_rtol/coarse_maxit steer the device PCG that stands
 * in for spsolve on the coarsest level (multigrid.py:239). */
int mg_set_params(mg_handle h, int mu1, int mu2, double omega, int restriction, int smoother,
                  double coarse_rtol, int coarse_maxit, int keep_err);
/* Chebyshev smoother (MG_SMOOTH_CHEBYSHEV; no reference counterpart).  A call of degree m on level l runs the three-term
 * recurrence (Saad, Iterative Methods, Alg. 12.1) on the interval [a, b] of that level, with theta = (b + a) / 2,
 * delta = (b - a) / 2, sigma = theta / delta, rho_0 = 1 / sigma:
 *     x_1     = x_0 + (1 / theta) D^-1 (f - A x_0)
 *     x_{k+1} = x_k + rho_k rho_{k-1} (x_k - x_{k-1}) + (2 rho_k / delta) D^-1 (f - A x_k),  rho_k = 1 / (2 sigma - rho_{k-1}),
 * i.e. step k computes (x + (alpha_k * (1 / d)) * (f - A x)) + beta_k * (x - x_{k-1}) row by row in every kernel, alpha_k and
 * beta_k evaluated on the host in double in this order; the first step does not read x_{k-1}.  x_{k-1} lives in the level's
 * second iterate buffer (MG_VEC_R, which the Jacobi ping-pong overwrites as well): no vector is added to the hierarchy.
 * mg_set_chebyshev: b = upper_factor * lambda_max(D^-1 A) as estimated, a = b / lower_ratio, per level (defaults: eig_steps 10,
 *   lower_ratio 6, upper_factor 1.1).  The estimate is eig_steps steps of Jacobi-preconditioned CG (Lanczos) from a start
 *   vector that hashes each node's global lexicographic index, then the largest eigenvalue of the small tridiagonal matrix on the
 *   host; dot products are fixed-order device sums (all-reduced over slabs: every rank gets the same bits).  It runs once per
 *   level from mg_prepare_cycle, the first cycle or a stand-alone mg_smooth (never inside a captured cycle), and again only after
 *   the level's matrix or these settings change.  Its four work vectors of the level's size are freed afterwards
 *   (mg_memory_bytes does not change; mg_chebyshev_estimate_bytes reports what the last estimate held).  Refused with an error:
 *   a level whose storage analysis found it non-symmetric (mg_level_storage), and one on which CG breaks down before two steps,
 *   unless the caller has set that level's interval.
 * mg_set_chebyshev_bounds: the caller's interval [lmin, lmax] for one level (lmin <= 0: lmax / lower_ratio); lmax <= 0 goes back
 *   to the estimate.
 * mg_chebyshev_bounds: the interval in use on a level and the estimate (0 if none has run); runs the estimate if it has not run.
 * Kernels: the one-sweep Jacobi kernels of every storage format with a Chebyshev epilogue, one step per launch, counted by
 *   mg_smoother_launches under MG_PATH_SLICE / MG_PATH_SWEEP1C; on levels that fit one CU ("fuse_small") up to 32 steps per
 *   launch of one workgroup (MG_PATH_SMALL); on 2-D five-point levels ("fuse_2d") a whole call of 2 .. "fuse_2d_k" steps in one
 *   launch (MG_PATH_K2D; longer calls one step per launch).  Every fused path is bit-identical to one step per launch
 *   ("Chebyshev smoother").  On slabs every entry point here is collective: each rank calls it alike. */
int mg_set_chebyshev(mg_handle h, int eig_steps, double lower_ratio, double upper_factor);
int mg_set_chebyshev_bounds(mg_handle h, int level, double lmin, double lmax);
int mg_chebyshev_bounds(mg_handle h, int level, double* lmin, double* lmax, double* lmax_estimate);
int mg_chebyshev_estimate_bytes(mg_handle h, int64_t* bytes);
/* Prolongation from a table instead of the reference's bilinear / trilinear Interpolation2D (multigrid.py:59-120): a fine
 * lattice point (i, j, k) combines the count[r] coarse lattice points 2 * floor((i, j, k) / 4) + offsets[r][t] (each
 * offset component 0..2, at most 10 entries) with weights[r][t], r = (i mod 4) + 4 (j mod 4) + 16 (k mod 4); 2-D levels
 * use the residues with j mod 4 = 0.  With poisson.p2_prolongation_table this is the natural embedding of the coarse P2
 * space into the fine one (BASELINE.json config 5; no reference counterpart).  All three NULL: back to the reference's
 * interpolation.  Slabs need halo_planes = 2. */
int mg_set_prolongation_table(mg_handle h, const int* count /*[64]*/, const int* offsets /*[64][10][3]*/,
                              const double* weights /*[64][10]*/);
/* Restriction from a table (MG_RESTRICT_TABLE), gathered per coarse lattice point: an interior coarse point A of type
 * (a & 1) + 2 (b & 1) + 4 (c & 1) sums weights[type][t] * r[2 A + offsets[type][t]] over the interior fine points (offset
 * components within +-4, max_entries per type); boundary coarse points take the coincident fine value.  With
 * poisson.p2_restriction_table this is the transpose of the P2 prolongation, <R r, v> = <r, P v>: the canonical restriction of
 * a finite-element residual (the reference injects it, multigrid.py:251-252, which under-scales the coarse correction:
 * SURVEY.md App. A Q1).  Whole levels only.  No reference counterpart. */
int mg_set_restriction_table(mg_handle h, int max_entries, const int* count /*[8]*/, const int* offsets /*[8][max][3]*/,
                             const double* weights /*[8][max]*/);
/* P1 natural-embedding transfers on the structured simplicial mesh of poisson.py (squares cut along (1, 1), cubes into six
 * Kuhn simplices; edges along the non-negative p in {0,1}^dim \ {0}).  No reference counterpart: the reference injects
 * (multigrid.py:123-132) and interpolates bilinearly (Interpolation2D, multigrid.py:59-120), which is not the embedding of the
 * coarse P1 space.  Results then differ from the reference's on purpose.
 *   prolongation (enable = 1): fine node 2I + p takes v_c(I) for p = 0 and 0.5 * (v_c(I) + v_c(I + p)) otherwise, with the
 *     ERR / add semantics of mg_prolong.  It and a prolongation table exclude each other: setting one clears the other
 *     (enable = 0: back to the reference's interpolation, or to whatever table is set afterwards).
 *   restriction MG_RESTRICT_P1_TRANSPOSE (mg_set_params / mg_restrict): R = P^T -- an interior coarse node I sums
 *     w * r_f(2I + d) over d in {0} U +-dirs (w = 1 for d = 0, 0.5 otherwise), multiplied first, then added in ascending fine
 *     lexicographic order (the convention of MG_RESTRICT_TABLE, which gives the same bits fed poisson.p1_restriction_table);
 *     boundary coarse nodes take the coincident fine value.
 * Both check at first use that the stencils of the levels involved lie in that Kuhn pattern: a level that couples other
 * nodes (a mesh cut the other way with its zero couplings kept, P2 rows) is refused with an error, on slabs by every rank
 * together.  A matrix with its zeros pruned cannot show how the mesh was cut: the 2-D Poisson matrices of both diagonal
 * directions have the same five-point stencil, pass the check, and the transfers are then those of poisson.py's mesh.
 * Slabs: the same halos as the Q1 interpolation / full weighting (halo_planes = 1). */
int mg_set_prolongation_p1(mg_handle h, int enable);
/* Galerkin coarse level: sets level - 1's matrix to P^T A_level P with the P1 embedding above, P restricted to interior fine
 * and interior coarse nodes, plus identity rows on the boundary, as the handed-over levels have.  Computed on the device by
 * one thread per coarse row from the fine level's storage, whichever format it has; entries summed in a fixed order (fine
 * rows of P's column, then their entries, in ascending lexicographic order), so repeated calls are bit-identical.  Nothing
 * is flushed to zero, but exact zeros are dropped as prune_zeros does.  The coarse level then gets the storage analysis of
 * mg_set_level_csr (symmetric diagonals, offset codes, row classes, "storage_auto").  Needs a whole (not slab) grid level
 * with an even elements_per_dim and a stencil in the Kuhn pattern.  Level - 1 is rebuilt from scratch: its vectors cross in
 * lexicographic numbering and start at zero, and mg_fmg on it needs mg_set_rhs_true again.  No reference counterpart.
 * mg_galerkin_hierarchy applies it from top_level down to level 1. */
int mg_galerkin_level(mg_handle h, int level);
int mg_galerkin_hierarchy(mg_handle h, int top_level);
/* Tuning and format knobs (defaults in parentheses; DESIGN.md sections 4-6 explain each):
 *   before any level is set:
 *     "rows_per_lane"      1 | 2 | 4 rows of a slice per lane (2)
 *     "offset_codes"       0 keeps int32 column indices (1)
 *     "symmetric_storage"  0 keeps lower entries even for bit-for-bit symmetric matrices (1)
 *     "require_diagonal"   0 accepts operators without a diagonal, e.g. D^-1 R for mg_smooth_split (1)
 *     "halo_planes"        grid planes exchanged with each slab neighbour: 1, or 2 for stencils that reach two planes
 *                          (P2 lattice levels) (1)
 *     "storage_ulps"       k > 0: matrix entries that agree within about k units in the last place count as equal in the
 *                          symmetry test (the upper entry of a pair is kept) and in the row dictionary (a class holds the first
 *                          such row seen): assemblies whose rows differ by round-off (h not a power of two, varying
 *                          summation order) then still get the compact formats.  This PERTURBS the matrix by up to k ulps
 *                          per entry -- below the round-off of the assembly itself for small k -- so results agree with the
 *                          exact-storage ones to ~k * 1e-16 relative, not bit for bit.  (0: everything bit for bit)
 *     "storage_auto"       1 = a level whose exact symmetry test or row dictionary fails is tried once more with entries within
 *                          4 units in the last place counting as equal (what an assembly with row-dependent round-off needs
 *                          to reach the compact formats: 2.6 x on the headline pass); the perturbation -- at most 4 ulps per
 *                          entry, below the assembly's own round-off -- is reported by mg_level_storage.  0 = exact storage
 *                          only (1)
 *     "fuse_block"         1 = whole seven-point levels with row classes of "fuse_block_min_rows" <= rows < "fuse_block_max_rows" --
 *                          the middle levels, too small for the plane marches -- are relaxed K sweeps per launch on blocks of
 *                          32 x 32 x EZ cells that stay on the CU (mg_jacobiblk.hip.h), each block recomputing a halo of K
 *                          cells; bit-identical to single sweeps.  2 = whatever the level's size (tests), 0 = off (1: alone the
 *                          pass is no faster per sweep than one launch per sweep, but a cycle has a third of the launches --
 *                          BASELINE config 3 132.8 -> 137.5 cycles/s)
 *     "fuse_block_min_rows"  see "fuse_block" (2^15)
 *     "fuse_block_max_rows"  see "fuse_block" (2^23)
 *     "fuse_block_k"       sweeps per launch of the block pass, 2..4; 0 = three, four on levels whose blocks then all run at
 *                          once (65^3 rows) (0)
 *     "fuse_block_ez"      planes per block of the block pass, 11 or 19 (19 spills registers and is slower) (11)
 *     "fuse_2d_lines"      lines per region of the 2-D K-sweep kernel ("fuse_2d"): 64, 32 or 16; 0 = chosen per level -- 32 (two
 *                          workgroups per CU: BASELINE config 2 451 -> 592 cycles/s against 64 lines), 16 on levels whose
 *                          tiles then still all run at once (621) (0)
 *     "direct_block_rows"  the coarsest level's exact solve (block-tridiagonal LU over groups of grid planes / lines) takes blocks
 *                          of at least this many rows, at most 2304: a solve is three dependent launches per block, so fewer,
 *                          larger blocks are faster while their dense inverses (rows^2 x 8 B each) stay small.  Before the first
 *                          cycle (2048)
 *     "gen_odd_rows"       mg_gen_poisson_level gives this many of 10000 interior rows, picked by a hash of their grid index, a
 *                          reaction term of their own on the diagonal (a.diag * (1 + r), 0 <= r < 1): rows unlike any other,
 *                          for measuring what "row_escape" costs.  Levels generated afterwards (0)
 *     "row_escape"         1 = a symmetric seven-point level with more than 255 distinct rows keeps row classes when at least three
 *                          quarters of its rows are copies of the 254 most frequent ones: the other rows ("escape rows":
 *                          another material, a perturbed coefficient) are read from the stored matrix by the K-sweep march
 *                          ("fuse_k"), which is then the only kernel that uses the classes -- same arithmetic, same results bit
 *                          for bit.  Needs whole levels (not slabs) and no 64 x 32 tile of the march with more than 1024 such rows in
 *                          K + 2 planes (512 for K = 5; the march takes the most sweeps per pass that fit); else, and with 0, such a level has no row classes.  Before level set-up (1)
 *     "row_classes"        0 skips the dictionary of distinct rows on symmetric 5- and 7-point levels (1)
 *     "halo_depth"         halo planes every vector of a slab has ROOM for, >= "halo_planes" (0 .. 5; 0: just those).  With K
 *                          planes of room the K-sweep march ("fuse_k") runs on slabs too: K planes of the iterate travel once per
 *                          K sweeps and the slab relaxes its neighbours' K - 1 planes next to it itself -- one grouped exchange
 *                          and two launches per K sweeps instead of a boundary chain per pair; bit-identical to the single
 *                          handle.  Every rank alike, before mg_set_comm / level set-up.  (0)
 *   any time:
 *     "xcd_chunk"          consecutive tiles per XCD in the chunked block -> tile map (8)
 *     "strip_slices"       slices per XCD strip, 0 = chunked map only (64)
 *     "nontemporal"        streaming loads for once-read matrix / right-hand-side data (1)
 *     "lds_pad"            dynamic LDS bytes per block of the one-sweep kernels on stored levels of at least 100000 slices
 *                          that run without row classes (none, or "class_sweeps" 0) = occupancy cap, 0..153600 (150 KiB: one block per CU); the kernels do not
 *                          use the bytes; bit-identical (32768)
 *     "overlap"            halo exchange on the communication stream behind the interior sweep (1)
 *     "overlap_min_rows"   ... only on levels with at least this many owned rows (4194304)
 *     "slab_pair_form"     overlapped pair sweeps on slabs: 0 = the exchange chain computes its own first sweep of the boundary
 *                          planes and runs beside ONE launch of the pass over the whole slab; 1 = the boundary segments of the
 *                          pass first, then its interior segments beside the chain (0); bit-identical, every rank alike
 *     "graph_comm"         1 = V-cycles on slabs are captured into hipGraphs too, RCCL exchanges included (the calls are
 *                          stream operations on both streams of the overlapped sweeps); every rank must set it alike.
 *                          Needs the RCCL transport (mg_comm_init_rccl).  (0: validated against the in-process stand-in of
 *                          tests/fake_rccl only, not against RCCL on a multi-GPU node)
 *     "fuse_restrict"      residual evaluated at the coarse nodes only when injecting (1)
 *     "fuse_sweeps"        Jacobi sweeps in pairs, two per pass over the matrix, on 3-D 7-point levels in
 *                          symmetric diagonal storage (1); bit-identical to single sweeps
 *     "fuse_min_rows"      ... only on levels with at least this many owned rows (16777216)
 *     "fuse_segments"      plane segments per tile of that pass, 0 = chosen by the cost model (0)
 *     "fuse_nontemporal"   streaming loads in that pass (0: measured slower)
 *     "fuse_k"             Jacobi sweeps per pass of the K-sweep march (mg_jacobik3d.hip.h) on whole seven-point levels with
 *                          row classes: a smoother call of nw sweeps (multigrid.py:223-228) runs as passes of 3 .. "fuse_k"
 *                          sweeps and at most one pair (50 = 10 x 5); 0 .. 2 = pairs only (5); bit-identical to single sweeps
 *     "fuse_k_shape"       tile of that march: 1 = 64 x 48 cells (12 waves x 4 grid lines), 4 = 64 x 24 by 8 waves with two
 *                          workgroups per CU (levels of at most 64 row classes), 7 = 64 x 32 by 16 waves (no register spills up to
 *                          five sweeps), 8 = 7 with one barrier per step, 9 = 8 on 64 x 36 tiles whose first and last wave own the four rim
 *                          lines each (28 result lines per tile instead of 24; five sweeps per pass on whole levels without
 *                          escape rows -- a handle that asks for 9 gets 8 on slabs and 7 below five sweeps); 1, 4, 7, 8, 9,
 *                          or -1: for five sweeps per pass 9 on whole levels of at least "fuse_k_rim_min_rows" rows and 8
 *                          elsewhere, 7 for three and four (-1).  The shapes 0, 2, 3, 5 and 6 were measured slower and retired:
 *                          those values are refused
 *     "fuse_k_rim_min_rows"  ... (67108864: 513^3 and 1025^3 rows, where shape 9 was measured against shape 8)
 *     "fuse_k_segments"    plane segments per tile of that march, 0 = chosen by its cost model (0)
 *     "fuse_k_slab_min_rows"  ... on slabs (below): levels whose smallest slab has at least this many rows (1048576)
 *     "fuse_k_slab_min_sweeps"  ... and smoother calls of at least this many sweeps (4)
 *     "fuse_k_min_rows"    ... on whole levels with at least this many rows; smaller levels keep single sweeps (16777216: with
 *                          2097152 the 129^3 level takes the march too -- 12.2 us per sweep against 14.3 alone, but whole cycles
 *                          of BASELINE config 3 are no faster; 65^3 rows: 11.6 against 4.0)
 *     "fuse_k_small_rows"  ... five sweeps per pass again on levels with fewer rows than this (4194304: 129^3 rows, 12.2 us per
 *                          sweep with five against 15.5 with four)
 *     "fuse_k4_min_rows"   ... more than three sweeps per pass only on levels with at least this many rows (0)
 *     "fuse_k5_min_rows"   ... more than four only on levels with at least this many rows (67108864: on 257^3 rows four
 *                          sweeps per pass measured best)
 *     "fuse_k_nt_store"    non-temporal stores of that march's result (experiment) (0)
 *     "fuse_k_min_side"    ... on whole levels whose grid lines and planes hold at least this many nodes / lines (32, like the other
 *                          plane marches; 16..32 -- tests: grids of a single tile whose lines end inside it)
 *     "fuse_k_tail"        the tiles left over for a last, nearly empty round of workgroups (fewer tiles than half the CUs) are cut
 *                          into shorter plane segments that fill that round once (1); bit-identical
 *     "fuse_k_small_tiles" 64 x 24 tiles (shape 4) on levels whose planes hold fewer 64 x 48 tiles than the GPU has CUs (0:
 *                          measured slower)
 *     "fuse_k_load_early"  tile shape 9: 1 = the loads of the next plane go out as soon as their registers are free -- f and, off
 *                          plan, the classes in front of the step's barrier, x of all the wave's lines in one group behind the
 *                          first piece of phase B -- instead of in five slices between the pieces (1); 0 or 1, bit-identical;
 *                          ignored where the launch is not of shape 9
 *     "fuse_k_load_early_min_rows"  ... on levels with at least this many rows (536870912: 1025^3 rows gain 4 %, 513^3 rows
 *                          measured no faster)
 *     "fuse_k_plan"        march plans: the level's class bytes are inspected once per level, tile shape and K (which planes of
 *                          which wave hold the main class only, or the classes of the plane before), and the steps of that
 *                          march that run inside such a run load and inspect no classes (1); 0 = every step does;
 *                          bit-identical.  Whole levels without escape rows, "fuse_k_shape" 7, 8 and 9; see
 *                          mg_march_plan
 *     "fuse_classes"       that pass reads one class byte per row instead of the 32-byte row where the level has
 *                          row classes (1); bit-identical either way
 *     "fuse_plain"         that pass on levels WITHOUT row classes: 2 = round-2 structure (sdia_jacobi2p), 1 = round 1's (2);
 *                          bit-identical either way
 *     "fuse_plain_shape"   ... its launch shape: 0 = 12 waves x 1 grid line, 1 = 8 x 2, 2 = 16 x 1 (0: the only one without
 *                          register spills, measured best)
 *     "class_sweeps"       the one-sweep kernels (residual, single sweeps, SpMV, Gauss-Seidel colours) read the class
 *                          byte too where the level has row classes (1); bit-identical either way
 *     "fuse_shape"         launch shape of the class-coded pass: 0 = 8 waves x 2 grid lines, 1 = 12 waves x 2 lines,
 *                          2 = 16 waves x 1 line, 3 = 8 waves x 3 lines (1)
 *     "fuse_even"          1 = the tile columns of the class-coded pass are equally wide, as narrow as covers the grid;
 *                          0 = always 124 cells, the last column nearly empty (0: measured faster); bit-identical
 *     "fuse_wi"            experiments: that width given directly (0 = chosen per level as above)
 *     "march_sweeps"       the one-sweep class kernels (residual, single Jacobi sweeps, Gauss-Seidel colours) run as a
 *                          plane march with x in LDS on whole 3-D seven-point levels (1); bit-identical either way
 *     "march_min_rows"     ... only on levels with at least this many rows (4194304)
 *     "march_shape"        ... 0 = 12 waves x 2 grid lines per workgroup, 1 = 16 x 2 (0)
 *     "fuse_small"         all Jacobi sweeps of a smoother call in ONE launch on levels with row classes that fit one CU's
 *                          LDS (a few thousand rows: the reference's own 65^2 / 33^2 levels) (1); bit-identical
 *     "fuse_small_2d_rows" ... on 2-D levels only up to this many rows: larger ones (65^2) are faster through the K-sweep 2-D
 *                          kernel, ten launches of a dozen small workgroups instead of one launch of one workgroup (2048)
 *     "fuse_2d"            up to "fuse_2d_k" Jacobi sweeps per launch on 2-D five-point levels with row classes (1);
 *                          bit-identical to single sweeps
 *     "fuse_2d_k"          ... at most this many per launch, 2..5 (5)
 *     "fuse_xcd_chunk"     consecutive tiles of that pass given to one XCD at a time (32)
 *     "cls_blocks_per_cu"  persistent blocks per CU of the one-sweep class kernels (4)
 *     "coarse_direct"      exact block-tridiagonal coarsest solve, 0 = PCG (1)
 *     "pcg_chunk"          PCG iterations enqueued between convergence checks (16)
 *     "mf_batch"           batched solves (mg_apply_batch, mg_pcg_batch): the most lanes one fused launch of the matrix-free march
 *                          takes, 0..4; 0 or 1 = never fuse, every lane runs the one-vector kernel (4; DESIGN.md, "Batched
 *                          solves"); bit-identical whatever the value
 *     "lattice_march"      wide lattice stencils (3-D P2 levels with stencil classes) as a plane march with five planes of x in
 *                          LDS instead of gathers from global memory (1); bit-identical either way
 *     "lattice_march_min_rows"  ... only on levels with at least this many owned rows (4194304)
 *     "dkappa_gather"      1 = mg_diffusion_dkappa runs one thread per cell with sixteen loads through the caches instead of the
 *                          plane march (0: the march measured 2.2 x faster at 1025^3); bit-identical either way
 *     "lattice_gs2"        1 = the nine-colour Gauss-Seidel sweep on whole 3-D lattice levels runs two colours per launch, out of
 *                          place (five passes over the vector instead of nine; the level's two iterate buffers swap);
 *                          bit-identical, but measured slower (its nine plane slots only fit 32-wide tiles) (0)
 *     "lattice_tile"       tile of that march: 0 / 1 = 64 x 16 cells (256 threads, two workgroups per CU), 2 = 128 x 16 where the
 *                          grid is 128 wide (512 threads, one per CU: fewer rim cells and partly used cache lines, but
 *                          measured slower) (0)
 *     "lattice_segments"   plane segments per tile of that march, 0 = chosen from the tile count (0)
 *     "graph"              replay V-cycles as hipGraphs on a single GPU (1)
 * None of them changes results beyond round-off; the tests pin which ones are bit-for-bit neutral. */
int mg_set_tuning(mg_handle h, const char* key, int64_t value);

/* ---- level queries ------------------------------------------------------------------- */
int mg_level_info(mg_handle h, int level, int64_t* n_global, int64_t* n_local, int64_t* row0,
                  int64_t* nnz_stored, int64_t* nnz_nonzero, int* ell_width, int* replicated,
                  int* offset_codes /* 0 = int32 columns; > 0 = offset codes (number of distinct
                                       offsets); < 0 = symmetric diagonal storage (-stored diagonals) */);
/* Number of distinct full rows (the all-zero row included) when the level's symmetric diagonal storage also
 * carries one class byte per row (the row's five or seven entries, bit for bit, from a table), 0 when it does not
 * (more than 255 distinct rows, another format, "row_classes" 0).  No reference counterpart: storage detail of jacobiRelaxation (multigrid.py:223-228). */
int mg_level_row_classes(mg_handle h, int level, int* classes);
/* Why a level has the storage it has (what `A.getValuesCSR()`, Multigrid_prototype.py:95-96, really delivered):
 *   symmetric             1 = every pair a_ij, a_ji agrees bit for bit, 2 = within `ulps_used` units in the last place (the
 *                         upper half is kept), 0 = not symmetric (the level keeps both halves), -1 = not tested (pattern not
 *                         symmetric, coarsest level, "symmetric_storage" 0)
 *   first_asymmetric_row  lowest row (lexicographic grid numbering, local to the rank) with a pair that differs, -1 = none
 *   max_pair_ulps         largest distance between the halves of a pair in units in the last place; -1 = a pair with one half
 *                         missing or of the other sign
 *   distinct_rows         distinct non-zero rows the row dictionary saw (more than 255: no row classes), -1 = not built
 *   ulps_used             0 = the stored matrix is the handed-over one bit for bit; k > 0: entries within k units in the last
 *                         place were identified ("storage_ulps", or the automatic second try "storage_auto" with k = 4)
 *   escape_rows           rows that have no class of their own although the level has row classes: the level had more than 255
 *                         distinct rows, the 254 most frequent ones became classes and these rows are read from the stored
 *                         matrix ("row_escape"); 0 = none
 * Any pointer may be null.  No reference counterpart: storage detail. */
int mg_level_storage(mg_handle h, int level, int* symmetric, int64_t* first_asymmetric_row, int64_t* max_pair_ulps,
                     int* distinct_rows, int* ulps_used, int64_t* escape_rows);

/* ---- vectors ---------------------------------------------------------------------------
 * Host <-> device copies in the caller's DoF numbering, (n,1) fp64 C-contiguous as the
 * reference's vectors (Multigrid_prototype.py:110).  In slab mode `host` still has
 * global length n: set reads the entries of owned (and halo) rows; get writes owned
 * rows only unless gather != 0, in which case slabs are all-gathered first. */
int mg_set_vector(mg_handle h, int level, int which, const double* host);
int mg_get_vector(mg_handle h, int level, int which, double* host, int gather);
/* The same two copies from / to DEVICE memory of the handle's device (no reference counterpart): `dev` holds n_global doubles in
 * the caller's DoF numbering, the permute kernels read / write it directly -- no staging copy, nothing crosses to the host,
 * mg_counters' uploads and downloads do not move.  The caller must have finished producing `dev` before the call (the handle's
 * stream does not wait for other streams); both calls wait for the handle's stream before they return.  Refused with an error:
 * slab handles, and a pointer hipPointerGetAttributes does not report as device memory of the handle's device (before anything
 * is launched). */
int mg_set_vector_device(mg_handle h, int level, int which, const double* dev);
int mg_get_vector_device(mg_handle h, int level, int which, double* dev);
int mg_zero_vector(mg_handle h, int level, int which);
int mg_copy_vector(mg_handle h, int level, int dst_which, int src_which);

/* ---- the hot path, device-resident --------------------------------------------------------
 * mg_smooth    nw weighted-Jacobi sweeps on MG_VEC_V            jacobiRelaxation   multigrid.py:223-228
 * mg_residual  MG_VEC_R = MG_VEC_F - A MG_VEC_V                 multigrid.py:244, :291
 * mg_restrict  MG_VEC_F[level-1] = R MG_VEC_R[level]            Restriction2D(_direct) multigrid.py:123-198
 * mg_prolong   MG_VEC_ERR[level] = P MG_VEC_V[level-1]; if add, MG_VEC_V[level] += it
 *                                                               Interpolation2D    multigrid.py:59-120, :260
 * mg_coarse_solve  MG_VEC_V[0] = A_0^-1 MG_VEC_F[0]             spsolve            multigrid.py:239-241
 * mg_vcycle    ncycles V(mu1,mu2) cycles on `level` starting from MG_VEC_V[level];
 *              resid_l2[c] (optional) = ||f - A v||_2 after cycle c   V_cycle_scheme multigrid.py:231-268
 * mg_norm2     out = ||x||_2 (all-reduced over slabs)           replaces the l2 part of res_calculator :203-208
 * mg_fmg       FullMultiGrid(_test): coarsest solve, interpolate up, mu0 cycles per level,
 *              on the finest either exactly mu0 cycles (tol <= 0; FullMultiGrid_test
 *              :312-339) or until ||r||_2 <= tol (FullMultiGrid :285-302).  Runs on levels
 *              0..top_level: MG_VEC_F[top_level] is the right-hand side there, the coarser
 *              levels use the true right-hand sides given with mg_set_rhs_true (b_dict,
 *              multigrid.py:279).  elements_per_dim == 0 in mg_set_level_csr declares a
 *              "flat" level (any square matrix, smoother/residual only, single GPU).
 * mg_pcg       solve to a tolerance: flexible CG preconditioned by one V-cycle per iteration
 *              (no reference counterpart; declared after mg_fmg_ex) */
int mg_smooth(mg_handle h, int level, int nw);
/* jacobiRelaxation on the reference's own split operands (multigrid.py:223-228), for callers that hand
 * over (D^-1 R, D^-1) rather than A: the level's matrix is D^-1 (A - D) (set with
 * mg_set_tuning("require_diagonal", 0)), MG_VEC_ERR holds the diagonal of D^-1, and every sweep is
 * (1-w) v + w (D^-1 f) - w (D^-1 R) v evaluated in the reference's order. */
int mg_smooth_split(mg_handle h, int level, int nw);
int mg_residual(mg_handle h, int level);
int mg_restrict(mg_handle h, int level, int kind);
int mg_prolong(mg_handle h, int level, int add);
int mg_coarse_solve(mg_handle h, int* iterations, double* rel_residual);
int mg_vcycle(mg_handle h, int level, int ncycles, double* resid_l2);
/* Builds and allocates now what the first V-cycle from `level` would build lazily (direct coarsest solve, colouring checks,
 * work vectors) and waits for it: the cycles that follow only enqueue work.  Optional; useful before timing, and on slabs
 * with "graph_comm" so that every rank enters its first (captured) cycle without set-up work of its own in between.  No
 * reference counterpart. */
int mg_prepare_cycle(mg_handle h, int level);
int mg_norm2(mg_handle h, int level, int which, double* out);
/* out = x^T A x for the level's matrix (one tile SpMV fused with the dot product).  With a P1 mass
 * matrix handed over as the level's matrix this is the square of the reference's L2(Omega) norm
 * (res_calculator / err_calculator, multigrid.py:203-218). */
int mg_quadratic_form(mg_handle h, int level, int which, double* out);
int mg_set_rhs_true(mg_handle h, int level, const double* host);
int mg_fmg(mg_handle h, int top_level, int mu0, double tol, int max_cycles, double* resid_l2,
           int* cycles_done);
/* FullMultiGrid with the reference's own norms, device-resident (multigrid.py:285-302: the stop test `resn <= 1e-11`
 * and the two histories use res_calculator / err_calculator = sqrt(int r_h^2), sqrt(int (u_h - u_exact)^2),
 * multigrid.py:203-218).  norm = MG_NORM_MASS evaluates them as sqrt(x^T M x) with the P1 mass matrix M of the
 * top level handed over by mg_set_mass_csr (same DoF numbering and CSR conventions as mg_set_level_csr; it stands
 * in for the dolfinx function space `V_fine_dolfx`); MG_NORM_L2 is the Euclidean norm.  err_hist (optional)
 * needs the exact solution's nodal values (mg_set_exact = `u_exact_fine`).  Per cycle only two doubles cross to
 * the host.  resid_hist / err_hist hold max(mu0, max_cycles) entries. */
enum { MG_NORM_L2 = 0, MG_NORM_MASS = 1 };
int mg_set_mass_csr(mg_handle h, int level, int64_t n_rows, int64_t nnz, const void* indptr, int indptr_is_64,
                    const int32_t* indices, const double* data);
int mg_set_exact(mg_handle h, int level, const double* host);
int mg_fmg_ex(mg_handle h, int top_level, int mu0, double tol, int max_cycles, int norm, double* resid_hist,
              double* err_hist, int* cycles_done);
/* Flexible CG on `level` preconditioned by one V(mu1,mu2) cycle per iteration.  Starts from MG_VEC_V, solves
 * A x = MG_VEC_F, stops when ||r_k||_2 <= rtol * ||F||_2 or after max_iter iterations (rtol <= 0: exactly
 * max_iter), or earlier if the recursive residual is exactly zero.  On return: MG_VEC_V = x, MG_VEC_F unchanged bit
 * for bit, MG_VEC_R = F - A x (recomputed, not the recursive residual).  resid_hist[k] (optional, max_iter entries)
 * = ||r_k||_2 of the recursion after iteration k + 1; *iterations = iterations done (0 if the start already meets the
 * tolerance).  The preconditioner is one V-cycle of the handle's hierarchy from a zero guess -- whatever restriction,
 * smoother, prolongation table and coarsest solve the handle has -- and is neither symmetric nor exactly linear, hence
 * the flexible (Polak-Ribiere) form beta = -alpha (z.q) / (r.z)_old.  Level >= 1, grid levels only; reaching max_iter
 * is not an error.  The first call on a level allocates four work vectors of its size (x, p, q = A p, the saved
 * right-hand side), freed with the handle; only one scalar per iteration crosses to the host (mg_counters' uploads and
 * downloads do not change).  Slabs: every dot product is all-reduced.  No reference counterpart (the reference solves
 * with V-cycles / FMG only). */
int mg_pcg(mg_handle h, int level, double rtol, int max_iter, double* resid_hist, int* iterations);

/* ---- batched solves: one operator, several right-hand sides (no reference counterpart) ----------------------------------------
 * A "lane" is one right-hand side with everything a solve and its V-cycle write: MG_VEC_V, its ping-pong partner (MG_VEC_R),
 * MG_VEC_F and MG_VEC_ERR of every level up to the call's, mg_pcg's four work vectors, its scalars and partial sums.  Lane 0 is
 * the handle's own set; lanes 1 .. nb - 1 are allocated by the first batch call that needs them, counted by mg_memory_bytes,
 * kept for later calls with the same or a smaller nb (and by mg_refresh_diffusion_hierarchy), and freed by mg_release_batch, by
 * mg_destroy and whenever a level of the hierarchy is set again with another size.  A handle that never calls a batch entry
 * allocates and launches exactly what it did without them.
 *
 * Every operation of the solve and of its V-cycle is done for all active lanes before the next operation starts.  On a
 * matrix-free diffusion level the Jacobi sweeps, the residual and the SpMV with its dot product take the active lanes in ascending
 * order in groups of at most "mf_batch" lanes, ONE launch per group: the march rebuilds each row from kappa once and applies it to
 * every vector of the group (diffusion_mf_batch, mg_diffusion_mf_batch.hip.h), with the level's own plan, so every double and every
 * partial sum has the bits of the one-vector kernel.  A group of one runs that kernel.  Everything else -- stored levels, the
 * transfers, the coarsest solve, mg_pcg's vector kernels and folds, a Chebyshev smoother -- runs once per lane with the one-vector
 * code.  Batched cycles run eagerly (no capture, no replay; eager and replayed cycles agree to the bit).  A fused launch counts
 * under MG_PATH_MATRIX_FREE as 1 launch and as many sweeps as it has lanes: sweeps / launches shows the fusion.
 *
 * Pointer arrays are HOST arrays of nb DEVICE pointers, each to the level's n_global doubles in the numbering of
 * mg_set_vector_device.  After a batch call the levels, the factorisation, the Chebyshev intervals, the cached graphs and the
 * tuning are as before, and a following mg_pcg gives the bits it gives on a handle that never ran a batch; the handle's own
 * MG_VEC_V, MG_VEC_F and MG_VEC_R are UNSPECIFIED (they were lane 0's).  Refused by name before anything is launched or
 * allocated: nb outside 1..MG_BATCH_MAX, null arrays or pointers, a pointer that is not device memory of the handle's device, an
 * output that overlaps another lane's output or any input (its own included: the march reads neighbours), slab handles, 2-D
 * handles, flat levels; mg_pcg_batch also level 0, a Gauss-Seidel smoother with a matrix-free level in the cycle, and whatever
 * mg_pcg refuses (face-set and transfer mismatches, levels without a matrix).
 *
 * mg_apply_batch  out_b = one Jacobi sweep of x_b with the handle's omega (MG_BATCH_JACOBI; the handle's smoother must be
 *                 Jacobi), f_b - A x_b (MG_BATCH_RESIDUAL) or A x_b (MG_BATCH_SPMV; f_dev is ignored and may be null), for
 *                 b = 0 .. nb - 1 on a stored or matrix-free level: the bits of mg_smooth(level, 1), mg_residual and the SpMV of
 *                 mg_pcg / mg_quadratic_form on MG_VEC_V = x_b, MG_VEC_F = f_b.  dots (SpMV only, may be null): dots[b] =
 *                 x_b . A x_b on the host, the bits of mg_quadratic_form.
 * mg_pcg_batch    lane b's x_dev[b] (the initial guess on entry, the solution on return), resid_hist[b * max(1, max_iter) + k]
 *                 and iterations[b] are, bit for bit, those of mg_set_vector_device(F = f_b), mg_set_vector_device(V = x_b),
 *                 mg_pcg(level, rtol, max_iter), mg_get_vector_device(V) on the same handle, for any nb and any mix of lanes.
 *                 The lanes run in lockstep, each with its own alpha, beta, dots and stopping test; a lane that has stopped
 *                 leaves the batch and its x is not touched again.  resid_hist and iterations may be null.
 * mg_batch_info   lanes held beyond the handle's own (0 until a call with nb >= 2) and their device bytes
 * mg_release_batch  frees them */
#define MG_BATCH_MAX 32
enum mg_batch_op { MG_BATCH_JACOBI = 0, MG_BATCH_RESIDUAL = 1, MG_BATCH_SPMV = 2 };
int mg_apply_batch(mg_handle h, int level, int op, int nb, const double* const* x_dev, const double* const* f_dev,
                   double* const* out_dev, double* dots /* [nb] or NULL */);
int mg_pcg_batch(mg_handle h, int level, int nb, const double* const* f_dev, double* const* x_dev, double rtol, int max_iter,
                 double* resid_hist /* [nb][max(1, max_iter)] */, int* iterations /* [nb] */);
int mg_batch_info(mg_handle h, int* lanes, int64_t* bytes);
int mg_release_batch(mg_handle h);

/* ---- smallest eigenpairs: K u = lambda M(rho) u by multigrid-preconditioned LOBPCG (no reference counterpart) -----------
 * K is the level's operator (A(kappa) + R(sigma) + B(alpha) on the free nodes of a generated diffusion level), M(rho) = R(rho)
 * the lumped mass of a cell field rho (the reaction_diag kernel, +0.0 on the Dirichlet nodes of the level's face set).  The
 * eigenvalues are the decay rates of rho u_t = div(kappa grad u) - sigma u under the handle's boundary conditions.
 *
 * mg_eigs  the k smallest eigenpairs with a block of `block` vectors, 1 <= k <= block <= MG_EIGS_MAX; the vectors beyond k are
 *          guards that keep a cluster at the block's edge from stalling the wanted ones.
 *   rho_dev   N^3 cell values > 0 on the device in the cell order of mg_gen_diffusion_level; NULL: rho = 1.
 *   x_dev     HOST array of `block` DEVICE pointers to n_global doubles each, in the numbering of mg_set_vector_device.  warm = 0:
 *             the library fills the start block itself, cheb_hash(row + lane * n_global) with `row` the level's lexicographic row
 *             (the global index of a whole level), zero on the Dirichlet nodes; warm = 1: the start block is read from x_dev, Dirichlet
 *             entries taken as 0.  On return x_dev[j], j < block, are the Ritz vectors: M-orthonormal, exactly +0.0 on Dirichlet nodes.
 *   lambda    [block], ascending; resid [block]: ||K x_j - lambda_j M x_j||_2 / (lambda_j ||M x_j||_2).
 *   iterations, restarts (may be null): iterations done / iterations that dropped P.
 *   It stops when resid[j] <= rtol for all j < k, or after max_iter iterations; reaching max_iter is not an error (as in mg_pcg).
 *
 *   The start block takes one Rayleigh-Ritz step by itself (K X by the level's SpMV, X^T K X and X^T M X, the dense solve, X and K X
 *   rotated); it counts as no iteration, so a converged warm start returns after 0 iterations.  One iteration:
 *     1. R_j = K x_j - lambda_j M x_j with both norms of the stopping test: ONE vector kernel per lane (eigs_residual: 24 B read, 8 B
 *        written per row, the sums in the same pass; a block_combine with the nodal weight would read as much and need the norms
 *        from two more Gram launches), a fold per lane, one download of 2 block doubles.
 *     2. W = one V-cycle from a zero guess on each R_j through the lanes of the batched solves (vcycle_batch: fused Jacobi and
 *        residual launches on matrix-free levels, eager like every batched cycle); W is lane j's MG_VEC_V and is not copied.
 *        Then W <- W - X (X^T M W), one Gram launch set, a download of block^2 doubles and one in-place block_combine: the
 *        residual of a vector that has converged below the rounding of its Ritz value is a multiple of M x, and its cycle a
 *        multiple of x.
 *     3. K W through the fused matrix-free SpMV (groups of "mf_batch" lanes) or the stored level's SpMV per lane.
 *     4. S = [X W P] (no P in the first iteration).  S^T K S and S^T M S by block_gram, tiles on and above the diagonal; X^T M X = I
 *        and X^T K X = diag lambda need no launch.  The columns are scaled to unit M-norm in the two matrices on the host and
 *        the scale goes into the coefficients: the numbers of scaled columns without a pass over the vectors.
 *     5. One download of the two matrices, the dense generalised eigenproblem on the host (Cholesky of S^T M S, cyclic Jacobi:
 *        mg_dense_eig.h), then block_combine for X, K X (in place) and P, K P: K is applied to W only.
 *     6. A failed Cholesky step (a pivot <= n eps times the largest diagonal entry) redoes the step with S = [X W] and counts a
 *        restart; if that fails too the call returns an error by name.
 *   The block that is about to be returned (converged, or max_iter reached) takes the start block's step once more -- K X applied,
 *   both Gram matrices computed, nothing taken as known -- and the stopping test is repeated on the result: the iteration rotates
 *   K X with X, and a nearly dependent [X W P] costs orthonormality of the order eps cond(S^T M S), which this step takes back to
 *   rounding level.  It counts as no iteration.  Soft locking of converged vectors is not done.
 *
 *   Work vectors X, K X, K W, P, K P (block each), M, the kernels' partial sums and the folded sums are allocated at the first
 *   call and kept for later calls on the same level with the same or a smaller block; the lanes of the batched solves (mg_batch_info)
 *   are used for R and W.  mg_memory_bytes and mg_eigs_info count them; mg_release_eigs, mg_destroy, mg_release_batch and a level
 *   set again with another size free them.  A handle that never calls these entries allocates and launches what it did before.
 *   After a call the levels, the factorisation, the Chebyshev intervals, the cached graphs and the tuning are as before and a
 *   following mg_pcg gives the bits it gives on a handle that never ran mg_eigs; the handle's own MG_VEC_V, MG_VEC_F and MG_VEC_R
 *   are UNSPECIFIED, as after a batch call.
 *
 *   Refused by name before anything is launched or allocated: everything mg_pcg_batch refuses (2-D and slab handles, flat levels,
 *   level 0, face-set and transfer mismatches, a Gauss-Seidel smoother with a matrix-free level in the cycle, pointers that are not
 *   this device's memory), k or block out of range, x pointers that overlap each other, a rho that is not finite or not > 0 (the
 *   first such cell is named; found by a kernel like the sigma check), rtol <= 0 together with max_iter <= 0.
 *
 * mg_block_gram     out[i * nb + j] = a_i . (d * b_j) over the level's n_global rows, na, nb in 1..24, d_dev NULL: no weight.  Tiles
 *                   of at most 4 x 4 pairs, one pass over 4 + 4 (+ 1) vectors each (block_gram, mg_block.hip.h); every block writes
 *                   its partial sums and a fold sums them in a fixed order: no atomics, the same bytes every time, and a pair has
 *                   the same bits whatever tile it was computed in (a 1 x 1 call gives the bits of the pair in a 9 x 9 call).
 *                   na == nb and a_dev[i] == b_dev[i] for all i: a symmetric Gram matrix, only the tiles on and above the diagonal
 *                   are computed, every pair i > j is the mirror of (j, i): the matrix is symmetric to the bit.
 * mg_block_combine  out_o = sum_i coeff[i * no + o] s_i, i ascending, the first product and then one fma per input; ns in 1..24, no
 *                   in 1..8.  An output may BE one of the inputs (every row of every input is read before an output row is
 *                   written); any other overlap is refused.
 *   Both take HOST arrays of DEVICE pointers to n_global doubles, 16-byte aligned, and apply the checks above to them.
 * mg_eigs_info      the largest block the work vectors were allocated for (0: none) and their device bytes
 * mg_release_eigs   frees them */
#define MG_EIGS_MAX 8
int mg_eigs(mg_handle h, int level, int k, int block, const double* rho_dev, double* const* x_dev, int warm,
            double rtol, int max_iter, double* lambda, double* resid, int* iterations, int* restarts);
int mg_block_gram(mg_handle h, int level, int na, const double* const* a_dev, int nb, const double* const* b_dev,
                  const double* d_dev /* nodal weight or NULL */, double* out /* host, na x nb, row-major */);
int mg_block_combine(mg_handle h, int level, int ns, const double* const* s_dev, int no, const double* coeff /* host, ns x no */,
                     double* const* out_dev);
int mg_eigs_info(mg_handle h, int* block, int64_t* bytes);
int mg_release_eigs(mg_handle h);
/* Bookkeeping for tests: whole-vector host -> device / device -> host copies made through this handle so far,
 * V-cycles replayed from a captured hipGraph, graphs currently cached.  No reference counterpart. */
int mg_counters(mg_handle h, int64_t* uploads, int64_t* downloads, int64_t* graph_replays, int* graphs_cached);

/* Which kernels the Jacobi smoother (mg_smooth, the smoother calls of a V-cycle) ran, per level and per path.  A smoother
 * call tries the paths in a fixed order -- MG_PATH_SMALL, MG_PATH_BLOCK, MG_PATH_K2D, MG_PATH_KSWEEP_SLAB, MG_PATH_KSWEEP /
 * MG_PATH_KSWEEP_ESCAPE, the pair passes, one sweep at a time -- and the first one that applies takes the sweeps it can
 * (DESIGN.md section 5 lists the size thresholds).  No reference counterpart; for tests.
 *   launches       kernel launches of that path (a pass split into several launches counts each of them)
 *   sweeps         Jacobi sweeps of the whole level those passes completed, each pass counted once: for mg_smooth calls
 *                  alone the sweeps summed over all paths equal the sum of their nw
 *   tail_launches  K-sweep launches whose planner split off a last, nearly empty round of tiles ("fuse_k_tail")
 * Counts are taken on the host when a launch is enqueued or captured into a V-cycle graph: replays of a captured
 * cycle add nothing (mg_counters counts those), and neither do the launches of mg_time_kernel.  Gauss-Seidel
 * smoothers are not counted.  mg_reset_smoother_launches sets every count of every level to zero. */
enum mg_smoother_path {
    MG_PATH_SLICE = 0,          /* one sweep per launch, persistent slice kernels (also the boundary sweeps of slabs)       */
    MG_PATH_SWEEP1C = 1,        /* one sweep per launch as a plane march with row classes (sdia_sweep1c, "march_min_rows")  */
    MG_PATH_PAIR_CLASS = 2,     /* two sweeps per pass through row classes (sdia_jacobi2c, "fuse_min_rows")                */
    MG_PATH_PAIR_PLAIN = 3,     /* two sweeps per pass on the stored rows (sdia_jacobi2p / sdia_jacobi2)                   */
    MG_PATH_KSWEEP = 4,         /* 3..5 sweeps per pass, the K-sweep march on whole levels (sdia_jacobikc, "fuse_k")       */
    MG_PATH_KSWEEP_ESCAPE = 5,  /* ... its variant for levels with escape rows (sdia_jacobikc_escape)                      */
    MG_PATH_KSWEEP_SLAB = 6,    /* ... on slabs with K halo planes ("halo_depth"): edge and rest launches of one pass      */
    MG_PATH_BLOCK = 7,          /* 2..4 sweeps per launch on blocks resident on the CU (sdia_jacobi_block, "fuse_block")   */
    MG_PATH_K2D = 8,            /* 2..5 sweeps per launch on 2-D levels (sdia_jacobik2d, "fuse_2d")                        */
    MG_PATH_SMALL = 9,          /* all sweeps of a call in one launch of one workgroup (sdia_jacobi_small, "fuse_small")  */
    MG_PATH_MATRIX_FREE = 10,   /* one sweep per launch on a matrix-free diffusion level (diffusion_mf)                    */
    MG_PATH_COUNT = 11
};
int mg_smoother_launches(mg_handle h, int level, int path, int64_t* launches, int64_t* sweeps, int64_t* tail_launches);
int mg_reset_smoother_launches(mg_handle h);

/* The march plan ("fuse_k_plan") the K-sweep march of `sweeps` sweeps per pass (3..5) uses on `level` under the handle's
 * present tuning.  A wave of a tile keeps its longest run of consecutive planes in which all the class bytes it loads are
 * the level's main class, and its longest run in which each of them is what it was in the plane before:
 *   waves, planes               the (tile, wave) pairs that have a run of the first kind; the planes of those runs summed
 *   const_waves, const_planes   the same for runs of the second kind that are not the pair's run of the first kind
 * All 0 where no plan exists: not built yet (the first such launch outside a capture, or mg_prepare_cycle, builds it),
 * "fuse_k_plan" 0, or a launch that takes none (slabs, levels with escape rows, other tile shapes).  A plan is dropped
 * when the level's classes are rebuilt.  Null pointers are skipped.  For tests. */
int mg_march_plan(mg_handle h, int level, int sweeps, int64_t* waves, int64_t* planes, int64_t* const_waves, int64_t* const_planes);

/* ---- measurement -----------------------------------------------------------------------------
 * mg_time_kernel: average duration in milliseconds of `reps` back-to-back launches of
 * one kernel of the path on `level`, measured with HIP events on the handle's own
 * stream ("jacobi", "residual", "restrict", "prolong", "norm2"; "jacobi2" = the two-sweep pass, an
 * error on levels where mg_smooth does not use it; "jacobi2!" = the same wherever the kernel applies;
 * "chebyshev" = one Chebyshev step that reads x_{k-1}, with whichever one-step kernel mg_smooth would launch on the level;
 * "lattice" = one Jacobi launch of the lattice plane march ("lattice_march"), an error on levels that do not use it;
 * "jacobi_small" = the mu1 sweeps of a small level in one launch, an error where mg_smooth does not do that;
 * "jacobik" = one launch of the K-sweep 2-D kernel with K = "fuse_2d_k", an error on levels that do not use it;
 * "jacobik3" = one launch of the K-sweep plane march on a 3-D level ("jacobik3!": wherever it applies), "jacobiblk" = one launch
 * of the block pass ("fuse_block"; "jacobiblk!": whatever the level's size), errors on levels that do not use them;
 * "gs" = one full Gauss-Seidel sweep, all colours, with the configured Gauss-Seidel smoother;
 * "spmv" = one SpMV without the dot product, with the level's one-step kernel; "diffusion_mf", "diffusion_mf:jacobi",
 * ":residual", ":spmv", ":chebyshev" = the matrix-free diffusion march in that mode, an error on stored levels;
 * "dkappa" / "dkappa_gather" = mg_diffusion_dkappa of (MG_VEC_V, MG_VEC_F) into MG_VEC_R as the plane march / one thread per cell;
 * "apply_dkappa" = mg_diffusion_apply_dkappa with dkappa = the first N^3 entries of MG_VEC_F and x = MG_VEC_V, into MG_VEC_R;
 * "dkappa:all" / "apply_dkappa:all" = the same operands through mg_diffusion_dkappa_ex / mg_diffusion_apply_dkappa_ex with both
 * node sets MG_NODES_ALL;
 * "dsigma" = mg_diffusion_dsigma of (MG_VEC_V, MG_VEC_F) into the first N^3 entries of MG_VEC_R; "apply_dsigma" =
 * mg_diffusion_apply_dsigma with dsigma = the first N^3 entries of MG_VEC_F and x = MG_VEC_V, into MG_VEC_R (the
 * "diffusion_mf" keys time the march with the reaction term on a level that has one);
 * "drobin" = mg_diffusion_drobin of face z+ of (MG_VEC_V, MG_VEC_F) into the first N^2 entries of MG_VEC_R; "apply_drobin" =
 * mg_diffusion_apply_drobin of face z+ with dalpha = the first N^2 entries of MG_VEC_F and x = MG_VEC_V, into MG_VEC_R (an
 * error where z+ is a Dirichlet face of the handle's set);
 * "kappa_ingest" = one launch of the fused copy and coarsening of mg_gen_diffusion_hierarchy_device on a matrix-free level, from a
 * scratch copy of its kappa back into the level's own (the same bytes: the level is unchanged) and into a scratch coarse field,
 * arithmetic averaging; an error on stored levels);
 * "diffusion_mf_batch<NV>:jacobi", ":residual", ":spmv" (NV = 2, 3, 4) = one fused launch of the matrix-free march over NV vectors
 * (mg_apply_batch, mg_pcg_batch): MG_VEC_V, MG_VEC_F, MG_VEC_R and scratch copies of them; an error on stored levels.
 * "cell_grad" = mg_diffusion_cell_gradient with w = the first N^3 entries of MG_VEC_F and x = MG_VEC_V into a scratch of 3 N^3 whose
 * first entries (as many as MG_VEC_R holds) are copied to MG_VEC_R after the timed region; "cell_grad_nw" = the same with w null;
 * "cell_grad_dot" = mg_diffusion_cell_gradient_dot of x = MG_VEC_V and a scratch p whose components x, y, z are the first N^3 entries
 * of MG_VEC_V, MG_VEC_F, MG_VEC_V, into the first N^3 entries of MG_VEC_R; "cell_grad_t" = mg_diffusion_cell_gradient_t of that w and
 * that p into MG_VEC_R; the scratch is allocated and freed outside the timed region.
 * Used by bench.py for the roofline figure; its launches leave mg_smoother_launches as they were.  mg_sync waits for
 * the handle's stream. */
int mg_time_kernel(mg_handle h, const char* kernel, int level, int reps, double* avg_ms);
int mg_sync(mg_handle h);
/* bytes of device memory held by the handle */
int mg_memory_bytes(mg_handle h, int64_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* MG_HIP_H */
