// C ABI of libmg_hip.so (see include/mg_hip.h): hierarchy handle, level loop of the V-cycle
// kept on the device, RCCL slab exchange.  Host code only orchestrates launches on the
// handle's stream; all arithmetic of the path runs in the kernels of mg_kernels.hip.h.
#include "../../include/mg_hip.h"
#include "mg_csr_check.h"
#include "mg_kernels.hip.h"
#include "mg_direct.hip.h"
#include "mg_jacobi2.hip.h"
#include "mg_jacobik3d.hip.h"
#include "mg_jacobiblk.hip.h"
#include "mg_lattice.hip.h"
#include "mg_diffusion_mf.hip.h"
#include "mg_diffusion_mf_batch.hip.h"
#include "mg_diffusion_adj.hip.h"
#include "mg_diffusion_flux.hip.h"
#include "mg_diffusion_points.hip.h"
#include "mg_diffusion_kappa.hip.h"
#include "mg_block.hip.h"
#include "mg_nullspace.hip.h"
#include "mg_dense_eig.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

using namespace mgk;

// lower_ratio of the Chebyshev interval unless mg_set_chebyshev says otherwise (the cycle study of tools/time_chebyshev.py,
// DESIGN.md section 5, "Chebyshev smoother")
constexpr double CHEB_DEFAULT_LOWER_RATIO = 6.0;

namespace {

thread_local std::string g_err;

int fail(const std::string& msg) {
    g_err = msg;
    return 1;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(std::string(#expr) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + \
                        ":" + std::to_string(__LINE__) + ")");                                \
    } while (0)

#define MG_TRY(expr)            \
    do {                        \
        int r_ = (expr);        \
        if (r_ != 0) return r_; \
    } while (0)

// Every host CSR hand-off starts here, before anything is freed, allocated, uploaded or launched (mg_csr_check.h).
int check_csr(int64_t n_rows, int64_t n_cols, int64_t nnz, const void* indptr, int indptr_is_64, const int32_t* indices,
              bool allow_duplicates) {
    const std::string why = csr_check(n_rows, n_cols, nnz, indptr, indptr_is_64, indices, allow_duplicates);
    return why.empty() ? 0 : fail(why);
}

}  // namespace

// DevBuf, DVector, DevTemp: who owns device memory.  The header opens an anonymous namespace of its own and uses HIP_TRY, MG_TRY
// and fail() from above (so that a test can compile it against a stand-in for HIP): hence the namespace closed and reopened here.
#include "mg_devbuf.h"

namespace {

struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

RcclApi g_rccl;

int load_rccl() {
    if (g_rccl.lib) return 0;
    // MG_RCCL_LIBRARY: load another implementation of the same ten entry points (tests use an in-process
    // stand-in to exercise the asynchronous stream / event ordering of the slab transport on one GPU)
    void* lib = nullptr;
    if (const char* override_path = getenv("MG_RCCL_LIBRARY")) {
        lib = dlopen(override_path, RTLD_NOW | RTLD_LOCAL);
        if (!lib) return fail(std::string("cannot load MG_RCCL_LIBRARY: ") + dlerror());
    }
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return fail(std::string("cannot load librccl: ") + dlerror());
#define SYM(field, name)                                                      \
    *reinterpret_cast<void**>(&g_rccl.field) = dlsym(lib, name);              \
    if (!g_rccl.field) return fail(std::string("librccl lacks ") + name)
    SYM(GetUniqueId, "ncclGetUniqueId");
    SYM(CommInitRank, "ncclCommInitRank");
    SYM(CommDestroy, "ncclCommDestroy");
    SYM(Send, "ncclSend");
    SYM(Recv, "ncclRecv");
    SYM(AllReduce, "ncclAllReduce");
    SYM(Broadcast, "ncclBroadcast");
    SYM(GroupStart, "ncclGroupStart");
    SYM(GroupEnd, "ncclGroupEnd");
    SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
    g_rccl.lib = lib;
    return 0;
}

#define NCCL_TRY(expr)                                                                   \
    do {                                                                                 \
        ncclResult_t r_ = (expr);                                                        \
        if (r_ != ncclSuccess)                                                           \
            return fail(std::string(#expr) + ": " + g_rccl.GetErrorString(r_));          \
    } while (0)

struct Comm {
    int rank = 0, world = 1;
    int64_t replicate_below = 0;
    ncclComm_t nccl = nullptr;
    mg_exchange_fn ex = nullptr;
    mg_allreduce_fn ar = nullptr;
    mg_allgatherv_fn ag = nullptr;
    void* user = nullptr;
    // pinned host staging for the callback transport
    double* h_stage = nullptr;
    size_t h_stage_elems = 0;
    bool active() const { return world > 1; }
};

struct Level {
    bool set = false;
    bool has_matrix = false;
    int N = 0;
    Grid g{};
    int64_t n_global = 0, row0 = 0, nloc = 0, xlen = 0, halo_lo = 0, halo_hi = 0;
    bool replicated = true;      // false: this rank holds one slab and exchanges halos
    int hd = 0;                  // halo planes each vector of this level has room for (slabs)
    // how the matrix got its storage (mg_level_storage): bit-for-bit symmetric / within 2^sym_qbits ulps / not; first
    // asymmetric row (local lexicographic, -1: none) and the largest ulp distance of a pair; distinct rows seen by the class
    // dictionary (-1: not built) and the tolerance it was built with
    int rep_sym = -1, rep_sym_qbits = 0, rep_cls_qbits = 0, rep_distinct = -1;
    int64_t rep_first_asym = -1, rep_max_ulps = 0;
    bool cls_escape = false;     // rows of class CLS_ESCAPE exist: read from the stored row (K-sweep march only; other class kernels off)
    bool grid_decoupled = false; // no entry couples cells that are no grid neighbours (sdia_grid_decoupled; levels with row classes)
    int esc_kmax = 0;            // ... and the most sweeps per pass whose tiles' escape rows fit the march's pool (jk3_escape_window)
    int64_t rep_escape = 0;      // ... how many
    int cls_halo = 0;            // row classes of the neighbours' planes next to this slab: 0 not built yet, 1 in place, -1 unavailable
    bool flat = false;           // no grid structure (stand-alone smoother on any matrix)
    int W = 0, R = 1;
    int64_t nslices = 0;
    DevBuf<double> vals;
    DevBuf<int> cols;                    // freed once the offset codes exist
    DevBuf<unsigned long long> codes;    // offset-coded columns (see mg_kernels.hip.h)
    DevBuf<int> offsets;
    int ntable = 0, dcode = 0;
    bool coded = false;
    bool rb_ok = false;                     // index parity is a valid red-black colouring of the matrix
    int mc_ok = -1;                         // the nine lattice colours are a valid colouring of the matrix (-1: not checked yet)
    // symmetric diagonal storage (replaces vals + codes when the matrix is bit-for-bit symmetric)
    DevBuf<double> dvals;
    bool sdia = false;
    int wu = 0;
    int up[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t mlead = 0, mslices = 0;
    // row classes of the symmetric diagonal storage (mg_jacobi2.hip.h): one byte per row + a 256 x 8 table of full rows
    DevBuf<unsigned char> cls;
    DevBuf<double> ctab;
    int ncls = 0;
    // stencil classes of an offset-coded level (mg_kernels.hip.h, ell_cls_apply): one byte per row + (offset, value) lists
    DevBuf<unsigned char> scls;
    DevBuf<int> s_off;
    DevBuf<double> s_val;
    DevBuf<int> s_cnt;
    int nscls = 0;
    // ... and what the plane march of wide lattice stencils needs (mg_lattice.hip.h): entries as (di, dj, dk), the
    // most frequent classes
    DevBuf<int> s_pack;
    int lm_ntop = 0;
    int lm_top[LM_K] = {0, 0, 0, 0, 0, 0, 0, 0};
    // march plans of the K-sweep pass (mg_jacobik3d.hip.h, jk3_plan): per (tile, wave) the run of planes whose classes are all
    // `cmain` and the run whose classes do not change from plane to plane, one plan per K = 3, 4, 5 and tile shape 7, 8, and
    // one for shape 9 (K = 5; march_plan_slot).  Built at the first such launch outside a capture (or by prepare_cycle), dropped wherever `cls` is
    // installed; waves[i] / planes[i]: waves with a run of kind i (a constant run that is the cmain run counts there only), planes in them
    struct MarchPlan {
        DevBuf<int> iv;
        int64_t waves[2] = {0, 0}, planes[2] = {0, 0};
    };
    MarchPlan plan[7];
    int cmain = 0;                          // the most frequent class and its entries (passed to the kernels by value)
    double cm[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t cls_lead = 0;                   // cls[row + cls_lead], zero padding of cls_lead entries on both sides
    DevBuf<double> dinv;
    // matrix-free diffusion level (mg_diffusion_mf.hip.h): kappa of the N^3 cells is all the matrix there is
    bool mf = false;
    DevBuf<double> kappa;
    int faces = MG_FACES_ALL;               // the face set a generated diffusion level was built with (mg_set_diffusion_faces)
    bool diffusion_hierarchy = false;       // generated by one of the diffusion hierarchy entries: mg_refresh_diffusion_hierarchy may renew it
    bool react = false;                     // generated with a reaction diagonal R(sigma) (mg_set_diffusion_reaction) ...
    DevBuf<double> rdiag;                   // ... which a matrix-free level keeps as one more row vector (nodal, not sigma itself)
    int robin = 0;                          // the faces whose Robin field the level was generated with (mg_set_diffusion_robin): B(alpha) is
                                            // one more term of that nodal vector, rdiag = B or R + B (react stays "generated with sigma")
    DVector v, v2, f, err, ftrue;
    DVector sw;                             // once-relaxed boundary planes of a slab (paired sweeps, world > 1)
    DVector fcg_x, fcg_p, fcg_q, fcg_b;     // mg_pcg on this level: iterate, direction, A p, the saved right-hand side
    // Chebyshev smoother (mg_set_chebyshev): the Lanczos estimate of lambda_max(D^-1 A) (cheb_est_ok: it is valid for the level's
    // matrix and the handle's settings) and the caller's interval for this level (cheb_user_lmax > 0: used instead)
    bool cheb_est_ok = false;
    double cheb_lmax_est = 0.0, cheb_user_lmin = 0.0, cheb_user_lmax = 0.0;
    DevBuf<int> perm;
    int p1_ok = -1;                         // stencil offsets within the Kuhn pattern of the P1 transfers (-1: not checked yet)
    std::vector<int> h_offsets;             // the offset table (linear offsets) of an offset-coded level, host copy
    unsigned long long nnz_stored = 0, nnz_nonzero = 0;
    // per-rank plane ownership (for gathers): k-plane boundaries s[0..world]
    std::vector<int> splits;
};

}  // namespace

// Block-tridiagonal LU of the coarsest level (mg_direct.hip.h)
struct DirectSolver {
    bool tried = false, ok = false;
    bool pinned = false;                    // a singular level 0 (level_singular): factorised with node 0 pinned
    BtGeom g{};
    DevBuf<double> T;                       // nb dense p x p inverses of the Schur complements
    DevBuf<int> lcol, ucol;                 // couplings, nb * p * W each
    DevBuf<double> lval, uval;
    DevBuf<double> y, x, w;
};

// One lane of a batched solve (mg_pcg_batch, mg_apply_batch): the per-level vectors a solve and its V-cycle write -- V, its
// ping-pong partner (= R), F, ERR and mg_pcg's four work vectors -- and mg_pcg's scalars and partial sums.  A lane is swapped
// into the levels (and the handle) around every call that runs per lane; lane 0 is the handle's own set.
struct LaneLevel {
    DVector v, v2, f, err, fcg_x, fcg_p, fcg_q, fcg_b;
};
struct Lane {
    std::vector<LaneLevel> lv;              // by level
    DevBuf<double> fcg_work, fcg_spmv;
};

// What mg_eigs keeps between calls: the block X and K X, K W, P, K P of the iteration on one level (W itself is the cycle's result
// in the lanes' MG_VEC_V), the lumped mass M(rho), the kernels' partial sums and the folded sums on their way to the host.
// Allocated at the first call, kept for calls with the same level and the same or a smaller block; counted in the ledger.
struct EigsWork {
    int level = -1, block = 0;
    int64_t vec_total = 0;
    std::vector<DVector> x, kx, kw, p, kp;
    DVector m;
    DevBuf<double> parts, sums;
    int64_t bytes() const {
        size_t n = m.raw.count() + parts.count() + sums.count();
        for (const auto* set : {&x, &kx, &kw, &p, &kp})
            for (const DVector& v : *set) n += v.raw.count();
        return (int64_t)(n * sizeof(double));
    }
};

// One captured V-cycle (hipGraph): valid for a level, a parameter epoch and a ping-pong state.
struct CycleGraph {
    int level = -1;
    uint64_t epoch = 0;
    std::vector<double*> pre, post;     // raw pointer of MG_VEC_V on levels 0..level before / after the cycle
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

// A located point set (mg_points_create; mg_diffusion_points.hip.h, "Located point sets"): device memory of its own, counted in
// the handle's ledger, owned by the handle's list `point_sets` -- an entry looks a set up there before it reads a member.
struct mg_points {
    int level = -1, N = 0;                  // the level it was located on and that level's cells per axis then
    int64_t M = 0, R = 0, longest = 0;      // points, runs of equal node among the 4 M sorted slots, slots in the longest run
    DevBuf<double> pts;                     // 3 M: the set's copy
    DevBuf<PtSlot> rec;                     // 4 M: the slots in the stable order by node
    DevBuf<int64_t> run_start, run_node;    // R + 1, R
    int64_t bytes() const {
        return (int64_t)(pts.count() * sizeof(double) + rec.count() * sizeof(PtSlot) + (run_start.count() + run_node.count()) * sizeof(int64_t));
    }
};

struct mg_context {
    int dim = 2, nlev = 0, device = 0;
    hipStream_t stream = nullptr;
    hipStream_t comm_stream = nullptr;      // halo exchange overlapped with interior sweeps (world > 1)
    hipEvent_t ev_boundary = nullptr, ev_halo = nullptr;
    int overlap = 1;
    int halo_planes = 1;                    // grid planes exchanged with each slab neighbour (2: stencils that reach two planes, P2)
    int halo_depth = 0;                     // halo planes ALLOCATED per vector (>= halo_planes; 0: just those): the K-sweep march on slabs
                                            // exchanges K planes once per K sweeps (mg_jacobik3d.hip.h)
    int64_t overlap_min_rows = (int64_t)1 << 22;
    std::vector<Level> L;
    int mu1 = 50, mu2 = 50;
    double omega = 2.0 / 3.0;
    int restriction = MG_RESTRICT_INJECTION, smoother = MG_SMOOTH_JACOBI;
    double coarse_rtol = 1e-14;
    int coarse_maxit = 20000;
    int keep_err = 0;
    // Chebyshev smoother (MG_SMOOTH_CHEBYSHEV, mg_set_chebyshev): Lanczos steps of the estimate, interval [b / lower_ratio, b]
    // with b = upper_factor * the estimate; device bytes the last estimate held while it ran (freed afterwards)
    int cheb_eig_steps = 10;
    double cheb_lower_ratio = CHEB_DEFAULT_LOWER_RATIO, cheb_upper_factor = 1.1;
    int64_t cheb_peak_bytes = 0;
    // tuning
    int use_codes = 1;          // offset-coded columns where a level allows it
    int use_sdia = 1;           // symmetric diagonal storage where a level is bit-for-bit symmetric
    int strip_slices = 64;      // XCD strip traversal for 3-D levels (0 = chunked map only)
    int nontemporal = 1;        // streaming loads for matrix / rhs data
    // Dynamic LDS bytes requested per block by the symmetric-diagonal launches on large levels.  The kernels do not
    // use it; it caps the resident blocks per CU at 160 KiB / pad = 5 (20 waves instead of the 28 the register
    // budget allows), which measured 2.4 % faster on the 1025^3 sweep in an interleaved A/B (tools/ab_lds_pad.py:
    // 11.64 vs 11.93 ms; 3 blocks per CU: 14.2 ms) -- fewer concurrent streams per HBM page.  At most kLdsPadMax: with the
    // 32 bytes of static LDS of the dot-product form a block still fits the CU's 160 KiB (one block per CU).
    static constexpr int kLdsPadMax = 150 * 1024;
    int lds_pad = 32768;
    int rows_per_lane = 2;      // measured best on MI355X (profiles/): 16 B value loads per lane
    unsigned chunk = 8;         // XCD chunk of the block -> tile map
    int pcg_chunk = 16;
    // scratch
    DevBuf<double> partials;        // 2 * kMaxParts doubles
    DevBuf<double> scalars;         // 8 doubles
    DevBuf<int> done;
    double* h_scalars = nullptr;    // pinned, 8 doubles + flag
    DevBuf<double> pcg_r, pcg_z, pcg_q, pcg_part_a, pcg_part_b;     // the coarse CG, sized for level 0 (they go with it: free_level)
    DVector pcg_p;
    int pcg_parts = 0, pcg_parts_a = 0;
    int pcg_predict = 0;
    // mg_pcg: scalars, folded / slab-reduced sums and the step kernels' partial sums (fcg_work); the
    // SpMV's partial sums of p.q (fcg_spmv: one per block of the level's SpMV, grown on demand)
    DevBuf<double> fcg_work, fcg_spmv;
    // batched solves: lanes 1, 2, ... (lane 0 is the handle's own vectors), allocated at the first batch call that needs them and
    // kept until mg_release_batch, mg_destroy or a level set again with another size; "mf_batch": the most lanes one fused
    // launch of the matrix-free march takes (0 / 1: never fuse; DESIGN.md, "Batched solves")
    std::vector<Lane> lanes;
    EigsWork eigs;                  // mg_eigs: its work vectors (freed by mg_release_eigs, mg_destroy and wherever the lanes are)
    int mf_batch = 4;
    double* h_lanes = nullptr;      // pinned, MG_BATCH_MAX doubles: every lane's ||r||^2 of an iteration in one host round trip (first mg_pcg_batch)
    int use_graph = 1;             // replay whole V-cycles as hipGraphs (single GPU, direct coarsest solve)
    int comm_priority = 1;          // communication stream created with the highest priority (MG_COMM_PRIORITY=0: lowest)
    int lattice_march = 1;          // wide lattice stencils (P2 levels) as a plane march with x in LDS (mg_lattice.hip.h)
    int64_t lattice_march_min_rows = 1 << 22;       // (measured on C5: the 129^3 and 65^3 lattices are faster with the gathering kernel)
    int lattice_gs2 = 0;            // nine-colour Gauss-Seidel on whole lattice levels: two colours per launch, out of place (lat_gs2;
                                    // measured slower than nine colour launches: 9.1 against 6.8 ms per sweep of the 513^3 lattice)
    int diffusion_faces = MG_FACES_ALL;     // mg_set_diffusion_faces: the faces with a Dirichlet condition in the diffusion levels generated
                                    // from now on, and what MG_NODES_INTERIOR masks; the other faces are no-flux faces
    // insulated bodies (mg_set_diffusion_insulated sets the face set 0): the lumped mass w of rho = 1 on the all-free grid of
    // ns_N cells per dimension with 1 / (w.1), built at the first projected solve of a level of that size, and the mean
    // removals' partial sums and total (ns_part: ns_blocks(rows) + 1 doubles, the total last)
    DevBuf<double> ns_w, ns_part;
    int ns_N = 0;
    double ns_inv_s = 0.0;
    DevBuf<double> sigma;           // mg_set_diffusion_reaction: the handle's copy of sigma, sigma_N^3 cells (empty: no reaction term), read
    int sigma_N = 0;                // where diffusion levels are generated
    DevBuf<double> alpha[6];        // mg_set_diffusion_robin: the handle's copies of the Robin fields by face bit (x-, x+, y-, y+, z-, z+),
    int alpha_N = 0;                // alpha_N^2 face-cells each (empty: no field on that face), read where sigma is
    int dkappa_gather = 0;          // mg_diffusion_dkappa: 1 = one thread per cell reading through the caches instead of the plane march
                                    // (1025^3: 12.5 ms against 5.75 for the march)
    int lattice_tile = 0;           // tile of that march: 0 / 1 = 64 x 16 cells (256 threads), 2 = 128 x 16 (512 threads)
    int lattice_segments = 0;       // plane segments per tile of that march, 0 = chosen from the tile count
    int slab_pair_form = 0;         // overlapped pair sweeps on slabs: 0 = chain beside one launch of the pass, 1 = boundary segments first
    int graph_comm = 0;             // ... on slabs too: the RCCL exchanges are captured with the kernels (opt-in)
    uint64_t epoch = 1;             // bumped by every call that changes what a V-cycle launches
    std::vector<CycleGraph> graphs;
    bool capturing = false;         // between hipStreamBeginCapture and hipStreamEndCapture of vcycle_graphed (zero_doubles)
    int use_direct = 1;             // exact block-tridiagonal coarsest solve where the level allows it
    int require_diagonal = 1;       // 0: operators without a diagonal (D^-1 R of the split smoother)
    int fuse_restrict = 1;          // residual evaluated at the coarse nodes only when restricting by injection
    // K sweeps per launch on blocks resident on the CU (mg_jacobiblk.hip.h): whole 3-D levels with row classes of
    // fuse_block_min_rows <= rows < fuse_block_max_rows (below the plane marches' sizes); 2: whatever the size (tests).
    // Three sweeps per launch on blocks of 11 planes: alone no faster per sweep than one launch per sweep (129^3: 13.2 us
    // against 14.3; 65^3: 3.9 against 4.0; profiles/r03_block_pass.txt), but a third of the launches inside a cycle, where a
    // one-sweep launch costs 14.8 / 5.8 us: BASELINE config 3 132.8 -> 137.5 cycles/s (profiles/r03_block_cycles.txt).  Blocks
    // of 19 planes spill and are slower (124.4).
    int fuse_block = 1;
    int64_t fuse_block_min_rows = (int64_t)1 << 15, fuse_block_max_rows = (int64_t)1 << 23;
    int fuse_block_k = 0, fuse_block_ez = 11;   // sweeps per launch (0: three, four on levels whose blocks then all run at once) / planes per block (11 or 19)
    int direct_block_rows = 2048;   // "direct_block_rows": rows per block of the coarsest level's block-tridiagonal LU, at least
    int fuse_2d_lines = 0;          // "fuse_2d_lines": lines per region of the 2-D K-sweep kernel (64, 32 or 16; 0: chosen per level)
    int gen_odd_rows = 0;           // "gen_odd_rows": mg_gen_poisson_level perturbs the diagonal of this many interior rows in 10000
    int cls_escape = 1;             // "row_escape": more than 255 distinct rows -> the frequent ones as classes, the rest read from their stored row
    int storage_auto = 1;           // "storage_auto": a level whose exact symmetry test / row dictionary fails is tried once more with 4 ulps
    int storage_qbits = 0;          // "storage_ulps": low mantissa bits ignored by the symmetry test and the row dictionary
    int use_classes = 1;            // one class byte per row where a level has <= 255 distinct rows (two-sweep pass)
    int fuse_sweeps = 1;            // pairs of Jacobi sweeps in one pass (mg_jacobi2.hip.h) on large 3-D levels
    int64_t fuse_min_rows = (int64_t)1 << 24;
    int fuse_segments = 0;          // plane segments per tile (0: chosen from the item count)
    int fuse_nontemporal = 0;       // streaming loads in the two-sweep kernel (measured slower: tiles re-read their rims)
    int fuse_classes = 1;           // the two-sweep pass reads row classes where the level has them
    int fuse_plain_shape = 0;       // ... its launch shape: 0 = 12 waves x 1 line (no spills), 1 = 8 x 2, 2 = 16 x 1
    int fuse_plain = 2;             // the pass on the stored rows (no classes): 2 = round-2 structure (sdia_jacobi2p), 1 = round 1's
    int class_sweeps = 1;           // so do the one-sweep kernels (residual, single Jacobi / Gauss-Seidel sweeps, SpMV)
    int fuse_k = 5;                 // sweeps per pass of the class-coded K-sweep march (mg_jacobik3d.hip.h): 3..5; < 3: pairs only
    int fuse_k_shape = -1;          // ... its tile: 1 = 64 x 48 cells (12 waves x 4 lines), 4 = 64 x 24 (8 waves x 3 lines, two workgroups
                                    // per CU), 7 = 64 x 32 by 16 waves (no spills up to five sweeps), 8 = shape 7
                                    // with one barrier per step (level 0 in registers, images double-buffered), 9 = shape 8 on 64 x 36
                                    // tiles whose first and last wave own the four rim lines (five sweeps on whole levels; elsewhere
                                    // it stands for 8, for 7 below five sweeps); -1: for five sweeps per pass 9 on whole levels of at
                                    // least "fuse_k_rim_min_rows" rows and 8 elsewhere, 7 for three and four (jk3_shape_for).  The
                                    // shapes 0, 2, 3, 5 and 6 were measured slower and retired ("Tile shape")
    int64_t fuse_k_rim_min_rows = (int64_t)1 << 26;    // ... (513^3 and 1025^3 rows: where shape 9 was measured against shape 8)
    int fuse_k_segments = 0;        // ... plane segments per tile (0: chosen from the item count)
    int timing_force_form = -1;     // mg_time_kernel("jacobik3:formN"): every step of the K-sweep pass in one form (wrong results; how fast
                                    // each form is by itself)
    int64_t fuse_k_slab_min_rows = (int64_t)1 << 20;   // ... on slabs: levels whose smallest slab has at least this many rows
    int fuse_k_slab_min_sweeps = 4; // ... on slabs: smoother calls of at least this many sweeps (fewer: pairs with the boundary chain)
    int64_t fuse_k_min_rows = (int64_t)1 << 24;        // ... on whole levels with at least this many rows (fewer: single sweeps.  129^3 rows:
                                                       //     12.2 us per sweep in the march against 14.3 alone, but whole C3 cycles do not
                                                       //     get faster with it, 127.4 against 127.9 per second; 65^3: 11.6 against 4.0)
    int64_t fuse_k_small_rows = (int64_t)1 << 22;      // ... five sweeps per pass again on levels with fewer rows than this (129^3: 12.2 us
                                                       //     per sweep with five, 15.5 with four: profiles/r03_small_levels.txt)
    int64_t fuse_k5_min_rows = (int64_t)1 << 26;       // ... five sweeps per pass on levels with at least this many rows (257^3: four measured best)
    int64_t fuse_k4_min_rows = 0;                      // ... more than three sweeps per pass on levels with at least this many rows
    int fuse_k_nt_store = 0;        // ... non-temporal stores of its result (experiment)
    int fuse_k_min_side = 32;       // ... the shortest grid lines / fewest lines per plane of a whole level that pass takes (tests: 16)
    int fuse_k_tail = 1;            // ... the tiles left over for a last, nearly empty round of workgroups get shorter plane segments
    int fuse_k_small_tiles = 0;     // ... 64 x 24 tiles (shape 4) on levels whose planes hold fewer 64 x 48 tiles than there are CUs
    int fuse_k_load_early = 1;      // ... tile shape 9: the next plane's loads go out as soon as their registers are free (jk3_rim_body)
    int64_t fuse_k_load_early_min_rows = (int64_t)1 << 29;     // ... on levels of at least this many rows (1025^3: -4 %; 513^3: no faster)
    int fuse_k_plan = 1;            // ... march plans: steps whose planes are known to hold the main class only, or the same classes
                                    // plane after plane, load and inspect no classes (whole levels without escape rows, tile
                                    // shapes 7 and 8; 0: every step does)
    std::vector<const void*> large_lds_kernels;     // kernels whose dynamic-LDS limit has been raised (allow_large_lds)
    int fuse_shape = 1;             // launch shape of the class-coded pass (launch_jacobi2); 1 measured best
    int fuse_wi = 0;                // experiments: cells per tile line with a second sweep (0: chosen per level)
    int fuse_even = 0;              // all tile columns of the class-coded pass equally wide (measured slower: more full tiles, same bytes)
    int march_sweeps = 1;           // one-sweep class kernels as a plane march on large 3-D levels (sdia_sweep1c)
    int64_t march_min_rows = (int64_t)1 << 22;
    int march_shape = 0;            // 0 = 12 waves x 2 lines, 1 = 16 waves x 2 lines
    int64_t fuse_small_2d_rows = 2048;  // ... 2-D levels only up to this many rows (larger ones: the K-sweep 2-D kernel)
    int fuse_small = 1;             // all sweeps of a level that fits one CU's LDS in one launch (sdia_jacobi_small)
    int fuse_2d = 1;                // K sweeps per launch on 2-D levels with row classes (sdia_jacobik2d)
    int fuse_2d_k = 5;              // ... at most this many (2..5)
    int fuse_xcd_chunk = 32;        // consecutive tiles of that pass per XCD at a time
    int cls_blocks_per_cu = 4;      // persistent blocks of the one-sweep class kernels (72 VGPRs, 94 SGPRs admit 7)
    DirectSolver direct;
    // the reference's L2(Omega) norms (res_calculator / err_calculator, multigrid.py:203-218) on the device: a mass
    // matrix M of one level (mg_set_mass_csr), optionally the exact solution's nodal values (mg_set_exact)
    // table prolongation (mg_set_prolongation_table; null: the reference's bilinear / trilinear interpolation)
    DevTemp ptab_count;                     // (int; the transfer tables are owned but not counted)
    int p1_prolong = 0;                     // mg_set_prolongation_p1: the P1 natural embedding (excludes the table)
    DevTemp rtab_count;                     // table restriction (mg_set_restriction_table), MG_RESTRICT_TABLE: int
    DevTemp rtab_off;                       // int
    DevTemp rtab_w;                         // double
    int rtab_m = 0;
    DevTemp ptab_off;                       // int
    DevTemp ptab_w;                         // double
    Level mass;
    int mass_level = -1;
    DVector mass_out, diff, uexact;
    int uexact_level = -1;
    int64_t uploads = 0, downloads = 0, graph_replays = 0;   // whole-vector host <-> device copies; hipGraphLaunch calls
    // Jacobi smoother passes per level and path (mg_smoother_launches), counted when enqueued or captured
    struct SmootherCount { int64_t launches = 0, sweeps = 0, tail = 0; };
    std::vector<std::array<SmootherCount, MG_PATH_COUNT>> smoother_counts;
    int jk3_tail = 0;               // the last launch of the K-sweep march split off a last round of tiles (a.ta < ntile)
    DevBuf<double> stage;           // device staging for host vectors (caller numbering)
    std::vector<std::unique_ptr<mg_points>> point_sets;     // mg_points_create .. mg_points_destroy; what is left goes with the handle
    int pt_group = PT_SET_NV;       // lanes per launch of the mg_points_* entries (MG_POINT_GROUP=1..8: measurements only; same bits)
    int64_t bytes = 0;
    Comm comm;
    hipDeviceProp_t prop{};
};

namespace {

constexpr int kMaxParts = 1024;

int64_t& tracked_bytes(mg_context* c) { return c->bytes; }

// Elements past the end of every vector: rows of the last, partly filled slice read (and ignore)
// x[row] for up to 64*R - 1 rows beyond nloc in the offset-coded kernels.
// The symmetric-diagonal kernels apply every offset to every row (absent entries are stored zeros), so
// the first / last rows also read x up to the largest offset before / after the vector.  Grid levels
// get zero-filled slack for the widest P1 pattern (offset plane + nx + 1) on both sides; a level whose
// offsets reach further keeps the coded format (repack_sdia checks against vec_reach).
constexpr int64_t kVecSlack = 260;

// (the class-coded two-sweep pass reads whole tiles without per-lane predicates: a plane + 2 lines + 2 beyond either end)
inline int64_t vec_reach(const Level& L) { return L.flat ? 0 : L.g.plane + 2 * (int64_t)L.g.nx + 8; }
inline int64_t vec_front(const Level& L) {
    // the first owned row starts a 128-byte line (hipMalloc returns 256-byte aligned memory)
    const int64_t slack = ((vec_reach(L) + 15) / 16) * 16;
    return slack + (16 - (L.g.lead % 16)) % 16;
}
inline int64_t vec_total(const Level& L) { return vec_front(L) + L.xlen + kVecSlack + vec_reach(L); }

int vec_alloc(mg_context* c, const Level& L, DVector* v) {
    return v->alloc(c, (size_t)vec_total(L), (size_t)vec_front(L), (size_t)L.g.lead, c->stream);
}

void vec_free(DVector* v) { *v = DVector{}; }

inline unsigned blocks_for(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// every row of the level has a class from the table (no escapes): what all class kernels but the K-sweep march need
inline bool cls_full(const Level& L) { return L.cls != nullptr && !L.cls_escape; }

// one thread per node of a plane (x), owned planes (y); block = kPlaneBlock threads
constexpr int kPlaneBlock = 256;
dim3 grid3(const Grid& g, int nk) { return dim3((unsigned)((g.plane + kPlaneBlock - 1) / kPlaneBlock), (unsigned)nk, 1u); }

int check_level(mg_context* c, int level, bool must_be_set = true) {
    if (!c) return fail("null handle");
    if (level < 0 || level >= c->nlev) return fail("level " + std::to_string(level) + " out of range");
    if (must_be_set && !c->L[level].set) return fail("level " + std::to_string(level) + " has not been set");
    return 0;
}

int need_matrix(mg_context* c, int level) {
    MG_TRY(check_level(c, level));
    if (!c->L[level].has_matrix) return fail("level " + std::to_string(level) + " has no matrix (grid-only level)");
    return 0;
}

// Code that reads a level's stored rows (values, columns, codes, diagonals, 1 / diagonal) asks here first: a matrix-free
// diffusion level has a matrix (has_matrix) but keeps kappa and none of those arrays.
int need_stored_rows(const mg_context* c, const Level& L, const std::string& who) {
    if (L.mf)
        return fail(who + ": level " + std::to_string((int)(&L - c->L.data())) + " is a matrix-free diffusion level (kappa only); " +
                    "this reads stored rows");
    return 0;
}

int need_grid(mg_context* c, int level) {
    MG_TRY(check_level(c, level));
    if (c->L[level].flat) return fail("level " + std::to_string(level) + " is flat (no grid): transfers are undefined");
    return 0;
}

// ---- slab geometry ---------------------------------------------------------------------------
// Plane boundaries on the coarsest grid t_g = floor(g*N0/G) (t_G = N0+1); level l uses
// t_g * 2^l, so coarse plane K and fine plane 2K always live on the same rank.
int setup_geometry_sized(mg_context* c, Level& L, int level, int N, int64_t flat_rows);

int setup_geometry(mg_context* c, Level& L, int level, int N, int64_t flat_rows = 0) {
    MG_TRY(setup_geometry_sized(c, L, level, N, flat_rows));
    // the lanes of batched solves hold vectors of the levels' sizes: a level that is set again with another size frees them all
    for (const Lane& lane : c->lanes)
        if ((size_t)level < lane.lv.size() && lane.lv[(size_t)level].v.raw && (int64_t)lane.lv[(size_t)level].v.raw.count() != vec_total(L)) {
            c->lanes.clear();
            c->eigs = EigsWork{};
            break;
        }
    if (c->eigs.level == level && c->eigs.vec_total != vec_total(L)) c->eigs = EigsWork{};
    return 0;
}

int setup_geometry_sized(mg_context* c, Level& L, int level, int N, int64_t flat_rows) {
    const int dim = c->dim;
    const Comm& cm = c->comm;
    Grid& g = L.g;
    L.flat = N == 0;
    if (L.flat) {
        // any square matrix: one "plane" holding every row; smoother / residual only
        if (cm.active()) return fail("flat levels are single-GPU only");
        if (flat_rows <= 0 || flat_rows >= (int64_t)INT32_MAX) return fail("bad row count");
        L.N = 0;
        g.nx = (int)flat_rows; g.ny = 1; g.nz = 1; g.plane = flat_rows; g.refine_y = 0;
        g.k0 = 0; g.nk = 1; g.lead = 0;
        L.n_global = L.nloc = L.xlen = flat_rows;
        L.row0 = L.halo_lo = L.halo_hi = 0;
        L.replicated = true;
        L.splits.assign(2, 0);
        L.splits[1] = 1;
        return 0;
    }
    L.N = N;
    g.nx = N + 1;
    g.ny = dim == 3 ? N + 1 : 1;
    g.nz = N + 1;
    g.plane = (int64_t)g.nx * g.ny;
    g.refine_y = dim == 3 ? 1 : 0;
    L.n_global = g.plane * g.nz;
    if (L.n_global >= (int64_t)INT32_MAX) return fail("level has more than 2^31-1 unknowns");
    L.replicated = !(cm.active() && L.n_global >= cm.replicate_below);
    if (level == 0 && cm.active()) L.replicated = true;      // the coarsest solve is never distributed
    L.splits.assign(cm.world + 1, 0);
    if ((N >> level) << level != N) return fail("elements_per_dim is not N0 * 2^level");
    const int N0 = N >> level;
    for (int r = 0; r < cm.world; ++r) L.splits[r] = (int)(((int64_t)r * N0) / cm.world) << level;
    L.splits[cm.world] = N + 1;
    if (!L.replicated) {
        if (N0 < cm.world) return fail("coarsest grid has fewer planes than ranks");
        g.k0 = L.splits[cm.rank];
        g.nk = L.splits[cm.rank + 1] - g.k0;
        if ((N0 / cm.world) << level < c->halo_planes) return fail("a slab is thinner than the halo");
        // room for "halo_depth" planes where the thinnest slab of the level has as many (every rank alike)
        L.hd = std::max(c->halo_planes, std::min(c->halo_depth, (N0 / cm.world) << level));
        L.halo_lo = cm.rank > 0 ? L.hd * g.plane : 0;
        L.halo_hi = cm.rank + 1 < cm.world ? L.hd * g.plane : 0;
    } else {
        g.k0 = 0;
        g.nk = g.nz;
        L.halo_lo = L.halo_hi = 0;
    }
    g.lead = L.halo_lo;
    L.row0 = (int64_t)g.k0 * g.plane;
    L.nloc = (int64_t)g.nk * g.plane;
    L.xlen = L.halo_lo + L.nloc + L.halo_hi;
    return 0;
}

int alloc_level_vectors(mg_context* c, Level& L) {
    MG_TRY(vec_alloc(c, L, &L.v));
    MG_TRY(vec_alloc(c, L, &L.v2));
    MG_TRY(vec_alloc(c, L, &L.f));
    return 0;
}

void free_direct(mg_context* c);

void drop_graphs(mg_context* c);

// The rule for device memory that is sized from a level: it is a member of that level, or it is released here with
// the level -- level 0's factorisation and the coarse CG's vectors, the mass matrix with its work vector, the exact
// solution with the difference vector -- because a level that is set again may have another size.  (fcg_spmv and the
// staging buffer grow on demand instead.)  The level itself goes back to what a fresh Level is: its default member
// initialisers are the one statement of that; only the caller's Chebyshev interval (mg_set_chebyshev_bounds, which may
// precede the level's set-up) stays.
void free_level(mg_context* c, Level& L) {
    ++c->epoch;
    drop_graphs(c);
    if (&L == &c->L[0]) {
        free_direct(c);
        c->pcg_r.reset(); c->pcg_z.reset(); c->pcg_q.reset(); c->pcg_part_a.reset(); c->pcg_part_b.reset();
        vec_free(&c->pcg_p);
        c->pcg_parts = c->pcg_parts_a = 0;
    }
    if (c->mass_level >= 0 && &L == &c->L[c->mass_level]) {
        vec_free(&c->mass_out);
        c->mass_level = -1;
        free_level(c, c->mass);
    }
    if (c->uexact_level >= 0 && &L == &c->L[c->uexact_level]) {
        vec_free(&c->uexact);
        vec_free(&c->diff);
        c->uexact_level = -1;
    }
    const double user_lmin = L.cheb_user_lmin, user_lmax = L.cheb_user_lmax;
    L = Level{};
    L.cheb_user_lmin = user_lmin; L.cheb_user_lmax = user_lmax;
}

// A level that is being set: what it held goes first, and unless the build ends with `return done()` what it got so far
// goes too, the error text kept (set-up paths have many early exits; they never leave a half-built level behind).
struct LevelBuild {
    mg_context* c;
    Level& L;
    bool built = false;
    LevelBuild(mg_context* c_, Level& L_) : c(c_), L(L_) { free_level(c, L); }
    LevelBuild(const LevelBuild&) = delete;
    LevelBuild& operator=(const LevelBuild&) = delete;
    ~LevelBuild() {
        if (built) return;
        const std::string why = g_err;
        free_level(c, L);
        g_err = why;
    }
    int done() {
        built = true;
        return 0;
    }
};

// ---- tile kernel dispatch --------------------------------------------------------------------
// A run-time value as a template argument: f(std::integral_constant<int, V>{}) for the V among Vs that equals v.
// false: v is none of them and f was not called (the caller keeps its own fallback: an error, or with_int_else).
template <int... Vs, class F>
bool with_int(int v, F&& f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// ... every other v takes the instance of Else (rows per lane in the set-up kernels: 1, 2, else 4)
template <int Else, int... Vs, class F>
void with_int_else(int v, F&& f) {
    if (!with_int<Vs...>(v, f)) f(std::integral_constant<int, Else>{});
}

template <class F>
void with_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// f(mode, dot) of a tile kernel: the four modes that have no dot product, and SpMV (any other mode) with or without one
template <class F>
void with_mode(int mode, bool dot, F&& f) {
    if (mode == MODE_RESIDUAL) f(std::integral_constant<int, MODE_RESIDUAL>{}, std::false_type{});
    else if (mode == MODE_JACOBI) f(std::integral_constant<int, MODE_JACOBI>{}, std::false_type{});
    else if (mode == MODE_CHEB) f(std::integral_constant<int, MODE_CHEB>{}, std::false_type{});
    else if (mode == MODE_GS) f(std::integral_constant<int, MODE_GS>{}, std::false_type{});
    else if (dot) f(std::integral_constant<int, MODE_SPMV>{}, std::true_type{});
    else f(std::integral_constant<int, MODE_SPMV>{}, std::false_type{});
}

// f(mode) of a plane march (lat_march, sdia_sweep1c): residual, Gauss-Seidel and Chebyshev; any other mode is a Jacobi sweep
template <class F>
void with_march_mode(int mode, F&& f) {
    with_mode(mode, false, [&](auto m, auto) {
        f(std::integral_constant<int, decltype(m)::value == MODE_SPMV ? MODE_JACOBI : decltype(m)::value>{});
    });
}

// prolongation kernels: (add, keep) = (true, true), (true, false), (false, true) -- a prolongation that does not add keeps
template <class F>
void with_add_keep(bool add, bool keep, F&& f) {
    if (add && keep) f(std::true_type{}, std::true_type{});
    else if (add) f(std::true_type{}, std::false_type{});
    else f(std::false_type{}, std::true_type{});
}

// offset codes are used for every width up to 64 entries per row (5, 7 and 15 have unrolled kernels)
inline bool coded_width(int W) { return W >= 1 && W <= 64; }

// The slices of one launch_ell: `count` slices from slice0 on (count < 0: up to the level's last).  gap > 0: they are
// [slice0, slice0 + split) and [slice0 + split + gap, ...) -- two ranges, one launch.
struct SliceRange {
    int64_t slice0 = 0, count = -1, split = 0, gap = 0;
    static SliceRange of(int64_t slice0, int64_t count) { return {slice0, count, 0, 0}; }
    // the first lo_count slices and those from hi_begin on, in one launch
    static SliceRange ends(const Level& L, int64_t lo_count, int64_t hi_begin) {
        return {0, lo_count + L.nslices - hi_begin, lo_count, hi_begin - lo_count};
    }
    // ... of a slab: the ends next to a neighbour (lo: below, hi: above); both in one launch where the slab has both
    static SliceRange ends_of_slab(const Level& L, bool lo, bool hi, int64_t lo_count, int64_t hi_begin) {
        if (lo && hi) return ends(L, lo_count, hi_begin);
        if (lo) return of(0, lo_count);
        return hi ? of(hi_begin, L.nslices - hi_begin) : of(0, 0);
    }
};

// What launch_ell is asked for: out = op(A, x) in `mode` over `slices` of the level (default: all of them).
struct EllRequest {
    int mode = MODE_JACOBI;
    bool dot = false;                   // MODE_SPMV: the partial sums of x . out go to `partials` as well
    const double* x_base = nullptr;     // x with its lower halo (DVector::base)
    const double* f_rows = nullptr;
    double* out_rows = nullptr;
    double* partials = nullptr;
    const int* done = nullptr;
    unsigned* grid_out = nullptr;       // the number of blocks launched (= partial sums written), if asked for
    SliceRange slices{};
    int color = 0;                      // MODE_GS: the colour that is relaxed
    double alpha = 0.0, beta = 0.0;     // MODE_CHEB: the step scalars; x_{k-1} is read from out_rows
};

// the usual operands on a level: x = v, f, out = v2
EllRequest level_op(const Level& L, int mode) {
    EllRequest q;
    q.mode = mode; q.x_base = L.v.base; q.f_rows = mode == MODE_SPMV ? nullptr : L.f.rows; q.out_rows = L.v2.rows;
    return q;
}

// the finest of several levels (its Jacobi kernels skip what only coarser levels need) / a slab that exchanges halos
inline bool is_finest(const mg_context* c, const Level& L) { return c->nlev > 1 && &L == &c->L[c->nlev - 1]; }
inline bool is_slab(const mg_context* c, const Level& L) { return !L.replicated && c->comm.active(); }

// The class fields of a kernel-argument struct from the level's row classes.  Two conventions: the tile and K-sweep
// kernels of mg_kernels / mg_jacobi2 (JKArgs, JSArgs, JBArgs, EllArgs) take the class of row 0 ...
template <class Args>
void fill_classes(Args& a, const Level& L) {
    a.cls = L.cls + L.cls_lead; a.ctab = L.ctab; a.ncls = L.ncls; a.cmain = L.cmain;
    for (int t = 0; t < 8; ++t) a.cm[t] = L.cm[t];
}
// ... the plane marches (J2Args, JK3Args) the start of the padded array and its lead
template <class Args>
void fill_classes_lead(Args& a, const Level& L) {
    a.cls = L.cls; a.clead = L.cls_lead; a.ctab = L.ctab; a.ncls = L.ncls; a.cmain = L.cmain;
    for (int t = 0; t < 8; ++t) a.cm[t] = L.cm[t];
}

// Plane segments per tile of a plane march: `ntile` tiles cut into n segments run in rounds of `resident` workgroups, a
// segment costs its planes plus `warmup` plane-times; the n in 1..most with the cheapest rounds x (planes + warm-up), the
// smallest such n.
int best_segments(int64_t ntile, int64_t resident, int planes, int most, double warmup) {
    int best = 1;
    double best_cost = 1e300;
    for (int n = 1; n <= std::max(1, most); ++n) {
        const double cost = (double)((ntile * n + resident - 1) / resident) * ((planes + n - 1) / n + warmup);
        if (cost < best_cost) { best_cost = cost; best = n; }
    }
    return best;
}

// `items` work items of a launch whose blocks walk them in chunks of xcd_chunk per XCD: the grid, whole groups of 8 chunks
int tile_grid(int64_t items, unsigned xcd_chunk, unsigned* grid) {
    if (items >= ((int64_t)1 << 31) - 4096) return fail("too many tiles");
    const int64_t group = 8 * (int64_t)xcd_chunk;
    *grid = (unsigned)(((items + group - 1) / group) * group);
    return 0;
}
int launch_sweep1c(mg_context* c, const Level& L, int mode, const double* x_rows, const double* f_rows, double* out_rows,
                   int color, double alpha = 0.0, double beta = 0.0);
bool sweep1c_ok(const mg_context* c, const Level& L);

int allow_large_lds(mg_context* c, const void* kernel, size_t bytes);

// Plane march of wide lattice stencils (mg_lattice.hip.h): 3-D grid levels with stencil classes whose entries reach at
// most two cells / lines / planes (prepare_lat_march found them decomposable).
bool lat_march_ok(const mg_context* c, const Level& L) {
    return c->lattice_march && L.scls && L.s_pack && L.lm_ntop > 0 && !L.flat && L.g.ny >= 16 && L.g.nx >= 32 &&
           L.nloc >= c->lattice_march_min_rows;
}

template <int TI, int TJ, int NT>
int launch_lat_march_t(mg_context* c, const Level& L, LatArgs a, int mode) {
    a.ntx = (L.g.nx + TI - 1) / TI; a.nty = (L.g.ny + TJ - 1) / TJ;
    const int64_t ntile = (int64_t)a.ntx * a.nty;
    const size_t lds = lm_lds_bytes(L.W, TI, TJ);
    const int per_cu = lds > (size_t)80 * 1024 ? 1 : 2;             // resident workgroups per CU
    const int64_t cus = std::max(1, c->prop.multiProcessorCount);
    // Segments per tile.  Many tiles (the 513^3 lattice: 297): about 6.5 rounds of the resident workgroups -- measured, 5 .. 12
    // segments per tile are within 4 %, the finer cuts ahead: with that many workgroups the rounds are not rigid.  Few tiles
    // (257^3: 85, 129^3: 27): the rounds are rigid, so the cut that minimises rounds x (planes per segment + 5 planes of
    // warm-up); segments of at least 16 planes.
    const int64_t resident = per_cu * cus;
    int nseg = c->lattice_segments;
    if (nseg <= 0 && 2 * ntile >= resident) nseg = (int)std::max<int64_t>(1, (13 * resident / 2 + ntile - 1) / ntile);
    if (nseg <= 0) nseg = best_segments(ntile, resident, L.g.nk, L.g.nk / 16, 5.0);
    nseg = std::max(1, std::min(nseg, std::max(1, L.g.nk / 16)));
    a.seglen = (L.g.nk + nseg - 1) / nseg;
    nseg = (L.g.nk + a.seglen - 1) / a.seglen;
    const int64_t items = ntile * nseg;
    a.xcd_chunk = 16;
    unsigned grid = 0;
    MG_TRY(tile_grid(items, a.xcd_chunk, &grid));
    a.nitems = (unsigned)items;
    void (*kern)(LatArgs) = nullptr;
    with_march_mode(mode, [&](auto m) { kern = lat_march<decltype(m)::value, TI, TJ, NT>; });
    if (lds > (size_t)150 * 1024) return fail("lattice march: class tables too wide");
    MG_TRY(allow_large_lds(c, reinterpret_cast<const void*>(kern), (size_t)150 * 1024));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), lds, c->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_lat_march(mg_context* c, const Level& L, int mode, const double* x_rows, const double* f_rows, double* out_rows,
                     int color, double alpha, double beta) {
    LatArgs a{};
    a.x = x_rows; a.f = f_rows; a.out = out_rows;
    a.xp = out_rows; a.beta = beta;
    a.cls = L.scls; a.s_pack = L.s_pack; a.s_val = L.s_val; a.s_cnt = L.s_cnt;
    a.W = L.W; a.WP = (L.W + 3) / 4 * 4 + 4; a.ntop = L.lm_ntop;
    for (int t = 0; t < LM_K; ++t) a.top[t] = L.lm_top[t];
    a.nloc = L.nloc; a.P = L.g.plane;
    a.xlo = -(L.halo_lo ? (int64_t)c->halo_planes * L.g.plane : 0); a.xhi = L.nloc + (L.halo_hi ? (int64_t)c->halo_planes * L.g.plane : 0);
    a.nx = L.g.nx; a.ny = L.g.ny; a.nz = L.g.nk; a.kg0 = (int)(L.row0 / L.g.plane);
    a.color = color; a.omega = mode == MODE_CHEB ? alpha : c->omega;
    // ("lattice_tile" 2: the wide tile moves 23 % fewer bytes but its one 512-thread workgroup per CU is slower than two of
    //  256 -- 8.0 against 6.9 ms per Gauss-Seidel sweep of the 513^3 lattice: kept for experiments)
    if (c->lattice_tile == 2 && L.g.nx >= 128) return launch_lat_march_t<128, 16, 512>(c, L, a, mode);
    return launch_lat_march_t<64, 16, 256>(c, L, a, mode);
}

// Tiles, plane segments and grid of the matrix-free diffusion march on a level.  Four workgroups fit a CU (35 KB of LDS
// each), so the launch runs in rounds of 4 x CUs items; a segment re-reads three planes to warm up.  The number of segments
// (of at least sixteen planes) is the one with the best product of the last round's filling and the planes a segment keeps.
struct MfPlan { int ntx, nty, nseg, seglen; unsigned nitems, ch, grid; };
MfPlan mf_plan_dims(const mg_context* c, int nx, int ny, int nz) {
    MfPlan p{};
    p.ntx = (nx + MF_TX - 1) / MF_TX;
    p.nty = (ny + MF_TY - 1) / MF_TY;
    const int64_t ntile = (int64_t)p.ntx * p.nty;
    const int64_t slots = 4 * (int64_t)std::max(1, c->prop.multiProcessorCount);
    int nseg = 1;
    double best = 0.0;
    for (int n = 1; n <= std::max(1, nz / 16); ++n) {
        const int len = (nz + n - 1) / n;
        const int64_t items = ntile * ((nz + len - 1) / len);
        const double score = (double)items / (double)((items + slots - 1) / slots * slots) * (double)len / (double)(len + 3);
        if (score > best) { best = score; nseg = n; }
    }
    p.seglen = (nz + nseg - 1) / nseg;
    p.nseg = (nz + p.seglen - 1) / p.seglen;
    p.nitems = (unsigned)(ntile * p.nseg);
    p.ch = p.nitems >= 8u * 16u * 4u ? 16u : 1u;
    p.grid = (p.nitems + 8u * p.ch - 1) / (8u * p.ch) * (8u * p.ch);
    return p;
}
MfPlan mf_plan(const mg_context* c, const Level& L) { return mf_plan_dims(c, L.g.nx, L.g.ny, L.g.nz); }

// A face set other than all six faces lives on whole 3-D handles only.  mg_set_diffusion_faces refuses the others; a handle
// that became a slab handle after the set was set is refused where the set is read: by the generators, the P1-transpose
// restriction and the sensitivity entries.
int face_set_handle(const mg_context* c, const std::string& who) {
    if (c->diffusion_faces == MG_FACES_ALL) return 0;
    if (c->dim != 3) return fail(who + ": the face set " + std::to_string(c->diffusion_faces) + " (mg_set_diffusion_faces) is 3-D only");
    if (c->comm.active())
        return fail(who + ": the face set " + std::to_string(c->diffusion_faces) + " (mg_set_diffusion_faces) needs a whole (not slab) handle");
    return 0;
}

// the free nodes of a face set on a whole 3-D level
FreeBox level_box(const Level& L, int faces) { return free_box(faces, L.g.nx, L.g.ny, L.g.nz); }

// The reaction field (mg_set_diffusion_reaction) lives on whole 3-D handles only, like a face set: a handle that became a
// slab handle after the field was set is refused where the field is read, by the generators.  So is a level of another size.
int reaction_handle(const mg_context* c, const std::string& who, int N) {
    if (!c->sigma) return 0;
    if (c->dim != 3) return fail(who + ": the reaction term (mg_set_diffusion_reaction) is 3-D only");
    if (c->comm.active()) return fail(who + ": the reaction term (mg_set_diffusion_reaction) needs a whole (not slab) handle");
    if (N != c->sigma_N)
        return fail(who + ": elements_per_dim = " + std::to_string(N) + ", the reaction field (mg_set_diffusion_reaction) has " +
                    std::to_string(c->sigma_N) + " cells per dimension: set a field of the level's size, or clear it");
    return 0;
}

// nodal R(w) of a cell field on a whole 3-D grid of N cells per dimension (reaction_diag, mg_kernels.hip.h); out: (N + 1)^3
int launch_reaction_diag(mg_context* c, const double* w, double* out, int N) {
    const double h = 1.0 / (double)N;
    const dim3 grid(blocks_for(((int64_t)N + 1) * (N + 1), RD_BLOCK), (unsigned)(N + 1), 1u);
    hipLaunchKernelGGL(reaction_diag, grid, dim3(RD_BLOCK), 0, c->stream, w, out, N, std::pow(h, 3.0));
    HIP_TRY(hipGetLastError());
    return 0;
}

// The Robin fields (mg_set_diffusion_robin) are read where the reaction field is, under the same conditions; a field on a
// face of the Dirichlet set has no free node to act on and is refused where levels are generated.
int robin_faces(const mg_context* c) {
    int faces = 0;
    for (int f = 0; f < 6; ++f)
        if (c->alpha[f]) faces |= 1 << f;
    return faces;
}

int robin_handle(const mg_context* c, const std::string& who, int N) {
    const int faces = robin_faces(c);
    if (!faces) return 0;
    if (c->dim != 3) return fail(who + ": Robin faces (mg_set_diffusion_robin) are 3-D only");
    if (c->comm.active()) return fail(who + ": Robin faces (mg_set_diffusion_robin) need a whole (not slab) handle");
    if (faces & c->diffusion_faces)
        return fail(who + ": the handle holds Robin fields on the faces " + std::to_string(faces) + " (mg_set_diffusion_robin) and its Dirichlet "
                    "face set is " + std::to_string(c->diffusion_faces) + " (mg_set_diffusion_faces): face " +
                    std::to_string(faces & c->diffusion_faces & -(faces & c->diffusion_faces)) + " cannot be both");
    if (N != c->alpha_N)
        return fail(who + ": elements_per_dim = " + std::to_string(N) + ", the Robin fields (mg_set_diffusion_robin) have " +
                    std::to_string(c->alpha_N) + " face-cells per dimension: set fields of the level's size, or clear them");
    return 0;
}

// The Robin fields of one level on their way down a hierarchy: the handle's on the top level (borrowed), below it the
// arithmetic mean of the 2 x 2 children whatever the kappa averaging (boundary mass is additive), held here.
struct RobinWalk {
    RobinFaces rf{};
    int faces = 0;
    DevTemp held[6], coarse[6];
    explicit RobinWalk(const mg_context* c) : faces(robin_faces(c)) {
        for (int f = 0; f < 6; ++f) rf.f[f] = c->alpha[f];
    }
    // the fields of the level below (Nc face-cells per dimension) into `coarse`, on the handle's stream
    int coarsen(mg_context* c, int Nc) {
        for (int f = 0; f < 6; ++f) {
            if (!rf.f[f]) continue;
            const int64_t nc = (int64_t)Nc * Nc;
            MG_TRY(coarse[f].alloc((size_t)nc * 8));
            const unsigned nb = (unsigned)std::max<int64_t>(1, std::min<int64_t>(2048, (nc + KI_BLOCK - 1) / KI_BLOCK));
            hipLaunchKernelGGL(kappa_ingest<2>, dim3(nb), dim3(KI_BLOCK), 0, c->stream, rf.f[f], (double*)nullptr, coarse[f].as<double>(), Nc, 0, 0);
            HIP_TRY(hipGetLastError());
        }
        return 0;
    }
    // one level down (the stream is synchronised: the fields of the level above go)
    void descend() {
        for (int f = 0; f < 6; ++f) {
            if (!rf.f[f]) continue;
            held[f] = std::move(coarse[f]);
            rf.f[f] = held[f].as<const double>();
        }
    }
};

// nodal B(alpha) of the level's Robin fields on a whole 3-D grid of N cells per dimension (robin_diag, mg_kernels.hip.h),
// +0.0 on the Dirichlet nodes of the face set; add: out holds R(sigma) and becomes R(sigma) + B(alpha)
int launch_robin_diag(mg_context* c, const RobinFaces& rf, int dirichlet_faces, double* out, int N, bool add) {
    const double h = 1.0 / (double)N;
    const dim3 grid(blocks_for(((int64_t)N + 1) * (N + 1), RD_BLOCK), (unsigned)(N + 1), 1u);
    hipLaunchKernelGGL(robin_diag, grid, dim3(RD_BLOCK), 0, c->stream, rf, free_box(dirichlet_faces, N + 1, N + 1, N + 1), out, N,
                       std::pow(h, 2.0), add ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the one nodal term d of a free row's diagonal: R(sigma), B(alpha), or R(sigma) + B(alpha) formed as that sum
int launch_nodal_diag(mg_context* c, const double* d_sigma, const RobinWalk& rw, double* out, int N) {
    if (d_sigma) MG_TRY(launch_reaction_diag(c, d_sigma, out, N));
    if (rw.faces) MG_TRY(launch_robin_diag(c, rw.rf, c->diffusion_faces, out, N, d_sigma != nullptr));
    return 0;
}

// T_alpha,F(w, x) = b_F(w) x on the free nodes of face F, +0.0 elsewhere / its adjoint D_alpha,F(a, b) per face-cell
// (mg_diffusion_adj.hip.h); whole 3-D grid levels, the caller's lexicographic buffers; fi: the face's bit number
DrArgs dr_args(const mg_context* c, const Level& L, int fi, const double* a, const double* b, double* out) {
    DrArgs d{};
    d.a = a; d.b = b; d.out = out;
    d.nx = L.g.nx; d.nz = L.g.nz; d.N = L.N; d.P = L.g.plane;
    d.axis = fi >> 1;
    d.at = (fi & 1) ? L.N : 0;
    d.box = level_box(L, c->diffusion_faces);
    return d;
}

int launch_apply_drobin(mg_context* c, const Level& L, int fi, const double* dalpha, const double* x, double* out) {
    DrArgs d = dr_args(c, L, fi, dalpha, x, out);
    d.scale = std::pow(1.0 / (double)L.N, 2.0);
    hipLaunchKernelGGL(diffusion_apply_drobin, dim3(blocks_for(L.g.plane, DK_BLOCK), (unsigned)L.g.nz, 1u), dim3(DK_BLOCK), 0, c->stream, d);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_drobin(mg_context* c, const Level& L, int fi, const double* a, const double* b, double* out) {
    DrArgs d = dr_args(c, L, fi, a, b, out);
    d.scale = std::pow(1.0 / (double)L.N, 2.0) / 6.0;
    hipLaunchKernelGGL(diffusion_drobin, dim3(blocks_for((int64_t)L.N * L.N, DK_BLOCK)), dim3(DK_BLOCK), 0, c->stream, d);
    HIP_TRY(hipGetLastError());
    return 0;
}

// T_sigma(w, x) = R(w) x on the free nodes of the handle's face set, +0.0 elsewhere / its adjoint D_sigma(a, b) per cell
// (mg_diffusion_adj.hip.h); whole 3-D grid levels, the caller's lexicographic buffers
DsArgs ds_args(const mg_context* c, const Level& L, const double* a, const double* b, double* out) {
    DsArgs d{};
    d.a = a; d.b = b; d.out = out;
    d.nx = L.g.nx; d.ny = L.g.ny; d.nz = L.g.nz; d.N = L.N; d.P = L.g.plane;
    d.box = level_box(L, c->diffusion_faces);
    return d;
}

int launch_apply_dsigma(mg_context* c, const Level& L, const double* dsigma, const double* x, double* out) {
    DsArgs d = ds_args(c, L, dsigma, x, out);
    d.scale = std::pow(1.0 / (double)L.N, 3.0);
    hipLaunchKernelGGL(diffusion_apply_dsigma, dim3(blocks_for(L.g.plane, DK_BLOCK), (unsigned)L.g.nz, 1u), dim3(DK_BLOCK), 0, c->stream, d);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_dsigma(mg_context* c, const Level& L, const double* a, const double* b, double* out) {
    DsArgs d = ds_args(c, L, a, b, out);
    d.scale = std::pow(1.0 / (double)L.N, 3.0) / 24.0;
    hipLaunchKernelGGL(diffusion_dsigma, dim3(blocks_for((int64_t)L.N * L.N, DK_BLOCK), (unsigned)L.N, 1u), dim3(DK_BLOCK), 0, c->stream, d);
    HIP_TRY(hipGetLastError());
    return 0;
}

MfArgs mf_args(const MfPlan& p, const Level& L, const double* kappa, const double* x_rows, double* out_rows) {
    MfArgs a{};
    a.x = x_rows; a.xp = out_rows; a.out = out_rows; a.kappa = kappa;
    a.nx = L.g.nx; a.ny = L.g.ny; a.nz = L.g.nz; a.N = L.N; a.P = L.g.plane;
    a.ntx = p.ntx; a.nty = p.nty; a.nseg = p.nseg; a.seglen = p.seglen; a.nitems = p.nitems; a.ch = p.ch;
    a.h = 1.0 / (double)L.N;
    return a;
}

int launch_diffusion_mf(mg_context* c, const Level& L, int mode, bool dot, const double* x_rows, const double* f_rows,
                        double* out_rows, double* partials, unsigned* grid_out, double alpha, double beta) {
    const MfPlan p = mf_plan(c, L);
    MfArgs a = mf_args(p, L, L.kappa, x_rows, out_rows);
    a.f = f_rows; a.partials = partials;
    a.omega = mode == MODE_CHEB ? alpha : c->omega;
    a.beta = beta;
    if (grid_out) *grid_out = p.grid;
    const dim3 grid(p.grid), blk(MF_NT);
    bool known = true;
    const MfFaceArgs fa{a, level_box(L, L.faces)};      // (levels generated with a face set: the march with the box of its free nodes)
    with_mode(mode, dot, [&](auto m, auto d) {
        constexpr int MODE = decltype(m)::value;
        if constexpr (MODE == MODE_GS) known = false;
        else if (L.rdiag) {                         // A(kappa) + R(sigma) and / or B(alpha): the march with the level's nodal diagonal term
            const MfReactArgs ra{a, fa.box, L.rdiag};
            if (L.faces != MG_FACES_ALL) hipLaunchKernelGGL((diffusion_mf_react<MODE, decltype(d)::value, true>), grid, blk, 0, c->stream, ra);
            else hipLaunchKernelGGL((diffusion_mf_react<MODE, decltype(d)::value, false>), grid, blk, 0, c->stream, ra);
        } else if (L.faces != MG_FACES_ALL) hipLaunchKernelGGL((diffusion_mf_faces<MODE, decltype(d)::value>), grid, blk, 0, c->stream, fa);
        else hipLaunchKernelGGL((diffusion_mf<MODE, decltype(d)::value>), grid, blk, 0, c->stream, a);
    });
    if (!known) return fail("matrix-free diffusion levels have no kernel for this mode");
    HIP_TRY(hipGetLastError());
    return 0;
}

// The same march over nv = 2 .. MF_BATCH_MAX vectors in one launch (mg_diffusion_mf_batch.hip.h): the level's plan, the row
// rebuilt once per node.  Jacobi, residual and SpMV (with or without the partial sums, one array of the plan's grid per vector).
int launch_diffusion_mf_batch(mg_context* c, const Level& L, int mode, bool dot, int nv, const double* const* x_rows,
                              const double* const* f_rows, double* const* out_rows, double* const* partials) {
    if (mode != MODE_JACOBI && mode != MODE_RESIDUAL && mode != MODE_SPMV)
        return fail("the batched matrix-free march runs Jacobi, residual and SpMV launches only");
    const MfPlan p = mf_plan(c, L);
    const dim3 grid(p.grid), blk(MF_NT);
    const bool known = with_int<2, 3, 4>(nv, [&](auto n) {
        constexpr int NV = decltype(n)::value;
        MfBatchArgs<NV> ba{};
        ba.a = mf_args(p, L, L.kappa, nullptr, nullptr);
        ba.a.omega = c->omega;
        ba.box = level_box(L, L.faces);
        ba.r = L.rdiag;
        for (int v = 0; v < NV; ++v) {
            ba.x[v] = x_rows[v]; ba.f[v] = f_rows ? f_rows[v] : nullptr; ba.out[v] = out_rows[v];
            ba.partials[v] = partials ? partials[v] : nullptr;
        }
        with_mode(mode, dot, [&](auto m, auto d) {
            constexpr int MODE = decltype(m)::value;
            constexpr bool DOT = decltype(d)::value;
            if constexpr (MODE == MODE_JACOBI || MODE == MODE_RESIDUAL || MODE == MODE_SPMV)
                with_bool(L.faces != MG_FACES_ALL, [&](auto fc) {
                    with_bool(L.rdiag.get() != nullptr, [&](auto re) {
                        hipLaunchKernelGGL((diffusion_mf_batch<NV, MODE, DOT, decltype(fc)::value, decltype(re)::value>), grid, blk, 0,
                                           c->stream, ba);
                    });
                });
        });
    });
    if (!known) return fail("the batched matrix-free march takes 2.." + std::to_string(MF_BATCH_MAX) + " vectors per launch");
    HIP_TRY(hipGetLastError());
    return 0;
}

// out = M_rows A^(dkappa) M_cols x on a whole 3-D grid level: the SpMV march with kappa := dkappa (diffusion_mf<MODE_SPMV, false,
// true, rows_all, cols_all>); (interior, interior) is (dA/dkappa . dkappa) x with +0.0 on boundary rows.  Reads the grid only;
// dkappa, x, out: the caller's, lexicographic, out != x.  "Interior" is the set of the free nodes of the handle's face set.
int launch_apply_dkappa(mg_context* c, const Level& L, const double* dkappa, const double* x, double* out, bool rows_all = false,
                        bool cols_all = false) {
    const MfPlan p = mf_plan(c, L);
    const MfArgs a = mf_args(p, L, dkappa, x, out);
    const dim3 grid(p.grid), blk(MF_NT);
    if (c->diffusion_faces != MG_FACES_ALL) {
        const MfFaceArgs fa{a, level_box(L, c->diffusion_faces)};
        if (rows_all && cols_all) hipLaunchKernelGGL((diffusion_mf_faces<MODE_SPMV, false, true, true, true>), grid, blk, 0, c->stream, fa);
        else if (rows_all) hipLaunchKernelGGL((diffusion_mf_faces<MODE_SPMV, false, true, true, false>), grid, blk, 0, c->stream, fa);
        else if (cols_all) hipLaunchKernelGGL((diffusion_mf_faces<MODE_SPMV, false, true, false, true>), grid, blk, 0, c->stream, fa);
        else hipLaunchKernelGGL((diffusion_mf_faces<MODE_SPMV, false, true>), grid, blk, 0, c->stream, fa);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (rows_all && cols_all) hipLaunchKernelGGL((diffusion_mf<MODE_SPMV, false, true, true, true>), grid, blk, 0, c->stream, a);
    else if (rows_all) hipLaunchKernelGGL((diffusion_mf<MODE_SPMV, false, true, true, false>), grid, blk, 0, c->stream, a);
    else if (cols_all) hipLaunchKernelGGL((diffusion_mf<MODE_SPMV, false, true, false, true>), grid, blk, 0, c->stream, a);
    else hipLaunchKernelGGL((diffusion_mf<MODE_SPMV, false, true>), grid, blk, 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// f (and / or 1 / diagonal) of the level gen_diffusion would store from a whole device kappa, without the matrix
int launch_diffusion_rhs(mg_context* c, const Level& L, const double* d_kappa, double* f_rows, double* dinv_rows) {
    DiffusionArgs d{};
    GenArgs& a = d.ga;
    a.g = L.g; a.N = L.N; a.dim = 3; a.prune = 1;
    a.h = 1.0 / (double)L.N;
    a.fh = -12.0 * std::pow(a.h, 3.0);
    d.kappa = d_kappa;
    d.kc0 = 0;
    d.box = level_box(L, L.faces);
    d.react = L.rdiag;                          // (a matrix-free level keeps it iff it has a reaction term or Robin fields)
    hipLaunchKernelGGL(gen_diffusion_rhs, grid3(L.g, L.g.nk), dim3(kPlaneBlock), 0, c->stream, d, f_rows, dinv_rows);
    HIP_TRY(hipGetLastError());
    return 0;
}

// out[cell] = d(a^T A(kappa) b) / d kappa_cell on a whole 3-D grid level (mg_diffusion_adj.hip.h); a, b: lexicographic nodes,
// their boundary entries taken as 0 unless a_all / b_all
int launch_dkappa(mg_context* c, const Level& L, const double* a, const double* b, double* out, bool gather, bool a_all = false,
                  bool b_all = false) {
    DkMarchArgs m{};
    DkArgs& d = m.d;
    d.a = a; d.b = b; d.out = out;
    d.a_all = a_all; d.b_all = b_all;
    d.nx = L.g.nx; d.ny = L.g.ny; d.nz = L.g.nz; d.N = L.N; d.P = L.g.plane;
    d.scale = (1.0 / (double)L.N) / 6.0;
    d.box = level_box(L, c->diffusion_faces);
    if (gather) {
        const dim3 grid(blocks_for((int64_t)L.N * L.N, DK_BLOCK), (unsigned)L.N, 1u);
        hipLaunchKernelGGL(diffusion_dkappa_gather, grid, dim3(DK_BLOCK), 0, c->stream, d);
    } else {
        const MfPlan p = mf_plan_dims(c, L.N, L.N, L.N);    // tiles of cells, segments of cell planes
        m.ntx = p.ntx; m.nty = p.nty; m.nseg = p.nseg; m.seglen = p.seglen; m.nitems = p.nitems; m.ch = p.ch;
        hipLaunchKernelGGL(diffusion_dkappa_march, dim3(p.grid), dim3(MF_NT), 0, c->stream, m);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// mg_diffusion_dkappa and the device-pointer vector calls: whole 3-D grid levels / whole handles, refused by name otherwise
int need_dkappa_level(mg_context* c, int level, const char* who, const char* field = "kappa") {
    if (!c) return fail("null handle");
    if (c->dim != 3) return fail(std::string(who) + ": the " + field + " sensitivity is 3-D only (this handle is 2-D)");
    if (c->comm.active()) return fail(std::string(who) + " needs a whole (not slab) handle");
    MG_TRY(check_level(c, level));
    if (c->L[level].flat) return fail(std::string(who) + ": level " + std::to_string(level) + " is flat (no grid): it has no cells");
    return 0;
}

// `p` must be device memory of the handle's device (hipPointerGetAttributes); nothing is launched otherwise
int need_device_pointer(mg_context* c, const void* p, const char* who, const char* what) {
    if (!p) return fail(std::string(who) + ": null pointer (" + what + ")");
    hipPointerAttribute_t at{};
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) (void)hipGetLastError();       // (an unregistered host pointer is an error of the query in some runtimes)
    if (e != hipSuccess || at.type != hipMemoryTypeDevice)
        return fail(std::string(who) + ": " + what + " is not device memory (a host pointer?)");
    if (at.device != c->device)
        return fail(std::string(who) + ": " + what + " lives on device " + std::to_string(at.device) + ", the handle on device " +
                    std::to_string(c->device));
    return 0;
}

// The cell gradient family on a whole 3-D grid level (mg_diffusion_flux.hip.h): F(w, x) -> 3 N^3 and C(p, x) -> N^3, one thread per
// cell; F^T(w, p) -> nodes, one thread per node.  The caller's lexicographic buffers.
CgArgs cg_args(const Level& L, const double* w, const double* p, const double* x, double* out) {
    CgArgs a{};
    a.w = w; a.p = p; a.x = x; a.out = out;
    a.nx = L.g.nx; a.ny = L.g.ny; a.nz = L.g.nz; a.N = L.N; a.P = L.g.plane;
    a.C3 = (int64_t)L.N * L.N * L.N;
    a.s = (double)L.N / 6.0;
    return a;
}

template <int KIND>
int launch_cell_grad(mg_context* c, const Level& L, const double* w, const double* p, const double* x, double* out) {
    const CgArgs a = cg_args(L, w, p, x, out);
    const dim3 grid(blocks_for((int64_t)L.N * L.N, DK_BLOCK), (unsigned)L.N, 1u);
    hipLaunchKernelGGL((cell_grad_cells<KIND>), grid, dim3(DK_BLOCK), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_cell_grad_t(mg_context* c, const Level& L, const double* w, const double* p, double* out) {
    const CgArgs a = cg_args(L, w, p, nullptr, out);
    hipLaunchKernelGGL(cell_grad_t, dim3(blocks_for(L.g.plane, DK_BLOCK), (unsigned)L.g.nz, 1u), dim3(DK_BLOCK), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// out = op(A, x) over the requested slices of the level (EllRequest)
int launch_ell(mg_context* c, const Level& L, const EllRequest& q) {
    const int mode = q.mode;
    const bool dot = q.dot;
    const int64_t slice0 = q.slices.slice0, gap = q.slices.gap;
    const int64_t slice_count = q.slices.count < 0 ? L.nslices - slice0 : q.slices.count;
    if (slice_count == 0) return 0;
    const bool whole = slice0 == 0 && slice_count == L.nslices;
    if (L.mf) {
        // matrix-free diffusion level: the rows rebuilt from kappa (mg_diffusion_mf.hip.h); whole levels only
        if (q.done || !whole || gap != 0 || mode == MODE_GS)
            return fail("matrix-free diffusion levels run whole-level Jacobi, residual, SpMV and Chebyshev launches only");
        return launch_diffusion_mf(c, L, mode, dot, q.x_base + L.g.lead, q.f_rows, q.out_rows, q.partials, q.grid_out, q.alpha, q.beta);
    }
    // whole large 3-D levels with row classes: one sweep as a plane march (mg_jacobi2.hip.h, sdia_sweep1c)
    if (!dot && !q.done && mode != MODE_SPMV && whole && sweep1c_ok(c, L))
        return launch_sweep1c(c, L, mode, q.x_base + L.g.lead, q.f_rows, q.out_rows, q.color, q.alpha, q.beta);
    EllArgs a{};
    a.vals = L.vals; a.cols = L.cols; a.x = q.x_base; a.f = q.f_rows; a.dinv = L.dinv; a.out = q.out_rows;
    a.partials = q.partials; a.done_flag = q.done; a.nloc = L.nloc; a.lead = L.g.lead;
    a.slice0 = slice0; a.nslices = slice_count; a.split = q.slices.split; a.gap = gap; a.omega = c->omega; a.W = L.W; a.chunk = c->chunk;
    if (mode == MODE_CHEB) { a.omega = q.alpha; a.xp = q.out_rows; a.beta = q.beta; }
    a.codes = L.codes; a.offsets = L.offsets; a.ntable = L.ntable; a.dcode = L.dcode;
    a.color = q.color; a.color_kind = c->smoother == MG_SMOOTH_MCGS ? COLOR_LATTICE9 : COLOR_PARITY;
    a.grow0 = L.row0; a.gnx = L.g.nx; a.gny = L.g.ny;
    unsigned grid = blocks_for(slice_count, WAVES_PER_BLOCK);
    // XCD strip traversal (optional): pays when a plane is much larger than a strip
    auto plan_strips = [&]() {
        const int64_t ps4 = (L.g.plane / (WAVE * L.R)) / 4;            // blocks per pseudo-plane
        const int64_t want = c->strip_slices / 4;                       // blocks per strip asked for
        // (sub-ranges of a slab -- interior slices while the halo travels -- are strip-walked too: the
        // pseudo-planes then start at slice0, which shifts them against the real planes by a constant)
        const int64_t nblocks = (slice_count + 3) / 4;
        if (!(want > 0 && !dot && L.g.nz > 1 && ps4 >= 16 * want && nblocks >= 4 * ps4)) return;
        const int64_t m = std::max<int64_t>(1, (ps4 + 4 * want) / (8 * want));     // round(ps4 / want / 8)
        const int64_t ns = 8 * m;
        const int64_t kp = (nblocks + ps4 - 1) / ps4;
        const int64_t bmax = (ps4 + ns - 1) / ns;
        const int64_t g = ns * kp * bmax;
        if (g < ((int64_t)1 << 31) && kp < ((int64_t)1 << 31)) {
            a.strip_ns = (unsigned)ns; a.strip_bmax = (unsigned)bmax; a.ps4 = (unsigned)ps4; a.kp = (unsigned)kp;
            grid = (unsigned)g;
        }
    };
    // Every tile kernel has the rows per lane, the mode and the dot product as template arguments, most of them the
    // streaming loads as well: launch(R, MODE, DOT, NT) is called with the level's and the request's.
    auto tiles = [&](auto&& launch) -> int {
        if (q.grid_out) *q.grid_out = grid;
        const bool known = with_int<1, 2, 4>(L.R, [&](auto r) {
            with_mode(mode, dot, [&](auto m, auto d) { with_bool(c->nontemporal != 0, [&](auto nt) { launch(r, m, d, nt); }); });
        });
        if (!known) return fail("unsupported rows_per_lane");
        HIP_TRY(hipGetLastError());
        return 0;
    };
    const dim3 blk(BLOCK);
    if (L.sdia) {
        a.vals = L.dvals; a.mlead = L.mlead;
        for (int t = 0; t < 8; ++t) a.up[t] = L.up[t];
        plan_strips();
        const bool finest = is_finest(c, L);
        if (cls_full(L) && c->class_sweeps) {
            // the rows through their classes: 25 instead of 56 bytes per row (mg_kernels.hip.h, sdia_cls_body);
            // persistent blocks (8 per CU, a multiple of 8 so that a block's groups stay on one XCD's share)
            fill_classes(a, L);
            a.nvirt = grid;
            // (with the dot product one group per block, as the other formats have it: the partial sums and with them
            //  the rounding of the result do not depend on the format)
            const unsigned resident = (unsigned)c->cls_blocks_per_cu * (unsigned)std::max(1, c->prop.multiProcessorCount);
            if (!dot) grid = std::min(grid, resident);
            return tiles([&](auto r, auto m, auto d, auto nt) {
                constexpr int R = decltype(r)::value, MODE = decltype(m)::value;
                constexpr bool DOT = decltype(d)::value, NT = decltype(nt)::value;
                with_int_else<4, 3>(L.wu, [&](auto wu) {
                    constexpr int WU = decltype(wu)::value;
                    if (MODE == MODE_JACOBI && finest) hipLaunchKernelGGL((sdia_cls_jacobi_finest<WU, R, NT>), dim3(grid), blk, 0, c->stream, a);
                    else hipLaunchKernelGGL((sdia_cls_apply<WU, R, MODE, DOT, NT>), dim3(grid), blk, 0, c->stream, a);
                });
            });
        }
        const unsigned lds = a.nslices >= 100000 ? (unsigned)c->lds_pad : 0u;      // ("lds_pad", see mg_context)
        // (a pad above the default is an experiment: like every launch that may ask for more than 64 KiB of dynamic LDS,
        //  the kernel gets the attribute first, once, for the largest pad mg_set_tuning accepts)
        int rc = 0;
        const int launched = tiles([&](auto r, auto m, auto d, auto nt) {
            constexpr int R = decltype(r)::value, MODE = decltype(m)::value;
            constexpr bool DOT = decltype(d)::value, NT = decltype(nt)::value;
            with_int_else<8, 3, 4>(L.wu, [&](auto wu) {
                constexpr int WU = decltype(wu)::value;
                void (*const kern[2])(EllArgs) = {sdia_apply<WU, R, MODE, DOT, NT>, sdia_jacobi_finest<WU, R, NT>};
                const int which = MODE == MODE_JACOBI && finest ? 1 : 0;
                if (lds > 48u * 1024u) rc =allow_large_lds(c, reinterpret_cast<const void*>(kern[which]), (size_t)mg_context::kLdsPadMax);
                if (rc == 0) hipLaunchKernelGGL(kern[which], dim3(grid), blk, lds, c->stream, a);
            });
        });
        return rc ? rc : launched;
    }
    if (L.coded && L.scls && c->class_sweeps) {
        // whole 3-D lattice levels: plane march with x in LDS (mg_lattice.hip.h)
        if (!dot && !q.done && mode != MODE_SPMV && whole && gap == 0 && lat_march_ok(c, L))
            return launch_lat_march(c, L, mode, q.x_base + L.g.lead, q.f_rows, q.out_rows, q.color, q.alpha, q.beta);
        // wide rows through their stencil classes: 25 bytes per row instead of the stored row (ell_cls_apply)
        return tiles([&](auto r, auto m, auto d, auto nt) {
            hipLaunchKernelGGL((ell_cls_apply<decltype(r)::value, decltype(m)::value, decltype(d)::value, decltype(nt)::value>), dim3(grid), blk, 0,
                               c->stream, a, L.scls, L.s_off, L.s_val, L.s_cnt);
        });
    }
    // (W not in {5, 7, 15}: the kernels that loop over the width)
    if (L.coded) {
        plan_strips();
        return tiles([&](auto r, auto m, auto d, auto nt) {
            with_int_else<0, 5, 7, 15>(L.W, [&](auto w) {
                hipLaunchKernelGGL((ell_apply_coded<decltype(w)::value, decltype(r)::value, decltype(m)::value, decltype(d)::value, decltype(nt)::value>),
                                   dim3(grid), blk, 0, c->stream, a);
            });
        });
    }
    return tiles([&](auto r, auto m, auto d, auto) {
        with_int_else<0, 5, 7, 15>(L.W, [&](auto w) {
            hipLaunchKernelGGL((ell_apply<decltype(w)::value, decltype(r)::value, decltype(m)::value, decltype(d)::value>), dim3(grid), blk, 0,
                               c->stream, a);
        });
    });
}
// ---- communication -----------------------------------------------------------------------------
int ensure_host_stage(mg_context* c, size_t elems) {
    Comm& cm = c->comm;
    if (cm.h_stage_elems >= elems) return 0;
    if (cm.h_stage) (void)hipHostFree(cm.h_stage);
    cm.h_stage = nullptr;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&cm.h_stage), elems * sizeof(double), hipHostMallocDefault));
    cm.h_stage_elems = elems;
    return 0;
}

// `count` doubles to and from each slab neighbour (device buffers; a rank without that neighbour passes nothing)
int exchange_raw(mg_context* c, const double* send_lo, const double* send_hi, double* recv_lo, double* recv_hi, size_t count,
                 hipStream_t stream) {
    Comm& cm = c->comm;
    const bool lo = cm.rank > 0, hi = cm.rank + 1 < cm.world;
    if (cm.nccl) {
        NCCL_TRY(g_rccl.GroupStart());
        if (lo) {
            NCCL_TRY(g_rccl.Send(send_lo, count, ncclDouble, cm.rank - 1, cm.nccl, stream));
            NCCL_TRY(g_rccl.Recv(recv_lo, count, ncclDouble, cm.rank - 1, cm.nccl, stream));
        }
        if (hi) {
            NCCL_TRY(g_rccl.Send(send_hi, count, ncclDouble, cm.rank + 1, cm.nccl, stream));
            NCCL_TRY(g_rccl.Recv(recv_hi, count, ncclDouble, cm.rank + 1, cm.nccl, stream));
        }
        NCCL_TRY(g_rccl.GroupEnd());
        return 0;
    }
    if (!cm.ex) return fail("no transport configured");
    MG_TRY(ensure_host_stage(c, 4 * count));
    double* h = cm.h_stage;
    if (lo) HIP_TRY(hipMemcpyAsync(h, send_lo, count * 8, hipMemcpyDeviceToHost, stream));
    if (hi) HIP_TRY(hipMemcpyAsync(h + count, send_hi, count * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (cm.ex(cm.user, lo ? h : nullptr, hi ? h + count : nullptr, lo ? h + 2 * count : nullptr,
              hi ? h + 3 * count : nullptr, (int64_t)count) != 0)
        return fail("exchange callback failed");
    if (lo) HIP_TRY(hipMemcpyAsync(recv_lo, h + 2 * count, count * 8, hipMemcpyHostToDevice, stream));
    if (hi) HIP_TRY(hipMemcpyAsync(recv_hi, h + 3 * count, count * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}

// Fill the `planes` halo planes of `v` NEXT TO its owned rows from the neighbouring slabs (the first owned planes go down,
// the last ones go up); planes < 0: as many as one application of the level's rows reaches ("halo_planes").
int exchange_halo(mg_context* c, const Level& L, DVector& v, hipStream_t stream = nullptr, int planes = -1) {
    if (!stream) stream = c->stream;
    Comm& cm = c->comm;
    if (L.replicated || !cm.active()) return 0;
    if (planes < 0) planes = c->halo_planes;
    if (planes > L.hd) return fail("the vectors of this level have no room for that many halo planes");
    const size_t count = (size_t)planes * (size_t)L.g.plane;       // elements per message
    return exchange_raw(c, v.rows, v.rows + L.nloc - count, v.rows - count, v.rows + L.nloc, count, stream);
}

// In-place sum of `count` device doubles over all ranks.
int allreduce_sum(mg_context* c, double* dev, int64_t count) {
    Comm& cm = c->comm;
    if (!cm.active()) return 0;
    if (cm.nccl) {
        NCCL_TRY(g_rccl.AllReduce(dev, dev, (size_t)count, ncclDouble, ncclSum, cm.nccl, c->stream));
        return 0;
    }
    if (!cm.ar) return fail("no transport configured");
    MG_TRY(ensure_host_stage(c, (size_t)count));
    HIP_TRY(hipMemcpyAsync(cm.h_stage, dev, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (cm.ar(cm.user, cm.h_stage, count) != 0) return fail("allreduce callback failed");
    HIP_TRY(hipMemcpyAsync(dev, cm.h_stage, (size_t)count * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// `full` holds every plane of a level (global lexicographic order); each rank has written the
// planes [splits[rank], splits[rank+1]) and receives the others.
int allgather_planes(mg_context* c, const std::vector<int>& splits, int64_t plane, double* full) {
    Comm& cm = c->comm;
    if (!cm.active()) return 0;
    if (cm.nccl) {
        NCCL_TRY(g_rccl.GroupStart());
        for (int r = 0; r < cm.world; ++r) {
            double* seg = full + (int64_t)splits[r] * plane;
            const size_t cnt = (size_t)(splits[r + 1] - splits[r]) * (size_t)plane;
            NCCL_TRY(g_rccl.Broadcast(seg, seg, cnt, ncclDouble, r, cm.nccl, c->stream));
        }
        NCCL_TRY(g_rccl.GroupEnd());
        return 0;
    }
    if (!cm.ag) return fail("no transport configured");
    const int64_t total = (int64_t)splits[cm.world] * plane;
    const int64_t mine = (int64_t)(splits[cm.rank + 1] - splits[cm.rank]) * plane;
    MG_TRY(ensure_host_stage(c, (size_t)(total + mine)));
    double* h_send = cm.h_stage + total;
    HIP_TRY(hipMemcpyAsync(h_send, full + (int64_t)splits[cm.rank] * plane, (size_t)mine * 8, hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<int64_t> counts(cm.world);
    for (int r = 0; r < cm.world; ++r) counts[r] = (int64_t)(splits[r + 1] - splits[r]) * plane;
    if (cm.ag(cm.user, h_send, mine, cm.h_stage, counts.data()) != 0) return fail("allgatherv callback failed");
    HIP_TRY(hipMemcpyAsync(full, cm.h_stage, (size_t)total * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- the path ----------------------------------------------------------------------------------------
DVector* pick(Level& L, int which) {
    switch (which) {
        case MG_VEC_V: return &L.v;
        case MG_VEC_F: return &L.f;
        case MG_VEC_R: return &L.v2;
        case MG_VEC_ERR: return &L.err;
        default: return nullptr;
    }
}

// Two sweeps in one pass (mg_jacobi2.hip.h): whole, undistributed 3-D levels whose stored diagonals are exactly
// {0, +1, +nx, +plane}.
// rows of the smallest slab of a level: decisions that every rank must take alike are made on it, not on the rank's
// own row count (uneven splits differ by 2^level planes)
int64_t min_slab_rows(const Level& L) {
    if (L.replicated || L.splits.size() < 2) return L.nloc;
    int nk = INT32_MAX;
    for (size_t r = 0; r + 1 < L.splits.size(); ++r) nk = std::min(nk, L.splits[r + 1] - L.splits[r]);
    return (int64_t)nk * L.g.plane;
}

bool fused_sweeps_ok(const mg_context* c, const Level& L, bool ignore_size = false, int min_side = 32) {
    if (!c->fuse_sweeps || !L.sdia || L.wu != 4 || L.flat) return false;
    if (L.g.nx < min_side || L.g.ny < min_side || min_slab_rows(L) < 8 * L.g.plane) return false;    // zero slack >= 3 slices, slabs >= 8 planes
    if (L.up[1] != 1 || L.up[2] != L.g.nx || (int64_t)L.up[3] != L.g.plane) return false;
    return ignore_size || min_slab_rows(L) >= c->fuse_min_rows;
}

// Kernels that ask for more than 64 KiB of dynamic LDS need the attribute once per function (and device: one
// device per handle); remembered in the handle.
// One launch of the two-colour Gauss-Seidel pass (mg_lattice.hip.h, lat_gs2): colours c1 and c2 (c2 < 0: c1 only) of the
// sweep that takes the level's iterate from `xold` to `xnew`.
int launch_lat_gs2(mg_context* c, const Level& L, int c1, int c2, const double* xold_rows, double* xnew_rows) {
    Gs2Args a{};
    a.xold = xold_rows; a.xnew = xnew_rows; a.f = L.f.rows;
    a.cls = L.scls; a.s_pack = L.s_pack; a.s_val = L.s_val; a.s_cnt = L.s_cnt;
    a.W = L.W; a.WP = (L.W + 3) / 4 * 4 + 4; a.ntop = L.lm_ntop;
    for (int t = 0; t < LM_K; ++t) a.top[t] = L.lm_top[t];
    a.nloc = L.nloc; a.P = L.g.plane; a.nx = L.g.nx; a.ny = L.g.ny; a.nz = L.g.nk;
    a.c1 = c1; a.c2 = c2; a.omega = c->omega;
    a.ntx = (L.g.nx + G2_TI - 1) / G2_TI; a.nty = (L.g.ny + G2_TJ - 1) / G2_TJ;
    const int64_t ntile = (int64_t)a.ntx * a.nty;
    const int64_t resident = 2 * (int64_t)std::max(1, c->prop.multiProcessorCount);
    // (as launch_lat_march_t; a segment pays 5 + 4 planes of warm-up and 3 of trailing second colour)
    int nseg = c->lattice_segments;
    if (nseg <= 0 && 2 * ntile >= resident) nseg = (int)std::max<int64_t>(1, (13 * resident / 2 + ntile - 1) / ntile);
    if (nseg <= 0) nseg = best_segments(ntile, resident, L.g.nk, L.g.nk / 16, 12.0);
    nseg = std::max(1, std::min(nseg, std::max(1, L.g.nk / 16)));
    a.seglen = (L.g.nk + nseg - 1) / nseg;
    nseg = (L.g.nk + a.seglen - 1) / a.seglen;
    const int64_t items = ntile * nseg;
    a.xcd_chunk = 16;
    unsigned grid = 0;
    MG_TRY(tile_grid(items, a.xcd_chunk, &grid));
    a.nitems = (unsigned)items;
    const size_t lds = g2_lds_bytes(L.W);
    if (lds > (size_t)80 * 1024) return fail("lattice march: class tables too wide");
    MG_TRY(allow_large_lds(c, reinterpret_cast<const void*>(lat_gs2), (size_t)80 * 1024));
    hipLaunchKernelGGL(lat_gs2, dim3(grid), dim3(G2_THREADS), lds, c->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int allow_large_lds(mg_context* c, const void* kernel, size_t bytes) {
    if (std::find(c->large_lds_kernels.begin(), c->large_lds_kernels.end(), kernel) != c->large_lds_kernels.end()) return 0;
    HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    c->large_lds_kernels.push_back(kernel);
    return 0;
}

constexpr int kJ2Lines = 16;        // grid lines per tile (8 waves x 2)

// How a level's owned planes are cut into segments (one work item = one tile x one segment).  Segment 0 is
// [0, zb), the last one [nk-zb, nk), the others cut the planes between into pieces of `seglen`.
//   whole levels: equal pieces, their number chosen by a cost model -- rounds of 256 resident workgroups times
//     (planes per piece + ~2.5 plane-times of warm-up) -- which is what measured best on 1025^3 (8 pieces);
//   slabs: zb short (the planes whose once-relaxed values travel to the neighbours, plus one), so that the
//     boundary work that the exchanges wait for is small, the interior cut by the same cost model.
struct J2Plan { int ntx, nty, nseg, zb, seglen, wi; };

// grid lines per tile: 16 for the plain pass; the class-coded pass has shapes with 16 and 32 ("fuse_shape")
int jacobi2_lines(const mg_context* c, const Level& L) {
    const int sh = c->fuse_shape;
    if (!(cls_full(L) && c->fuse_classes)) return (c->fuse_plain == 2 && c->fuse_plain_shape == 0) ? 12 : kJ2Lines;
    return (sh == 1 || sh == 3) ? 24 : kJ2Lines;
}

J2Plan jacobi2_plan(const mg_context* c, const Level& L, bool slab, int64_t boundary_rows) {
    J2Plan p{};
    const int lines = jacobi2_lines(c, L);
    p.ntx = (L.g.nx + J2_EX - 3) / (J2_EX - 2);
    p.nty = (L.g.ny + lines - 3) / (lines - 2);
    if ((cls_full(L) && c->fuse_classes) || c->fuse_plain == 2) {
        // class-coded pass / round-2 plain pass: the x ring is part of the tile (124 cells with a second sweep at most), and all tile
        // columns have the same width, the smallest that covers the grid ("fuse_even" 0: always the widest)
        p.ntx = (L.g.nx + J2_EX - 5) / (J2_EX - 4);
        p.wi = c->fuse_even ? (L.g.nx + p.ntx - 1) / p.ntx : J2_EX - 4;
        if (c->fuse_wi > 0) {                                       // experiments: a given width
            p.wi = std::min(J2_EX - 4, std::max(8, c->fuse_wi));
            p.ntx = (L.g.nx + p.wi - 1) / p.wi;
        }
    }
    const int64_t ntile = (int64_t)p.ntx * p.nty;
    const int nk = L.g.nk;
    const int64_t cus = std::max(1, c->prop.multiProcessorCount);      // one resident workgroup per CU
    auto pieces = [&](int planes, int most) { return best_segments(ntile, cus, planes, most, 2.5); };
    if (slab) {
        // one plane more than the rows the neighbours wait for (3 planes + 1 on a 1025^2 plane)
        const int zb = (int)std::max<int64_t>(4, (boundary_rows + L.g.plane - 1) / L.g.plane + 1);
        if (nk >= 2 * zb + 8) {
            const int inner = nk - 2 * zb;
            int m = c->fuse_segments > 2 ? c->fuse_segments - 2 : pieces(inner, inner / 8);
            m = std::max(1, std::min(m, inner));
            p.zb = zb; p.seglen = (inner + m - 1) / m; p.nseg = 2 + (inner + p.seglen - 1) / p.seglen;
            return p;
        }
        p.zb = nk; p.seglen = nk; p.nseg = 1;      // too thin to split: one segment, exchanges in sequence
        return p;
    }
    int n = c->fuse_segments > 0 ? c->fuse_segments : pieces(nk, nk / 16);
    n = std::max(1, std::min(n, nk));
    if (n <= 2) {
        p.zb = (nk + n - 1) / n; p.seglen = nk; p.nseg = n;
    } else {
        p.zb = std::max(1, nk / n);
        const int inner = nk - 2 * p.zb;
        p.seglen = (inner + n - 3) / (n - 2);
        p.nseg = 2 + (inner + p.seglen - 1) / p.seglen;
    }
    return p;
}

template <int NW, int LPW>
int launch_jacobi2c_t(mg_context* c, const J2Args& a, int nseg, bool finest) {
    const int64_t items = (int64_t)a.ntx * a.nty * nseg;
    J2Args b = a;
    b.xcd_chunk = (unsigned)c->fuse_xcd_chunk;
    unsigned grid = 0;
    MG_TRY(tile_grid(items, b.xcd_chunk, &grid));
    b.nitems = (unsigned)items;
    constexpr size_t lds = j2c_lds_bytes<NW, LPW>();
    void (*const kern[2])(J2Args) = {sdia_jacobi2c<NW, LPW>, sdia_jacobi2c_finest<NW, LPW>};
    MG_TRY(allow_large_lds(c, reinterpret_cast<const void*>(kern[finest ? 1 : 0]), lds));
    hipLaunchKernelGGL(kern[finest ? 1 : 0], dim3(grid), dim3(NW * WAVE), lds, c->stream, b);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int R, int NW, int LPW>
int launch_jacobi2p_t(mg_context* c, const J2Args& a, int nseg, bool finest) {
    const int64_t items = (int64_t)a.ntx * a.nty * nseg;
    J2Args b = a;
    b.xcd_chunk = (unsigned)c->fuse_xcd_chunk;
    unsigned grid = 0;
    MG_TRY(tile_grid(items, b.xcd_chunk, &grid));
    b.nitems = (unsigned)items;
    constexpr size_t lds = j2p_lds_bytes<NW, LPW>();
    void (*const kern[2])(J2Args) = {sdia_jacobi2p<R, NW, LPW>, sdia_jacobi2p_finest<R, NW, LPW>};
    MG_TRY(allow_large_lds(c, reinterpret_cast<const void*>(kern[finest ? 1 : 0]), lds));
    hipLaunchKernelGGL(kern[finest ? 1 : 0], dim3(grid), dim3(NW * WAVE), lds, c->stream, b);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int R, int NW, int LPW>
int launch_jacobi2_t(mg_context* c, const J2Args& a, int nseg, bool finest) {
    static_assert(NW * LPW == kJ2Lines, "tile height");
    const int64_t items = (int64_t)a.ntx * a.nty * nseg;
    if (items >= ((int64_t)1 << 31) - 512) return fail("too many tiles");
    J2Args b = a;
    b.nitems = (unsigned)items;
    const unsigned grid = (unsigned)((items + 255) / 256) * 256u;      // whole groups of 8 XCDs x 32 items
    constexpr size_t lds = j2_lds_bytes<NW, LPW>();
    void (*const kern[4])(J2Args) = {sdia_jacobi2<R, NW, LPW, false>, sdia_jacobi2<R, NW, LPW, true>,
                                     sdia_jacobi2_finest<R, NW, LPW, false>, sdia_jacobi2_finest<R, NW, LPW, true>};
    MG_TRY(allow_large_lds(c, reinterpret_cast<const void*>(kern[(finest ? 2 : 0) + (c->fuse_nontemporal ? 1 : 0)]), lds));
    hipLaunchKernelGGL(kern[(finest ? 2 : 0) + (c->fuse_nontemporal ? 1 : 0)], dim3(grid), dim3(NW * WAVE), lds, c->stream, b);
    HIP_TRY(hipGetLastError());
    return 0;
}

// out = two Jacobi sweeps applied to x, for `count` plane segments seg0, seg0 + stride, ... of `plan`
// (slabs: the second sweep is stored for the rows [st_lo, st_hi) only and the once-relaxed iterate of the rows
// within reach of the others goes to v1_rows, see smooth())
int launch_jacobi2(mg_context* c, const Level& L, const J2Plan& plan, int seg0, int stride, int count, const double* x_rows,
                   const double* f_rows, double* out_rows, int64_t st_lo = 0, int64_t st_hi = INT64_MAX,
                   double* v1_rows = nullptr) {
    if (count <= 0) return 0;
    J2Args a{};
    a.vals = L.dvals; a.x = x_rows; a.f = f_rows; a.out = out_rows;
    a.nloc = L.nloc; a.mlead = L.mlead; a.P = L.g.plane;
    a.nx = L.g.nx; a.ny = L.g.ny; a.nz = L.g.nk; a.omega = c->omega;
    a.zero = L.f.raw;
    a.xlo = -(L.halo_lo ? (int64_t)c->halo_planes * L.g.plane : 0); a.xhi = L.nloc + (L.halo_hi ? (int64_t)c->halo_planes * L.g.plane : 0);
    a.slo = a.xlo;
    a.st_lo = st_lo; a.st_hi = st_hi; a.v1out = v1_rows;
    a.k1_lo = st_lo + L.g.plane + L.g.nx + 2; a.k1_hi = st_hi - L.g.plane - L.g.nx - 2;
    a.ntx = plan.ntx; a.nty = plan.nty; a.nseg = plan.nseg; a.zb = plan.zb; a.seglen = plan.seglen;
    a.seg0 = seg0; a.seg_stride = stride;
    const int n = count;
    // 8 waves x 2 grid lines each (16 waves x 1 line measured slower and does not fit 128 registers)
    const bool finest = is_finest(c, L);
    if (cls_full(L) && c->fuse_classes) {
        fill_classes_lead(a, L);
        a.wi = plan.wi;
        switch (c->fuse_shape) {
            case 0: return launch_jacobi2c_t<8, 2>(c, a, n, finest);       // 16 lines, 512 threads
            case 2: return launch_jacobi2c_t<16, 1>(c, a, n, finest);      // 16 lines, 1024 threads
            case 3: return launch_jacobi2c_t<8, 3>(c, a, n, finest);       // 24 lines, 512 threads
            default: return launch_jacobi2c_t<12, 2>(c, a, n, finest);     // 24 lines, 768 threads (measured best)
        }
    }
    int rc = 0;
    with_int_else<4, 1, 2>(L.R, [&](auto r) {
        constexpr int R = decltype(r)::value;
        if (c->fuse_plain != 2) { rc = launch_jacobi2_t<R, 8, 2>(c, a, n, finest); return; }
        a.wi = plan.wi;                  // round-2 structure of the pass on the stored rows (sdia_jacobi2p)
        if (c->fuse_plain_shape == 0) rc = launch_jacobi2p_t<R, 12, 1>(c, a, n, finest);        // 12 waves x 1 grid line (155 VGPRs, no spills: measured best)
        else if (c->fuse_plain_shape == 2) rc = launch_jacobi2p_t<R, 16, 1>(c, a, n, finest);   // 16 waves x 1 grid line
        else rc = launch_jacobi2p_t<R, 8, 2>(c, a, n, finest);
    });
    return rc;
}

// ---- row classes of the neighbours' planes (slabs, K-sweep march) --------------------------------------------------
__global__ void bytes_to_doubles(const unsigned char* __restrict__ in, double* __restrict__ out, int64_t n) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) out[t] = (double)in[t];
}
__global__ void doubles_to_classes(const double* __restrict__ in, const int* __restrict__ map, unsigned char* __restrict__ out, int64_t n) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
        out[t] = (unsigned char)map[(int)in[t] & 255];
}

// The march relaxes the K - 1 planes of either neighbour next to this slab along with its own (mg_jacobik3d.hip.h), so
// it needs their rows: as class bytes in front of / behind the slab's own in `cls`, in THIS rank's class numbering.
// Every rank builds its dictionary by itself, so the neighbours send their class bytes together with their tables, and
// a class is translated by looking its row up in the own table (bit for bit; an unknown row is appended).  Collective:
// every rank of a distributed level calls it at the same point; if one of them cannot translate (more than 255 classes),
// all of them leave the march alone on this level.
int ensure_class_halos(mg_context* c, Level& L) {
    if (L.cls_halo != 0) return 0;
    L.cls_halo = -1;
    Comm& cm = c->comm;
    const bool lo = cm.rank > 0, hi = cm.rank + 1 < cm.world;
    const size_t n = (size_t)L.hd * (size_t)L.g.plane, nt = 256 * CLS_W + 8;
    DevTemp send_t, recv_t, tsend_t, trecv_t, dmap;
    MG_TRY(send_t.alloc(2 * n * sizeof(double)));
    MG_TRY(recv_t.alloc(2 * n * sizeof(double)));
    MG_TRY(tsend_t.alloc(nt * sizeof(double)));
    MG_TRY(trecv_t.alloc(2 * nt * sizeof(double)));
    MG_TRY(dmap.alloc(2 * 256 * sizeof(int)));
    double *const send = send_t.as<double>(), *const recv = recv_t.as<double>();
    double *const tsend = tsend_t.as<double>(), *const trecv = trecv_t.as<double>();
    const unsigned nb = (unsigned)std::min<size_t>(4096, (n + 255) / 256);
    int ok = cls_full(L) && L.ncls > 0 && L.sdia && L.wu == 4 && L.up[1] == 1 && L.up[2] == L.g.nx && (int64_t)L.up[3] == L.g.plane ? 1 : 0;
    std::vector<double> mine(nt, 0.0), theirs(2 * nt, 0.0);
    if (ok) {
        hipLaunchKernelGGL(bytes_to_doubles, dim3(nb), dim3(256), 0, c->stream, L.cls + L.cls_lead, send, (int64_t)n);
        hipLaunchKernelGGL(bytes_to_doubles, dim3(nb), dim3(256), 0, c->stream, L.cls + L.cls_lead + L.nloc - (int64_t)n, send + n, (int64_t)n);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(mine.data() + 8, L.ctab, 256 * CLS_W * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        mine[0] = (double)L.ncls;
    }
    // (a rank without classes still takes part in the exchanges: ncls = 0 tells the neighbours)
    HIP_TRY(hipMemcpyAsync(tsend, mine.data(), nt * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (!ok) HIP_TRY(hipMemsetAsync(send, 0, 2 * n * sizeof(double), c->stream));
    MG_TRY(exchange_raw(c, send, send + n, recv, recv + n, n, c->stream));
    MG_TRY(exchange_raw(c, tsend, tsend, trecv, trecv + nt, nt, c->stream));
    HIP_TRY(hipMemcpyAsync(theirs.data(), trecv, 2 * nt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<int> map(512, 0);
    int ncls = L.ncls;
    bool grown = false;
    for (int side = 0; side < 2 && ok; ++side) {
        if (!(side == 0 ? lo : hi)) continue;
        const double* t = theirs.data() + (size_t)side * nt;
        const int n_theirs = (int)t[0];
        if (n_theirs <= 0 || n_theirs > 256) { ok = 0; break; }
        for (int j = 0; j < n_theirs && ok; ++j) {
            const double* row = t + 8 + (size_t)j * CLS_W;
            int found = -1;
            for (int i = 0; i < ncls && found < 0; ++i)
                if (std::memcmp(mine.data() + 8 + (size_t)i * CLS_W, row, 7 * sizeof(double)) == 0) found = i;
            if (found < 0) {
                if (ncls >= 256) { ok = 0; break; }
                std::memcpy(mine.data() + 8 + (size_t)ncls * CLS_W, row, 7 * sizeof(double));
                mine[8 + (size_t)ncls * CLS_W + 7] = 0.0;
                found = ncls++;
                grown = true;
            }
            map[(size_t)side * 256 + j] = found;
        }
    }
    // every rank or none
    double flag = ok ? 0.0 : 1.0;
    HIP_TRY(hipMemcpyAsync(c->scalars + 7, &flag, sizeof(double), hipMemcpyHostToDevice, c->stream));
    MG_TRY(allreduce_sum(c, c->scalars + 7, 1));
    HIP_TRY(hipMemcpyAsync(&flag, c->scalars + 7, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (flag != 0.0) return 0;
    if (grown) {
        HIP_TRY(hipMemcpyAsync(L.ctab, mine.data() + 8, 256 * CLS_W * sizeof(double), hipMemcpyHostToDevice, c->stream));
        L.ncls = ncls;
    }
    HIP_TRY(hipMemcpyAsync(dmap.p, map.data(), 512 * sizeof(int), hipMemcpyHostToDevice, c->stream));
    const int* dm = dmap.as<const int>();
    if (lo) hipLaunchKernelGGL(doubles_to_classes, dim3(nb), dim3(256), 0, c->stream, recv, dm, L.cls + L.cls_lead - (int64_t)n, (int64_t)n);
    if (hi) hipLaunchKernelGGL(doubles_to_classes, dim3(nb), dim3(256), 0, c->stream, recv + n, dm + 256, L.cls + L.cls_lead + L.nloc, (int64_t)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    L.cls_halo = 1;
    return 0;
}

// K sweeps per pass (mg_jacobik3d.hip.h): seven-point levels with row classes that use the two-sweep pass -- whole levels,
// and slabs whose vectors have room for K halo planes ("halo_depth").
bool sweepsk_ok(const mg_context* c, const Level& L, bool ignore_size = false) {
    if (c->fuse_k < 3 || !L.cls || !c->fuse_classes) return false;
    if (L.cls_escape) {
        // (nothing else on such a level uses its classes: the march wherever it runs at all, whatever the level's size)
        if (L.esc_kmax < 3) return false;
        ignore_size = true;
    }
    const bool slab = is_slab(c, L);
    if (slab && (L.hd < 2 || L.cls_halo < 0 || c->halo_planes != 1)) return false;
    if (!ignore_size && (slab ? min_slab_rows(L) < c->fuse_k_slab_min_rows : L.nloc < c->fuse_k_min_rows)) return false;
    // (the size test of the K-sweep pass is the one above: "fuse_min_rows" is the pair pass's)
    // (whole levels with classes only: the march reads x, f and the class bytes, all padded by vec_reach whatever nx is)
    const int side = slab || L.cls_escape ? 32 : c->fuse_k_min_side;
    return fused_sweeps_ok(c, L, true, side) && L.g.nk >= 8;
}

// sweeps per pass on a whole level (with the 64 x 32 tiles of 16 waves five sweeps per pass measured best on 1025^3 and 513^3
// rows, four on 257^3, profiles/r03_ksweep_levels.txt; "fuse_k4_min_rows" caps smaller levels at three)
int sweepsk_max(const mg_context* c, const Level& L) {
    const int k = std::min(std::min(c->fuse_k, 5), L.nloc < c->fuse_k4_min_rows ? 3 : L.nloc < c->fuse_k_small_rows ? 5 : L.nloc < c->fuse_k5_min_rows ? 4 : 5);
    return L.cls_escape ? std::min(k, L.esc_kmax) : k;
}

// the most pool rows a tile of the escape variant of the march takes within K + 2 planes (jk3_escape_window)
template <int K>
int escape_window_k(mg_context* c, const Level& L, const unsigned char* cls, int64_t clead, unsigned* most) {
    constexpr int WI = 64 - 2 * K, HY = 16 * 2 - 2 * K + 2;
    JK3WindowArgs a{};
    a.cls = cls; a.clead = clead; a.P = L.g.plane; a.nx = L.g.nx; a.ny = L.g.ny; a.nz = L.g.nk;
    a.ntx = (a.nx + WI - 1) / WI; a.nty = (a.ny + HY - 1) / HY;
    a.most = reinterpret_cast<unsigned*>(c->partials.get());
    HIP_TRY(hipMemsetAsync(a.most, 0, sizeof(unsigned), c->stream));
    hipLaunchKernelGGL((jk3_escape_window<K, 16, 2>), dim3((unsigned)(a.ntx * a.nty)), dim3(256), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(most, a.most, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (std::getenv("MG_DEBUG_STORAGE"))
        std::fprintf(stderr, "[mg] escape rows: at most %u in %d planes of a tile (%d sweeps per pass, pool of %d)\n", *most, K + 2, K, jk3_pool(K));
    return 0;
}

int escape_kmax(mg_context* c, const Level& L, const unsigned char* cls, int64_t clead, int* kmax) {
    *kmax = 0;
    if (L.wu != 4 || L.g.nk < 8 || L.g.nx < 32 || L.g.ny < 32) return 0;
    unsigned most = 0;
    MG_TRY(escape_window_k<5>(c, L, cls, clead, &most));
    if (most <= (unsigned)jk3_pool(5)) { *kmax = 5; return 0; }
    MG_TRY(escape_window_k<4>(c, L, cls, clead, &most));
    if (most <= (unsigned)jk3_pool(4)) { *kmax = 4; return 0; }
    MG_TRY(escape_window_k<3>(c, L, cls, clead, &most));
    if (most <= (unsigned)jk3_pool(3)) *kmax = 3;
    return 0;
}

// plane ranges of one launch of the march: [za0, za1) and then [zb0, zb1)
struct JK3Range { int za0, za1, zb0, zb1; };

// the tile shape of a K-sweep pass ("fuse_k_shape"; -1: chosen by K)
// (shape 9, rim waves, exists for five sweeps per pass: with fewer it stands for shape 7)
int jk3_shape(const mg_context* c, int K) {
    const int shape = c->fuse_k_shape >= 0 ? c->fuse_k_shape : (K >= 5 ? 8 : 7);
    return shape == 9 && K < 5 ? 7 : shape;
}

// ... on a level with `ncls` classes (shapes 3 and up keep 64 rows of the class table in LDS or run one workgroup of 16 waves
// per CU: levels with more classes take shape 1) and `rows` rows; `whole`: not a slab.  Shape 9 marches whole levels: slabs
// take shape 8; chosen by K, five sweeps per pass take it on whole levels of at least "fuse_k_rim_min_rows" rows (the sizes it
// was measured at, 513^3 and 1025^3).
int jk3_shape_for(const mg_context* c, int K, int ncls, bool whole, int64_t rows) {
    int shape = jk3_shape(c, K);
    if (c->fuse_k_shape < 0 && K >= 5 && rows >= c->fuse_k_rim_min_rows) shape = 9;
    if (shape >= 3 && ncls > 64) return 1;
    return shape == 9 && !whole ? 8 : shape;
}

// March plans (jk3_plan).  Which launches take one: whole levels without escape rows on the 64 x 32 tiles of 16 waves
// (shapes 7 and 8), three to five sweeps per pass, and on the 64 x 36 tiles of shape 9 (five sweeps: the last slot).  Slabs
// and levels with escape rows are deliberately left out: a slab's plane range differs per rank and its launches are split,
// and escape rows are what the class loads are there to find.
constexpr int MARCH_PLAN_SLOT_RIM = 6;
int march_plan_slot(const mg_context* c, const Level& L, int K) {
    if (!c->fuse_k_plan || K < 3 || K > 5 || !L.cls || L.cls_escape || is_slab(c, L)) return -1;
    const int shape = jk3_shape_for(c, K, L.ncls, true, L.nloc);
    if (shape == 9) return MARCH_PLAN_SLOT_RIM;
    return shape == 7 || shape == 8 ? (K - 3) * 2 + (shape - 7) : -1;
}

// builds the level's plan of `slot` if it is missing (allocates and synchronises: not inside a capture)
int ensure_march_plan(mg_context* c, Level& L, int K, int slot) {
    Level::MarchPlan& mp = L.plan[slot];
    if (mp.iv) return 0;
    JK3PlanArgs a{};
    a.cls = L.cls; a.clead = L.cls_lead; a.P = L.g.plane; a.nx = L.g.nx; a.ny = L.g.ny; a.nz = L.g.nk; a.cmain = L.cmain;
    const bool rim = slot == MARCH_PLAN_SLOT_RIM;           // (K = 5)
    const int WI = 64 - 2 * K, HY = rim ? jk3_rim_map<5>::HY : 32 - 2 * K + 2;         // (shapes 7 and 8 share their tiles)
    a.ntx = (a.nx + WI - 1) / WI; a.nty = (a.ny + HY - 1) / HY;
    const size_t n = (size_t)a.ntx * a.nty * 16 * 4;
    DevBuf<int> iv;
    MG_TRY(iv.alloc(c, n));
    a.plan = iv;
    if (rim) hipLaunchKernelGGL((jk3_plan_rim<5>), dim3((unsigned)(a.ntx * a.nty)), dim3(16 * WAVE), 0, c->stream, a);
    else with_int<3, 4, 5>(K, [&](auto k) { hipLaunchKernelGGL((jk3_plan<decltype(k)::value, 16, 2>), dim3((unsigned)(a.ntx * a.nty)), dim3(16 * WAVE), 0, c->stream, a); });
    HIP_TRY(hipGetLastError());
    std::vector<int> h(n);
    HIP_TRY(hipMemcpyAsync(h.data(), iv, n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; i += 4) {
        if (h[i + 1] > h[i]) { ++mp.waves[0]; mp.planes[0] += h[i + 1] - h[i]; }
        if (h[i + 3] > h[i + 2] && (h[i + 2] != h[i] || h[i + 3] != h[i + 1])) { ++mp.waves[1]; mp.planes[1] += h[i + 3] - h[i + 2]; }
    }
    mp.iv = std::move(iv);
    return 0;
}

// (RIM: the tiles of shape 9, jk3_rim_map -- sixteen waves, the lines per wave are the map's; EARLY: its variant that issues
// the next plane's loads early, "fuse_k_load_early")
template <int K, int NW, int LPW, int WPE = (NW == 12 ? 3 : 2), int TR = 256, bool ESC = false, bool B1 = false, bool RIM = false, bool EARLY = false>
int launch_jacobikc_t(mg_context* c, JK3Args a, bool finest, const JK3Range& zr, int seglen) {
    static_assert(!RIM || (NW == jk3_rim_map<K>::NW && WPE == 4 && !ESC && B1), "shape 9 is shape 8 with another line map");
    static_assert(RIM || !EARLY, "only shape 9 has the variant");
    constexpr int EX = 64, EY = RIM ? jk3_rim_map<K>::EY : NW * LPW, WI = EX - 2 * K, HY = EY - 2 * K + 2;
    a.ntx = (a.nx + WI - 1) / WI;
    a.nty = (a.ny + HY - 1) / HY;
    const int64_t ntile = (int64_t)a.ntx * a.nty;
    constexpr size_t lds = RIM ? jk3r_lds_bytes<K, TR>() : B1 ? jk3b_lds_bytes<K, NW, LPW, TR>() : jk3_lds_bytes<K, NW, LPW, TR, ESC>();
    static_assert(lds <= 160 * 1024, "one CU's LDS");
    a.za0 = zr.za0; a.za1 = zr.za1; a.zb0 = zr.zb0; a.zb1 = zr.zb1;
    const int planes = std::max(0, zr.za1 - zr.za0) + std::max(0, zr.zb1 - zr.zb0);
    if (planes <= 0) return 0;
    a.ta = (int)ntile; a.seglen_b = 1;
    int64_t items = 0;
    if (seglen <= 0) {
        // Plane segments.  The items run in rounds of the resident workgroups (by LDS and by waves per SIMD), each paying 2K
        // steps of warm-up (which do about two thirds of a step's work).  A last round that only a few tiles are left for
        // would keep most CUs idle for a whole segment: those tiles -- fewer than there are CUs -- are cut into as many shorter
        // segments as fill the round once, and come last ("fuse_k_tail" 0: every tile alike).
        int64_t cus = std::max(1, c->prop.multiProcessorCount) * (int64_t)std::max<size_t>(1, std::min<size_t>(160 * 1024 / lds, (size_t)(4 * WPE / NW)));
        if (c->fuse_k_tail > 1) cus = c->fuse_k_tail;       // (tests: a tail on grids of a few tiles)
        const double warm = 1.4 * K;
        int best = 1, best_ta = (int)ntile, best_m = 1;
        double best_cost = 1e300;
        const bool tail = c->fuse_k_tail && zr.zb1 <= zr.zb0;
        for (int n = 1; n <= std::max(1, planes / 8); ++n) {
            const int len = (planes + n - 1) / n;
            const int64_t full = ntile * n / cus;
            int64_t ta = tail ? std::min<int64_t>(ntile, full * cus / n) : ntile;
            if (ta <= 0 || (ntile - ta) * 2 > cus) ta = ntile;           // (a tail of more than half a round is a round)
            const int64_t tb = ntile - ta;
            const int m = tb > 0 ? (int)std::max<int64_t>(1, std::min<int64_t>(cus / tb, planes / 4)) : 1;
            const double cost = (double)((ta * n + cus - 1) / cus) * (len + warm) + (tb > 0 ? (planes + m - 1) / m + warm : 0.0);
            if (cost < best_cost) { best_cost = cost; best = n; best_ta = (int)ta; best_m = m; }
        }
        if (c->fuse_k_segments > 0) { best = std::min(c->fuse_k_segments, planes); best_ta = (int)ntile; }
        seglen = (planes + best - 1) / best;
        a.ta = best_ta;
        a.seglen_b = best_ta < ntile ? (planes + best_m - 1) / best_m : 1;
    }
    a.seglen = seglen;
    {
        const int nseg = (std::max(0, zr.za1 - zr.za0) + seglen - 1) / seglen + (std::max(0, zr.zb1 - zr.zb0) + seglen - 1) / seglen;
        items = (int64_t)a.ta * nseg;
        if (a.ta < ntile) items += (ntile - a.ta) * (int64_t)((planes + a.seglen_b - 1) / a.seglen_b);
    }
    a.xcd_chunk = (unsigned)c->fuse_xcd_chunk;
    unsigned grid = 0;
    MG_TRY(tile_grid(items, a.xcd_chunk, &grid));
    a.nitems = (unsigned)items;
    if (a.ncls > TR) return fail("more row classes than this tile shape keeps in LDS");
    void (*kern)(JK3Args) = nullptr;
    if constexpr (ESC) kern = sdia_jacobikc_escape<K, NW, LPW, WPE, TR>;
    else if constexpr (RIM && EARLY) kern = finest ? sdia_jacobikc_finest_rim_early<K, TR> : sdia_jacobikc_rim_early<K, TR>;
    else if constexpr (RIM) kern = finest ? sdia_jacobikc_finest_rim<K, TR> : sdia_jacobikc_rim<K, TR>;
    else if constexpr (B1) kern = finest ? sdia_jacobikc_finest_b1<K, NW, LPW, WPE, TR> : sdia_jacobikc_b1<K, NW, LPW, WPE, TR>;
    else kern = finest ? sdia_jacobikc_finest<K, NW, LPW, WPE, TR> : sdia_jacobikc<K, NW, LPW, WPE, TR>;
    MG_TRY(allow_large_lds(c, reinterpret_cast<const void*>(kern), lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NW * WAVE), lds, c->stream, a);
    HIP_TRY(hipGetLastError());
    c->jk3_tail = a.ta < ntile ? 1 : 0;
    return 0;
}

template <int K>
int launch_jacobikc_k(mg_context* c, const JK3Args& a, bool finest, const JK3Range& zr, int seglen, bool whole) {
    // levels with rows of class CLS_ESCAPE: the variant that fetches them, one tile shape (the one escape_window() checked)
    if (a.escape) {
        if constexpr (K >= 3) return launch_jacobikc_t<K, 16, 2, 4, 256, true>(c, a, finest, zr, seglen);
        else return fail("levels with escape rows take three to five sweeps per pass");
    }
    // (two sweeps per pass: slabs only, where a pass also saves an exchange; one tile shape)
    if constexpr (K == 2) {
        return launch_jacobikc_t<K, 12, 4>(c, a, finest, zr, seglen);
    } else {
        // shape 4 and shapes 7 to 9 keep 64 rows of the class table in LDS or run one workgroup of 16 waves per CU; levels with
        // more classes take shape 1
        int shape = jk3_shape_for(c, K, a.ncls, whole, a.P * a.nz);
        // planes with fewer 64 x 48 tiles than the GPU has CUs (the 513^2 and 257^2 planes of a slab's coarser levels): half
        // as tall tiles, two workgroups per CU
        if (shape == 1 && a.ncls <= 64 && K <= 4 && c->fuse_k_small_tiles) {
            constexpr int WI = 64 - 2 * K, HY = 48 - 2 * K + 2;
            if ((int64_t)((a.nx + WI - 1) / WI) * ((a.ny + HY - 1) / HY) < std::max(1, c->prop.multiProcessorCount)) shape = 4;
        }
        switch (shape) {
            case 1: return launch_jacobikc_t<K, 12, 4>(c, a, finest, zr, seglen);                           // 64 x 48 by 12 waves
            case 4: return launch_jacobikc_t<K, 8, 3, 4, 64>(c, a, finest, zr, seglen);                     // 64 x 24 by 8 waves, two workgroups per CU
            case 7: return launch_jacobikc_t<K, 16, 2, 4>(c, a, finest, zr, seglen);                        // 64 x 32 by 16 waves
            case 8: return launch_jacobikc_t<K, 16, 2, 4, 256, false, true>(c, a, finest, zr, seglen);      // ... one barrier per step
            case 9: if constexpr (K == 5) {                                                                 // ... rim waves, 64 x 36
                        if (c->fuse_k_load_early && a.P * a.nz >= c->fuse_k_load_early_min_rows)
                            return launch_jacobikc_t<K, 16, 2, 4, 64, false, true, true, true>(c, a, finest, zr, seglen);
                        return launch_jacobikc_t<K, 16, 2, 4, 64, false, true, true>(c, a, finest, zr, seglen);
                    } else return fail("tile shape 9 takes five sweeps per pass");
            default: return fail("no such tile shape");
        }
    }
}

// out = K Jacobi sweeps applied to x (2 <= K <= 5) on the owned planes [zr) of the level (null: all of them); on slabs the
// level's K halo planes of x and K - 1 of f must be valid
int launch_jacobikc(mg_context* c, Level& L, int K, const double* x_rows, const double* f_rows, double* out_rows,
                    const JK3Range* zr = nullptr, int seglen = 0) {
    JK3Args a{};
    a.x = x_rows; a.f = f_rows; a.out = out_rows;
    fill_classes_lead(a, L);
    a.P = L.g.plane; a.nx = L.g.nx; a.ny = L.g.ny; a.nz = L.g.nk; a.omega = c->omega;
    const bool dist = is_slab(c, L);
    a.plo = dist && c->comm.rank > 0 ? K : 0;
    a.phi = dist && c->comm.rank + 1 < c->comm.world ? K : 0;
    if (dist && (L.hd < K || L.cls_halo != 1)) return fail("the level's halos are not prepared for that many sweeps per pass");
    if (L.cls_escape && K > L.esc_kmax) return fail("too many escape rows per tile for that many sweeps per pass");
    a.force_form = c->timing_force_form;
    a.nt_store = c->fuse_k_nt_store;
    // the march plan: built here when it is missing, but for a launch that is being captured (prepare_cycle builds the plans
    // of captured cycles) -- that one runs without, to the same result
    if (const int slot = march_plan_slot(c, L, K); slot >= 0 && a.force_form < 0 && !zr) {
        if (!L.plan[slot].iv) {
            hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
            HIP_TRY(hipStreamIsCapturing(c->stream, &st));
            if (st == hipStreamCaptureStatusNone) MG_TRY(ensure_march_plan(c, L, K, slot));
        }
        a.plan = L.plan[slot].iv;
    }
    a.escape = L.cls_escape ? 1 : 0; a.dvals = L.dvals; a.mlead = L.mlead; a.sshift = L.R == 1 ? 6 : (L.R == 2 ? 7 : 8);
    const JK3Range whole{0, L.g.nk, 0, 0};
    c->jk3_tail = 0;
    int rc = 0;
    if (!with_int<2, 3, 4, 5>(K, [&](auto k) { rc = launch_jacobikc_k<decltype(k)::value>(c, a, is_finest(c, L), zr ? *zr : whole, seglen, !dist); }))
        return fail("sweeps per pass must be in 2..5");
    return rc;
}

// Is lattice_color(COLOR_LATTICE9) a valid Gauss-Seidel colouring of the level's matrix?  (structure of the stored
// non-zeros, in whatever format the level has)
int check_coloring(mg_context* c, Level& L) {
    MG_TRY(need_stored_rows(c, L, "the colouring check of the Gauss-Seidel smoothers"));
    EllArgs a{};
    a.vals = L.vals; a.cols = L.cols; a.codes = L.codes; a.offsets = L.offsets; a.W = L.W;
    a.nloc = L.nloc; a.lead = L.g.lead; a.dinv = L.dinv; a.color_kind = COLOR_LATTICE9; a.grow0 = L.row0; a.gnx = L.g.nx; a.gny = L.g.ny;
    int* d_flag = reinterpret_cast<int*>(c->partials.get());
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int), c->stream));
    const dim3 grid(blocks_for(L.nloc, 256)), blk(256);
    if (L.sdia) {
        a.vals = L.dvals; a.mlead = L.mlead;
        for (int t = 0; t < 8; ++t) a.up[t] = L.up[t];
        with_int_else<4, 1, 2>(L.R, [&](auto r) { hipLaunchKernelGGL(sdia_check_coloring<decltype(r)::value>, grid, blk, 0, c->stream, a, L.wu, d_flag); });
    } else {
        with_int_else<4, 1, 2>(L.R, [&](auto r) { hipLaunchKernelGGL(ell_check_coloring<decltype(r)::value>, grid, blk, 0, c->stream, a, L.nslices, d_flag); });
    }
    HIP_TRY(hipGetLastError());
    int flag = 1;
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    L.mc_ok = flag ? 0 : 1;
    return 0;
}

// K sweeps per launch on 2-D levels (mg_jacobi2.hip.h, sdia_jacobik2d): whole, undistributed five-point levels
// with row classes whose stored diagonals are exactly {0, +1, +nx}.
bool sweeps2d_ok(const mg_context* c, const Level& L) {
    if (!c->fuse_2d || !L.sdia || L.wu != 3 || !cls_full(L) || !c->fuse_classes || L.flat || !L.replicated) return false;
    return L.g.ny == 1 && L.up[1] == 1 && L.up[2] == L.g.nx && L.g.nx >= 8 && L.g.nz >= 8;
}

// Lines per region ("fuse_2d_lines"; 0 = chosen here).  Regions of 32 lines (four cells per thread, 56 registers, 80 KB of LDS)
// run two workgroups per CU, which hides the barriers of one behind the other: 0.039 ms per five sweeps on 2049^2 rows against
// 0.049 with 64 lines although a sweep keeps 22 of 32 lines instead of 54 of 64 -- BASELINE config 2 451 -> 592 cycles/s
// (profiles/r03_2d_lines.txt).  A launch on a small level takes as long as ONE workgroup does, about 2 us plus 1.3 us per cell
// a thread owns: 16 lines (two cells) while all tiles still run at once.
template <int K, int H>
int launch_jacobik_th(mg_context* c, const JKArgs& a, bool cheb) {
    constexpr size_t lds = jk_lds_bytes<H>();
    void (*const kern)(JKArgs) = cheb ? sdia_jacobik2d<K, H, true> : sdia_jacobik2d<K, H>;
    MG_TRY(allow_large_lds(c, reinterpret_cast<const void*>(kern), lds));
    JKArgs b = a;
    b.ntx = (a.nx + JK_W - 2 * K - 1) / (JK_W - 2 * K);
    b.nty = (a.nlines + H - 2 * K - 1) / (H - 2 * K);
    hipLaunchKernelGGL(kern, dim3((unsigned)(b.ntx * b.nty)), dim3(1024), lds, c->stream, b);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int K>
int launch_jacobik_t(mg_context* c, const JKArgs& a, bool cheb) {
    const int64_t cus = std::max(1, c->prop.multiProcessorCount);
    const int64_t ntx = (a.nx + JK_W - 2 * K - 1) / (JK_W - 2 * K);
    int best = c->fuse_2d_lines;
    if (!best) best = K <= 5 && ntx * ((a.nlines + 16 - 2 * K - 1) / (16 - 2 * K)) <= 2 * cus ? 16 : 32;
    int rc = 0;
    with_int_else<64, 16, 32>(best, [&](auto h) { rc = launch_jacobik_th<K, decltype(h)::value>(c, a, cheb); });
    return rc;
}

// out = K Jacobi sweeps applied to x (2 <= K <= 5); with al / be: the K steps of a whole Chebyshev call (be[0] == 0)
int launch_jacobik(mg_context* c, const Level& L, int K, const double* x_rows, const double* f_rows, double* out_rows,
                   const double* al = nullptr, const double* be = nullptr) {
    JKArgs a{};
    a.x = x_rows; a.f = f_rows; a.out = out_rows;
    fill_classes(a, L);
    a.n = L.nloc; a.nx = L.g.nx; a.nlines = L.g.nz; a.omega = c->omega;
    const bool cheb = al != nullptr;
    if (cheb) {
        if (K > 5 || be[0] != 0.0) return fail("Chebyshev: one launch of the 2-D kernel takes a whole call of at most 5 steps");
        a.omega = 1.0;                                  // (the class table then holds 1 / d, bit for bit)
        for (int t = 0; t < K; ++t) { a.al[t] = al[t]; a.be[t] = be[t]; }
    }
    int rc = 0;
    if (!with_int<2, 3, 4, 5>(K, [&](auto k) { rc = launch_jacobik_t<decltype(k)::value>(c, a, cheb); }))
        return fail("sweeps per launch must be in 2..5");
    return rc;
}

// One sweep as a plane march (sdia_sweep1c): whole, undistributed 3-D seven-point levels with row classes, large enough
// for the march to pay ("march_min_rows").
bool sweep1c_ok(const mg_context* c, const Level& L) {
    if (!c->march_sweeps || !cls_full(L) || !c->class_sweeps || !L.sdia || L.wu != 4 || L.flat || !L.replicated) return false;
    if (L.g.nx < 32 || L.g.ny < 32 || L.g.nk < 8) return false;
    if (L.up[1] != 1 || L.up[2] != L.g.nx || (int64_t)L.up[3] != L.g.plane) return false;
    return L.nloc >= c->march_min_rows;
}

template <int NW, int LPW>
int launch_sweep1c_t(mg_context* c, J2Args& a, int mode) {
    constexpr int EY = NW * LPW;
    a.ntx = (a.nx + J2_EX - 3) / (J2_EX - 2);
    a.nty = (a.ny + EY - 1) / EY;
    const int64_t ntile = (int64_t)a.ntx * a.nty;
    // plane segments: enough work items for a few rounds of the CUs, each paying ~2.5 plane-times of warm-up
    const int64_t cus = std::max(1, c->prop.multiProcessorCount);
    int best = best_segments(ntile, cus, a.nz, a.nz / 16, 2.5);
    if (c->fuse_segments > 0) best = std::min(c->fuse_segments, a.nz);
    a.seglen = (a.nz + best - 1) / best;
    const int nseg = (a.nz + a.seglen - 1) / a.seglen;
    const int64_t items = ntile * nseg;
    a.xcd_chunk = (unsigned)c->fuse_xcd_chunk;
    unsigned grid = 0;
    MG_TRY(tile_grid(items, a.xcd_chunk, &grid));
    a.nitems = (unsigned)items;
    constexpr size_t lds = j1c_lds_bytes<NW, LPW>();
    void (*kern)(J2Args) = nullptr;
    with_march_mode(mode, [&](auto m) { kern = sdia_sweep1c<NW, LPW, decltype(m)::value>; });
    MG_TRY(allow_large_lds(c, reinterpret_cast<const void*>(kern), lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NW * WAVE), lds, c->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_sweep1c(mg_context* c, const Level& L, int mode, const double* x_rows, const double* f_rows, double* out_rows,
                   int color, double alpha, double beta) {
    J2Args a{};
    a.x = x_rows; a.f = f_rows; a.out = out_rows;
    a.xp = out_rows; a.beta = beta;
    a.nloc = L.nloc; a.P = L.g.plane; a.nx = L.g.nx; a.ny = L.g.ny; a.nz = L.g.nk; a.omega = mode == MODE_CHEB ? alpha : c->omega;
    fill_classes_lead(a, L);
    a.color = color; a.color_kind = c->smoother == MG_SMOOTH_MCGS ? COLOR_LATTICE9 : COLOR_PARITY; a.grow0 = L.row0;
    if (c->march_shape == 1) return launch_sweep1c_t<16, 2>(c, a, mode);
    return launch_sweep1c_t<12, 2>(c, a, mode);
}

// All sweeps of a small level in one launch (mg_jacobi2.hip.h, sdia_jacobi_small): whole five- / seven-point levels with
// row classes that fit one CU's LDS.
// K sweeps per launch on blocks resident on the CU (mg_jacobiblk.hip.h): whole seven-point levels with row classes, sizes
// below the plane marches'
bool block_sweeps_ok(const mg_context* c, const Level& L) {
    if (!c->fuse_block || !L.sdia || L.wu != 4 || !cls_full(L) || !c->fuse_classes || L.flat || !L.replicated) return false;
    if (!L.grid_decoupled || L.ncls > 128 || L.g.nx < 8 || L.g.ny < 8 || L.g.nk < 8 || L.nloc >= ((int64_t)1 << 28)) return false;
    return c->fuse_block >= 2 || (L.nloc >= c->fuse_block_min_rows && L.nloc < c->fuse_block_max_rows);
}

// sweeps per launch and planes per block: the launch runs in rounds of one workgroup per CU, a workgroup loads EZ planes
// of 32 x 32 cells (about 0.33 us per plane) and relaxes them K times (0.13 us per plane and sweep), of which it keeps
// (32 - 2K)^2 (EZ - 2K) cells
struct JBPlan { int K, EZ; };

JBPlan block_plan(const mg_context* c, const Level& L) {
    const int64_t cus = std::max(1, c->prop.multiProcessorCount);
    const int EZ = c->fuse_block_ez ? c->fuse_block_ez : 11;
    auto blocks = [&](int K) {
        const int ow = JB_E - 2 * K, oz = EZ - 2 * K;
        return (int64_t)((L.g.nx + ow - 1) / ow) * ((L.g.ny + ow - 1) / ow) * ((L.g.nk + oz - 1) / oz);
    };
    // three sweeps per launch; four where the blocks then still all run at once (65^3 rows: 3.4 against 3.9 us per sweep)
    const int K = c->fuse_block_k ? c->fuse_block_k : blocks(4) <= cus ? 4 : 3;
    return JBPlan{K, EZ};
}

template <int K, int EZ>
int launch_jacobi_block_t(mg_context* c, const Level& L, JBArgs a) {
    constexpr int ow = JB_E - 2 * K, oz = EZ - 2 * K;
    a.nbx = (a.nx + ow - 1) / ow;
    a.nby = (a.ny + ow - 1) / ow;
    const int64_t nb = (int64_t)a.nbx * a.nby * ((a.nz + oz - 1) / oz);
    if (nb >= ((int64_t)1 << 31)) return fail("too many blocks");
    const size_t lds = jb_lds_bytes<EZ>(a.ncls);
    if (lds > (size_t)160 * 1024) return fail("block pass: class table too large");
    void (*const kern)(JBArgs) = sdia_jacobi_block<K, EZ>;
    MG_TRY(allow_large_lds(c, reinterpret_cast<const void*>(kern), (size_t)160 * 1024));
    hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(1024), lds, c->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// out = K Jacobi sweeps applied to x (2 <= K <= 4), blocks of EZ planes (11 or 19)
int launch_jacobi_block(mg_context* c, const Level& L, int K, int EZ, const double* x_rows, const double* f_rows, double* out_rows) {
    JBArgs a{};
    a.x = x_rows; a.f = f_rows; a.out = out_rows;
    fill_classes(a, L);
    a.omega = c->omega; a.nx = L.g.nx; a.ny = L.g.ny; a.nz = L.g.nk; a.P = L.g.plane;
    int rc = 0;
    const bool known = with_int<2, 3, 4>(K, [&](auto k) {
        if (!with_int<11, 19>(EZ, [&](auto ez) { rc = launch_jacobi_block_t<decltype(k)::value, decltype(ez)::value>(c, L, a); })) rc = -1;
    });
    if (!known || rc == -1) return fail("block pass: 2..4 sweeps per launch on blocks of 11 or 19 planes");
    return rc;
}

bool small_level_ok(const mg_context* c, const Level& L) {
    if (!c->fuse_small || !L.sdia || !cls_full(L) || !c->fuse_classes || L.flat || !L.replicated) return false;
    if (L.wu != 3 && L.wu != 4) return false;
    if (L.up[1] != 1 || L.up[2] <= 1 || (L.wu == 4 && L.up[3] <= L.up[2])) return false;
    const int pad = L.wu == 4 ? L.up[3] : L.up[2];
    // (2-D levels of more than "fuse_small_2d_rows" rows are faster through the K-sweep 2-D kernel -- ten launches of a dozen
    //  small workgroups on as many CUs instead of one launch of one workgroup: 65^2 rows 55 against 72 us per 50 sweeps)
    if (L.wu == 3 && L.nloc > c->fuse_small_2d_rows && sweeps2d_ok(c, L)) return false;
    return L.nloc <= 16384 && js_lds_bytes((int)L.nloc, pad) <= (size_t)150 * 1024;
}

// nw Jacobi sweeps; with al / be: nw <= JS_CHEB_STEPS Chebyshev steps, continuing from x_{k-1} in out_rows when be[0] != 0
// and leaving x_{nw-1} in x_rows (the state of the one-step sequence once v and v2 swap)
int launch_jacobi_small(mg_context* c, const Level& L, int nw, const double* x_rows, const double* f_rows, double* out_rows,
                        const double* al = nullptr, const double* be = nullptr) {
    JSArgs a{};
    a.x = x_rows; a.f = f_rows; a.out = out_rows;
    fill_classes(a, L);
    a.n = (int)L.nloc; a.nw = nw; a.up1 = L.up[1]; a.up2 = L.up[2]; a.up3 = L.wu == 4 ? L.up[3] : 0; a.omega = c->omega;
    const bool cheb = al != nullptr;
    if (cheb) {
        if (nw > JS_CHEB_STEPS) return fail("Chebyshev: too many steps for one launch of the small-level kernel");
        a.omega = 1.0;                                  // (the class table then holds 1 / d, bit for bit)
        a.xp = out_rows; a.xm = const_cast<double*>(x_rows);
        for (int t = 0; t < nw; ++t) { a.al[t] = al[t]; a.be[t] = be[t]; }
    }
    const size_t lds = js_lds_bytes(a.n, L.wu == 4 ? a.up3 : a.up2);
    // rows per thread: the smallest instance that covers the level
    const int need = (a.n + 1023) / 1024;
    void (*kern)(JSArgs) = nullptr;
    auto pick = [&](auto wu_tag) {
        constexpr int WU = decltype(wu_tag)::value;
        auto k = [&](auto rpt_tag) {
            constexpr int RPT = decltype(rpt_tag)::value;
            kern = cheb ? sdia_jacobi_small<WU, RPT, true, true> : sdia_jacobi_small<WU, RPT>;
        };
        if (need <= 1) k(std::integral_constant<int, 1>{});
        else if (need <= 2) k(std::integral_constant<int, 2>{});
        else if (need <= 3) k(std::integral_constant<int, 3>{});
        else if (need <= 4) k(std::integral_constant<int, 4>{});
        else if (need <= 5) k(std::integral_constant<int, 5>{});
        else if (need <= 6) k(std::integral_constant<int, 6>{});
        else if (need <= 8) k(std::integral_constant<int, 8>{});
        else if (need <= 12) k(std::integral_constant<int, 12>{});
        else k(std::integral_constant<int, 16>{});
    };
    with_int_else<3, 4>(L.wu, pick);
    MG_TRY(allow_large_lds(c, reinterpret_cast<const void*>(kern), (size_t)150 * 1024));
    hipLaunchKernelGGL(kern, dim3(1), dim3(1024), lds, c->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// a slab level on which calls of enough sweeps take the K-sweep march with K-plane exchanges (the same answer on every rank)
bool slab_ksweep_level(const mg_context* c, const Level& L) {
    return is_slab(c, L) && c->fuse_k >= 3 && c->fuse_sweeps && c->fuse_classes && c->use_classes && c->use_sdia &&
           L.hd >= 2 && c->halo_planes == 1 && !L.flat && L.g.nx >= 32 && L.g.ny >= 32 &&
           min_slab_rows(L) >= std::max<int64_t>(8 * L.g.plane, c->fuse_k_slab_min_rows);
}

// mg_smoother_launches: one pass of `sweeps` Jacobi sweeps of the whole level, made of `launches` launches of `path`
// (host-side bookkeeping when the pass is enqueued or captured)
void count_pass(mg_context* c, int level, int path, int launches, int sweeps, int tail_launches = 0) {
    auto& n = c->smoother_counts[(size_t)level][(size_t)path];
    n.launches += launches;
    n.sweeps += sweeps;
    n.tail += tail_launches;
}

int cheb_interval(mg_context* c, int level, double* lo, double* hi);

// The step scalars of a Chebyshev polynomial of degree m on [lo, hi] (Saad, Iterative Methods, Alg. 12.1): step k is
// x_{k+1} = x_k + alpha[k] D^-1 (f - A x_k) + beta[k] (x_k - x_{k-1}), beta[0] = 0.  Host doubles in this fixed order, so that
// tests/cheb_reference.py gets the same bits; they reach the kernels as arguments (a captured cycle replays them).
void cheb_steps(double lo, double hi, int m, double* alpha, double* beta) {
    const double theta = 0.5 * (hi + lo), delta = 0.5 * (hi - lo), sigma = theta / delta;
    double rho = 1.0 / sigma;
    if (m > 0) { alpha[0] = 1.0 / theta; beta[0] = 0.0; }
    for (int k = 1; k < m; ++k) {
        const double rn = 1.0 / (2.0 * sigma - rho);
        alpha[k] = 2.0 * rn / delta;
        beta[k] = rn * rho;
        rho = rn;
    }
}

int smooth_matrix_free(mg_context* c, int level, int nw);
int smooth_chebyshev(mg_context* c, int level, int nw);
int smooth_rbgs(mg_context* c, int level, int nw);
int smooth_mcgs(mg_context* c, int level, int nw);
int smooth_jacobi(mg_context* c, int level, int nw);

// nw Jacobi sweeps (Chebyshev: a polynomial of degree nw); v halos must be valid on entry and are valid on exit.
int smooth(mg_context* c, int level, int nw) {
    const Level& L = c->L[level];
    if (L.mf && c->smoother != MG_SMOOTH_JACOBI && c->smoother != MG_SMOOTH_CHEBYSHEV)
        return fail("level " + std::to_string(level) + " is a matrix-free diffusion level: Gauss-Seidel smoothers (RBGS, MCGS) "
                    "need stored rows; use Jacobi or Chebyshev");
    switch (c->smoother) {
        case MG_SMOOTH_CHEBYSHEV: return smooth_chebyshev(c, level, nw);
        case MG_SMOOTH_RBGS: return smooth_rbgs(c, level, nw);
        case MG_SMOOTH_MCGS: return smooth_mcgs(c, level, nw);
        default: return L.mf ? smooth_matrix_free(c, level, nw) : smooth_jacobi(c, level, nw);
    }
}

// Jacobi on a matrix-free diffusion level: one sweep per launch, the rows rebuilt from kappa (the fused passes all read
// stored rows or row classes)
int smooth_matrix_free(mg_context* c, int level, int nw) {
    Level& L = c->L[level];
    for (int s = 0; s < nw; ++s) {
        MG_TRY(launch_ell(c, L, level_op(L, MODE_JACOBI)));
        count_pass(c, level, MG_PATH_MATRIX_FREE, 1, 1);
        std::swap(L.v, L.v2);
    }
    return 0;
}

int smooth_chebyshev(mg_context* c, int level, int nw) {
    Level& L = c->L[level];
    // one step per launch of whatever kernel launch_ell picks for a Jacobi sweep of the level (counted under its path):
    // x_{k-1} lives in v2, which each step overwrites row by row with x_{k+1} before v and v2 swap; slabs exchange the
    // halo of v after each step (x_{k-1} needs none)
    if (nw == 0) return 0;
    double lo = 0.0, hi = 0.0;
    MG_TRY(cheb_interval(c, level, &lo, &hi));
    std::vector<double> al((size_t)nw), be((size_t)nw);
    cheb_steps(lo, hi, nw, al.data(), be.data());
    const bool dist = is_slab(c, L);
    if (!dist && nw >= 2 && small_level_ok(c, L)) {
        // levels that fit one CU: up to JS_CHEB_STEPS steps per launch of one workgroup, x_{k-1} in registers; a launch
        // continues from and leaves the one-step sequence's state (v = x_k, v2 = x_{k-1}), so longer calls chain launches
        for (int s0 = 0; s0 < nw; s0 += JS_CHEB_STEPS) {
            const int k = std::min(JS_CHEB_STEPS, nw - s0);
            MG_TRY(launch_jacobi_small(c, L, k, L.v.rows, L.f.rows, L.v2.rows, al.data() + s0, be.data() + s0));
            count_pass(c, level, MG_PATH_SMALL, 1, k);
            std::swap(L.v, L.v2);
        }
        return 0;
    }
    if (!dist && nw >= 2 && nw <= std::min(5, c->fuse_2d_k) && sweeps2d_ok(c, L)) {
        // 2-D levels: a whole call of at most "fuse_2d_k" steps in one launch.  (Tiles read their halo of x_{k-1}: a launch
        // that continued a call would read cells that other tiles overwrite, so longer calls run one step per launch.)
        MG_TRY(launch_jacobik(c, L, nw, L.v.rows, L.f.rows, L.v2.rows, al.data(), be.data()));
        count_pass(c, level, MG_PATH_K2D, 1, nw);
        std::swap(L.v, L.v2);
        return 0;
    }
    // (launch_ell's choice for a whole level)
    const int one_path = L.mf ? MG_PATH_MATRIX_FREE : sweep1c_ok(c, L) ? MG_PATH_SWEEP1C : MG_PATH_SLICE;
    for (int s = 0; s < nw; ++s) {
        EllRequest step = level_op(L, MODE_CHEB);
        step.alpha = al[(size_t)s]; step.beta = be[(size_t)s];
        MG_TRY(launch_ell(c, L, step));
        count_pass(c, level, one_path, 1, 1);
        std::swap(L.v, L.v2);
        MG_TRY(exchange_halo(c, L, L.v));
    }
    return 0;
}

// one Gauss-Seidel colour of the level, in place
int launch_gs_color(mg_context* c, const Level& L, int color) {
    EllRequest q = level_op(L, MODE_GS);
    q.out_rows = L.v.rows; q.color = color;
    return launch_ell(c, L, q);
}

// red-black Gauss-Seidel: two in-place half sweeps per sweep, halos refreshed after each colour
int smooth_rbgs(mg_context* c, int level, int nw) {
    Level& L = c->L[level];
    if (!L.rb_ok)
        return fail("red-black ordering is not a valid two-colouring of level " + std::to_string(level) +
                    " (needs a pruned grid matrix with an odd number of nodes per axis)");
    for (int s = 0; s < nw; ++s)
        for (int color = 0; color < 2; ++color) {
            MG_TRY(launch_gs_color(c, L, color));
            MG_TRY(exchange_halo(c, L, L.v));
        }
    return 0;
}

// nine-colour Gauss-Seidel for P2 rows (lattice_color): one in-place launch per colour, in ascending order
int smooth_mcgs(mg_context* c, int level, int nw) {
    Level& L = c->L[level];
    if (L.flat) return fail("multi-colour Gauss-Seidel needs a grid level");
    if (L.mc_ok < 0) MG_TRY(check_coloring(c, L));
    if (!L.mc_ok)
        return fail("the nine lattice colours are not a valid colouring of level " + std::to_string(level) +
                    " (needs a pruned P1 / P2 grid matrix)");
    // whole 3-D lattice levels: two colours per launch, out of place (v -> v2, then the two swap)
    const bool pairs = c->lattice_gs2 && c->class_sweeps && lat_march_ok(c, L) && (L.replicated || !c->comm.active());
    for (int s = 0; s < nw; ++s) {
        if (pairs) {
            for (int color = 0; color < 9; color += 2)
                MG_TRY(launch_lat_gs2(c, L, color, color + 1 < 9 ? color + 1 : -1, L.v.rows, L.v2.rows));
            std::swap(L.v, L.v2);
            continue;
        }
        for (int color = 0; color < 9; ++color) {
            if (c->dim == 2 && (color & 2)) continue;            // (nx, 1, nz) storage: j is always 0
            MG_TRY(launch_gs_color(c, L, color));
            MG_TRY(exchange_halo(c, L, L.v));
        }
    }
    return 0;
}

// ---- Jacobi: the paths, in the order smooth_jacobi tries them.  Each takes the sweeps it can of *nw and leaves the rest. ----

// sweeps of the next launch of a kernel that takes up to kmax and at least two: kmax, but 6 = 3 + 3 rather than 5 + 1
// (the rest, at most one, is a single sweep)
int up_to(int kmax, int left) {
    const int k = std::min(kmax, left);
    return left - k == 1 && k > 2 ? k - 1 : k;
}

// sweeps of the next pass of the K-sweep march: kmax while that leaves no single sweep over (50 = 12 x 4 + 2, 7 = 4 + 3,
// 5 = 3 + 2)
int next_pass(int left, int kmax) { return left >= kmax + 2 || left == kmax ? kmax : left == kmax + 1 ? kmax - 1 : left; }

// What follows on the communication stream waits for everything enqueued on the main stream so far ...
int fork_to_comm(mg_context* c) {
    HIP_TRY(hipEventRecord(c->ev_boundary, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->comm_stream, c->ev_boundary, 0));
    return 0;
}
// ... and what follows on the main stream for everything enqueued on the communication stream so far.
int join_comm(mg_context* c) {
    HIP_TRY(hipEventRecord(c->ev_halo, c->comm_stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_halo, 0));
    return 0;
}
// f() with the communication stream in the main stream's place (the launchers and exchanges enqueue on c->stream)
template <class F>
int on_comm_stream(mg_context* c, F&& f) {
    std::swap(c->stream, c->comm_stream);
    const int rc = f();
    std::swap(c->stream, c->comm_stream);
    return rc;
}

// all sweeps of a level that fits one CU's LDS in one launch
int jacobi_small(mg_context* c, int level, int* nw) {
    Level& L = c->L[level];
    if (is_slab(c, L) || *nw < 2 || !small_level_ok(c, L)) return 0;
    MG_TRY(launch_jacobi_small(c, L, *nw, L.v.rows, L.f.rows, L.v2.rows));
    count_pass(c, level, MG_PATH_SMALL, 1, *nw);
    std::swap(L.v, L.v2);
    *nw = 0;
    return 0;
}

// middle 3-D levels: K sweeps per launch on blocks resident on the CU, the rest (at most one) as a single sweep
int jacobi_blocks(mg_context* c, int level, int* nw) {
    Level& L = c->L[level];
    if (is_slab(c, L) || *nw < 2 || !block_sweeps_ok(c, L)) return 0;
    const JBPlan plan = block_plan(c, L);
    while (*nw >= 2) {
        const int k = up_to(plan.K, *nw);                   // 4 = 2 + 2 rather than 3 + 1
        MG_TRY(launch_jacobi_block(c, L, k, plan.EZ, L.v.rows, L.f.rows, L.v2.rows));
        count_pass(c, level, MG_PATH_BLOCK, 1, k);
        std::swap(L.v, L.v2);
        *nw -= k;
    }
    return 0;
}

// 2-D levels: up to fuse_2d_k sweeps per launch, the rest (at most one) as a single sweep
int jacobi_2d(mg_context* c, int level, int* nw) {
    Level& L = c->L[level];
    if (is_slab(c, L) || !sweeps2d_ok(c, L)) return 0;
    while (*nw >= 2) {
        const int k = up_to(c->fuse_2d_k, *nw);
        MG_TRY(launch_jacobik(c, L, k, L.v.rows, L.f.rows, L.v2.rows));
        count_pass(c, level, MG_PATH_K2D, 1, k);
        std::swap(L.v, L.v2);
        *nw -= k;
    }
    return 0;
}

// Slabs with room for K halo planes ("halo_depth"): K sweeps per pass AND per exchange -- K planes of the iterate travel
// once per pass (the same volume as one plane per sweep) and the march relaxes the neighbours' K - 1 planes next to the
// slab itself, so there is no boundary chain: two launches and one grouped send / receive per K sweeps.  With the
// overlap on, the planes the neighbours wait for are relaxed first (one launch), and travel on the communication
// stream while a second launch relaxes the rest.  (Everything that decides is the same on every rank.)
int jacobi_ksweep_slab(mg_context* c, int level, int* nw) {
    Level& L = c->L[level];
    if (!is_slab(c, L) || *nw < c->fuse_k_slab_min_sweeps || !slab_ksweep_level(c, L)) return 0;
    if (L.cls_halo == 0) MG_TRY(ensure_class_halos(c, L));
    if (L.cls_halo != 1) return 0;
    const int kmax = std::min(std::min(c->fuse_k, 5), L.hd);
    // (a pass on a slab also saves an exchange: two sweeps are worth one)
    auto next_k = [&](int left) { return left < 2 ? 0 : std::max(2, std::min(next_pass(left, kmax), kmax)); };
    const bool lo = c->comm.rank > 0, hi = c->comm.rank + 1 < c->comm.world;
    const int nk = L.g.nk;
    int k = next_k(*nw);
    MG_TRY(exchange_halo(c, L, L.f, nullptr, std::max(1, kmax - 1)));
    MG_TRY(exchange_halo(c, L, L.v, nullptr, k));
    while (k) {
        const int kn = next_k(*nw - k);                     // the pass after this one
        const int e = kn ? kn : c->halo_planes;             // planes of the new iterate the neighbours need next
        const bool split = c->overlap && c->comm_stream && min_slab_rows(L) >= c->overlap_min_rows &&
                           min_slab_rows(L) >= (int64_t)(4 * e + 8) * L.g.plane;
        if (split) {
            const int lob = lo ? e : 0, hib = hi ? e : 0;
            const JK3Range edge{0, lob, nk - hib, nk}, rest{lob, nk - hib, 0, 0};
            MG_TRY(launch_jacobikc(c, L, k, L.v.rows, L.f.rows, L.v2.rows, &edge, e));
            const int edge_tail = c->jk3_tail;
            MG_TRY(fork_to_comm(c));
            MG_TRY(exchange_halo(c, L, L.v2, c->comm_stream, e));
            MG_TRY(launch_jacobikc(c, L, k, L.v.rows, L.f.rows, L.v2.rows, &rest));
            count_pass(c, level, MG_PATH_KSWEEP_SLAB, 2, k, edge_tail + c->jk3_tail);
            MG_TRY(join_comm(c));
        } else {
            MG_TRY(launch_jacobikc(c, L, k, L.v.rows, L.f.rows, L.v2.rows));
            count_pass(c, level, MG_PATH_KSWEEP_SLAB, 1, k, c->jk3_tail);
            MG_TRY(exchange_halo(c, L, L.v2, nullptr, e));
        }
        std::swap(L.v, L.v2);
        *nw -= k;
        k = kn;
    }
    return 0;
}

// whole levels: K sweeps per pass (at least three)
int jacobi_ksweep(mg_context* c, int level, int* nw) {
    Level& L = c->L[level];
    if (is_slab(c, L) || *nw < 3 || !sweepsk_ok(c, L)) return 0;
    const int kmax = sweepsk_max(c, L);
    while (*nw >= 3) {
        const int k = next_pass(*nw, kmax);
        if (k < 3) break;
        MG_TRY(launch_jacobikc(c, L, k, L.v.rows, L.f.rows, L.v2.rows));
        count_pass(c, level, L.cls_escape ? MG_PATH_KSWEEP_ESCAPE : MG_PATH_KSWEEP, 1, k, c->jk3_tail);
        std::swap(L.v, L.v2);
        *nw -= k;
    }
    return 0;
}

// What the pair and single-sweep paths of a level share.
struct PairPlan {
    int64_t S = 0;                      // rows per slice
    int64_t lo_end = 0, hi_begin = 0;   // slices [0, lo_end) and [hi_begin, nslices) hold rows of the first / last owned planes:
                                        // their results are what the neighbours need
    bool overlap = false;               // slabs: the exchanges run on the communication stream beside the interior's sweep
    bool fused = false;                 // two sweeps per pass (mg_jacobi2.hip.h)
    J2Plan plan{};
};

int plan_pairs(mg_context* c, Level& L, int nw, PairPlan* pp) {
    const bool dist = is_slab(c, L);
    pp->S = (int64_t)WAVE * L.R;
    const int64_t hplanes = (int64_t)c->halo_planes * L.g.plane;
    pp->lo_end = std::min(L.nslices, (hplanes + pp->S - 1) / pp->S);
    pp->hi_begin = std::max<int64_t>(pp->lo_end, (L.nloc - hplanes) / pp->S);
    // below a few million rows a sweep is shorter than the extra launches and event hops of the overlapped
    // form: exchange in-stream there
    // (taken alike on every rank: every slab of a distributed level has at least 2^level >= 2 planes)
    const bool two_planes = min_slab_rows(L) >= 2 * hplanes;
    pp->overlap = dist && c->overlap && two_planes && pp->hi_begin > pp->lo_end && c->comm_stream &&
                  min_slab_rows(L) >= c->overlap_min_rows;
    // (the paired pass on slabs is written for one halo plane)
    pp->fused = fused_sweeps_ok(c, L) && (!dist || (c->halo_planes == 1 && two_planes && pp->hi_begin > pp->lo_end));
    if (pp->fused && nw > 1) {
        if (dist) MG_TRY(vec_alloc(c, L, &L.sw));
        pp->plan = jacobi2_plan(c, L, dist, pp->lo_end * pp->S + L.g.plane + L.g.nx + 2);
    }
    return 0;
}

// Two sweeps of a slab in one pass.  The rows of the slices that hold the first / last owned plane need the neighbours'
// once-relaxed planes for their second sweep: the pass leaves them out and parks v1 around them in `sw`, whose halos
// are then exchanged like any iterate's, and the one-sweep kernel finishes those slices.
int jacobi_pair_slab(mg_context* c, int level, const PairPlan& pp, int pair_path) {
    Level& L = c->L[level];
    const J2Plan& plan = pp.plan;
    const int64_t S = pp.S, lo_end = pp.lo_end, hi_begin = pp.hi_begin;
    const bool lo = c->comm.rank > 0, hi = c->comm.rank + 1 < c->comm.world;
    const int64_t st_lo = lo ? lo_end * S : 0, st_hi = hi ? hi_begin * S : INT64_MAX;
    // one sweep from `from` into `to_rows` on the slab's end slices next to a neighbour: the first lo_count, those from hi_from on
    auto sweep_ends = [&](const DVector& from, double* to_rows, int64_t lo_count, int64_t hi_from) {
        EllRequest q = level_op(L, MODE_JACOBI);
        q.x_base = from.base; q.out_rows = to_rows; q.slices = SliceRange::ends_of_slab(L, lo, hi, lo_count, hi_from);
        return launch_ell(c, L, q);
    };
    auto boundary_chain = [&]() -> int {
        MG_TRY(exchange_halo(c, L, L.sw, c->stream));
        MG_TRY(sweep_ends(L.sw, L.v2.rows, lo_end, hi_begin));
        MG_TRY(exchange_halo(c, L, L.v2, c->stream));
        return 0;
    };
    // slices whose once-relaxed values the finishing sweep of the first / last slices reads
    const int64_t reach = L.g.plane + L.g.nx + 2;
    const int64_t lo2 = std::min(L.nslices, (lo_end * S + reach + S - 1) / S);
    const int64_t hi2 = std::max<int64_t>(0, (hi_begin * S - reach) / S);
    if (pp.overlap && c->slab_pair_form == 1 && plan.nseg >= 3) {
        // ("slab_pair_form" 1.)  The two boundary segments of the pass first, alone on the GPU -- launched beside
        // the interior they are dispatched AFTER it, the event hop delays them, and finish late --, then the
        // interior segments on the main stream while the chain runs on the communication stream; the once-
        // relaxed boundary planes come from the pass (`sw`).
        MG_TRY(launch_jacobi2(c, L, plan, 0, plan.nseg - 1, 2, L.v.rows, L.f.rows, L.v2.rows, st_lo, st_hi, L.sw.rows));
        MG_TRY(fork_to_comm(c));
        MG_TRY(launch_jacobi2(c, L, plan, 1, 1, plan.nseg - 2, L.v.rows, L.f.rows, L.v2.rows, st_lo, st_hi, L.sw.rows));
        MG_TRY(on_comm_stream(c, boundary_chain));
        count_pass(c, level, pair_path, 3, 2);                 // two launches of the pass, the boundary chain's
        MG_TRY(join_comm(c));
    } else if (pp.overlap && c->slab_pair_form != 1 && hi2 > lo2) {
        // Everything that waits for the neighbours -- the first sweep of the planes next to them, the exchange of
        // its boundary planes, the second sweep of the first / last slices, the exchange of the result -- runs
        // on the (high-priority) communication stream from the start of the pair and needs nothing from the
        // pass itself: four small operations beside ONE launch of the pass over the whole slab, which stores the
        // second sweep of all other rows.  (Measured on one slab of eight, tools/slab_rank_probe.py: a separate
        // boundary launch of the pass in front costs 0.1 ms of the pair's 0.8; beside the interior launch it
        // is dispatched after it and finishes late.)  The first sweep of those few planes is computed twice.
        MG_TRY(fork_to_comm(c));
        const J2Plan whole = jacobi2_plan(c, L, false, 0);
        MG_TRY(launch_jacobi2(c, L, whole, 0, 1, whole.nseg, L.v.rows, L.f.rows, L.v2.rows, st_lo, st_hi, nullptr));
        MG_TRY(on_comm_stream(c, [&]() -> int {
            MG_TRY(sweep_ends(L.v, L.sw.rows, lo2, hi2));
            return boundary_chain();
        }));
        count_pass(c, level, pair_path, 3, 2);                 // the pass, the first sweep of the boundary planes, the chain's
        MG_TRY(join_comm(c));
    } else {
        MG_TRY(launch_jacobi2(c, L, plan, 0, 1, plan.nseg, L.v.rows, L.f.rows, L.v2.rows, st_lo, st_hi, L.sw.rows));
        MG_TRY(boundary_chain());
        count_pass(c, level, pair_path, 2, 2);                 // the pass, the boundary chain's one-sweep launch
    }
    std::swap(L.v, L.v2);
    return 0;
}

// one sweep of a slab whose exchange overlaps: boundary planes first, then their exchange on the communication stream
// while the interior runs
int jacobi_single_overlapped(mg_context* c, int level, const PairPlan& pp) {
    Level& L = c->L[level];
    EllRequest q = level_op(L, MODE_JACOBI);
    q.slices = SliceRange::ends(L, pp.lo_end, pp.hi_begin);
    MG_TRY(launch_ell(c, L, q));
    MG_TRY(fork_to_comm(c));
    MG_TRY(exchange_halo(c, L, L.v2, c->comm_stream));
    q.slices = SliceRange::of(pp.lo_end, pp.hi_begin - pp.lo_end);
    MG_TRY(launch_ell(c, L, q));
    count_pass(c, level, MG_PATH_SLICE, 2, 1);                   // boundary slices, interior slices
    MG_TRY(join_comm(c));
    std::swap(L.v, L.v2);
    return 0;
}

// what is left: pairs of sweeps where the level takes the two-sweep pass, single sweeps otherwise and for an odd one
int jacobi_pairs_singles(mg_context* c, int level, int nw, const PairPlan& pp) {
    Level& L = c->L[level];
    const bool dist = is_slab(c, L);
    const int pair_path = cls_full(L) && c->fuse_classes ? MG_PATH_PAIR_CLASS : MG_PATH_PAIR_PLAIN;
    const int single_path = sweep1c_ok(c, L) ? MG_PATH_SWEEP1C : MG_PATH_SLICE;     // (launch_ell's choice for a whole level)
    for (int s = 0; s < nw; ++s) {
        if (pp.fused && s + 1 < nw) {
            if (dist) {
                MG_TRY(jacobi_pair_slab(c, level, pp, pair_path));
            } else {
                MG_TRY(launch_jacobi2(c, L, pp.plan, 0, 1, pp.plan.nseg, L.v.rows, L.f.rows, L.v2.rows));
                count_pass(c, level, pair_path, 1, 2);
                std::swap(L.v, L.v2);
            }
            ++s;
        } else if (pp.overlap) {
            MG_TRY(jacobi_single_overlapped(c, level, pp));
        } else {
            MG_TRY(launch_ell(c, L, level_op(L, MODE_JACOBI)));
            count_pass(c, level, single_path, 1, 1);
            std::swap(L.v, L.v2);
            MG_TRY(exchange_halo(c, L, L.v));
        }
    }
    return 0;
}

// small -> block -> 2-D -> slab K-sweep -> whole-level K-sweep -> pairs / singles
int smooth_jacobi(mg_context* c, int level, int nw) {
    Level& L = c->L[level];
    MG_TRY(jacobi_small(c, level, &nw));
    MG_TRY(jacobi_blocks(c, level, &nw));
    MG_TRY(jacobi_2d(c, level, &nw));
    // (planned here, with the sweeps the K-sweep paths may still take: a slab's `sw` is allocated by the first call of two sweeps or more)
    PairPlan pp;
    MG_TRY(plan_pairs(c, L, nw, &pp));
    MG_TRY(jacobi_ksweep_slab(c, level, &nw));
    MG_TRY(jacobi_ksweep(c, level, &nw));
    return jacobi_pairs_singles(c, level, nw, pp);
}
int residual(mg_context* c, int level) {
    Level& L = c->L[level];
    return launch_ell(c, L, level_op(L, MODE_RESIDUAL));
}

// Grid of the coarse planes this rank produces when restricting from `fine`: its own slab if the
// coarse level is distributed, otherwise the planes matching its fine slab inside the replica.
Grid coarse_target_grid(const mg_context* c, const Level& C, const Level& F) {
    Grid g = C.g;
    if (C.replicated && !F.replicated) {
        g.k0 = C.splits[c->comm.rank];
        g.nk = C.splits[c->comm.rank + 1] - g.k0;
        g.lead = (int64_t)g.k0 * g.plane;
    }
    return g;
}

// The Kuhn pattern of the P1 transfers as linear offsets on level L (kuhn_off order; dj = 0 in 2-D).
int kuhn_lin(const mg_context* c, const Level& L, int64_t* lin) {
    const int K = c->dim == 3 ? 15 : 7;
    for (int t = 0; t < K; ++t) {
        const int di = c->dim == 3 ? kuhn_off<3>(t, 0) : kuhn_off<2>(t, 0), dj = c->dim == 3 ? kuhn_off<3>(t, 1) : 0;
        const int dk = c->dim == 3 ? kuhn_off<3>(t, 2) : kuhn_off<2>(t, 2);
        lin[t] = di + (int64_t)dj * L.g.nx + (int64_t)dk * L.g.plane;
    }
    return K;
}

// The P1 transfers and the Galerkin product assume the mesh of poisson.py: a level whose matrix couples a node to anything
// but its Kuhn neighbours (a mesh cut the other way whose zero couplings were kept, P2 rows) is refused.  A pruned matrix
// cannot show how the mesh was cut: the Poisson matrices of both 2-D orientations have the same five-point stencil and pass.
// Levels without a matrix pass.  On slabs the ranks' verdicts are all-reduced (every rank checks the same levels in the same
// order), so all of them refuse together.  Synchronises for int32-column levels and slabs (prepare_cycle runs it before a
// V-cycle is captured).
int check_p1_stencil(mg_context* c, Level& L) {
    if (L.p1_ok < 0) {
        int64_t lin[15];
        const int K = kuhn_lin(c, L, lin);
        auto in = [&](int64_t o) { return std::find(lin, lin + K, o) != lin + K; };
        bool ok = true;
        if (!L.has_matrix || L.mf) {           // (matrix-free diffusion levels: the seven axis offsets, by construction)
        } else if (L.flat) {
            ok = false;
        } else if (L.sdia) {
            for (int t = 1; t < 8; ++t) ok = ok && (L.up[t] == 0 || in(L.up[t]));
        } else if (L.coded) {
            for (int o : L.h_offsets) ok = ok && in(o);
        } else {
            DevTemp d_lin;
            MG_TRY(d_lin.alloc(sizeof(lin)));
            int* flag = reinterpret_cast<int*>(c->partials.get());
            HIP_TRY(hipMemcpyAsync(d_lin.p, lin, sizeof(lin), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), c->stream));
            hipLaunchKernelGGL(p1_pattern_check, dim3(blocks_for(L.nloc, 256)), dim3(256), 0, c->stream, L.cols, L.nloc, L.W, L.R,
                               L.g.lead, d_lin.as<const int64_t>(), K, flag);
            HIP_TRY(hipGetLastError());
            int h = 1;
            HIP_TRY(hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            ok = h == 0;
        }
        if (is_slab(c, L)) {
            // one verdict for every rank: a rank that refused alone would leave the others waiting in the next exchange
            double bad = ok ? 0.0 : 1.0;
            double* d_bad = c->partials;
            HIP_TRY(hipMemcpyAsync(d_bad, &bad, sizeof(double), hipMemcpyHostToDevice, c->stream));
            MG_TRY(allreduce_sum(c, d_bad, 1));
            HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            ok = bad == 0.0;
        }
        L.p1_ok = ok ? 1 : 0;
    }
    if (!L.p1_ok)
        return fail("the P1 transfers need levels whose stencil lies in the Kuhn pattern of the structured simplicial mesh "
                    "(poisson._offsets: squares cut along (1, 1), cubes into six Kuhn simplices); this level couples other nodes");
    return 0;
}

int restrict_to(mg_context* c, int level, int kind) {
    Level& F = c->L[level];
    Level& C = c->L[level - 1];
    if (F.faces != MG_FACES_ALL || C.faces != MG_FACES_ALL) {       // (a single mg_restrict call; cycles are refused before they start)
        if (F.faces != C.faces)
            return fail("levels " + std::to_string(level) + " and " + std::to_string(level - 1) + " were generated with different face sets (" +
                        std::to_string(F.faces) + " and " + std::to_string(C.faces) + "): generate them with one mg_set_diffusion_faces");
        if (kind != MG_RESTRICT_P1_TRANSPOSE)
            return fail("level " + std::to_string(level) + " was generated with the face set " + std::to_string(F.faces) +
                        " (mg_set_diffusion_faces): its no-flux faces need the P1 transfers (MG_RESTRICT_P1_TRANSPOSE)");
        if (c->comm.active()) return fail("levels with a face set need a whole (not slab) handle");
    }
    Grid gc = coarse_target_grid(c, C, F);
    if (kind == MG_RESTRICT_TABLE) {
        if (!c->rtab_count.p) return fail("no restriction table (mg_set_restriction_table)");
        // (the transpose of the P2 prolongation reaches three fine planes: on slabs the residual's halo must have room for them)
        if (is_slab(c, F)) {
            if (F.hd < 3) return fail("the table restriction reaches three fine planes: \"halo_depth\" must be at least 3 on slabs");
            MG_TRY(exchange_halo(c, F, F.v2, nullptr, 3));
        }
        const RestrictTable t{c->rtab_count.as<int>(), c->rtab_off.as<int>(), c->rtab_w.as<double>(), c->rtab_m};
        hipLaunchKernelGGL(restrict_table, grid3(gc, gc.nk), dim3(kPlaneBlock), 0, c->stream, gc, F.g, t, F.v2.base, C.f.base);
    } else if (kind == MG_RESTRICT_P1_TRANSPOSE) {
        MG_TRY(check_p1_stencil(c, F));
        MG_TRY(check_p1_stencil(c, C));
        MG_TRY(exchange_halo(c, F, F.v2));          // (the same fine planes as full weighting)
        if (C.faces != MG_FACES_ALL)                // (3-D whole levels: mg_set_diffusion_faces refuses the others)
            hipLaunchKernelGGL(restrict_p1t_faces, grid3(gc, gc.nk), dim3(kPlaneBlock), 0, c->stream, gc, F.g,
                               free_box(C.faces, gc.nx, gc.ny, gc.nz), F.v2.base, C.f.base);
        else
            with_int_else<2, 3>(c->dim, [&](auto dim) {
                hipLaunchKernelGGL(restrict_p1t<decltype(dim)::value>, grid3(gc, gc.nk), dim3(kPlaneBlock), 0, c->stream, gc, F.g, F.v2.base, C.f.base);
            });
    } else if (kind == MG_RESTRICT_FULL_WEIGHTING) {
        MG_TRY(exchange_halo(c, F, F.v2));
        hipLaunchKernelGGL(restrict_full_weighting, grid3(gc, gc.nk), dim3(kPlaneBlock), 0, c->stream, gc, F.g, F.v2.base,
                           C.f.base);
    } else {
        hipLaunchKernelGGL(restrict_inject, grid3(gc, gc.nk), dim3(kPlaneBlock), 0, c->stream, gc, F.g, F.v2.base, C.f.base);
    }
    HIP_TRY(hipGetLastError());
    if (C.replicated && !F.replicated) MG_TRY(allgather_planes(c, C.splits, C.g.plane, C.f.base));
    return 0;
}

// r = f - A v evaluated at the coarse nodes only and injected (one launch instead of residual + restrict)
int residual_restrict_fused(mg_context* c, int level) {
    Level& F = c->L[level];
    Level& C = c->L[level - 1];
    const Grid gc = coarse_target_grid(c, C, F);
    FusedRestrictArgs a{};
    a.vals = F.vals; a.cols = F.cols; a.codes = F.codes; a.offsets = F.offsets;
    a.x = F.v.base; a.f = F.f.rows; a.fc = C.f.base;
    a.W = F.W; a.R = F.R; a.coded = F.coded ? 1 : 0; a.gc = gc; a.gf = F.g;
    if (F.coded && F.scls && c->class_sweeps) {
        a.coded = 4; a.cls = F.scls; a.s_off = F.s_off; a.s_val = F.s_val; a.s_cnt = F.s_cnt;
    }
    if (F.sdia) {
        a.vals = F.dvals; a.W = F.wu; a.coded = 2; a.mlead = F.mlead;
        for (int t = 0; t < 8; ++t) a.up[t] = F.up[t];
        if (cls_full(F) && c->class_sweeps) {
            a.coded = 3; a.cls = F.cls + F.cls_lead; a.ctab = F.ctab;
        }
    }
    hipLaunchKernelGGL(residual_inject, grid3(gc, gc.nk), dim3(kPlaneBlock), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    if (C.replicated && !F.replicated) MG_TRY(allgather_planes(c, C.splits, C.g.plane, C.f.base));
    return 0;
}

int prolong(mg_context* c, int level, int add) {
    Level& F = c->L[level];
    Level& C = c->L[level - 1];
    if (F.faces != MG_FACES_ALL || C.faces != MG_FACES_ALL) {       // (a single mg_prolong call; cycles are refused before they start)
        if (F.faces != C.faces)
            return fail("levels " + std::to_string(level) + " and " + std::to_string(level - 1) + " were generated with different face sets (" +
                        std::to_string(F.faces) + " and " + std::to_string(C.faces) + "): generate them with one mg_set_diffusion_faces");
        if (!c->p1_prolong)
            return fail("level " + std::to_string(level) + " was generated with the face set " + std::to_string(F.faces) +
                        " (mg_set_diffusion_faces): its no-flux faces need the P1 transfers (mg_set_prolongation_p1)");
    }
    const bool keep = !add || c->keep_err;
    if (keep) MG_TRY(vec_alloc(c, F, &F.err));
    double* const err = keep ? F.err.base : nullptr;        // (kept: the prolonged coarse iterate goes there as well)
    if (c->p1_prolong) {
        // the coarse planes K and K + 1, as the Q1 interpolation reads them
        MG_TRY(check_p1_stencil(c, F));
        MG_TRY(check_p1_stencil(c, C));
        const dim3 grid = grid3(F.g, F.g.nk), blk(kPlaneBlock);
        with_add_keep(add, keep, [&](auto ad, auto kp) {
            hipLaunchKernelGGL((prolong_p1<decltype(ad)::value, decltype(kp)::value>), grid, blk, 0, c->stream, C.g, F.g, C.v.base, F.v.base, err);
        });
        HIP_TRY(hipGetLastError());
        if (add) MG_TRY(exchange_halo(c, F, F.v));
        return 0;
    }
    if (c->ptab_count.p) {
        if (is_slab(c, F) && c->halo_planes < 2)
            return fail("the table prolongation reaches two coarse planes: halo_planes must be 2 on slabs");
        const ProlongTable t{c->ptab_count.as<int>(), c->ptab_off.as<int>(), c->ptab_w.as<double>()};
        const dim3 grid = grid3(F.g, F.g.nk), blk(kPlaneBlock);
        with_add_keep(add, keep, [&](auto ad, auto kp) {
            hipLaunchKernelGGL((prolong_table<decltype(ad)::value, decltype(kp)::value>), grid, blk, 0, c->stream, C.g, F.g, t, C.v.base, F.v.base, err);
        });
        HIP_TRY(hipGetLastError());
        if (add) MG_TRY(exchange_halo(c, F, F.v));
        return 0;
    }
    // one thread per pair of fine nodes along x
    const int64_t pairs = (int64_t)((F.g.nx + 1) / 2) * F.g.ny;
    const dim3 grid((unsigned)((pairs + kPlaneBlock - 1) / kPlaneBlock), (unsigned)F.g.nk, 1u);
    with_add_keep(add, keep, [&](auto ad, auto kp) {
        hipLaunchKernelGGL((prolong_correct<decltype(ad)::value, decltype(kp)::value>), grid, dim3(kPlaneBlock), 0, c->stream, C.g, F.g, C.v.base, F.v.base, err);
    });
    HIP_TRY(hipGetLastError());
    if (add) MG_TRY(exchange_halo(c, F, F.v));
    return 0;
}

// Zeroes `count` doubles at `p` on the handle's stream.  Inside a captured V-cycle (vcycle_graphed) a kernel does it: with
// memset nodes, a cycle replayed from torch.autograd's backward thread gave other results than the eager launches on
// hierarchies of four and more levels -- the same key, the same addresses; with kernel nodes it
// is bit-identical.
int zero_doubles(mg_context* c, double* p, size_t count) {
    if (c->capturing && count > 0) {
        const unsigned nb = (unsigned)std::min<size_t>((count + 4 * BLOCK - 1) / (4 * BLOCK), (size_t)8 * std::max(1, c->prop.multiProcessorCount));
        hipLaunchKernelGGL(fill_zero, dim3(std::max(1u, nb)), dim3(BLOCK), 0, c->stream, p, (int64_t)count);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    HIP_TRY(hipMemsetAsync(p, 0, count * sizeof(double), c->stream));
    return 0;
}

int zero_vec(mg_context* c, const Level& L, DVector& v) { return zero_doubles(c, v.base, (size_t)L.xlen); }

// sum over owned rows of x.y on the device -> c->scalars[slot]; all-reduced over slabs
int dot_device(mg_context* c, const Level& L, const double* x_rows, const double* y_rows, int slot) {
    const int np = (int)std::min<int64_t>(kMaxParts, std::max<int64_t>(1, (L.nloc + 2 * BLOCK - 1) / (2 * BLOCK)));
    hipLaunchKernelGGL(dot_partial, dim3(np), dim3(BLOCK), 0, c->stream, x_rows, y_rows, L.nloc, c->partials);
    hipLaunchKernelGGL(reduce_partials, dim3(1), dim3(BLOCK), 0, c->stream, c->partials, np, c->scalars + slot);
    HIP_TRY(hipGetLastError());
    if (!L.replicated) MG_TRY(allreduce_sum(c, c->scalars + slot, 1));
    return 0;
}

int norm2(mg_context* c, const Level& L, const double* x_rows, double* out) {
    MG_TRY(dot_device(c, L, x_rows, x_rows, 0));
    HIP_TRY(hipMemcpyAsync(c->h_scalars, c->scalars, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = std::sqrt(c->h_scalars[0]);
    return 0;
}

// ---- Chebyshev smoother: interval per level -------------------------------------------------------------------------------
// Largest eigenvalue of the symmetric tridiagonal matrix (diagonal d, off-diagonal e) by bisection on Sturm counts
double tridiag_max_eig(const std::vector<double>& d, const std::vector<double>& e) {
    const int n = (int)d.size();
    double lo = 1e300, hi = -1e300;
    for (int i = 0; i < n; ++i) {
        const double r = (i > 0 ? std::fabs(e[(size_t)i - 1]) : 0.0) + (i + 1 < n ? std::fabs(e[(size_t)i]) : 0.0);
        lo = std::min(lo, d[(size_t)i] - r);
        hi = std::max(hi, d[(size_t)i] + r);
    }
    auto below = [&](double x) {            // eigenvalues < x
        int k = 0;
        double q = d[0] - x;
        if (q < 0.0) ++k;
        for (int i = 1; i < n; ++i) {
            q = d[(size_t)i] - x - e[(size_t)i - 1] * e[(size_t)i - 1] / (q != 0.0 ? q : 1e-300);
            if (q < 0.0) ++k;
        }
        return k;
    };
    for (int it = 0; it < 2000; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (!(mid > lo && mid < hi)) break;
        if (below(mid) < n) lo = mid; else hi = mid;
    }
    return hi;
}

// lambda_max(D^-1 A) of one level: cheb_eig_steps steps of Jacobi-preconditioned CG (Lanczos) from a start vector that hashes
// each node's global lexicographic index, then the largest eigenvalue of the CG tridiagonal matrix on the host.  Four temporary
// vectors of the level's layout (freed on return: mg_memory_bytes does not change); dot products are the fixed-order partial
// sums of dot_device, all-reduced over slabs, so that every rank gets the same bits.  Synchronises: never inside a capture.
int cheb_estimate(mg_context* c, int level) {
    Level& L = c->L[level];
    // (slabs: each rank tested its own rows, so the refusal is voted before the first collective -- every rank refuses
    //  together, none waits in an all-reduce for a rank that has left)
    bool asym = L.rep_sym == 0;
    if (is_slab(c, L)) {
        c->h_scalars[0] = asym ? 1.0 : 0.0;
        HIP_TRY(hipMemcpyAsync(c->scalars, c->h_scalars, sizeof(double), hipMemcpyHostToDevice, c->stream));
        MG_TRY(allreduce_sum(c, c->scalars, 1));
        HIP_TRY(hipMemcpyAsync(c->h_scalars, c->scalars, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        asym = c->h_scalars[0] != 0.0;
    }
    if (asym)
        return fail("Chebyshev smoother: level " + std::to_string(level) +
                    " is not symmetric (mg_level_storage), so CG cannot estimate its spectrum: set its interval with "
                    "mg_set_chebyshev_bounds");
    const int64_t vt = (vec_total(L) + 31) / 32 * 32;         // (each vector 256-byte aligned, like hipMalloc's)
    DevTemp tmp;
    MG_TRY(tmp.alloc((size_t)(4 * vt) * sizeof(double)));
    HIP_TRY(hipMemsetAsync(tmp.p, 0, (size_t)(4 * vt) * sizeof(double), c->stream));
    c->cheb_peak_bytes = 4 * vt * (int64_t)sizeof(double);
    double* const raw = tmp.as<double>();
    DVector p;                  // (a view into tmp: it owns nothing)
    p.base = raw + vec_front(L); p.rows = p.base + L.g.lead;
    double* const r = raw + vt + vec_front(L) + L.g.lead;
    double* const z = raw + 2 * vt + vec_front(L) + L.g.lead;
    double* const q = raw + 3 * vt + vec_front(L) + L.g.lead;
    const int64_t n = L.nloc;
    // (a matrix-free level keeps no 1 / diagonal: the estimate rebuilds it from kappa for as long as it runs)
    DevTemp mf_dinv;
    const double* dinv = L.dinv;
    if (L.mf) {
        MG_TRY(mf_dinv.alloc((size_t)n * sizeof(double)));
        c->cheb_peak_bytes += n * (int64_t)sizeof(double);
        MG_TRY(launch_diffusion_rhs(c, L, L.kappa, nullptr, mf_dinv.as<double>()));
        dinv = mf_dinv.as<const double>();
    }
    const dim3 grid((unsigned)std::min<int64_t>(4096, std::max<int64_t>(1, (n + 255) / 256))), blk(256);
    auto scalar = [&](const double* x, const double* y, double* out) -> int {
        MG_TRY(dot_device(c, L, x, y, 0));
        HIP_TRY(hipMemcpyAsync(c->h_scalars, c->scalars, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        *out = c->h_scalars[0];
        return 0;
    };
    hipLaunchKernelGGL(cheb_start, grid, blk, 0, c->stream, r, z, p.rows, dinv, n, L.row0);
    HIP_TRY(hipGetLastError());
    double rz = 0.0;
    MG_TRY(scalar(r, z, &rz));
    std::vector<double> al, be;
    if (rz > 0.0 && std::isfinite(rz)) {
        for (int j = 0; j < c->cheb_eig_steps; ++j) {
            MG_TRY(exchange_halo(c, L, p));
            MG_TRY(launch_ell(c, L, {.mode = MODE_SPMV, .x_base = p.base, .out_rows = q}));
            double pq = 0.0;
            MG_TRY(scalar(p.rows, q, &pq));
            if (!(pq > 0.0) || !std::isfinite(pq)) break;          // breakdown: A not positive definite on the Krylov space
            const double alpha = rz / pq;
            al.push_back(alpha);
            hipLaunchKernelGGL(cheb_cg_update, grid, blk, 0, c->stream, r, z, q, dinv, n, alpha);
            HIP_TRY(hipGetLastError());
            double rz_new = 0.0;
            MG_TRY(scalar(r, z, &rz_new));
            if (!(rz_new > 0.0) || !std::isfinite(rz_new) || j + 1 == c->cheb_eig_steps) break;
            const double beta = rz_new / rz;
            be.push_back(beta);
            rz = rz_new;
            hipLaunchKernelGGL(cheb_cg_direction, grid, blk, 0, c->stream, p.rows, z, n, beta);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int m = (int)al.size();
    if (m < 2)
        return fail("Chebyshev smoother: CG on level " + std::to_string(level) + " broke down after " + std::to_string(m) +
                    " step(s), so its spectrum cannot be estimated: set its interval with mg_set_chebyshev_bounds");
    // Lanczos matrix of the CG coefficients: T_jj = 1/alpha_j + beta_{j-1}/alpha_{j-1}, T_{j,j+1} = sqrt(beta_j)/alpha_j
    std::vector<double> d((size_t)m), e((size_t)m - 1);
    for (int j = 0; j < m; ++j) {
        d[(size_t)j] = 1.0 / al[(size_t)j] + (j > 0 ? be[(size_t)j - 1] / al[(size_t)j - 1] : 0.0);
        if (j + 1 < m) e[(size_t)j] = std::sqrt(be[(size_t)j]) / al[(size_t)j];
    }
    L.cheb_lmax_est = tridiag_max_eig(d, e);
    L.cheb_est_ok = true;
    return 0;
}

// The interval [lo, hi] the Chebyshev smoother damps on `level`: the caller's (mg_set_chebyshev_bounds), else
// hi = upper_factor * the estimate and lo = hi / lower_ratio.  Runs the estimate when it is missing -- not inside a capture.
int cheb_interval(mg_context* c, int level, double* lo, double* hi) {
    Level& L = c->L[level];
    if (L.cheb_user_lmax > 0.0) {
        *hi = L.cheb_user_lmax;
        *lo = L.cheb_user_lmin > 0.0 ? L.cheb_user_lmin : L.cheb_user_lmax / c->cheb_lower_ratio;
        return 0;
    }
    if (!L.cheb_est_ok) {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        HIP_TRY(hipStreamIsCapturing(c->stream, &st));
        if (st != hipStreamCaptureStatusNone)
            return fail("Chebyshev smoother: the estimate of level " + std::to_string(level) + " is missing inside a capture");
        MG_TRY(cheb_estimate(c, level));
    }
    *hi = c->cheb_upper_factor * L.cheb_lmax_est;
    *lo = *hi / c->cheb_lower_ratio;
    return 0;
}

void free_direct(mg_context* c) { c->direct = DirectSolver{}; }

// ---- insulated bodies: levels with no Dirichlet node (mg_set_diffusion_insulated) -----------------------------------------
// A generated level with the face set 0 and neither a reaction nor a Robin diagonal has zero row sums: its null space is the
// constants.  A cycle from `level` is singular when its levels are (face_set_refusals: they share one face set).
bool level_singular(const Level& L) { return L.set && L.faces == 0 && !L.react && !L.robin; }
bool cycle_singular(const mg_context* c, int level) {
    for (int l = 0; l <= level; ++l)
        if (!level_singular(c->L[l])) return false;
    return true;
}

// what has no projected form (batched solves, eigenpairs, FMG) refuses a singular cycle by name, before anything is launched
int singular_refusal(const mg_context* c, const std::string& who, int level) {
    if (!cycle_singular(c, level)) return 0;
    return fail(who + ": the levels are those of an insulated body with neither a reaction nor a Robin term (mg_set_diffusion_insulated): "
                "the operator is singular, and only mg_pcg, mg_vcycle and the single-level operations handle its null space");
}

// the partial sums of a mean removal over n rows; an allocation: not inside a capture (prepare_cycle, fcg_start)
// (sized for the largest level that is set, so a cycle from a higher level finds it in place; should it grow all the same,
// the captured cycles that hold its address go first)
void drop_graphs(mg_context* c);
int ns_workspace(mg_context* c, int64_t n) {
    for (int l = 0; l < c->nlev; ++l)
        if (c->L[l].set) n = std::max<int64_t>(n, c->L[l].nloc);
    const size_t need = (size_t)ns_blocks(n) + 1;
    if (c->ns_part.count() >= need) return 0;
    drop_graphs(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    return c->ns_part.alloc(c, need);
}

// x -= u * inv_denom * sum(w x) over n rows (w null: sum(x); u null: the constant), mg_nullspace.hip.h; x, w and u are
// 16-byte aligned row pointers.  Three kernel launches and nothing else, so a captured cycle gains kernel nodes only.
int ns_remove(mg_context* c, double* x, const double* w, const double* u, int64_t n, double inv_denom, double* mean_out = nullptr) {
    for (const double* v : {(const double*)x, w, u})
        if (reinterpret_cast<uintptr_t>(v) % 16) return fail("mean removal: misaligned vector");
    const int64_t nb = ns_blocks(n);
    if ((int64_t)c->ns_part.count() < nb + 1) return fail("mean removal: no workspace");
    double* const part = c->ns_part;
    hipLaunchKernelGGL(ns_partial, dim3((unsigned)nb), dim3(BLOCK), 0, c->stream, (const double*)x, w, n, part);
    hipLaunchKernelGGL(fcg_fold, dim3(1), dim3(BLOCK), 0, c->stream, (const double*)part, nb, 1, part + nb);
    hipLaunchKernelGGL(ns_subtract, dim3((unsigned)nb), dim3(BLOCK), 0, c->stream, x, u, n, (const double*)(part + nb), inv_denom, mean_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_reaction_diag(mg_context* c, const double* w, double* out, int N);

// w = the lumped mass of rho = 1 on the all-free grid of L (reaction_diag of ones) and 1 / (w.1); kept until a level of
// another size asks.  Allocates and synchronises: not inside a capture.
int ns_weights(mg_context* c, const Level& L) {
    const int64_t n1 = (int64_t)L.N + 1;
    if (L.N < 1 || L.n_global != n1 * n1 * n1 || L.g.lead != 0 || L.xlen != L.nloc)
        return fail("insulated solve: the level is no whole grid of (N + 1)^3 nodes");
    MG_TRY(ns_workspace(c, L.nloc));
    if (c->ns_w && c->ns_N == L.N) return 0;
    c->ns_N = 0;
    const size_t cells = (size_t)L.N * L.N * L.N;
    DevTemp ones;
    MG_TRY(ones.alloc(cells * 8));
    std::vector<double> h(cells, 1.0);
    HIP_TRY(hipMemcpyAsync(ones.p, h.data(), cells * 8, hipMemcpyHostToDevice, c->stream));
    MG_TRY(c->ns_w.alloc(c, (size_t)L.nloc));
    MG_TRY(launch_reaction_diag(c, ones.as<const double>(), c->ns_w, L.N));
    const int64_t nb = ns_blocks(L.nloc);
    double* const part = c->ns_part;
    hipLaunchKernelGGL(ns_partial, dim3((unsigned)nb), dim3(BLOCK), 0, c->stream, (const double*)c->ns_w, (const double*)nullptr, (int64_t)L.nloc, part);
    hipLaunchKernelGGL(fcg_fold, dim3(1), dim3(BLOCK), 0, c->stream, (const double*)part, nb, 1, part + nb);
    HIP_TRY(hipGetLastError());
    double s = 0.0;
    HIP_TRY(hipMemcpyAsync(&s, part + nb, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!(s > 0.0)) return fail("insulated solve: the lumped mass does not sum to a positive number");
    c->ns_inv_s = 1.0 / s;
    c->ns_N = L.N;
    return 0;
}

EllView ell_view(const Level& L) {
    EllView e{};
    e.vals = L.vals; e.cols = L.cols; e.codes = L.codes; e.offsets = L.offsets;
    e.W = L.W; e.R = L.R; e.coded = L.coded ? 1 : 0; e.n = L.nloc;
    return e;
}

// Factor the coarsest level once: T_k = (D_k - L_k T_{k-1} U_{k-1})^-1 for every block of planes.
int build_direct(mg_context* c) {
    DirectSolver& d = c->direct;
    d.tried = true;
    Level& L = c->L[0];
    MG_TRY(need_stored_rows(c, L, "the coarsest solve"));
    if (!c->use_direct || L.flat || L.g.lead != 0) return 0;
    const int64_t plane = L.g.plane;
    const int nz = L.g.nz;
    // planes per block: at least "direct_block_rows" rows (a solve is 3 dependent launches per block, each of them a few
    // microseconds whatever the block's size: fewer, larger blocks while the dense inverses stay small), and at least as many
    // planes as the stencil reaches (P2 rows reach two: the blocks must couple to their neighbours only)
    int64_t reach = 1;
    if (L.coded && L.ntable > 0) {
        std::vector<int> offs(256);
        HIP_TRY(hipMemcpy(offs.data(), L.offsets, 256 * sizeof(int), hipMemcpyDeviceToHost));
        for (int t = 0; t < L.ntable; ++t) reach = std::max<int64_t>(reach, (std::llabs((long long)offs[t]) + plane / 2) / plane);
    }
    int64_t G = std::max<int64_t>(reach, std::min<int64_t>(nz, (c->direct_block_rows + plane - 1) / plane));
    while (G > reach && G > 1 && G * plane > 2304) --G;               // (the dense blocks' size limit below)
    const int64_t p = G * plane;
    const int64_t nb = (nz + G - 1) / G;
    if (p > 2304 || nb * p * p * 8 > ((int64_t)3 << 29)) return 0;     // too large to store densely: PCG
    d.g.n = L.nloc; d.g.p = (int)p; d.g.plane = (int)plane; d.g.nb = (int)nb; d.g.W = L.W;
    // a singular level 0 is factorised with node 0 pinned: the rest of the operator is regular, and for a consistent
    // right-hand side the solve is exact in every row, node 0's included (mg_nullspace.hip.h; DESIGN.md, "Insulated bodies")
    d.pinned = level_singular(L);
    const size_t pw = (size_t)nb * p * L.W, np = (size_t)nb * p, pp = (size_t)p * p;
    DevTemp A_t, B_t, P_t, status_t;                       // A: block being inverted, B: row panel, P: pivot block
    int rc = [&]() -> int {                                // (a lambda: any failure must still reach free_direct below)
        MG_TRY(d.T.alloc(c, np * p));
        MG_TRY(d.lcol.alloc(c, pw)); MG_TRY(d.ucol.alloc(c, pw));
        MG_TRY(d.lval.alloc(c, pw)); MG_TRY(d.uval.alloc(c, pw));
        MG_TRY(d.y.alloc(c, np)); MG_TRY(d.x.alloc(c, np)); MG_TRY(d.w.alloc(c, (size_t)p));
        MG_TRY(A_t.alloc(pp * 8));
        MG_TRY(B_t.alloc((size_t)GJ_NB * p * 8));
        MG_TRY(P_t.alloc((size_t)GJ_NB * GJ_NB * 8));
        MG_TRY(status_t.alloc(sizeof(int)));
        double *const A = A_t.as<double>(), *const B = B_t.as<double>(), *const P = P_t.as<double>();
        int* const d_status = status_t.as<int>();
        HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(int), c->stream));
        const EllView e = ell_view(L);
        const dim3 rows_grid(blocks_for(p, 128)), rows_blk(128);
        const dim3 gj_blk(256);
        for (int k = 0; k < (int)nb; ++k) {
            const size_t ko = (size_t)k * p * L.W;
            HIP_TRY(hipMemsetAsync(A, 0, pp * 8, c->stream));
            hipLaunchKernelGGL(bt_extract_dense, rows_grid, rows_blk, 0, c->stream, e, d.g, k, A, d_status);
            if (k == 0 && d.pinned) hipLaunchKernelGGL(ns_pin_dense, rows_grid, rows_blk, 0, c->stream, A, (int)p);
            hipLaunchKernelGGL(bt_extract_coupling, rows_grid, rows_blk, 0, c->stream, e, d.g, k, d.lcol + ko, d.lval + ko,
                               d.ucol + ko, d.uval + ko);
            if (k > 0) {
                const size_t po = (size_t)(k - 1) * p * L.W;
                hipLaunchKernelGGL(bt_schur_update, rows_grid, rows_blk, 0, c->stream, d.g, d.lcol + ko, d.lval + ko,
                                   d.ucol + po, d.uval + po, d.T + (size_t)(k - 1) * pp, A);
            }
            for (int k0 = 0; k0 < (int)p; k0 += GJ_NB) {
                const int nbk = std::min<int>(GJ_NB, (int)p - k0);
                hipLaunchKernelGGL(gj_pivot_block, dim3(1), gj_blk, 0, c->stream, (int)p, k0, nbk, A, P);
                hipLaunchKernelGGL(gj_row_panel, dim3(blocks_for(p, 256), (unsigned)nbk), gj_blk, 0, c->stream, (int)p, k0,
                                   nbk, A, P, B);
                hipLaunchKernelGGL(gj_trailing, dim3(blocks_for(p, 256), (unsigned)p), gj_blk, 0, c->stream, (int)p, k0, nbk,
                                   A, B);
                hipLaunchKernelGGL(gj_finish, dim3(blocks_for(p, 128)), dim3(128), 0, c->stream, (int)p, k0, nbk, A, P, B);
            }
            if (k == 0 && d.pinned) hipLaunchKernelGGL(ns_unpin_inverse, dim3(1), dim3(64), 0, c->stream, A);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(d.T + (size_t)k * pp, A, pp * 8, hipMemcpyDeviceToDevice, c->stream));
        }
        int status = 0;
        HIP_TRY(hipMemcpyAsync(&status, d_status, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        d.ok = status == 0;
        return 0;
    }();
    if (rc || !d.ok) { free_direct(c); d.tried = true; }
    return rc;
}

int direct_solve(mg_context* c);

// The factorisation uses no pivoting, which is safe for the SPD / M-matrices this path is meant for but not
// for an arbitrary hand-off: solve once against a known right-hand side (all ones) and keep the direct
// solver only if the residual is at round-off; otherwise the coarsest level falls back to PCG.
int validate_direct(mg_context* c) {
    DirectSolver& d = c->direct;
    if (!d.ok) return 0;
    Level& L = c->L[0];
    DevTemp saved_t;
    MG_TRY(saved_t.alloc((size_t)L.xlen * 8));
    double* const saved = saved_t.as<double>();
    int rc = [&]() -> int {                                // (a lambda: a failed check must still drop the factorisation)
        HIP_TRY(hipMemcpyAsync(saved, L.f.base, (size_t)L.xlen * 8, hipMemcpyDeviceToDevice, c->stream));
        std::vector<double> ones((size_t)L.nloc, 1.0);
        double fn = std::sqrt((double)L.nloc);
        if (d.pinned) {                             // a singular level solves consistent loads only: a ramp with sum zero
            double ff = 0.0;
            for (int64_t i = 0; i < L.nloc; ++i) {
                ones[(size_t)i] = (double)i - 0.5 * (double)(L.nloc - 1);
                ff += ones[(size_t)i] * ones[(size_t)i];
            }
            fn = std::sqrt(ff);
        }
        HIP_TRY(hipMemcpyAsync(L.f.rows, ones.data(), (size_t)L.nloc * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        MG_TRY(direct_solve(c));
        MG_TRY(residual(c, 0));
        double rn = 0.0;
        MG_TRY(norm2(c, L, L.v2.rows, &rn));
        const double rel = rn / fn;
        if (!(rel <= 1e-9)) d.ok = false;           // also catches NaN
        HIP_TRY(hipMemcpyAsync(L.f.base, saved, (size_t)L.xlen * 8, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return 0;
    }();
    if (rc || !d.ok) { free_direct(c); d.tried = true; }
    return rc;
}

int direct_solve(mg_context* c) {
    DirectSolver& d = c->direct;
    Level& L = c->L[0];
    const int p = d.g.p, nb = d.g.nb;
    const size_t pp = (size_t)p * p, pw = (size_t)p * d.g.W;
    const int64_t first = std::min<int64_t>(L.nloc, p);
    MG_TRY(zero_doubles(c, d.y, (size_t)p));
    HIP_TRY(hipMemcpyAsync(d.y, L.f.rows, (size_t)first * 8, hipMemcpyDeviceToDevice, c->stream));
    const dim3 wave_grid(blocks_for(p, WAVES_PER_BLOCK)), blk(BLOCK);
    // wide rows (P2: ~20 couplings into the previous block per row): T_{k-1} y_{k-1} once, then the sparse part -- 19 + 3 us
    // per block instead of 136 us at p = 2178; narrow rows keep the single launch (fewer launches on the 2-D levels)
    const bool two_step = d.g.W > 12;
    for (int k = 1; k < nb; ++k) {
        if (two_step) {
            hipLaunchKernelGGL(bt_matvec, wave_grid, blk, 0, c->stream, p, d.T + (size_t)(k - 1) * pp, d.y + (size_t)(k - 1) * p, d.w);
            hipLaunchKernelGGL(bt_forward_sparse, dim3(blocks_for(p, 128)), dim3(128), 0, c->stream, d.g, k, d.lcol + k * pw,
                               d.lval + k * pw, d.w, L.f.rows, d.y);
        } else {
            hipLaunchKernelGGL(bt_forward, wave_grid, blk, 0, c->stream, d.g, k, d.lcol + k * pw, d.lval + k * pw,
                               d.T + (size_t)(k - 1) * pp, L.f.rows, d.y);
        }
    }
    for (int k = nb - 1; k >= 0; --k) {
        hipLaunchKernelGGL(bt_backward_rhs, dim3(blocks_for(p, 128)), dim3(128), 0, c->stream, d.g, k, d.ucol + k * pw,
                           d.uval + k * pw, d.y, d.x, d.w);
        hipLaunchKernelGGL(bt_backward, wave_grid, blk, 0, c->stream, d.g, k, d.T + (size_t)k * pp, d.w, d.x, L.v.rows);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int pcg_solve(mg_context* c, int* iters_out, double* rel_out);

// Coarsest level: v = A^-1 f, standing in for the reference's exact spsolve (multigrid.py:239-241):
// the block-tridiagonal LU where the level allows it, otherwise Jacobi-preconditioned CG.
int coarse_solve_regular(mg_context* c, int* iters_out, double* rel_out) {
    if (!c->direct.tried) { MG_TRY(build_direct(c)); MG_TRY(validate_direct(c)); }
    if (c->direct.ok) {
        if (iters_out) *iters_out = 0;
        if (rel_out) *rel_out = 0.0;
        return direct_solve(c);
    }
    return pcg_solve(c, iters_out, rel_out);
}

// A singular level 0 (level_singular): the right-hand side is made mean-free first -- restricted residuals are, up to
// rounding, because the P1 embedding reproduces constants when every node is free -- and so is the result, which makes it
// K0^+ f: the pinned factorisation (build_direct) or the coarse CG solve the consistent system exactly.
int coarse_solve(mg_context* c, int* iters_out, double* rel_out) {
    Level& L = c->L[0];
    if (!level_singular(L)) return coarse_solve_regular(c, iters_out, rel_out);
    if (!c->capturing) MG_TRY(ns_workspace(c, L.nloc));
    const double inv_n = 1.0 / (double)L.nloc;
    MG_TRY(ns_remove(c, L.f.rows, nullptr, nullptr, L.nloc, inv_n));
    MG_TRY(coarse_solve_regular(c, iters_out, rel_out));
    return ns_remove(c, L.v.rows, nullptr, nullptr, L.nloc, inv_n);
}

// Jacobi-preconditioned CG run to `coarse_rtol`.  Iterations are enqueued in batches; only the 4-byte
// convergence flag crosses to the host between batches.
int pcg_solve(mg_context* c, int* iters_out, double* rel_out) {
    Level& L = c->L[0];
    if (L.g.lead != 0) return fail("coarsest level must not be distributed");
    const int64_t n = L.nloc;
    if (!c->pcg_r) {
        MG_TRY(c->pcg_r.alloc(c, (size_t)n + 4));
        MG_TRY(c->pcg_z.alloc(c, (size_t)n + 4));
        MG_TRY(c->pcg_q.alloc(c, (size_t)n + 4));
        MG_TRY(vec_alloc(c, L, &c->pcg_p));
        c->pcg_parts = (int)std::min<int64_t>(512, std::max<int64_t>(1, (n + BLOCK - 1) / BLOCK));
        c->pcg_parts_a = (int)std::max<unsigned>(blocks_for(L.nslices, WAVES_PER_BLOCK), (unsigned)c->pcg_parts);
        MG_TRY(c->pcg_part_a.alloc(c, (size_t)c->pcg_parts_a));
        MG_TRY(c->pcg_part_b.alloc(c, (size_t)2 * c->pcg_parts));
    }
    PcgArgs a{};
    a.x = L.v.rows; a.r = c->pcg_r; a.z = c->pcg_z; a.p = c->pcg_p.rows; a.q = c->pcg_q;
    a.b = L.f.rows; a.dinv = L.dinv; a.part_a = c->pcg_part_a; a.part_b = c->pcg_part_b;
    a.nparts = c->pcg_parts; a.sc = c->scalars; a.done = c->done; a.n = n;
    a.rtol2 = c->coarse_rtol * c->coarse_rtol;
    const dim3 grid(c->pcg_parts), blk(BLOCK);
    hipLaunchKernelGGL(pcg_init, grid, blk, 0, c->stream, a);
    hipLaunchKernelGGL(pcg_init_finish, dim3(1), blk, 0, c->stream, a);
    int it = 0;
    int batch = c->pcg_predict > 0 ? c->pcg_predict : c->pcg_chunk;
    int* h_done = reinterpret_cast<int*>(c->h_scalars + 8);
    for (;;) {
        batch = std::min(batch, c->coarse_maxit - it);
        for (int b = 0; b < batch; ++b) {
            unsigned np_spmv = 0;
            MG_TRY(launch_ell(c, L, {.mode = MODE_SPMV, .dot = true, .x_base = c->pcg_p.base, .out_rows = c->pcg_q, .partials = c->pcg_part_a,
                                     .done = c->done, .grid_out = &np_spmv}));
            hipLaunchKernelGGL(pcg_update, grid, blk, 0, c->stream, a, (int)np_spmv, it + b);
            hipLaunchKernelGGL(pcg_direction, grid, blk, 0, c->stream, a, it + b);
        }
        it += batch;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_done, c->done, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(c->h_scalars, c->scalars, 8 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (*h_done || it >= c->coarse_maxit) break;
        batch = c->pcg_chunk;
    }
    const int used = (int)c->h_scalars[5];
    const double bb = c->h_scalars[3], rr = c->h_scalars[2];
    const double rel = bb > 0.0 ? std::sqrt(rr / bb) : 0.0;
    if (iters_out) *iters_out = used;
    if (rel_out) *rel_out = rel;
    if (!*h_done)
        return fail("coarse solve did not converge: " + std::to_string(used) + " iterations, relative residual " +
                    std::to_string(rel));
    c->pcg_predict = used;
    return 0;
}

// One V(mu1, mu2) cycle on `level` (V_cycle_scheme, multigrid.py:231-268): pre-smooth, residual,
// restrict, recurse from a zero guess, interpolate + correct, post-smooth; exact solve on level 0.
int vcycle(mg_context* c, int level) {
    if (level == 0) return coarse_solve(c, nullptr, nullptr);
    Level& C = c->L[level - 1];
    MG_TRY(smooth(c, level, c->mu1));
    if (c->restriction == MG_RESTRICT_INJECTION && c->fuse_restrict && !c->L[level].mf) {
        MG_TRY(residual_restrict_fused(c, level));
    } else {
        MG_TRY(residual(c, level));
        MG_TRY(restrict_to(c, level, c->restriction));
    }
    MG_TRY(zero_vec(c, C, C.v));
    MG_TRY(vcycle(c, level - 1));
    MG_TRY(prolong(c, level, 1));
    MG_TRY(smooth(c, level, c->mu2));
    return 0;
}

void drop_graphs(mg_context* c) {
    // (mg_vcycle and mg_fmg enqueue replays without a host synchronisation: an executable graph is not destroyed under a
    //  launch that is still in flight.  Rare -- the cache is full, or the levels or the tuning change)
    if (!c->graphs.empty() && c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& g : c->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    c->graphs.clear();
}

// A V-cycle is a fixed sequence of launches once the coarsest solve is the direct one (no host round
// trip), so it is captured into a hipGraph the first time and replayed afterwards: the launch-bound coarse
// levels then cost a kernel boundary instead of a host launch each.  The Jacobi ping-pong swaps the
// MG_VEC_V buffers mu1+mu2 times per level; the captured pointer state is part of the cache key and the
// swaps are re-applied on the host after a replay.
// Everything a V-cycle from `level` builds or allocates on first use (the direct coarsest solve and its validation, the
// colouring checks, the parked-sweep and error vectors): afterwards a cycle -- and its capture -- only enqueues work.
// Levels generated with a face set (mg_set_diffusion_faces) run cycles with the P1 transfers only: the other restrictions
// and prolongations hard-code "the boundary".  Only checks.
int face_set_refusals(mg_context* c, int level) {
    for (int l = 0; l <= level; ++l) {
        const int faces = c->L[l].faces;
        if (faces == MG_FACES_ALL && c->L[level].faces == MG_FACES_ALL) continue;
        if (faces != c->L[level].faces)
            return fail("levels " + std::to_string(level) + " and " + std::to_string(l) + " were generated with different face sets (" +
                        std::to_string(c->L[level].faces) + " and " + std::to_string(faces) + "): generate them with one mg_set_diffusion_faces");
        if (!c->p1_prolong || c->restriction != MG_RESTRICT_P1_TRANSPOSE)
            return fail("level " + std::to_string(l) + " was generated with the face set " + std::to_string(faces) + " (mg_set_diffusion_faces): "
                        "its no-flux faces need the P1 transfers (mg_set_prolongation_p1 and MG_RESTRICT_P1_TRANSPOSE)");
    }
    return 0;
}

int prepare_cycle(mg_context* c, int level) {
    MG_TRY(face_set_refusals(c, level));
    if (cycle_singular(c, level)) {
        if (c->smoother != MG_SMOOTH_JACOBI)
            return fail("the levels are those of an insulated body with neither a reaction nor a Robin term (mg_set_diffusion_insulated): "
                        "the operator is singular, and the Chebyshev and Gauss-Seidel smoothers (CHEBYSHEV, RBGS, MCGS) were not written "
                        "for one; use Jacobi");
        MG_TRY(ns_workspace(c, std::max(c->L[level].nloc, c->L[0].nloc)));
    }
    // (refused here, before the colouring check and before anything is captured; smooth() refuses a single call)
    if (c->smoother == MG_SMOOTH_RBGS || c->smoother == MG_SMOOTH_MCGS)
        for (int l = 1; l <= level; ++l)
            if (c->L[l].mf)
                return fail("level " + std::to_string(l) + " is a matrix-free diffusion level: Gauss-Seidel smoothers (RBGS, MCGS) "
                            "need stored rows; use Jacobi or Chebyshev");
    if (!c->direct.tried) { MG_TRY(build_direct(c)); MG_TRY(validate_direct(c)); }
    if (c->smoother == MG_SMOOTH_MCGS)                   // (the check synchronises: not inside a capture)
        for (int l = 1; l <= level; ++l)
            if (c->L[l].mc_ok < 0 && !c->L[l].flat) MG_TRY(check_coloring(c, c->L[l]));
    if (c->comm.active())
        for (int l = 1; l <= level; ++l)
            if (!c->L[l].replicated) {
                MG_TRY(vec_alloc(c, c->L[l], &c->L[l].sw));
                // (the neighbours' class bytes next to the slab: allocations, exchanges and a vote -- not inside a capture)
                if (c->L[l].cls_halo == 0 && slab_ksweep_level(c, c->L[l]) && std::max(c->mu1, c->mu2) >= c->fuse_k_slab_min_sweeps)
                    MG_TRY(ensure_class_halos(c, c->L[l]));
            }
    if (c->keep_err)
        for (int l = 1; l <= level; ++l) MG_TRY(vec_alloc(c, c->L[l], &c->L[l].err));
    // (the march plans of the passes jacobi_ksweep makes of mu1 and mu2 sweeps: an allocation and a synchronisation each)
    if (c->smoother == MG_SMOOTH_JACOBI)
        for (int l = 1; l <= level; ++l) {
            Level& L = c->L[l];
            if (L.mf || is_slab(c, L) || !sweepsk_ok(c, L)) continue;
            for (const int mu : {c->mu1, c->mu2})
                for (int nw = mu, k; nw >= 3 && (k = next_pass(nw, sweepsk_max(c, L))) >= 3; nw -= k)
                    if (const int slot = march_plan_slot(c, L, k); slot >= 0) MG_TRY(ensure_march_plan(c, L, k, slot));
        }
    if (c->smoother == MG_SMOOTH_CHEBYSHEV)                // (the estimate synchronises: not inside a capture)
        for (int l = 1; l <= level; ++l) {
            double lo = 0.0, hi = 0.0;
            MG_TRY(cheb_interval(c, l, &lo, &hi));
        }
    if (c->p1_prolong || c->restriction == MG_RESTRICT_P1_TRANSPOSE)       // (may synchronise: not inside a capture)
        for (int l = 0; l <= level; ++l) MG_TRY(check_p1_stencil(c, c->L[l]));
    return 0;
}

int vcycle_graphed(mg_context* c, int level) {
    MG_TRY(prepare_cycle(c, level));
    // Slabs: RCCL's point-to-point calls are stream operations and are captured with the kernels (both streams of the
    // overlapped sweeps join the capture through their events).  Opt-in ("graph_comm"): every rank must take the same
    // decision, and this build could only be validated against the in-process stand-in (tests/fake_rccl).
    const bool slabs = c->comm.active();
    if (!c->use_graph || level == 0 || !c->direct.ok || (slabs && !(c->graph_comm && c->comm.nccl))) return vcycle(c, level);
    std::vector<double*> pre(level + 1);
    for (int l = 0; l <= level; ++l) pre[l] = c->L[l].v.raw;
    for (auto& g : c->graphs) {
        if (g.level != level || g.epoch != c->epoch || g.pre != pre) continue;
        HIP_TRY(hipGraphLaunch(g.exec, c->stream));
        ++c->graph_replays;
        for (int l = 0; l <= level; ++l)
            if (c->L[l].v.raw != g.post[l]) std::swap(c->L[l].v, c->L[l].v2);
        return 0;
    }
    if (c->graphs.size() >= 8) drop_graphs(c);
    CycleGraph g;
    g.level = level; g.epoch = c->epoch; g.pre = pre;
    HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    c->capturing = true;
    const int rc = vcycle(c, level);
    c->capturing = false;
    const hipError_t e = hipStreamEndCapture(c->stream, &g.graph);
    if (rc != 0 || e != hipSuccess) {
        if (g.graph) (void)hipGraphDestroy(g.graph);
        (void)hipGetLastError();
        if (rc != 0) return rc;
        return fail(std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    }
    g.post.resize(level + 1);
    for (int l = 0; l <= level; ++l) g.post[l] = c->L[l].v.raw;
    HIP_TRY(hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
    HIP_TRY(hipGraphLaunch(g.exec, c->stream));
    c->graphs.push_back(std::move(g));
    return 0;
}

// ---- flexible CG preconditioned by one V-cycle (mg_pcg) ---------------------------------------------------------------
// Vector roles during the iteration: r is the level's MG_VEC_F (the cycle's right-hand side), z the cycle's iterate
// MG_VEC_V; x, p, q and the saved right-hand side b are the level's fcg_* vectors.  The step kernels (mg_kernels.hip.h,
// fcg_*) run eagerly around the captured V-cycle; per iteration one 8-byte scalar (||r||^2) crosses to the host.
constexpr int kFcgFold = 256;       // SpMV partial sums beyond this many are folded to this many before fcg_update

// 4 blocks of 256 threads per CU, fewer where a thread would stream less than four pairs of rows
unsigned fcg_grid(const mg_context* c, const Level& L) {
    const int64_t want = (L.nloc / 2 + 4 * BLOCK - 1) / (4 * BLOCK);
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, 4 * std::max(1, c->prop.multiProcessorCount)));
}

// Layout of c->fcg_work: [0, 8) scalars (fcg kernels' sc, then the slab totals pq, rr, rz, zq), [8, 8 + kFcgFold) folded
// p.q, then the step kernels' partial sums: r.r (gmax), r.z / z.q interleaved (2 gmax).
struct FcgWork {
    double *sc, *tot_pq, *tot_rr, *tot_dots, *fold_pq, *part_rr, *part_dots;
};
FcgWork fcg_work(const mg_context* c) {
    const int64_t gmax = 4 * std::max(1, c->prop.multiProcessorCount);
    double* w = c->fcg_work;
    return FcgWork{w, w + 2, w + 3, w + 4, w + 8, w + 8 + kFcgFold, w + 8 + kFcgFold + gmax};
}

// Sums the kernels reduce in every block: `np` groups of `stride` partial sums at `parts`.  On slabs they are summed to one
// group here and all-reduced (1-2 doubles); on one GPU more than `fold_above` groups are folded to kFcgFold first.  Every
// order is fixed by the level and the device.
int fcg_sums(mg_context* c, const Level& L, const double*& parts, int64_t& np, int stride, int64_t fold_above, double* fold,
             double* total) {
    const bool slab = is_slab(c, L);
    if (!slab && np > fold_above) {
        hipLaunchKernelGGL(fcg_fold, dim3(kFcgFold), dim3(BLOCK), 0, c->stream, parts, np, stride, fold);
        parts = fold;
        np = kFcgFold;
    }
    if (slab) {
        hipLaunchKernelGGL(fcg_fold, dim3(1), dim3(BLOCK), 0, c->stream, parts, np, stride, total);
        HIP_TRY(hipGetLastError());
        MG_TRY(allreduce_sum(c, total, stride));
        parts = total;
        np = 1;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// The steps of one solve, in the order fcg_solve calls them; fcg_solve_batch calls the same steps for every lane in lockstep,
// each with the lane's vectors in the level.  What a solve carries from step to step:
struct FcgState {
    const char* who;        // "mg_pcg" / "mg_pcg_batch": the prefix of a refusal
    FcgArgs a{};
    FcgWork w{};
    double tol = 0.0;
    double bnorm = 0.0;     // ||b||, the right-hand side the tolerance is relative to
    bool go = false;        // the first residual is above the tolerance: there is an iteration to do
    int it = 0;
};

// partial sums of the SpMV (launch_ell with dot): one per block of the level's kernel
int64_t fcg_spmv_blocks(const mg_context* c, const Level& L) {
    return L.mf ? (int64_t)mf_plan(c, L).grid : (int64_t)blocks_for(L.nslices, WAVES_PER_BLOCK);
}

// start: the level's fcg_* vectors and the work buffers; x = V, b = F
int fcg_start(mg_context* c, int level, FcgState& t) {
    Level& L = c->L[level];
    MG_TRY(prepare_cycle(c, level));
    MG_TRY(vec_alloc(c, L, &L.fcg_x));
    MG_TRY(vec_alloc(c, L, &L.fcg_p));
    MG_TRY(vec_alloc(c, L, &L.fcg_q));
    MG_TRY(vec_alloc(c, L, &L.fcg_b));
    const int64_t gmax = 4 * std::max(1, c->prop.multiProcessorCount);
    if (!c->fcg_work) MG_TRY(c->fcg_work.alloc(c, (size_t)(8 + kFcgFold + 3 * gmax)));
    const int64_t nspmv = fcg_spmv_blocks(c, L);
    if ((int64_t)c->fcg_spmv.count() < nspmv) MG_TRY(c->fcg_spmv.alloc(c, (size_t)nspmv));
    t.w = fcg_work(c);
    const size_t bytes = (size_t)L.xlen * sizeof(double);
    HIP_TRY(hipMemcpyAsync(L.fcg_b.base, L.f.base, bytes, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(L.fcg_x.base, L.v.base, bytes, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

// ... and the first residual, r = b - A x (in F); a step of its own because the batch fuses it over lanes where it can
int fcg_first_residual(mg_context* c, Level& L) {
    return launch_ell(c, L, {.mode = MODE_RESIDUAL, .x_base = L.fcg_x.base, .f_rows = L.fcg_b.rows, .out_rows = L.f.rows});
}

// tolerance and arguments
int fcg_arguments(mg_context* c, Level& L, FcgState& t, double rtol, int max_iter) {
    double bnorm = 0.0, rnorm = 0.0;
    MG_TRY(norm2(c, L, L.fcg_b.rows, &bnorm));
    MG_TRY(norm2(c, L, L.f.rows, &rnorm));
    t.tol = rtol > 0.0 ? rtol * bnorm : -1.0;
    t.bnorm = bnorm;
    FcgArgs& a = t.a;
    a.x = L.fcg_x.rows; a.r = L.f.rows; a.p = L.fcg_p.rows; a.q = L.fcg_q.rows; a.sc = t.w.sc; a.n = L.nloc;
    for (const double* v : {(const double*)a.x, (const double*)a.r, (const double*)a.p, a.q})
        if (reinterpret_cast<uintptr_t>(v) % 16) return fail(std::string(t.who) + ": misaligned work vector");
    t.go = max_iter > 0 && rnorm > t.tol && rnorm > 0.0;
    return 0;
}

// the partial sums of fcg_dots (r.z and z.q) summed for fcg_direction
int fcg_dots_summed(mg_context* c, const Level& L, FcgState& t, int64_t nd) {
    const double* dots = t.w.part_dots;
    MG_TRY(fcg_sums(c, L, dots, nd, 2, INT64_MAX, nullptr, t.w.tot_dots));
    t.a.dots = dots; t.a.nd = (int)nd;
    return 0;
}

// first direction, after z = M r: p = z
int fcg_first_direction(mg_context* c, const Level& L, FcgState& t) {
    const dim3 grid(fcg_grid(c, L)), blk(BLOCK);
    t.a.out = t.w.part_dots;
    hipLaunchKernelGGL(fcg_dots<false>, grid, blk, 0, c->stream, t.a);
    hipLaunchKernelGGL(fcg_direction<true>, grid, blk, 0, c->stream, t.a);
    return fcg_dots_summed(c, L, t, grid.x);
}

// q = A p with the partial sums of p.q in c->fcg_spmv (one lane; the batch fuses lanes where it can)
int fcg_spmv(mg_context* c, Level& L, const FcgState& t, unsigned* nsp) {
    MG_TRY(launch_ell(c, L, {.mode = MODE_SPMV, .dot = true, .x_base = L.fcg_p.base, .out_rows = L.fcg_q.rows, .partials = c->fcg_spmv,
                             .grid_out = nsp}));
    if ((size_t)*nsp > c->fcg_spmv.count()) return fail(std::string(t.who) + ": SpMV partial sums overflow");
    return 0;
}

// update: alpha from the npq partial sums of p.q, x += alpha p, r -= alpha q, and ||r||^2 (summed over the slabs where
// `slabs`) on its way to the host slot `rr`; the caller synchronises the stream before it reads it
int fcg_update_step(mg_context* c, Level& L, FcgState& t, int64_t npq, bool slabs, double* rr) {
    const dim3 grid(fcg_grid(c, L)), blk(BLOCK);
    const double* pq = c->fcg_spmv;
    MG_TRY(fcg_sums(c, L, pq, npq, 1, kFcgFold, t.w.fold_pq, t.w.tot_pq));
    t.a.pq = pq; t.a.npq = (int)npq;
    t.a.out = t.w.part_rr;
    t.a.vz = L.g.lead == 0 && L.xlen == L.nloc ? L.v.rows : nullptr;    // whole levels: fcg_update zeroes V for the next cycle
    hipLaunchKernelGGL(fcg_update, grid, blk, 0, c->stream, t.a);
    hipLaunchKernelGGL(fcg_fold, dim3(1), blk, 0, c->stream, t.w.part_rr, (int64_t)grid.x, 1, t.w.tot_rr);
    HIP_TRY(hipGetLastError());
    if (slabs) MG_TRY(allreduce_sum(c, t.w.tot_rr, 1));
    HIP_TRY(hipMemcpyAsync(rr, t.w.tot_rr, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return 0;
}

// what the host does with ||r||^2: the history, the count, and whether the solve goes on
bool fcg_goes_on(FcgState& t, double rr, int max_iter, double* hist) {
    const double rn = std::sqrt(rr);
    if (hist) hist[t.it] = rn;
    ++t.it;
    return !(rn <= t.tol || rn == 0.0 || t.it >= max_iter);
}

// next direction, after z = M r: r.z and z.q; p = z + beta p
int fcg_next_direction(mg_context* c, const Level& L, FcgState& t) {
    const dim3 grid(fcg_grid(c, L)), blk(BLOCK);
    t.a.out = t.w.part_dots;
    hipLaunchKernelGGL(fcg_dots<true>, grid, blk, 0, c->stream, t.a);
    MG_TRY(fcg_dots_summed(c, L, t, grid.x));
    hipLaunchKernelGGL(fcg_direction<false>, grid, blk, 0, c->stream, t.a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// finish: V = x, F = b bit for bit (R = F - A x is the caller's)
int fcg_finish(mg_context* c, Level& L) {
    const size_t bytes = (size_t)L.xlen * sizeof(double);
    HIP_TRY(hipMemcpyAsync(L.v.base, L.fcg_x.base, bytes, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(L.f.base, L.fcg_b.base, bytes, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

// z = one V(mu1, mu2) cycle from a zero guess on r (= F); the cycle may swap the level's V buffers, so z is read after it.
// v_zeroed: fcg_update has zeroed V (whole levels: V is the owned rows and nothing else)
int fcg_precondition(mg_context* c, int level, FcgArgs& a, bool v_zeroed) {
    Level& L = c->L[level];
    if (!v_zeroed) MG_TRY(zero_vec(c, L, L.v));
    MG_TRY(vcycle_graphed(c, level));
    a.z = L.v.rows;
    if (reinterpret_cast<uintptr_t>(a.z) % 16) return fail("mg_pcg: misaligned iterate");
    return 0;
}

int fcg_solve(mg_context* c, int level, double rtol, int max_iter, double* hist, int* iters_out) {
    Level& L = c->L[level];
    FcgState t{"mg_pcg"};
    // An insulated body's singular operator (cycle_singular; DESIGN.md, "Insulated bodies"): the solve is x = Q A^+ Q^T b.
    // b becomes Q^T b once, every preconditioned residual is made mean-free (Euclidean weights: the preconditioner stays
    // symmetric on the complement of the constants and the iterate cannot drift along them), the result is Q x; the
    // stopping test is relative to Q^T b, which is what MG_VEC_F holds afterwards.
    const bool ns = cycle_singular(c, level);
    if (ns) MG_TRY(ns_weights(c, L));
    const double inv_n = 1.0 / (double)L.nloc;
    MG_TRY(fcg_start(c, level, t));
    if (ns) MG_TRY(ns_remove(c, L.fcg_b.rows, nullptr, c->ns_w, L.nloc, c->ns_inv_s));
    MG_TRY(exchange_halo(c, L, L.fcg_x));
    MG_TRY(fcg_first_residual(c, L));
    MG_TRY(fcg_arguments(c, L, t, rtol, max_iter));
    if (ns && t.bnorm == 0.0) t.go = false;      // a projected right-hand side of zero: Q x0 after zero iterations
    if (t.go) {
        MG_TRY(fcg_precondition(c, level, t.a, false));
        if (ns) MG_TRY(ns_remove(c, L.v.rows, nullptr, nullptr, L.nloc, inv_n));
        MG_TRY(fcg_first_direction(c, L, t));
        for (;;) {
            MG_TRY(exchange_halo(c, L, L.fcg_p));
            unsigned nsp = 0;
            MG_TRY(fcg_spmv(c, L, t, &nsp));
            MG_TRY(fcg_update_step(c, L, t, nsp, !L.replicated, c->h_scalars));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (!fcg_goes_on(t, c->h_scalars[0], max_iter, hist)) break;
            MG_TRY(fcg_precondition(c, level, t.a, t.a.vz != nullptr));
            if (ns) MG_TRY(ns_remove(c, L.v.rows, nullptr, nullptr, L.nloc, inv_n));
            MG_TRY(fcg_next_direction(c, L, t));
        }
    }
    if (ns) MG_TRY(ns_remove(c, L.fcg_x.rows, c->ns_w, nullptr, L.nloc, c->ns_inv_s));
    // ... and R = F - A x
    MG_TRY(fcg_finish(c, L));
    MG_TRY(exchange_halo(c, L, L.v));
    MG_TRY(residual(c, level));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (iters_out) *iters_out = t.it;
    return 0;
}

// ---- batched solves: one operator, several right-hand sides (mg_apply_batch, mg_pcg_batch) ----------------------------------
// Every operation of a solve and of its V-cycle is done for all active lanes before the next one starts.  On a matrix-free level
// the Jacobi sweeps, the residual and the SpMV take the active lanes in ascending order in groups of at most "mf_batch", one
// fused launch per group (a group of one: the one-vector kernel); everything else -- stored levels, transfers, the coarsest solve,
// the fcg_* kernels and folds, a Chebyshev smoother -- runs once per lane with the one-vector code, the lane's vectors swapped
// into the levels around the call.  Cycles run eagerly (no capture, no replay): eager and replayed cycles agree to the bit.

void swap_lane(mg_context* c, Lane& lane, int lo, int top) {
    for (int l = lo; l <= top; ++l) {
        Level& L = c->L[l];
        LaneLevel& v = lane.lv[(size_t)l];
        std::swap(L.v, v.v); std::swap(L.v2, v.v2); std::swap(L.f, v.f); std::swap(L.err, v.err);
        std::swap(L.fcg_x, v.fcg_x); std::swap(L.fcg_p, v.fcg_p); std::swap(L.fcg_q, v.fcg_q); std::swap(L.fcg_b, v.fcg_b);
    }
    std::swap(c->fcg_work, lane.fcg_work);
    std::swap(c->fcg_spmv, lane.fcg_spmv);
}

int64_t lane_bytes(const Lane& lane) {
    size_t n = lane.fcg_work.count() + lane.fcg_spmv.count();
    for (const LaneLevel& v : lane.lv)
        for (const DVector* d : {&v.v, &v.v2, &v.f, &v.err, &v.fcg_x, &v.fcg_p, &v.fcg_q, &v.fcg_b}) n += d->raw.count();
    return (int64_t)(n * sizeof(double));
}

// lanes 1 .. nb - 1 with V, its partner and F on levels lo .. top (what a level's set-up gives the handle's own lane); the
// rest is allocated where the one-vector code allocates it, with the lane swapped in
int ensure_lanes(mg_context* c, int nb, int lo, int top) {
    if ((int)c->lanes.size() < nb - 1) c->lanes.resize((size_t)(nb - 1));
    for (int b = 0; b < nb - 1; ++b) {
        Lane& lane = c->lanes[(size_t)b];
        lane.lv.resize((size_t)c->nlev);
        for (int l = lo; l <= top; ++l) {
            LaneLevel& v = lane.lv[(size_t)l];
            MG_TRY(vec_alloc(c, c->L[l], &v.v));
            MG_TRY(vec_alloc(c, c->L[l], &v.v2));
            MG_TRY(vec_alloc(c, c->L[l], &v.f));
        }
    }
    return 0;
}

// The lanes of one batch call.  While it lives the handle's own vectors of levels lo .. top are lane 0's record and the levels
// hold the lane that is entered (none: empty vectors); its end puts the handle's own back, whatever happened in between.
struct BatchScope {
    mg_context* c;
    int lo, top, in = -1;
    Lane own;
    std::vector<Lane*> lane;
    BatchScope(mg_context* c_, int lo_, int top_, int nb) : c(c_), lo(lo_), top(top_) {
        own.lv.resize((size_t)c->nlev);
        swap_lane(c, own, lo, top);
        lane.push_back(&own);
        for (int b = 1; b < nb; ++b) lane.push_back(&c->lanes[(size_t)(b - 1)]);
    }
    BatchScope(const BatchScope&) = delete;
    BatchScope& operator=(const BatchScope&) = delete;
    ~BatchScope() {
        if (in >= 0) leave();
        swap_lane(c, own, lo, top);
    }
    void enter(int b) { swap_lane(c, *lane[(size_t)b], lo, top); in = b; }
    void leave() { swap_lane(c, *lane[(size_t)in], lo, top); in = -1; }
    LaneLevel& at(int b, int level) { return lane[(size_t)b]->lv[(size_t)level]; }
    // f(b) with lane b's vectors in the levels, for every lane of `act` in ascending order
    template <class F>
    int each(const std::vector<int>& act, F&& f) {
        for (int b : act) {
            enter(b);
            const int rc = f(b);
            leave();
            MG_TRY(rc);
        }
        return 0;
    }
};

inline bool mf_fused(const mg_context* c, const Level& L, size_t lanes) { return L.mf && c->mf_batch >= 2 && lanes >= 2; }

// One launch of the march per group of at most "mf_batch" lanes of `act`.  ops(b, &x_rows, &f_rows, &out_rows, &partials) names
// lane b's operands; single(b) runs the one-vector kernel for a group of one (lane b entered); after(b, nv) follows the launch for
// each of its lanes, nv = the lanes of the launch for the first of them and 0 for the others (so a launch is counted once).
template <class Ops, class Single, class After>
int mf_groups(mg_context* c, BatchScope& s, const Level& L, int mode, bool dot, const std::vector<int>& act, Ops&& ops, Single&& single,
              After&& after) {
    const size_t most = (size_t)std::min(c->mf_batch, MF_BATCH_MAX);
    for (size_t g0 = 0; g0 < act.size(); g0 += most) {
        const int nv = (int)std::min(most, act.size() - g0);
        if (nv == 1) {
            const int b = act[g0];
            s.enter(b);
            const int rc = single(b);
            s.leave();
            MG_TRY(rc);
            after(b, 1);
            continue;
        }
        const double *x[MF_BATCH_MAX] = {}, *f[MF_BATCH_MAX] = {};
        double *out[MF_BATCH_MAX] = {}, *parts[MF_BATCH_MAX] = {};
        for (int v = 0; v < nv; ++v) ops(act[g0 + (size_t)v], &x[v], &f[v], &out[v], &parts[v]);
        MG_TRY(launch_diffusion_mf_batch(c, L, mode, dot, nv, x, f, out, parts));
        for (int v = 0; v < nv; ++v) after(act[g0 + (size_t)v], v == 0 ? nv : 0);
    }
    return 0;
}

// nw smoother sweeps of every lane of `act` on `level`
int smooth_batch(mg_context* c, BatchScope& s, int level, int nw, const std::vector<int>& act) {
    Level& L = c->L[level];
    if (!(mf_fused(c, L, act.size()) && c->smoother == MG_SMOOTH_JACOBI)) return s.each(act, [&](int) { return smooth(c, level, nw); });
    for (int sw = 0; sw < nw; ++sw)
        MG_TRY(mf_groups(c, s, L, MODE_JACOBI, false, act,
            [&](int b, const double** x, const double** f, double** out, double**) {
                LaneLevel& v = s.at(b, level);
                *x = v.v.base + L.g.lead; *f = v.f.rows; *out = v.v2.rows;
            },
            [&](int) { return smooth_matrix_free(c, level, 1); },
            [&](int b, int nv) {
                if (nv > 1) count_pass(c, level, MG_PATH_MATRIX_FREE, 1, nv);      // one launch, a sweep of each of its lanes
                if (nv != 1) std::swap(s.at(b, level).v, s.at(b, level).v2);       // (a group of one swapped its own)
            }));
    return 0;
}

// R = F - A V of every lane of `act` on `level`
int residual_batch(mg_context* c, BatchScope& s, int level, const std::vector<int>& act) {
    Level& L = c->L[level];
    if (!mf_fused(c, L, act.size())) return s.each(act, [&](int) { return residual(c, level); });
    return mf_groups(c, s, L, MODE_RESIDUAL, false, act,
        [&](int b, const double** x, const double** f, double** out, double**) {
            LaneLevel& v = s.at(b, level);
            *x = v.v.base + L.g.lead; *f = v.f.rows; *out = v.v2.rows;
        },
        [&](int) { return residual(c, level); }, [](int, int) {});
}

// vcycle() for every lane of `act`, operation by operation
int vcycle_batch(mg_context* c, BatchScope& s, int level, const std::vector<int>& act) {
    if (level == 0) return s.each(act, [&](int) { return coarse_solve(c, nullptr, nullptr); });
    Level& C = c->L[level - 1];
    MG_TRY(smooth_batch(c, s, level, c->mu1, act));
    if (c->restriction == MG_RESTRICT_INJECTION && c->fuse_restrict && !c->L[level].mf) {
        MG_TRY(s.each(act, [&](int) { return residual_restrict_fused(c, level); }));
    } else {
        MG_TRY(residual_batch(c, s, level, act));
        MG_TRY(s.each(act, [&](int) { return restrict_to(c, level, c->restriction); }));
    }
    MG_TRY(s.each(act, [&](int) { return zero_vec(c, C, C.v); }));
    MG_TRY(vcycle_batch(c, s, level - 1, act));
    MG_TRY(s.each(act, [&](int) { return prolong(c, level, 1); }));
    MG_TRY(smooth_batch(c, s, level, c->mu2, act));
    return 0;
}

// fcg_solve() for nb lanes in lockstep: every lane has its own alpha, beta, dots and stopping test, and a lane that has stopped
// leaves the batch.  On entry lane b's V and F of `level` hold its start and right-hand side; on return V = x, F = b, R = F - A x
// as fcg_solve leaves them.  hist: nb rows of `stride` entries.
int fcg_solve_batch(mg_context* c, BatchScope& s, int level, int nb, double rtol, int max_iter, double* hist, int stride, int* iters_out) {
    Level& L = c->L[level];
    std::vector<FcgState> st((size_t)nb, FcgState{"mg_pcg_batch"});
    std::vector<int> all((size_t)nb), act;
    for (int b = 0; b < nb; ++b) all[(size_t)b] = b;
    if (!c->h_lanes) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->h_lanes), MG_BATCH_MAX * sizeof(double), hipHostMallocDefault));

    MG_TRY(s.each(all, [&](int b) { return fcg_start(c, level, st[(size_t)b]); }));
    auto first_residual = [&](int) { return fcg_first_residual(c, L); };
    if (mf_fused(c, L, all.size())) {
        MG_TRY(mf_groups(c, s, L, MODE_RESIDUAL, false, all,
            [&](int b, const double** x, const double** f, double** out, double**) {
                LaneLevel& v = s.at(b, level);
                *x = v.fcg_x.base + L.g.lead; *f = v.fcg_b.rows; *out = v.f.rows;
            },
            first_residual, [](int, int) {}));
    } else {
        MG_TRY(s.each(all, first_residual));
    }
    MG_TRY(s.each(all, [&](int b) -> int {
        MG_TRY(fcg_arguments(c, L, st[(size_t)b], rtol, max_iter));
        if (st[(size_t)b].go) act.push_back(b);
        return 0;
    }));

    // z = one V-cycle from a zero guess on r, for every active lane (fcg_precondition)
    auto precondition = [&](bool v_zeroed) -> int {
        if (!v_zeroed) MG_TRY(s.each(act, [&](int) { return zero_vec(c, L, L.v); }));
        MG_TRY(vcycle_batch(c, s, level, act));
        for (int b : act) {
            st[(size_t)b].a.z = s.at(b, level).v.rows;
            if (reinterpret_cast<uintptr_t>(st[(size_t)b].a.z) % 16) return fail("mg_pcg_batch: misaligned iterate");
        }
        return 0;
    };
    if (!act.empty()) {
        MG_TRY(precondition(false));
        MG_TRY(s.each(act, [&](int b) { return fcg_first_direction(c, L, st[(size_t)b]); }));
    }
    const int64_t nspmv = fcg_spmv_blocks(c, L);
    while (!act.empty()) {
        auto spmv_one = [&](int b) -> int {
            unsigned nsp = 0;
            return fcg_spmv(c, L, st[(size_t)b], &nsp);
        };
        if (mf_fused(c, L, act.size())) {
            MG_TRY(mf_groups(c, s, L, MODE_SPMV, true, act,
                [&](int b, const double** x, const double**, double** out, double** parts) {
                    LaneLevel& v = s.at(b, level);
                    *x = v.fcg_p.base + L.g.lead; *out = v.fcg_q.rows; *parts = s.lane[(size_t)b]->fcg_spmv;
                },
                spmv_one, [](int, int) {}));
        } else {
            MG_TRY(s.each(act, spmv_one));
        }
        // every lane's ||r||^2 to the host in one round trip; who goes on
        MG_TRY(s.each(act, [&](int b) { return fcg_update_step(c, L, st[(size_t)b], nspmv, false, c->h_lanes + b); }));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const bool v_zeroed = st[(size_t)act.back()].a.vz != nullptr;
        std::vector<int> next;
        for (int b : act)
            if (fcg_goes_on(st[(size_t)b], c->h_lanes[b], max_iter, hist ? hist + (size_t)b * (size_t)stride : nullptr)) next.push_back(b);
        act = next;
        if (act.empty()) break;
        MG_TRY(precondition(v_zeroed));
        MG_TRY(s.each(act, [&](int b) { return fcg_next_direction(c, L, st[(size_t)b]); }));
    }
    // ... and R = F - A x
    MG_TRY(s.each(all, [&](int b) -> int {
        if (iters_out) iters_out[b] = st[(size_t)b].it;
        return fcg_finish(c, L);
    }));
    MG_TRY(residual_batch(c, s, level, all));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// the permute kernels of mg_set_vector_device / mg_get_vector_device on a vector of the level (no synchronisation)
int scatter_to(mg_context* c, Level& L, DVector& v, const double* dev) {
    MG_TRY(vec_alloc(c, L, &v));
    const unsigned nb = (unsigned)std::min<int64_t>(4096, (L.n_global + 255) / 256);
    hipLaunchKernelGGL(scatter_in, dim3(nb), dim3(256), 0, c->stream, dev, L.perm, L.n_global, L.row0, L.g.lead, L.xlen, v.base);
    HIP_TRY(hipGetLastError());
    return 0;
}
int gather_from(mg_context* c, Level& L, DVector& v, double* dev) {
    const unsigned nb = (unsigned)std::min<int64_t>(4096, (L.n_global + 255) / 256);
    hipLaunchKernelGGL(gather_out, dim3(nb), dim3(256), 0, c->stream, v.base, L.perm, L.n_global, L.row0, L.nloc, L.g.lead, dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// true where [p, p + np) and [q, q + nq) have a byte in common
static bool overlaps(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq && b < a + np;
}

// What both batch entries refuse before anything is launched or allocated: the handle, the level, the lane count, the pointers.
// in[k] / out: host arrays of nb device pointers of n_global doubles (in[k] may be null: not read); no out may overlap another
// lane's out or any input.
int batch_refusals(mg_context* c, const std::string& who, int level, int nb, const double* const* in0, const double* const* in1,
                   double* const* out, const char* in0_name, const char* in1_name, const char* out_name) {
    if (!c) return fail("null handle");
    if (c->dim != 3) return fail(who + ": batched solves are 3-D only (this handle is 2-D)");
    if (c->comm.active()) return fail(who + " needs a whole (not slab) handle");
    MG_TRY(check_level(c, level));
    const Level& L = c->L[level];
    if (L.flat) return fail(who + ": level " + std::to_string(level) + " is flat (no grid)");
    if (nb < 1 || nb > MG_BATCH_MAX)
        return fail(who + ": nb = " + std::to_string(nb) + " is outside 1.." + std::to_string(MG_BATCH_MAX) + " (MG_BATCH_MAX)");
    if (!out || (in0_name && !in0) || (in1_name && !in1)) return fail(who + ": null pointer array");
    HIP_TRY(hipSetDevice(c->device));
    const size_t len = (size_t)L.n_global * sizeof(double);
    struct Range { const char* p; const char* name; int lane; bool out; };
    std::vector<Range> r;
    for (int b = 0; b < nb; ++b) {
        const std::string lane = "[" + std::to_string(b) + "]";
        if (in0_name) {
            MG_TRY(need_device_pointer(c, in0[b], who.c_str(), (in0_name + lane).c_str()));
            r.push_back({reinterpret_cast<const char*>(in0[b]), in0_name, b, false});
        }
        if (in1_name) {
            MG_TRY(need_device_pointer(c, in1[b], who.c_str(), (in1_name + lane).c_str()));
            r.push_back({reinterpret_cast<const char*>(in1[b]), in1_name, b, false});
        }
        MG_TRY(need_device_pointer(c, out[b], who.c_str(), (out_name + lane).c_str()));
        r.push_back({reinterpret_cast<const char*>(out[b]), out_name, b, true});
    }
    for (const Range& o : r) {
        if (!o.out) continue;
        for (const Range& q : r) {
            if (&q == &o || (q.out && q.lane <= o.lane)) continue;
            if (overlaps(o.p, len, q.p, len))
                return fail(who + ": " + o.name + "[" + std::to_string(o.lane) + "] overlaps " + q.name + "[" + std::to_string(q.lane) +
                            "]: every lane's output is memory of its own");
        }
    }
    return 0;
}

// ---- smallest eigenpairs by LOBPCG (mg_eigs) and its two block kernels (mg_block.hip.h) -----------------------------------------

// the grid of the streaming block kernels: fcg_grid, a function of the level and the device alone (block_gram's sums depend on it)
unsigned gram_grid(const mg_context* c, const Level& L) { return fcg_grid(c, L); }

constexpr size_t kEigsSums = 2 * (size_t)BC_MAX_IN * BC_MAX_IN + 2 * MG_EIGS_MAX;   // two Gram matrices, or the residual norms

// partial sums of the block kernels (one tile at a time) and the folded sums; uncounted scratch where `ew` is a temporary's
int ensure_block_scratch(mg_context* c, const Level& L, EigsWork& ew) {
    const size_t parts = (size_t)gram_grid(c, L) * BG_MAX * BG_MAX;
    if (ew.parts.count() < parts) MG_TRY(ew.parts.alloc(c, parts));
    if (ew.sums.count() < kEigsSums) MG_TRY(ew.sums.alloc(c, kEigsSums));
    return 0;
}

// Tiles of block_gram launches whose folded sums wait in ew.sums for one download; each knows where its pairs go on the host.
struct GramBatch {
    struct Tile { double* dst; int ld, r, col, na, nb; size_t off; bool mirror, upper; };
    std::vector<Tile> tiles;
    size_t used = 0;
};

// a_i . (d * b_j), i < na, j < nb, tiled by BG_MAX x BG_MAX: pair (i, j) goes to dst[(r0 + i) * ld + c0 + j].  sym: a == b, only
// the tiles on and above the diagonal are computed and of a tile on the diagonal the pairs i <= j are used, so the matrix is
// symmetric to the bit.  mirror: a pair of any tile (always where sym) also goes to dst[(c0 + j) * ld + r0 + i].
int gram_enqueue(mg_context* c, const Level& L, EigsWork& ew, GramBatch& gb, double* dst, int ld, int r0, int c0, int na,
                 const double* const* a, int nb, const double* const* b, const double* d, bool sym, bool mirror) {
    const dim3 grid(gram_grid(c, L)), blk(BLOCK);
    for (int ti = 0; ti < na; ti += BG_MAX)
        for (int tj = sym ? ti : 0; tj < nb; tj += BG_MAX) {
            const int NA = std::min(BG_MAX, na - ti), NB = std::min(BG_MAX, nb - tj);
            if (gb.used + (size_t)(NA * NB) > ew.sums.count()) return fail("block_gram: more sums than the buffer holds");
            GramArgs g{};
            for (int i = 0; i < NA; ++i) g.a[i] = a[ti + i];
            for (int j = 0; j < NB; ++j) g.b[j] = b[tj + j];
            g.d = d; g.out = ew.parts; g.n = L.nloc;
            with_int<1, 2, 3, 4>(NA, [&](auto ia) {
                with_int<1, 2, 3, 4>(NB, [&](auto ib) {
                    with_bool(d != nullptr, [&](auto w) {
                        hipLaunchKernelGGL((block_gram<decltype(ia)::value, decltype(ib)::value, decltype(w)::value>), grid, blk, 0, c->stream, g);
                    });
                });
            });
            hipLaunchKernelGGL(fcg_fold, dim3(1), blk, 0, c->stream, ew.parts.get(), (int64_t)grid.x, NA * NB, ew.sums.get() + gb.used);
            HIP_TRY(hipGetLastError());
            gb.tiles.push_back({dst, ld, r0 + ti, c0 + tj, NA, NB, gb.used, sym || mirror, sym && tj == ti});
            gb.used += (size_t)(NA * NB);
        }
    return 0;
}

// one download of everything enqueued, then every pair to its place
int gram_collect(mg_context* c, EigsWork& ew, GramBatch& gb) {
    std::vector<double> h(std::max<size_t>(1, gb.used));
    HIP_TRY(hipMemcpyAsync(h.data(), ew.sums.get(), gb.used * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (const GramBatch::Tile& t : gb.tiles)
        for (int i = 0; i < t.na; ++i)
            for (int j = t.upper ? i : 0; j < t.nb; ++j) {
                const double v = h[t.off + (size_t)(i * t.nb + j)];
                t.dst[(size_t)(t.r + i) * t.ld + t.col + j] = v;
                if (t.mirror) t.dst[(size_t)(t.col + j) * t.ld + t.r + i] = v;
            }
    gb.tiles.clear();
    gb.used = 0;
    return 0;
}

// out_o = sum_i coeff[i * no + o] s_i over the level's rows; an output may be one of the inputs
int launch_block_combine(mg_context* c, const Level& L, int ns, const double* const* s, int no, const double* coeff, double* const* out) {
    CombineArgs g{};
    for (int i = 0; i < ns; ++i) g.s[i] = s[i];
    for (int o = 0; o < no; ++o) g.out[o] = out[o];
    for (int i = 0; i < ns * no; ++i) g.c[i] = coeff[i];
    g.n = L.nloc;
    const dim3 grid(gram_grid(c, L)), blk(BLOCK);
    const bool known = with_int<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24>(ns, [&](auto is) {
        with_int<1, 2, 3, 4, 5, 6, 7, 8>(no, [&](auto io) {
            hipLaunchKernelGGL((block_combine<decltype(is)::value, decltype(io)::value>), grid, blk, 0, c->stream, g);
        });
    });
    if (!known || no < 1 || no > BC_MAX_OUT) return fail("block_combine takes 1..24 inputs and 1..8 outputs");
    HIP_TRY(hipGetLastError());
    return 0;
}

// what mg_block_gram and mg_block_combine refuse about the handle, the level and one array of device pointers
int block_level_refusals(mg_context* c, const std::string& who, int level) {
    if (!c) return fail("null handle");
    if (c->dim != 3) return fail(who + ": the block kernels are 3-D only (this handle is 2-D)");
    if (c->comm.active()) return fail(who + " needs a whole (not slab) handle");
    MG_TRY(check_level(c, level));
    if (c->L[level].flat) return fail(who + ": level " + std::to_string(level) + " is flat (no grid)");
    return 0;
}
int block_pointer_refusals(mg_context* c, const std::string& who, int n, const double* const* p, const char* name) {
    if (!p) return fail(who + ": null pointer array (" + name + ")");
    for (int i = 0; i < n; ++i) {
        const std::string what = std::string(name) + "[" + std::to_string(i) + "]";
        MG_TRY(need_device_pointer(c, p[i], who.c_str(), what.c_str()));
        if (reinterpret_cast<uintptr_t>(p[i]) % 16) return fail(who + ": " + what + " is not 16-byte aligned");
    }
    return 0;
}

// the first cell of a device rho that is not a finite double > 0, as an error (check_sigma's wording)
int check_rho(mg_context* c, const std::string& who, const double* d_rho, int64_t n, int N) {
    DevTemp d_first;
    MG_TRY(d_first.alloc(sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(d_first.p, 0xff, sizeof(unsigned long long), c->stream));
    const unsigned nb = (unsigned)std::max<int64_t>(1, std::min<int64_t>(8192, (n + 255) / 256));
    hipLaunchKernelGGL(rho_check, dim3(nb), dim3(256), 0, c->stream, d_rho, n, d_first.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    unsigned long long first = 0;
    HIP_TRY(hipMemcpyAsync(&first, d_first.p, sizeof(first), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (first == ~0ull) return 0;
    double x = 0.0;
    HIP_TRY(hipMemcpy(&x, d_rho + first, sizeof(double), hipMemcpyDeviceToHost));
    const int64_t q = (int64_t)first;
    char val[40];
    snprintf(val, sizeof(val), "%.17g", x);
    return fail(who + ": rho must be finite and positive: cell (" + std::to_string(q % N) + ", " + std::to_string((q / N) % N) + ", " +
                std::to_string(q / ((int64_t)N * N)) + ") = index " + std::to_string(q) + " holds " + val);
}

// the work vectors of mg_eigs for `block` vectors on `level` (kept: a call with the same level and a smaller block finds them)
int ensure_eigs(mg_context* c, int level, int block) {
    const Level& L = c->L[level];
    EigsWork& ew = c->eigs;
    if (ew.level != level || ew.vec_total != vec_total(L)) ew = EigsWork{};
    ew.level = level;
    ew.vec_total = vec_total(L);
    MG_TRY(vec_alloc(c, L, &ew.m));
    for (auto* set : {&ew.x, &ew.kx, &ew.kw, &ew.p, &ew.kp}) {
        if ((int)set->size() < block) set->resize((size_t)block);
        for (int j = 0; j < block; ++j) MG_TRY(vec_alloc(c, L, &(*set)[(size_t)j]));
    }
    ew.block = std::max(ew.block, block);
    return ensure_block_scratch(c, L, ew);
}

// The iteration of mg_eigs (see include/mg_hip.h).  On entry lanes 0 .. block - 1 exist and `s` holds them.
int eigs_solve(mg_context* c, BatchScope& s, int level, int k, int block, const double* rho_dev, double* const* x_dev, int warm,
               double rtol, int max_iter, double* lambda, double* resid, int* iterations, int* restarts) {
    const std::string who = "mg_eigs";
    Level& L = c->L[level];
    EigsWork& ew = c->eigs;
    const int64_t n = L.nloc;
    const int b = block;
    const unsigned nbk = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (n + 255) / 256));
    const dim3 fgrid(gram_grid(c, L)), blk(BLOCK);
    std::vector<int> all((size_t)b);
    for (int j = 0; j < b; ++j) all[(size_t)j] = j;

    // M = R(rho), +0.0 on the Dirichlet nodes of the level's face set
    {
        DevTemp ones;
        const int64_t cells = (int64_t)L.N * L.N * L.N;
        if (!rho_dev) {
            MG_TRY(ones.alloc((size_t)cells * sizeof(double)));
            hipLaunchKernelGGL(eigs_fill, dim3(nbk), dim3(256), 0, c->stream, ones.as<double>(), cells, 1.0);
            HIP_TRY(hipGetLastError());
        }
        MG_TRY(launch_reaction_diag(c, rho_dev ? rho_dev : ones.as<const double>(), ew.m.rows, L.N));
        hipLaunchKernelGGL(eigs_mass_mask, dim3(nbk), dim3(256), 0, c->stream, ew.m.rows, level_box(L, L.faces), L.g.nx, L.g.ny, n);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));       // (`ones` goes)
    }
    const double* const m = ew.m.rows;

    // the start block
    for (int j = 0; j < b; ++j) {
        if (warm) {
            MG_TRY(scatter_to(c, L, ew.x[(size_t)j], x_dev[j]));
            hipLaunchKernelGGL(eigs_mask, dim3(nbk), dim3(256), 0, c->stream, ew.x[(size_t)j].rows, m, n);
        } else {
            hipLaunchKernelGGL(eigs_start, dim3(nbk), dim3(256), 0, c->stream, ew.x[(size_t)j].rows, m, n, (uint64_t)j * (uint64_t)L.n_global);
        }
        HIP_TRY(hipGetLastError());
    }

    // out_j = K x_j for the whole block: one fused launch per group of lanes on a matrix-free level, the level's SpMV per lane
    // elsewhere.  xs null: x_j is the cycle's result, lane j's MG_VEC_V.
    auto apply_K = [&](std::vector<DVector>* xs, std::vector<DVector>& outs) -> int {
        auto one = [&](int j) {
            return launch_ell(c, L, {.mode = MODE_SPMV, .x_base = xs ? (*xs)[(size_t)j].base : L.v.base, .out_rows = outs[(size_t)j].rows});
        };
        if (!mf_fused(c, L, all.size())) return s.each(all, one);
        return mf_groups(c, s, L, MODE_SPMV, false, all,
            [&](int j, const double** x, const double**, double** out, double** parts) {
                *x = (xs ? (*xs)[(size_t)j].base : s.at(j, level).v.base) + L.g.lead; *out = outs[(size_t)j].rows; *parts = nullptr;
            },
            one, [](int, int) {});
    };

    // One Rayleigh-Ritz step on the columns S (and K S), `known` leading columns being M-orthonormal Ritz vectors with the
    // values lam[] (their Gram blocks need no launch).  The columns are scaled to unit M-norm in the Gram matrices, and the scale
    // goes into the coefficients: the same numbers as scaling the vectors, without a pass over them.  X, K X <- the b lowest
    // Ritz vectors, P, K P <- their part outside X.  1: the Cholesky factorisation of S^T M S failed.
    std::vector<double> lam((size_t)b, 0.0);
    auto rayleigh_ritz = [&](int mcols, const std::vector<const double*>& S, const std::vector<const double*>& KS, int known) -> int {
        std::vector<double> gk((size_t)(mcols * mcols), 0.0), gm((size_t)(mcols * mcols), 0.0);
        GramBatch gb;
        for (int pass = 0; pass < 2; ++pass) {
            double* dst = pass == 0 ? gk.data() : gm.data();
            const double* const* right = pass == 0 ? KS.data() : S.data();
            const double* d = pass == 0 ? nullptr : m;
            if (known > 0 && mcols > known)
                MG_TRY(gram_enqueue(c, L, ew, gb, dst, mcols, 0, known, known, S.data(), mcols - known, right + known, d, false, true));
            MG_TRY(gram_enqueue(c, L, ew, gb, dst, mcols, known, known, mcols - known, S.data() + known, mcols - known, right + known, d, true, false));
        }
        MG_TRY(gram_collect(c, ew, gb));
        for (int i = 0; i < known; ++i) { gk[(size_t)(i * mcols + i)] = lam[(size_t)i]; gm[(size_t)(i * mcols + i)] = 1.0; }
        std::vector<double> scale((size_t)mcols);
        for (int i = 0; i < mcols; ++i) {
            const double d = gm[(size_t)(i * mcols + i)];
            if (!std::isfinite(d)) return fail(who + ": a basis vector has a non-finite M-norm");
            if (!(d > 0.0)) return 1;       // (a zero column: as dependent as a basis gets)
            scale[(size_t)i] = 1.0 / std::sqrt(d);
        }
        for (int i = 0; i < mcols; ++i)
            for (int j = 0; j < mcols; ++j) {
                gk[(size_t)(i * mcols + j)] *= scale[(size_t)i] * scale[(size_t)j];
                gm[(size_t)(i * mcols + j)] = i == j ? 1.0 : gm[(size_t)(i * mcols + j)] * (scale[(size_t)i] * scale[(size_t)j]);
            }
        std::vector<double> theta((size_t)mcols), C((size_t)(mcols * mcols));
        if (!dense_sym_def_eig(mcols, gk.data(), gm.data(), theta.data(), C.data())) return 1;
        std::vector<double> cx((size_t)(mcols * b)), cp((size_t)(std::max(1, mcols - b) * b));
        for (int i = 0; i < mcols; ++i)
            for (int e = 0; e < b; ++e) {
                const double v = C[(size_t)(i * mcols + e)] * scale[(size_t)i];
                if (!std::isfinite(v)) return fail(who + ": the Ritz step gave a non-finite coefficient");
                cx[(size_t)(i * b + e)] = v;
                if (i >= b) cp[(size_t)((i - b) * b + e)] = v;
            }
        for (int e = 0; e < b; ++e) lam[(size_t)e] = theta[(size_t)e];
        std::vector<double*> ox((size_t)b), okx((size_t)b), op((size_t)b), okp((size_t)b);
        for (int e = 0; e < b; ++e) {
            ox[(size_t)e] = ew.x[(size_t)e].rows; okx[(size_t)e] = ew.kx[(size_t)e].rows;
            op[(size_t)e] = ew.p[(size_t)e].rows; okp[(size_t)e] = ew.kp[(size_t)e].rows;
        }
        // X before P: X reads the old P, P reads no X (rows of one launch are read before they are written: in place)
        MG_TRY(launch_block_combine(c, L, mcols, S.data(), b, cx.data(), ox.data()));
        MG_TRY(launch_block_combine(c, L, mcols, KS.data(), b, cx.data(), okx.data()));
        if (mcols > b) {
            MG_TRY(launch_block_combine(c, L, mcols - b, S.data() + b, b, cp.data(), op.data()));
            MG_TRY(launch_block_combine(c, L, mcols - b, KS.data() + b, b, cp.data(), okp.data()));
        }
        return 0;
    };

    auto columns = [&](bool with_w, bool with_p, std::vector<const double*>& S, std::vector<const double*>& KS) {
        S.clear(); KS.clear();
        for (int j = 0; j < b; ++j) { S.push_back(ew.x[(size_t)j].rows); KS.push_back(ew.kx[(size_t)j].rows); }
        if (with_w) for (int j = 0; j < b; ++j) { S.push_back(s.at(j, level).v.rows); KS.push_back(ew.kw[(size_t)j].rows); }
        if (with_p) for (int j = 0; j < b; ++j) { S.push_back(ew.p[(size_t)j].rows); KS.push_back(ew.kp[(size_t)j].rows); }
    };

    // Rayleigh-Ritz on the start block alone: M-orthonormal X, K X and lambda
    std::vector<const double*> S, KS;
    MG_TRY(apply_K(&ew.x, ew.kx));
    columns(false, false, S, KS);
    {
        const int rc = rayleigh_ritz(b, S, KS, 0);
        if (rc == 1) return fail(who + ": the start block is linearly dependent to working precision (the Cholesky factorisation of X^T M X failed)");
        MG_TRY(rc);
    }

    // `fresh`: X, K X and lambda come from a Rayleigh-Ritz step on X alone with K X applied and both Gram matrices computed (the
    // start block's step).  The iteration rotates K X with X and takes X^T M X = I and X^T K X = diag lambda as known, and a nearly
    // dependent [X W P] costs the Ritz vectors orthonormality of the order eps cond(S^T M S); so the block that is about to be
    // returned takes such a step once more, and the stopping test is repeated on what it gives.
    int it = 0, dropped = 0;
    bool have_p = false, fresh = true;
    std::vector<double> h(2 * (size_t)b);
    for (;;) {
        // R_j = K x_j - lambda_j M x_j into lane j's MG_VEC_F with both norms of the stopping test: one kernel per lane
        for (int j = 0; j < b; ++j) {
            EigsResidArgs a{ew.kx[(size_t)j].rows, ew.x[(size_t)j].rows, m, s.at(j, level).f.rows, ew.parts, lam[(size_t)j], n};
            hipLaunchKernelGGL(eigs_residual, fgrid, blk, 0, c->stream, a);
            hipLaunchKernelGGL(fcg_fold, dim3(1), blk, 0, c->stream, ew.parts.get(), (int64_t)fgrid.x, 2, ew.sums.get() + 2 * j);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h.data(), ew.sums.get(), h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        bool converged = true;
        for (int j = 0; j < b; ++j) {
            resid[j] = std::sqrt(h[2 * (size_t)j]) / (std::fabs(lam[(size_t)j]) * std::sqrt(h[2 * (size_t)j + 1]));
            if (j < k && !(resid[j] <= rtol)) converged = false;
        }
        if (converged || it >= max_iter) {
            if (fresh) break;
            MG_TRY(apply_K(&ew.x, ew.kx));
            columns(false, false, S, KS);
            const int rc = rayleigh_ritz(b, S, KS, 0);
            if (rc == 1) return fail(who + ": the Ritz vectors are linearly dependent to working precision (the Cholesky factorisation of X^T M X failed)");
            MG_TRY(rc);
            fresh = true;
            continue;
        }
        fresh = false;

        // W = one V-cycle from a zero guess on each R_j, +0.0 on the Dirichlet rows; K W
        MG_TRY(s.each(all, [&](int) { return zero_vec(c, L, L.v); }));
        MG_TRY(vcycle_batch(c, s, level, all));
        for (int j = 0; j < b; ++j) {
            double* w = s.at(j, level).v.rows;
            if (reinterpret_cast<uintptr_t>(w) % 16) return fail(who + ": misaligned iterate");
            hipLaunchKernelGGL(eigs_mask, dim3(nbk), dim3(256), 0, c->stream, w, m, n);
        }
        HIP_TRY(hipGetLastError());
        // W <- W - X (X^T M W).  The residual of a vector that has converged below the rounding of its Ritz value is that
        // rounding times M x, whose cycle is a multiple of x: without the projection [X W] is then dependent to working precision.
        {
            columns(true, false, S, KS);
            std::vector<double> xw((size_t)(b * b)), coeff((size_t)(2 * b * b), 0.0);
            GramBatch gb;
            MG_TRY(gram_enqueue(c, L, ew, gb, xw.data(), b, 0, 0, b, S.data(), b, S.data() + b, m, false, false));
            MG_TRY(gram_collect(c, ew, gb));
            for (int i = 0; i < b; ++i)
                for (int j = 0; j < b; ++j) {
                    if (!std::isfinite(xw[(size_t)(i * b + j)])) return fail(who + ": iteration " + std::to_string(it) + ": the cycle gave a non-finite vector");
                    coeff[(size_t)(i * b + j)] = -xw[(size_t)(i * b + j)];
                }
            for (int j = 0; j < b; ++j) coeff[(size_t)((b + j) * b + j)] = 1.0;
            std::vector<double*> w((size_t)b);
            for (int j = 0; j < b; ++j) w[(size_t)j] = s.at(j, level).v.rows;
            MG_TRY(launch_block_combine(c, L, 2 * b, S.data(), b, coeff.data(), w.data()));
        }
        MG_TRY(apply_K(nullptr, ew.kw));

        columns(true, have_p, S, KS);
        int rc = rayleigh_ritz((have_p ? 3 : 2) * b, S, KS, b);
        if (rc == 1 && have_p) {        // [X W P] is dependent to working precision: once more without P
            ++dropped;
            columns(true, false, S, KS);
            rc = rayleigh_ritz(2 * b, S, KS, b);
        }
        if (rc == 1)
            return fail(who + ": iteration " + std::to_string(it) + ": the basis [X W] is linearly dependent to working precision (the Cholesky "
                        "factorisation of its Gram matrix failed)");
        MG_TRY(rc);
        have_p = true;
        ++it;
    }

    for (int j = 0; j < b; ++j) {
        lambda[j] = lam[(size_t)j];
        hipLaunchKernelGGL(eigs_mask, dim3(nbk), dim3(256), 0, c->stream, ew.x[(size_t)j].rows, m, n);
        HIP_TRY(hipGetLastError());
        MG_TRY(gather_from(c, L, ew.x[(size_t)j], x_dev[j]));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (iterations) *iterations = it;
    if (restarts) *restarts = dropped;
    return 0;
}

int ensure_stage(mg_context* c, int64_t elems) {
    if ((int64_t)c->stage.count() >= elems) return 0;
    return c->stage.alloc(c, (size_t)elems);
}

int upload_vector(mg_context* c, Level& L, DVector& v, const double* host) {
    MG_TRY(ensure_stage(c, L.n_global));
    ++c->uploads;
    HIP_TRY(hipMemcpyAsync(c->stage, host, (size_t)L.n_global * 8, hipMemcpyHostToDevice, c->stream));
    const unsigned nb = (unsigned)std::min<int64_t>(4096, (L.n_global + 255) / 256);
    hipLaunchKernelGGL(scatter_in, dim3(nb), dim3(256), 0, c->stream, c->stage, L.perm, L.n_global, L.row0, L.g.lead,
                       L.xlen, v.base);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// Replace the int32 column array by offset codes when the level has <= 255 distinct col - row
// values and a specialised width; otherwise the int32 kernels stay in use.
int encode_level(mg_context* c, Level& L) {
    if (!c->use_codes || !coded_width(L.W)) return 0;
    std::vector<int> h_table(kDeltaSlots, kDeltaEmpty);
    int h_counts[2] = {0, 0};
    {
        DevTemp table_t, count_t;
        MG_TRY(table_t.alloc(kDeltaSlots * sizeof(int)));
        MG_TRY(count_t.alloc(2 * sizeof(int)));
        int *const d_table = table_t.as<int>(), *const d_count = count_t.as<int>();
        HIP_TRY(hipMemcpyAsync(d_table, h_table.data(), kDeltaSlots * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(d_count, 0, 2 * sizeof(int), c->stream));
        const int64_t total = L.nslices * L.W * (WAVE * L.R);
        const dim3 grid(blocks_for(total, 256)), blk(256);
        with_int_else<4, 1, 2>(L.R, [&](auto r) { hipLaunchKernelGGL(ell_collect_deltas<decltype(r)::value>, grid, blk, 0, c->stream, L.cols, L.nslices, L.W, L.nloc, L.g.lead, d_table, d_count); });
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_counts, d_count, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(h_table.data(), d_table, kDeltaSlots * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    const int h_count = h_counts[0];
    if (h_counts[1] || h_count > 255) return 0;     // irregular numbering: keep int32 columns
    std::vector<int> offs;
    for (int v : h_table)
        if (v != kDeltaEmpty) offs.push_back(v);
    std::sort(offs.begin(), offs.end());
    if ((int)offs.size() != h_count) return fail("offset table is inconsistent");
    const auto zero = std::find(offs.begin(), offs.end(), 0);
    if (zero == offs.end()) return fail("offset table lacks the diagonal");
    L.ntable = (int)offs.size();
    L.dcode = (int)(zero - offs.begin());
    L.h_offsets = offs;
    L.rb_ok = !L.flat && (L.g.nx & 1) && (L.g.ny & 1);
    for (int o : offs)
        if (o != 0 && (o & 1) == 0) L.rb_ok = false;       // a coupling inside one colour
    offs.resize(256, 0);
    MG_TRY(L.offsets.alloc(c, 256));
    HIP_TRY(hipMemcpyAsync(L.offsets, offs.data(), 256 * sizeof(int), hipMemcpyHostToDevice, c->stream));
    const int CW = (L.W + 7) / 8;
    MG_TRY(L.codes.alloc(c, (size_t)L.nslices * CW * (WAVE * L.R)));
    const dim3 grid(blocks_for(L.nslices * (WAVE * L.R), 256)), blk(256);
    with_int_else<4, 1, 2>(L.R, [&](auto r) { hipLaunchKernelGGL(ell_encode<decltype(r)::value>, grid, blk, 0, c->stream, L.cols, L.codes, L.nslices, L.W, L.nloc, L.g.lead, L.offsets, L.ntable, L.dcode); });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    L.cols.reset();                                                   // 4*W bytes per row back
    L.coded = true;
    return 0;
}

// Row classes (mg_jacobi2.hip.h, "row classes"): a dictionary of the level's distinct FULL rows (five- or seven-point),
// built and verified on the device; levels with more than 255 distinct non-zero rows go without.
int build_row_classes_q(mg_context* c, Level& L, int qbits);

int build_row_classes(mg_context* c, Level& L) {
    if (!c->use_classes || !L.sdia || (L.wu != 3 && L.wu != 4)) return 0;
    MG_TRY(build_row_classes_q(c, L, c->storage_qbits));
    // "storage_auto": rows that are almost repetitive (entries assembled with row-dependent round-off) get one more try
    // in which entries within 4 units in the last place (2^-50 relative: one ulp either way, across a power of two) count as equal
    if (!L.cls && c->storage_auto && c->storage_qbits == 0) MG_TRY(build_row_classes_q(c, L, 2));
    return 0;
}

int build_row_classes_q(mg_context* c, Level& L, int qbits) {
    // scratch: hash tags | slot values | count, flag, slot_class[CLS_SLOTS], hist[256]
    DevTemp scratch_t;
    const size_t tag_bytes = CLS_SLOTS * sizeof(unsigned long long), val_bytes = (size_t)CLS_SLOTS * CLS_W * sizeof(double);
    const size_t int_bytes = (2 + CLS_SLOTS + 256) * sizeof(int);
    MG_TRY(scratch_t.alloc(tag_bytes + val_bytes + int_bytes));
    char* const scratch = scratch_t.as<char>();
    HIP_TRY(hipMemsetAsync(scratch, 0, tag_bytes + val_bytes + int_bytes, c->stream));
    int* const ints = reinterpret_cast<int*>(scratch + tag_bytes + val_bytes);
    // padded like the vectors (vec_reach) so that the pass can read whole tiles around the level unpredicated
    const int64_t cls_lead = ((std::max(L.mlead, vec_reach(L) + (int64_t)L.hd * L.g.plane) + 255) / 256) * 256;
    const int64_t cls_rows = cls_lead + L.nloc + cls_lead + 512;
    DevBuf<unsigned char> cls;          // built here, the level's once the dictionary holds
    DevBuf<double> ctab;
    MG_TRY(cls.alloc(c, (size_t)cls_rows));
    MG_TRY(ctab.alloc(c, 256 * CLS_W));
    ClsArgs a{};
    a.dvals = L.dvals; a.wu = L.wu; a.nloc = L.nloc; a.mlead = L.mlead;
    for (int t = 0; t < 4; ++t) a.up[t] = L.up[t];
    a.tags = reinterpret_cast<unsigned long long*>(scratch);
    a.svals = reinterpret_cast<double*>(scratch + tag_bytes);
    a.count = ints; a.flag = ints + 1; a.slot_class = ints + 2;
    a.hist = reinterpret_cast<unsigned*>(ints + 2 + CLS_SLOTS);
    a.ctab = ctab; a.cls = cls; a.crows = cls_rows; a.clead = cls_lead; a.qbits = qbits;
    const dim3 grid(blocks_for(L.nloc, 256)), egrid(blocks_for(cls_rows, 256)), blk(256);
    int h[2] = {0, 0};
    std::vector<unsigned> hist(256, 0u);
    std::vector<double> tab(256 * CLS_W, 0.0);
    with_int_else<4, 1, 2>(L.R, [&](auto r) { hipLaunchKernelGGL(cls_insert<64 * decltype(r)::value>, grid, blk, 0, c->stream, a); });
    hipLaunchKernelGGL(cls_assign, dim3(1), dim3(64), 0, c->stream, a);
    with_int_else<4, 1, 2>(L.R, [&](auto r) { hipLaunchKernelGGL(cls_encode<64 * decltype(r)::value>, egrid, blk, 0, c->stream, a); });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, ints, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(hist.data(), a.hist, 256 * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(tab.data(), ctab, 256 * CLS_W * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    L.rep_distinct = h[0]; L.rep_cls_qbits = qbits;
    int rc = 0;
    bool escape = false;
    if ((h[0] > 255 || h[1]) && c->cls_escape && L.wu == 4 && !L.flat && L.nloc >= (1 << 16)) {
        // More than 255 distinct rows.  If most rows are still copies of a few (a uniform mesh with some odd rows: other
        // material, other boundary condition), the 254 most frequent rows -- found on a sample of 2^20 rows spread over the
        // level -- keep their class bytes and every other row gets CLS_ESCAPE: the K-sweep march reads such a row from the
        // symmetric diagonal storage.  Worth it while at least three quarters of the rows have a class.
        rc = [&]() -> int {
            DevTemp slot_count_t;       // (slot counts | one bit per hash value: seen once)
            MG_TRY(slot_count_t.alloc((CLS_SLOTS + CLS_SEEN_BITS / 32) * sizeof(unsigned)));
            unsigned* const slot_count = slot_count_t.as<unsigned>();
            HIP_TRY(hipMemsetAsync(slot_count, 0, (CLS_SLOTS + CLS_SEEN_BITS / 32) * sizeof(unsigned), c->stream));
            HIP_TRY(hipMemsetAsync(scratch, 0, tag_bytes + val_bytes + int_bytes, c->stream));
            const int64_t nsample = std::min<int64_t>(L.nloc, (int64_t)1 << 20);
            const dim3 sgrid(blocks_for(nsample, 256));
            with_int_else<4, 1, 2>(L.R, [&](auto r) { hipLaunchKernelGGL(cls_sample_insert<64 * decltype(r)::value>, sgrid, blk, 0, c->stream, a, nsample, slot_count, slot_count + CLS_SLOTS); });
            HIP_TRY(hipGetLastError());
            std::vector<unsigned> cnt(CLS_SLOTS);
            std::vector<double> sv((size_t)CLS_SLOTS * CLS_W);
            HIP_TRY(hipMemcpyAsync(cnt.data(), slot_count, CLS_SLOTS * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(sv.data(), a.svals, val_bytes, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            std::vector<int> order(CLS_SLOTS);
            for (int i = 0; i < CLS_SLOTS; ++i) order[i] = i;
            std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cnt[x] > cnt[y]; });
            std::vector<int> slot_class(CLS_SLOTS, 0);
            std::fill(tab.begin(), tab.end(), 0.0);
            for (int id = 1; id < CLS_ESCAPE && cnt[order[id - 1]] > 0; ++id) {
                slot_class[order[id - 1]] = id;
                for (int t = 0; t < 7; ++t) tab[(size_t)CLS_W * id + t] = sv[(size_t)CLS_W * order[id - 1] + t];
            }
            HIP_TRY(hipMemcpyAsync(a.slot_class, slot_class.data(), CLS_SLOTS * sizeof(int), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(ctab, tab.data(), 256 * CLS_W * sizeof(double), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemsetAsync(a.hist, 0, 256 * sizeof(unsigned), c->stream));
            with_int_else<4, 1, 2>(L.R, [&](auto r) { hipLaunchKernelGGL(cls_encode_escape<64 * decltype(r)::value>, egrid, blk, 0, c->stream, a); });
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(hist.data(), a.hist, 256 * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            return 0;
        }();
        escape = !rc && (double)hist[CLS_ESCAPE] <= 0.25 * (double)L.nloc;
        int kmax = 0;
        // ... and no tile of the march meets more of them at a time than its pool holds
        if (escape && hist[CLS_ESCAPE] > 0) {
            rc = escape_kmax(c, L, cls, cls_lead, &kmax);
            escape = !rc && kmax >= 3;
        }
        if (std::getenv("MG_DEBUG_STORAGE"))
            std::fprintf(stderr, "[mg] row dictionary with escape: %lld rows, tolerance %d bits, %u escape rows, sweeps per pass that fit %d, rc %d\n",
                         (long long)L.nloc, qbits, hist[CLS_ESCAPE], kmax, rc);
        if (escape) { h[0] = 254; h[1] = 0; L.esc_kmax = kmax; L.rep_escape = hist[CLS_ESCAPE]; }
    }
    if (rc || h[0] > 255 || h[1]) return rc;        // too many distinct rows (or a hash collision): plain pass
    L.cls = std::move(cls); L.ctab = std::move(ctab); L.ncls = h[0] + 1; L.cls_lead = cls_lead;
    for (auto& mp : L.plan) mp = Level::MarchPlan{};            // (march plans describe the classes they were built from)
    L.cls_escape = escape && L.rep_escape > 0;
    if (escape) hist[CLS_ESCAPE] = 0;               // (never the most frequent class)
    L.cmain = 0;
    for (int k = 1; k < L.ncls; ++k)
        if (L.cmain == 0 || hist[k] > hist[L.cmain]) L.cmain = k;
    for (int t = 0; t < 8; ++t) L.cm[t] = tab[(size_t)CLS_W * L.cmain + t];
    // what the block pass (mg_jacobiblk.hip.h) needs to know: blocks are cut in grid coordinates
    if (L.wu == 4 && !L.cls_escape && !L.flat && L.up[1] == 1 && L.up[2] == L.g.nx && (int64_t)L.up[3] == L.g.plane) {
        JBCheckArgs k{};
        k.cls = L.cls + L.cls_lead; k.ctab = L.ctab; k.nx = L.g.nx; k.ny = L.g.ny; k.nz = L.g.nk; k.P = L.g.plane; k.n = L.nloc;
        k.flag = reinterpret_cast<int*>(c->partials.get());
        HIP_TRY(hipMemsetAsync(k.flag, 0, sizeof(int), c->stream));
        hipLaunchKernelGGL(sdia_grid_decoupled, dim3(blocks_for(L.nloc, 256)), dim3(256), 0, c->stream, k);
        HIP_TRY(hipGetLastError());
        int flag = 1;
        HIP_TRY(hipMemcpyAsync(&flag, k.flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        L.grid_decoupled = flag == 0;
    }
    return 0;
}

// Stencil classes of an offset-coded level that did not qualify for symmetric diagonals (wide stencils: P2): a
// dictionary of its distinct rows -- the W (offset, value) pairs in stored order, bit for bit -- built and verified on
// the device; levels with more than 255 distinct rows go without.
// What the plane march of mg_lattice.hip.h needs on top of the stencil classes: every entry's offset as (di, dj, dk)
// with |d| <= 2 (else the level keeps the gathering kernel), and the LM_K most frequent classes.
int prepare_lat_march(mg_context* c, Level& L) {
    L.lm_ntop = 0;
    if (L.flat || L.g.ny < 5 || L.g.nx < 5 || !L.scls) return 0;
    const size_t n = (size_t)256 * L.W;
    std::vector<int> off(n), cnt(256), pack(n, 0), hist(256, 0);
    HIP_TRY(hipMemcpy(off.data(), L.s_off, n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cnt.data(), L.s_cnt, 256 * sizeof(int), hipMemcpyDeviceToHost));
    const int64_t P = L.g.plane, nx = L.g.nx;
    for (int cl = 0; cl < L.nscls; ++cl)
        for (int t = 0; t < cnt[cl]; ++t) {
            const int64_t o = off[(size_t)cl * L.W + t];
            const int64_t dk = (o + (o >= 0 ? P / 2 : -(P / 2))) / P, rem = o - dk * P;
            const int64_t dj = (rem + (rem >= 0 ? nx / 2 : -(nx / 2))) / nx, di = rem - dj * nx;
            if (std::llabs(dk) > 2 || std::llabs(dj) > 2 || std::llabs(di) > 2) return 0;
            pack[(size_t)cl * L.W + t] = (int)(((dk + 2) << 16) | ((dj + 2) << 8) | (di + 2));
        }
    int* d_hist = reinterpret_cast<int*>(c->partials.get());
    HIP_TRY(hipMemsetAsync(d_hist, 0, 256 * sizeof(int), c->stream));
    hipLaunchKernelGGL(lm_class_histogram, dim3(1024), dim3(256), 0, c->stream, L.scls, L.nloc, d_hist);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hist.data(), d_hist, 256 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<int> order(L.nscls);
    for (int i = 0; i < L.nscls; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return hist[x] > hist[y]; });
    MG_TRY(L.s_pack.alloc(c, n));
    HIP_TRY(hipMemcpy(L.s_pack, pack.data(), n * sizeof(int), hipMemcpyHostToDevice));
    L.lm_ntop = std::min<int>(LM_K, L.nscls);
    for (int t = 0; t < L.lm_ntop; ++t) L.lm_top[t] = order[t];
    return 0;
}

int build_stencil_classes(mg_context* c, Level& L) {
    if (!c->use_classes || !L.coded || L.sdia || L.flat || L.W < 8) return 0;
    DevTemp scratch_t;
    const size_t tag_bytes = SCLS_SLOTS * sizeof(unsigned long long), row_bytes = SCLS_SLOTS * sizeof(int64_t);
    const size_t int_bytes = (2 + SCLS_SLOTS) * sizeof(int);
    MG_TRY(scratch_t.alloc(tag_bytes + row_bytes + int_bytes));
    char* const scratch = scratch_t.as<char>();
    HIP_TRY(hipMemsetAsync(scratch, 0, tag_bytes + row_bytes + int_bytes, c->stream));
    int* const ints = reinterpret_cast<int*>(scratch + tag_bytes + row_bytes);
    DevBuf<unsigned char> cls;          // built here, the level's once the dictionary holds
    DevBuf<int> s_off, s_cnt;
    DevBuf<double> s_val;
    const size_t crows = (size_t)L.nslices * WAVE * L.R;
    MG_TRY(cls.alloc(c, crows));
    MG_TRY(s_off.alloc(c, (size_t)256 * L.W));
    MG_TRY(s_val.alloc(c, (size_t)256 * L.W));
    MG_TRY(s_cnt.alloc(c, 256));
    HIP_TRY(hipMemsetAsync(cls, 0, crows, c->stream));
    HIP_TRY(hipMemsetAsync(s_off, 0, (size_t)256 * L.W * sizeof(int), c->stream));
    HIP_TRY(hipMemsetAsync(s_val, 0, (size_t)256 * L.W * sizeof(double), c->stream));
    HIP_TRY(hipMemsetAsync(s_cnt, 0, 256 * sizeof(int), c->stream));
    SclsArgs a{};
    a.vals = L.vals; a.codes = L.codes; a.offsets = L.offsets; a.W = L.W; a.dcode = L.dcode; a.nloc = L.nloc; a.nslices = L.nslices;
    a.tags = reinterpret_cast<unsigned long long*>(scratch);
    a.slot_row = reinterpret_cast<int64_t*>(scratch + tag_bytes);
    a.count = ints; a.flag = ints + 1; a.slot_class = ints + 2;
    a.cls = cls; a.s_off = s_off; a.s_val = s_val; a.s_cnt = s_cnt;
    const dim3 grid(blocks_for(L.nloc, 256)), blk(256);
    int h[2] = {0, 0};
    with_int_else<4, 1, 2>(L.R, [&](auto r) {
        constexpr int R = decltype(r)::value;
        hipLaunchKernelGGL(scls_insert<R>, grid, blk, 0, c->stream, a);
        hipLaunchKernelGGL(scls_assign<R>, dim3(1), blk, 0, c->stream, a);
        hipLaunchKernelGGL(scls_encode<R>, grid, blk, 0, c->stream, a);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, ints, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (h[0] > 255 || h[1]) return 0;               // too many distinct rows (or a hash collision): the gathering kernel
    L.scls = std::move(cls); L.s_off = std::move(s_off); L.s_val = std::move(s_val); L.s_cnt = std::move(s_cnt); L.nscls = h[0];
    return prepare_lat_march(c, L);
}

// Symmetric diagonal storage: possible when the level is offset-coded, its offsets come in +/- pairs
// and every lower entry equals its transposed partner bit for bit (mg_kernels.hip.h, sdia_*).
// The coarsest level keeps the coded form (the direct solver reads it).
int repack_sdia(mg_context* c, Level& L, int level) {
    if (!c->use_sdia || !L.coded || level == 0 || L.flat) return 0;
    std::vector<int> offs(256);
    HIP_TRY(hipMemcpy(offs.data(), L.offsets, 256 * sizeof(int), hipMemcpyDeviceToHost));
    offs.resize(L.ntable);
    std::vector<int> up{0};
    for (int o : offs) {
        if (o > 0) up.push_back(o);
        if (o != 0 && std::find(offs.begin(), offs.end(), -o) == offs.end()) return 0;     // not a symmetric pattern
    }
    const int wu = (int)up.size();
    if (2 * wu - 1 != L.ntable || wu > 8) return 0;
    if (up.back() > vec_reach(L)) return 0;                     // x slack would not cover the reach
    const int wu_t = wu <= 3 ? 3 : (wu <= 4 ? 4 : 8);          // template width actually launched
    const int64_t S = (int64_t)WAVE * L.R;
    const int64_t mlead = ((up.back() + S - 1) / S) * S;
    const int64_t mslices = (L.nloc + mlead + S - 1) / S;
    SdiaArgs a{};
    a.vals = L.vals; a.codes = L.codes; a.offsets = L.offsets; a.W = L.W; a.WU = wu_t; a.NU = wu; a.dcode = L.dcode;
    for (int t = 0; t < 8; ++t) a.up[t] = t < wu ? up[t] : 0;
    a.nloc = L.nloc; a.mlead = mlead;
    DevBuf<double> dvals;               // built here, the level's once the matrix has proved symmetric
    MG_TRY(dvals.alloc(c, (size_t)mslices * wu_t * S));
    a.dvals = dvals;
    DevTemp flag_t;                     // flag | pad | report[2] (first asymmetric row + 1, largest ulp distance of a pair)
    int flag = 0;
    unsigned long long report[2] = {~0ull, 0ull};
    int qbits = c->storage_qbits;
    MG_TRY(flag_t.alloc(8 + 2 * sizeof(unsigned long long)));
    int* const d_flag = flag_t.as<int>();
    unsigned long long* d_report = reinterpret_cast<unsigned long long*>(d_flag + 2);
    HIP_TRY(hipMemsetAsync(dvals, 0, (size_t)mslices * wu_t * S * sizeof(double), c->stream));
    const dim3 grid(blocks_for(L.nloc, 256)), blk(256);
    with_int_else<4, 1, 2>(L.R, [&](auto r) { hipLaunchKernelGGL(sdia_fill<decltype(r)::value>, grid, blk, 0, c->stream, a); });
    for (int attempt = 0; attempt < 2; ++attempt) {
        // ("storage_auto": pairs that differ by at most 4 units in the last place -- round-off of an assembly that sums its
        //  element contributions in varying order -- get a second try with that tolerance; the upper half of a pair is kept)
        HIP_TRY(hipMemsetAsync(d_flag, 0, 8, c->stream));
        HIP_TRY(hipMemcpyAsync(d_report, report, sizeof(report), hipMemcpyHostToDevice, c->stream));
        with_int_else<4, 1, 2>(L.R, [&](auto r) { hipLaunchKernelGGL(sdia_check<decltype(r)::value>, grid, blk, 0, c->stream, a, d_flag, qbits, d_report); });
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(report, d_report, sizeof(report), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (!(flag && attempt == 0 && c->storage_auto && qbits == 0 && report[1] <= 4)) break;
        qbits = 2;
        report[0] = ~0ull; report[1] = 0ull;
    }
    L.rep_first_asym = report[0] == ~0ull ? -1 : (int64_t)report[0] - 1;
    L.rep_max_ulps = report[1] >= (1ull << 62) ? -1 : (int64_t)report[1];
    L.rep_sym = flag ? 0 : (report[0] == ~0ull ? 1 : 2);
    L.rep_sym_qbits = flag ? 0 : qbits;
    if (flag) return 0;                                         // not symmetric: keep the coded form
    L.dvals = std::move(dvals); L.sdia = true; L.wu = wu_t; L.mlead = mlead; L.mslices = mslices;
    for (int t = 0; t < 8; ++t) L.up[t] = t < wu ? up[t] : 0;
    // padded template slots (wu < wu_t) hold zeros and offset 0: they add 0 * x[row]
    L.vals.reset();
    L.codes.reset();
    return build_row_classes(c, L);
}

int finish_level(mg_context* c, Level& L) {
    MG_TRY(alloc_level_vectors(c, L));
    L.set = true;
    return 0;
}

// the storage analysis of a level whose tiles (vals, cols, dinv) are written: every generated or handed-over matrix
int finish_stored_rows(mg_context* c, Level& L, int level) {
    MG_TRY(encode_level(c, L));
    MG_TRY(repack_sdia(c, L, level));
    MG_TRY(build_stencil_classes(c, L));
    L.has_matrix = true;
    return 0;
}

int alloc_ell(mg_context* c, Level& L) {
    L.R = c->rows_per_lane;
    L.nslices = (L.nloc + (int64_t)WAVE * L.R - 1) / ((int64_t)WAVE * L.R);
    const size_t ell = (size_t)L.nslices * L.W * (WAVE * L.R);
    MG_TRY(L.vals.alloc(c, ell));
    MG_TRY(L.cols.alloc(c, ell));
    MG_TRY(L.dinv.alloc(c, (size_t)L.nslices * WAVE * L.R));
    const unsigned nb = blocks_for((int64_t)ell, 256);
    const bool known = with_int<1, 2, 4>(L.R, [&](auto r) {
        hipLaunchKernelGGL(ell_fill_padding<decltype(r)::value>, dim3(nb), dim3(256), 0, c->stream, L.vals, L.cols, L.nslices, L.W, L.nloc, L.g.lead);
    });
    if (!known) return fail("rows_per_lane must be 1, 2 or 4");
    HIP_TRY(hipGetLastError());
    return 0;
}

void sorted_offsets(int dim, int out[15][3], int* n) {
    std::vector<std::array<int, 3>> offs;
    if (dim == 2) {
        const int b[3][2] = {{1, 0}, {0, 1}, {1, 1}};
        offs.push_back({0, 0, 0});
        for (auto& o : b) {
            offs.push_back({o[0], 0, o[1]});
            offs.push_back({-o[0], 0, -o[1]});
        }
    } else {
        const int b[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};
        offs.push_back({0, 0, 0});
        for (auto& o : b) {
            offs.push_back({o[0], o[1], o[2]});
            offs.push_back({-o[0], -o[1], -o[2]});
        }
    }
    std::sort(offs.begin(), offs.end(), [](const std::array<int, 3>& a, const std::array<int, 3>& b) {
        if (a[2] != b[2]) return a[2] < b[2];
        if (a[1] != b[1]) return a[1] < b[1];
        return a[0] < b[0];
    });
    *n = (int)offs.size();
    for (int t = 0; t < *n; ++t)
        for (int d = 0; d < 3; ++d) out[t][d] = offs[t][d];
}

// The stored-level pipeline of every generator: geometry, tiles of width W, vectors, the generating kernel, the storage
// analysis, and F once more as the level's true right-hand side.  `launch(L, grid, counts)` enqueues the kernel for L.R rows
// per lane: it writes the tiles, 1 / diagonal and F and counts the kept and the non-zero entries into counts[0], counts[1].
template <class Launch>
int gen_stored_level(mg_context* c, int level, int N, int W, Launch launch) {
    Level& L = c->L[level];
    LevelBuild build(c, L);
    MG_TRY(setup_geometry(c, L, level, N));
    L.W = W;
    MG_TRY(alloc_ell(c, L));
    MG_TRY(alloc_level_vectors(c, L));
    unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(c->partials.get());
    HIP_TRY(hipMemsetAsync(d_counts, 0, 2 * sizeof(unsigned long long), c->stream));
    launch(L, grid3(L.g, L.g.nk), d_counts);
    HIP_TRY(hipGetLastError());
    unsigned long long counts[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    L.nnz_stored = counts[0];
    L.nnz_nonzero = counts[1];
    MG_TRY(finish_stored_rows(c, L, level));
    // the generated right-hand side is also this level's true right-hand side for mg_fmg
    if (level + 1 < c->nlev) {
        MG_TRY(vec_alloc(c, L, &L.ftrue));
        HIP_TRY(hipMemcpyAsync(L.ftrue.base, L.f.base, (size_t)L.xlen * 8, hipMemcpyDeviceToDevice, c->stream));
    }
    L.set = true;
    return build.done();
}

// what gen_poisson and gen_diffusion take alike: the mesh width, the load's scale, the stencil's offsets and the level
// width W (the grid follows at the launch, once the level has its geometry)
GenArgs gen_args(const mg_context* c, int N, int prune_zeros) {
    GenArgs a{};
    a.N = N; a.dim = c->dim; a.prune = prune_zeros;
    a.h = 1.0 / (double)N;
    a.fh = (c->dim == 2 ? -6.0 : -12.0) * std::pow(a.h, (double)c->dim);
    sorted_offsets(c->dim, a.off, &a.noff);
    a.W = prune_zeros ? (c->dim == 2 ? 5 : 7) : a.noff;
    return a;
}

// The end of a handle, whole or half-created: what is no device memory is destroyed by hand, the memory by its owners
// (DevBuf / DVector members of the handle, its levels and the direct solver).
struct ContextDeleter {
    void operator()(mg_context* c) const {
        (void)hipSetDevice(c->device);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
        drop_graphs(c);
        if (c->h_scalars) (void)hipHostFree(c->h_scalars);
        if (c->h_lanes) (void)hipHostFree(c->h_lanes);
        if (c->comm.h_stage) (void)hipHostFree(c->comm.h_stage);
        if (c->comm.nccl) g_rccl.CommDestroy(c->comm.nccl);
        if (c->ev_boundary) (void)hipEventDestroy(c->ev_boundary);
        if (c->ev_halo) (void)hipEventDestroy(c->ev_halo);
        if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
        if (c->stream) (void)hipStreamDestroy(c->stream);
        delete c;
    }
};

}  // namespace

// =====================================================================================================
extern "C" {

const char* mg_last_error(void) { return g_err.c_str(); }

int mg_create(int n_levels, int dim, int device, mg_handle* out) {
    if (!out) return fail("null output handle");
    *out = nullptr;
    if (n_levels < 1 || n_levels > 32) return fail("n_levels must be in 1..32");
    if (dim != 2 && dim != 3) return fail("dim must be 2 or 3");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail("no HIP device visible: this library has no CPU path");
    if (device < 0 || device >= ndev) return fail("device index out of range");
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<mg_context, ContextDeleter> owner(new mg_context());       // (a failure below leaves nothing behind)
    mg_context* const c = owner.get();
    if (const char* e = std::getenv("MG_COMM_PRIORITY")) c->comm_priority = std::atoi(e) != 0;      // experiments only
    if (const char* e = std::getenv("MG_POINT_GROUP")) c->pt_group = std::min(8, std::max(1, std::atoi(e)));    // measurements only
    c->dim = dim;
    c->nlev = n_levels;
    c->device = device;
    c->L.resize(n_levels);
    c->smoother_counts.resize(n_levels);
    HIP_TRY(hipGetDeviceProperties(&c->prop, device));
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    {
        // the communication stream outranks the main one: the exchange chain of a slab sweep runs beside a pass whose
        // workgroups fill every CU (measured on one slab of eight it makes no difference: 53.2 against 53.7 ms per cycle)
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipStreamCreateWithPriority(&c->comm_stream, hipStreamNonBlocking, c->comm_priority ? greatest : least));
    }
    HIP_TRY(hipEventCreateWithFlags(&c->ev_boundary, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_halo, hipEventDisableTiming));
    MG_TRY(c->partials.alloc(c, 2 * kMaxParts));
    MG_TRY(c->scalars.alloc(c, 8));
    MG_TRY(c->done.alloc(c, 1));
    HIP_TRY(hipMemsetAsync(c->done, 0, sizeof(int), c->stream));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->h_scalars), 16 * sizeof(double), hipHostMallocDefault));
    *out = owner.release();
    return 0;
}

int mg_destroy(mg_handle c) {
    if (c) ContextDeleter{}(c);
    return 0;
}

int mg_device_info(mg_handle c, char* buf, size_t buflen) {
    if (!c || !buf || buflen == 0) return fail("bad arguments");
    snprintf(buf, buflen, "%s %s %d CUs %.1f GiB", c->prop.name, c->prop.gcnArchName, c->prop.multiProcessorCount,
             (double)c->prop.totalGlobalMem / (1024.0 * 1024.0 * 1024.0));
    return 0;
}

int mg_comm_unique_id(void* id_out, size_t id_bytes) {
    if (!id_out || id_bytes < sizeof(ncclUniqueId)) return fail("id buffer must hold 128 bytes");
    MG_TRY(load_rccl());
    ncclUniqueId id;
    NCCL_TRY(g_rccl.GetUniqueId(&id));
    memcpy(id_out, &id, sizeof(id));
    return 0;
}

int mg_comm_selftest(int device) {
    MG_TRY(load_rccl());
    HIP_TRY(hipSetDevice(device));
    ncclUniqueId id;
    NCCL_TRY(g_rccl.GetUniqueId(&id));
    ncclComm_t comm = nullptr;
    NCCL_TRY(g_rccl.CommInitRank(&comm, 1, id, 0));
    hipStream_t s = nullptr;
    DevTemp d_t;
    const int n = 1024;
    std::vector<double> h(3 * n);
    for (int i = 0; i < n; ++i) { h[i] = 1.0 + i; h[n + i] = 0.0; h[2 * n + i] = -1.0; }
    int rc = [&]() -> int {
        HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        MG_TRY(d_t.alloc(3 * n * sizeof(double)));
        double* const d = d_t.as<double>();
        HIP_TRY(hipMemcpyAsync(d, h.data(), 3 * n * sizeof(double), hipMemcpyHostToDevice, s));
        NCCL_TRY(g_rccl.AllReduce(d, d, n, ncclDouble, ncclSum, comm, s));            // one rank: unchanged
        NCCL_TRY(g_rccl.GroupStart());
        NCCL_TRY(g_rccl.Broadcast(d, d, n, ncclDouble, 0, comm, s));
        NCCL_TRY(g_rccl.GroupEnd());
        NCCL_TRY(g_rccl.GroupStart());
        NCCL_TRY(g_rccl.Send(d, n, ncclDouble, 0, comm, s));                          // to self
        NCCL_TRY(g_rccl.Recv(d + n, n, ncclDouble, 0, comm, s));
        NCCL_TRY(g_rccl.GroupEnd());
        HIP_TRY(hipMemcpyAsync(h.data(), d, 3 * n * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int i = 0; i < n; ++i)
            if (h[i] != 1.0 + i || h[n + i] != 1.0 + i || h[2 * n + i] != -1.0) return fail("RCCL self-test: wrong data");
        return 0;
    }();
    if (s) (void)hipStreamDestroy(s);
    g_rccl.CommDestroy(comm);
    return rc;
}

static int comm_common(mg_handle c, int rank, int world, int64_t replicate_below) {
    if (!c) return fail("null handle");
    if (world < 1 || rank < 0 || rank >= world) return fail("bad rank/world");
    for (auto& L : c->L)
        if (L.set) return fail("mg_set_comm must precede level set-up");
    c->comm.rank = rank;
    c->comm.world = world;
    c->comm.replicate_below = replicate_below;
    return 0;
}

int mg_set_comm(mg_handle c, int rank, int world, const void* nccl_unique_id, size_t id_bytes, int64_t replicate_below) {
    MG_TRY(comm_common(c, rank, world, replicate_below));
    if (world == 1) return 0;
    if (!nccl_unique_id || id_bytes < sizeof(ncclUniqueId)) return fail("missing RCCL unique id");
    MG_TRY(load_rccl());
    HIP_TRY(hipSetDevice(c->device));
    ncclUniqueId id;
    memcpy(&id, nccl_unique_id, sizeof(id));
    NCCL_TRY(g_rccl.CommInitRank(&c->comm.nccl, world, id, rank));
    return 0;
}

int mg_set_comm_callbacks(mg_handle c, int rank, int world, mg_exchange_fn ex, mg_allreduce_fn ar, mg_allgatherv_fn ag,
                          void* user, int64_t replicate_below) {
    MG_TRY(comm_common(c, rank, world, replicate_below));
    if (world > 1 && (!ex || !ar || !ag)) return fail("all three callbacks are required");
    c->comm.ex = ex;
    c->comm.ar = ar;
    c->comm.ag = ag;
    c->comm.user = user;
    return 0;
}

int mg_set_params(mg_handle c, int mu1, int mu2, double omega, int restriction, int smoother, double coarse_rtol,
                  int coarse_maxit, int keep_err) {
    if (!c) return fail("null handle");
    if (mu1 < 0 || mu2 < 0) return fail("mu1/mu2 must be >= 0");
    if (restriction != MG_RESTRICT_INJECTION && restriction != MG_RESTRICT_FULL_WEIGHTING && restriction != MG_RESTRICT_TABLE &&
        restriction != MG_RESTRICT_P1_TRANSPOSE)
        return fail("unknown restriction");
    if (smoother != MG_SMOOTH_JACOBI && smoother != MG_SMOOTH_RBGS && smoother != MG_SMOOTH_MCGS && smoother != MG_SMOOTH_CHEBYSHEV)
        return fail("unknown smoother");
    const double rtol = coarse_rtol > 0 ? coarse_rtol : c->coarse_rtol;
    const int maxit = coarse_maxit > 0 ? coarse_maxit : c->coarse_maxit;
    // captured V-cycles (vcycle_graphed) are keyed on the epoch: callers such as the Python shim set the same
    // parameters before every cycle, which must not throw the graphs away
    if (mu1 == c->mu1 && mu2 == c->mu2 && omega == c->omega && restriction == c->restriction && smoother == c->smoother &&
        rtol == c->coarse_rtol && maxit == c->coarse_maxit && keep_err == c->keep_err)
        return 0;
    ++c->epoch;
    c->mu1 = mu1; c->mu2 = mu2; c->omega = omega; c->restriction = restriction; c->smoother = smoother;
    c->coarse_rtol = rtol; c->coarse_maxit = maxit;
    c->keep_err = keep_err;
    return 0;
}

int mg_set_chebyshev(mg_handle c, int eig_steps, double lower_ratio, double upper_factor) {
    if (!c) return fail("null handle");
    if (eig_steps < 2 || eig_steps > 1000) return fail("eig_steps must be in 2..1000");
    if (!(lower_ratio > 1.0) || !std::isfinite(lower_ratio)) return fail("lower_ratio must be a finite number > 1");
    if (!(upper_factor > 0.0) || !std::isfinite(upper_factor)) return fail("upper_factor must be a finite number > 0");
    if (eig_steps == c->cheb_eig_steps && lower_ratio == c->cheb_lower_ratio && upper_factor == c->cheb_upper_factor) return 0;
    ++c->epoch;
    c->cheb_eig_steps = eig_steps; c->cheb_lower_ratio = lower_ratio; c->cheb_upper_factor = upper_factor;
    for (auto& L : c->L) L.cheb_est_ok = false;
    return 0;
}

int mg_set_chebyshev_bounds(mg_handle c, int level, double lmin, double lmax) {
    MG_TRY(check_level(c, level, false));
    if (lmax > 0.0 && (!std::isfinite(lmax) || !std::isfinite(lmin) || !(lmin < lmax)))
        return fail("Chebyshev bounds must be finite with lmin < lmax");
    ++c->epoch;
    Level& L = c->L[level];
    L.cheb_user_lmax = lmax > 0.0 ? lmax : 0.0;
    L.cheb_user_lmin = lmax > 0.0 && lmin > 0.0 ? lmin : 0.0;
    return 0;
}

int mg_chebyshev_bounds(mg_handle c, int level, double* lmin, double* lmax, double* lmax_estimate) {
    MG_TRY(need_matrix(c, level));
    HIP_TRY(hipSetDevice(c->device));
    Level& L = c->L[level];
    // (the estimate runs if it has not, except on a non-symmetric level with the caller's interval: it would be refused)
    if (!L.cheb_est_ok && (L.cheb_user_lmax <= 0.0 || L.rep_sym != 0)) MG_TRY(cheb_estimate(c, level));
    double lo = 0.0, hi = 0.0;
    MG_TRY(cheb_interval(c, level, &lo, &hi));
    if (lmin) *lmin = lo;
    if (lmax) *lmax = hi;
    if (lmax_estimate) *lmax_estimate = L.cheb_est_ok ? L.cheb_lmax_est : 0.0;
    return 0;
}

int mg_chebyshev_estimate_bytes(mg_handle c, int64_t* bytes) {
    if (!c || !bytes) return fail("bad arguments");
    *bytes = c->cheb_peak_bytes;
    return 0;
}

int mg_set_prolongation_table(mg_handle c, const int* count, const int* offsets, const double* weights) {
    if (!c) return fail("null handle");
    HIP_TRY(hipSetDevice(c->device));
    ++c->epoch;
    (void)hipStreamSynchronize(c->stream);
    c->ptab_count.reset(); c->ptab_off.reset(); c->ptab_w.reset();
    c->p1_prolong = 0;                                            // (a table and the P1 embedding exclude each other)
    if (!count && !offsets && !weights) return 0;                 // back to the reference's interpolation
    if (!count || !offsets || !weights) return fail("null table");
    for (int r = 0; r < 64; ++r) {
        if (count[r] < 0 || count[r] > 10) return fail("a residue has more than 10 entries");
        for (int e = 0; e < count[r]; ++e)
            for (int d = 0; d < 3; ++d)
                if (offsets[(r * 10 + e) * 3 + d] < 0 || offsets[(r * 10 + e) * 3 + d] > 2) return fail("table offsets must be 0..2");
    }
    MG_TRY(c->ptab_count.alloc(64 * sizeof(int)));
    MG_TRY(c->ptab_off.alloc(64 * 10 * 3 * sizeof(int)));
    MG_TRY(c->ptab_w.alloc(64 * 10 * sizeof(double)));
    HIP_TRY(hipMemcpy(c->ptab_count.p, count, 64 * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->ptab_off.p, offsets, 64 * 10 * 3 * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->ptab_w.p, weights, 64 * 10 * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

int mg_set_prolongation_p1(mg_handle c, int enable) {
    if (!c) return fail("null handle");
    if (enable != 0 && enable != 1) return fail("enable must be 0 or 1");
    HIP_TRY(hipSetDevice(c->device));
    ++c->epoch;
    if (enable && c->ptab_count.p) {                                // a table and the P1 embedding exclude each other
        (void)hipStreamSynchronize(c->stream);
        c->ptab_count.reset(); c->ptab_off.reset(); c->ptab_w.reset();
    }
    c->p1_prolong = enable;
    return 0;
}

int mg_set_restriction_table(mg_handle c, int max_entries, const int* count, const int* offsets, const double* weights) {
    if (!c) return fail("null handle");
    HIP_TRY(hipSetDevice(c->device));
    ++c->epoch;
    (void)hipStreamSynchronize(c->stream);
    c->rtab_count.reset(); c->rtab_off.reset(); c->rtab_w.reset(); c->rtab_m = 0;
    if (!count && !offsets && !weights) return 0;
    if (!count || !offsets || !weights || max_entries < 1 || max_entries > 4096) return fail("bad restriction table");
    for (int t = 0; t < 8; ++t) {
        if (count[t] < 0 || count[t] > max_entries) return fail("a type has more entries than max_entries");
        for (int e = 0; e < count[t]; ++e)
            for (int d = 0; d < 3; ++d)
                if (std::abs(offsets[((size_t)t * max_entries + e) * 3 + d]) > 4) return fail("table offsets must be within +-4");
    }
    const size_t n = (size_t)8 * max_entries;
    MG_TRY(c->rtab_count.alloc(8 * sizeof(int)));
    MG_TRY(c->rtab_off.alloc(n * 3 * sizeof(int)));
    MG_TRY(c->rtab_w.alloc(n * sizeof(double)));
    HIP_TRY(hipMemcpy(c->rtab_count.p, count, 8 * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->rtab_off.p, offsets, n * 3 * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->rtab_w.p, weights, n * sizeof(double), hipMemcpyHostToDevice));
    c->rtab_m = max_entries;
    return 0;
}

int mg_set_tuning(mg_handle c, const char* key, int64_t value) {
    if (!c || !key) return fail("bad arguments");
    ++c->epoch;
    const std::string k(key);
    if (k == "graph") {
        c->use_graph = value != 0;
        return 0;
    }
    if (k == "slab_pair_form") {
        if (value != 0 && value != 1) return fail("slab_pair_form must be 0 or 1");
        c->slab_pair_form = (int)value;
        return 0;
    }
    if (k == "graph_comm") {
        c->graph_comm = value != 0;
        return 0;
    }
    if (k == "rows_per_lane") {
        if (value != 1 && value != 2 && value != 4) return fail("rows_per_lane must be 1, 2 or 4");
        for (auto& L : c->L)
            if (L.set) return fail("rows_per_lane must be chosen before level set-up");
        c->rows_per_lane = (int)value;
    } else if (k == "xcd_chunk") {
        if (value < 1 || value > 4096) return fail("xcd_chunk out of range");
        c->chunk = (unsigned)value;
    } else if (k == "offset_codes") {
        for (auto& L : c->L)
            if (L.set) return fail("offset_codes must be chosen before level set-up");
        c->use_codes = value != 0;
    } else if (k == "symmetric_storage") {
        for (auto& L : c->L)
            if (L.set) return fail("symmetric_storage must be chosen before level set-up");
        c->use_sdia = value != 0;
    } else if (k == "storage_ulps") {
        for (auto& L : c->L)
            if (L.set) return fail("storage_ulps must be chosen before level set-up");
        if (value < 0 || value > 4096) return fail("storage_ulps must be in 0..4096");
        int q = 0;
        while ((1ll << q) < value) ++q;
        c->storage_qbits = value > 0 ? std::max(1, q) : 0;
    } else if (k == "fuse_block") {
        if (value < 0 || value > 2) return fail("fuse_block must be 0, 1 or 2");
        c->fuse_block = (int)value;
    } else if (k == "fuse_block_min_rows") {
        c->fuse_block_min_rows = value;
    } else if (k == "fuse_block_max_rows") {
        c->fuse_block_max_rows = value;
    } else if (k == "fuse_block_k") {
        if (value != 0 && (value < 2 || value > 4)) return fail("fuse_block_k must be 0 or 2..4");
        c->fuse_block_k = (int)value;
    } else if (k == "fuse_block_ez") {
        if (value != 0 && value != 11 && value != 19) return fail("fuse_block_ez must be 0, 11 or 19");
        c->fuse_block_ez = (int)value;
    } else if (k == "direct_block_rows") {
        if (value < 1 || value > 2304) return fail("direct_block_rows must be in 1..2304");
        if (c->direct.tried) return fail("direct_block_rows must be chosen before the coarsest level is factored");
        c->direct_block_rows = (int)value;
    } else if (k == "fuse_2d_lines") {
        if (value != 0 && value != 16 && value != 32 && value != 64) return fail("fuse_2d_lines must be 0, 16, 32 or 64");
        c->fuse_2d_lines = (int)value;
    } else if (k == "gen_odd_rows") {
        if (value < 0 || value > 10000) return fail("gen_odd_rows: rows in 10000");
        c->gen_odd_rows = (int)value;
    } else if (k == "row_escape") {
        for (auto& L : c->L)
            if (L.set) return fail("row_escape must be chosen before level set-up");
        c->cls_escape = value != 0;
    } else if (k == "storage_auto") {
        for (auto& L : c->L)
            if (L.set) return fail("storage_auto must be chosen before level set-up");
        c->storage_auto = value != 0;
    } else if (k == "row_classes") {
        for (auto& L : c->L)
            if (L.set) return fail("row_classes must be chosen before level set-up");
        c->use_classes = value != 0;
    } else if (k == "strip_slices") {
        if (value < 0 || value > 4096 || value % 4) return fail("strip_slices must be a multiple of 4 in 0..4096");
        c->strip_slices = (int)value;
    } else if (k == "nontemporal") {
        c->nontemporal = value != 0;
    } else if (k == "lds_pad") {
        if (value < 0 || value > mg_context::kLdsPadMax) return fail("lds_pad must be in 0.." + std::to_string(mg_context::kLdsPadMax));
        c->lds_pad = (int)value;
    } else if (k == "halo_planes") {
        if (value != 1 && value != 2) return fail("halo_planes must be 1 or 2");
        for (auto& L : c->L)
            if (L.set) return fail("halo_planes must be chosen before level set-up");
        c->halo_planes = (int)value;
    } else if (k == "halo_depth") {
        if (value < 0 || value > 5) return fail("halo_depth must be in 0..5");
        for (auto& L : c->L)
            if (L.set) return fail("halo_depth must be chosen before level set-up");
        c->halo_depth = (int)value;
    } else if (k == "overlap") {
        c->overlap = value != 0;
    } else if (k == "overlap_min_rows") {
        c->overlap_min_rows = value;
    } else if (k == "require_diagonal") {
        c->require_diagonal = value != 0;
    } else if (k == "fuse_restrict") {
        c->fuse_restrict = value != 0;
    } else if (k == "fuse_sweeps") {
        c->fuse_sweeps = value != 0;
    } else if (k == "fuse_min_rows") {
        c->fuse_min_rows = value;
    } else if (k == "fuse_shape") {
        if (value < 0 || value > 3) return fail("fuse_shape must be 0..3");
        c->fuse_shape = (int)value;
    } else if (k == "march_sweeps") {
        c->march_sweeps = value != 0;
    } else if (k == "march_min_rows") {
        c->march_min_rows = value;
    } else if (k == "march_shape") {
        if (value < 0 || value > 1) return fail("march_shape must be 0 or 1");
        c->march_shape = (int)value;
    } else if (k == "fuse_small_2d_rows") {
        c->fuse_small_2d_rows = value;
    } else if (k == "fuse_small") {
        c->fuse_small = value != 0;
    } else if (k == "fuse_2d") {
        c->fuse_2d = value != 0;
    } else if (k == "fuse_2d_k") {
        if (value < 2 || value > 5) return fail("fuse_2d_k must be in 2..5");
        c->fuse_2d_k = (int)value;
    } else if (k == "lattice_march") {
        c->lattice_march = value != 0;
    } else if (k == "lattice_march_min_rows") {
        c->lattice_march_min_rows = value;
    } else if (k == "dkappa_gather") {
        c->dkappa_gather = value != 0;
    } else if (k == "lattice_gs2") {
        c->lattice_gs2 = value != 0;
    } else if (k == "lattice_tile") {
        if (value < 0 || value > 2) return fail("lattice_tile must be 0, 1 or 2");
        c->lattice_tile = (int)value;
    } else if (k == "lattice_segments") {
        if (value < 0 || value > 4096) return fail("lattice_segments must be in 0..4096");
        c->lattice_segments = (int)value;
    } else if (k == "fuse_xcd_chunk") {
        if (value < 1 || value > 512) return fail("fuse_xcd_chunk must be in 1..512");
        c->fuse_xcd_chunk = (int)value;
    } else if (k == "cls_blocks_per_cu") {
        if (value < 1 || value > 64) return fail("cls_blocks_per_cu must be in 1..64");
        c->cls_blocks_per_cu = (int)value;
    } else if (k == "fuse_wi") {
        c->fuse_wi = (int)value;
    } else if (k == "fuse_even") {
        c->fuse_even = value != 0;
    } else if (k == "class_sweeps") {
        c->class_sweeps = value != 0;
    } else if (k == "fuse_plain_shape") {
        if (value < 0 || value > 2) return fail("fuse_plain_shape must be 0..2");
        c->fuse_plain_shape = (int)value;
    } else if (k == "fuse_plain") {
        if (value != 1 && value != 2) return fail("fuse_plain must be 1 or 2");
        c->fuse_plain = (int)value;
    } else if (k == "fuse_k") {
        if (value < 0 || value > 5) return fail("fuse_k must be in 0..5 (below 3: pairs of sweeps only)");
        c->fuse_k = (int)value;
    } else if (k == "fuse_k_shape") {
        if (value == 0 || value == 2 || value == 3 || value == 5 || value == 6) return fail("fuse_k_shape: the tile shapes 0, 2, 3, 5 and 6 were retired");
        if (value != -1 && value != 1 && value != 4 && (value < 7 || value > 9)) return fail("fuse_k_shape must be 1, 4, 7, 8 or 9, or -1 (by sweeps per pass)");
        c->fuse_k_shape = (int)value;
    } else if (k == "fuse_k_slab_min_rows") {
        c->fuse_k_slab_min_rows = value;
    } else if (k == "fuse_k_slab_min_sweeps") {
        if (value < 2) return fail("fuse_k_slab_min_sweeps must be at least 2");
        c->fuse_k_slab_min_sweeps = (int)value;
    } else if (k == "fuse_k_min_rows") {
        c->fuse_k_min_rows = value;
    } else if (k == "fuse_k_small_rows") {
        c->fuse_k_small_rows = value;
    } else if (k == "fuse_k5_min_rows") {
        c->fuse_k5_min_rows = value;
    } else if (k == "fuse_k_rim_min_rows") {
        c->fuse_k_rim_min_rows = value;
    } else if (k == "fuse_k4_min_rows") {
        c->fuse_k4_min_rows = value;
    } else if (k == "fuse_k_nt_store") {
        c->fuse_k_nt_store = value != 0;
    } else if (k == "fuse_k_min_side") {
        if (value < 16 || value > 32) return fail("fuse_k_min_side must be in 16..32");
        c->fuse_k_min_side = (int)value;
    } else if (k == "fuse_k_tail") {
        if (value < 0) return fail("fuse_k_tail must be >= 0");
        c->fuse_k_tail = (int)value;            // (> 1: the number of resident workgroups to plan for -- tests)
    } else if (k == "fuse_k_small_tiles") {
        c->fuse_k_small_tiles = value != 0;
    } else if (k == "fuse_k_load_early") {
        if (value != 0 && value != 1) return fail("fuse_k_load_early must be 0 or 1");
        c->fuse_k_load_early = (int)value;
    } else if (k == "fuse_k_load_early_min_rows") {
        if (value < 0) return fail("fuse_k_load_early_min_rows must be >= 0");
        c->fuse_k_load_early_min_rows = value;
    } else if (k == "fuse_k_plan") {
        c->fuse_k_plan = value != 0;
    } else if (k == "fuse_k_segments") {
        if (value < 0) return fail("fuse_k_segments must be >= 0");
        c->fuse_k_segments = (int)value;
    } else if (k == "fuse_classes") {
        c->fuse_classes = value != 0;
    } else if (k == "fuse_nontemporal") {
        c->fuse_nontemporal = value != 0;
    } else if (k == "fuse_segments") {
        if (value < 0) return fail("fuse_segments must be >= 0");
        c->fuse_segments = (int)value;
    } else if (k == "coarse_direct") {
        c->use_direct = value != 0;
        free_direct(c);
    } else if (k == "pcg_chunk") {
        if (value < 1) return fail("pcg_chunk must be positive");
        c->pcg_chunk = (int)value;
    } else if (k == "mf_batch") {
        if (value < 0 || value > MF_BATCH_MAX) return fail("mf_batch must be in 0.." + std::to_string(MF_BATCH_MAX) + " (0 or 1: never fuse)");
        c->mf_batch = (int)value;
    } else {
        return fail("unknown tuning key " + k);
    }
    return 0;
}

namespace {

// grid_index[dof] (int64, caller) -> L.perm (int32, device), validated as a permutation of the nodes.
int upload_permutation(mg_context* c, Level& L, const int64_t* grid_index, int64_t n_rows) {
    if (!grid_index) return 0;
    std::vector<int> p32((size_t)n_rows);
    std::vector<char> seen((size_t)n_rows, 0);
    for (int64_t d = 0; d < n_rows; ++d) {
        const int64_t p = grid_index[d];
        if (p < 0 || p >= n_rows || seen[(size_t)p]) return fail("grid_index is not a permutation of the grid nodes");
        seen[(size_t)p] = 1;
        p32[(size_t)d] = (int)p;
    }
    MG_TRY(L.perm.alloc(c, (size_t)n_rows));
    HIP_TRY(hipMemcpy(L.perm, p32.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice));
    return 0;
}

// `local_cols` (per-rank hand-off): the matrix holds this rank's owned rows only, its column indices are local ids in
// [0, n_cols) and local_cols[id] is the global lexicographic node of each (ids 0 .. n_rows-1 are the rows themselves);
// otherwise rows and columns are global DoF numbers and `grid_index` (or the identity) maps them to nodes.
int build_level_from_csr(mg_context* c, int level, Level& L, int64_t n_rows, int64_t nnz, const void* indptr,
                         int indptr_is_64, const int32_t* indices, const double* data, const int64_t* grid_index,
                         int prune_zeros, bool vectors = true, const int64_t* local_cols = nullptr, int64_t n_cols = 0,
                         bool device_csr = false) {
    // upload the hand-off (device_csr: the three arrays are device memory already -- mg_galerkin_level)
    DevTemp d_ptr, d_idx, d_val;
    const size_t ptr_bytes = (size_t)(n_rows + 1) * (indptr_is_64 ? 8 : 4);
    if (!device_csr) {
        MG_TRY(d_ptr.alloc(ptr_bytes));
        MG_TRY(d_idx.alloc((size_t)nnz * 4));
        MG_TRY(d_val.alloc((size_t)nnz * 8));
        HIP_TRY(hipMemcpyAsync(d_ptr.p, indptr, ptr_bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_idx.p, indices, (size_t)nnz * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_val.p, data, (size_t)nnz * 8, hipMemcpyHostToDevice, c->stream));
    }
    const void* const dp_ptr = device_csr ? indptr : d_ptr.p;
    const void* const dp_idx = device_csr ? static_cast<const void*>(indices) : d_idx.p;
    const void* const dp_val = device_csr ? static_cast<const void*>(data) : d_val.p;
    DevTemp d_map;
    if (local_cols) {
        // vectors keep crossing in the caller's GLOBAL numbering (grid_index, n_global entries); the matrix kernels see the
        // local ids through their own map
        MG_TRY(upload_permutation(c, L, grid_index, L.n_global));
        std::vector<int> m32((size_t)n_cols);
        std::vector<char> seen((size_t)L.nloc, 0);
        const int64_t lo = L.row0 - L.halo_lo, hi = L.row0 + L.nloc + L.halo_hi;
        for (int64_t d = 0; d < n_cols; ++d) {
            const int64_t p = local_cols[d];
            if (d < n_rows) {
                if (p < L.row0 || p >= L.row0 + L.nloc || seen[(size_t)(p - L.row0)])
                    return fail("the handed-over rows are not exactly this rank's slab of the level");
                seen[(size_t)(p - L.row0)] = 1;
            } else if (p < lo || p >= hi) {
                return fail("a ghost column lies outside the slab's halo");
            }
            m32[(size_t)d] = (int)p;
        }
        MG_TRY(d_map.alloc((size_t)n_cols * sizeof(int)));
        HIP_TRY(hipMemcpyAsync(d_map.p, m32.data(), (size_t)n_cols * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    } else {
        MG_TRY(upload_permutation(c, L, grid_index, n_rows));
    }
    CsrArgs a{};
    a.indptr = dp_ptr; a.indptr64 = indptr_is_64; a.indices = static_cast<const int*>(dp_idx); a.data = static_cast<const double*>(dp_val);
    a.perm = local_cols ? d_map.as<const int>() : L.perm;
    a.n = n_rows; a.row0 = L.row0; a.nloc = L.nloc; a.lead = L.g.lead; a.xlen = L.xlen;
    a.prune = prune_zeros;
    a.sort = device_csr ? 0 : 1;
    // pass 1: widest kept row, kept entries, sanity flags
    unsigned long long* d_stats = reinterpret_cast<unsigned long long*>(c->partials.get());
    HIP_TRY(hipMemsetAsync(d_stats, 0, 4 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(csr_scan, dim3(blocks_for(n_rows, 256)), dim3(256), 0, c->stream, a, d_stats);
    unsigned long long stats[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(stats, d_stats, sizeof(stats), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (stats[2] & 1ull)
        return fail("a matrix row couples unknowns more than one grid plane apart (not a slab-local stencil)");
    if ((stats[2] & 2ull) && c->require_diagonal) return fail("a matrix row has a zero or missing diagonal");
    L.W = (int)std::max<unsigned long long>(1, stats[0]);
    L.nnz_stored = stats[1];
    // pass 2: tiles
    MG_TRY(alloc_ell(c, L));
    const dim3 g1(blocks_for(n_rows, 256)), b1(256);
    with_int_else<4, 1, 2>(L.R, [&](auto r) { hipLaunchKernelGGL(csr_to_ell<decltype(r)::value>, g1, b1, 0, c->stream, a, L.vals, L.cols, L.dinv, L.W); });
    HIP_TRY(hipGetLastError());
    // true non-zeros among the kept entries (== kept when pruned); counted on the caller's copy (set-up only)
    L.nnz_nonzero = L.nnz_stored;
    if (!prune_zeros && (!c->comm.active() || L.replicated) && !local_cols && !device_csr) {
        unsigned long long nz = 0;
        for (int64_t q = 0; q < nnz; ++q) nz += data[q] != 0.0;
        L.nnz_nonzero = nz;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    MG_TRY(finish_stored_rows(c, L, level));
    if (!vectors) { L.set = true; return 0; }
    return finish_level(c, L);
}

// Galerkin coarse level: level - 1's matrix = P^T A_level P on the interior nodes (identity rows on the boundary), computed on
// the device from the fine level's storage and handed to the CSR builder as device arrays (K entries per row, exact zeros
// dropped): the coarse level then gets the same storage analysis as any handed-over level.
extern "C++" {
template <int DIM>
int launch_galerkin(mg_context* c, int fmt, const GalerkinArgs& a, dim3 grid) {
    with_int_else<3, 0, 1, 2>(fmt, [&](auto f) {
        hipLaunchKernelGGL((galerkin_p1<DIM, decltype(f)::value>), grid, dim3(kPlaneBlock), 0, c->stream, a);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}
}  // extern "C++"

int galerkin_level(mg_context* c, int level) {
    if (level < 1) return fail("mg_galerkin_level: level must be >= 1 (it sets level - 1)");
    MG_TRY(need_matrix(c, level));
    MG_TRY(need_grid(c, level));
    Level& F = c->L[level];
    if (F.faces != MG_FACES_ALL)
        return fail("mg_galerkin_level: level " + std::to_string(level) + " was generated with the face set " + std::to_string(F.faces) +
                    " (mg_set_diffusion_faces): the Galerkin product knows Dirichlet conditions on all six faces only; generate the "
                    "coarse level with mg_gen_diffusion_level or a diffusion hierarchy call instead");
    MG_TRY(need_stored_rows(c, F, "mg_galerkin_level (the Galerkin product; generate the level with mg_gen_diffusion_level instead)"));
    if (!F.replicated) return fail("Galerkin coarse levels need a whole fine level, not a slab");
    if (F.N < 2 || (F.N & 1)) return fail("Galerkin coarse levels need an even elements_per_dim");
    MG_TRY(check_p1_stencil(c, F));
    GalerkinArgs a{};
    a.gf = F.g;
    a.R = F.R; a.W = F.W; a.lead = F.g.lead;
    const int K = kuhn_lin(c, F, a.flin);
    for (int q = 0; q < 15; ++q) a.code[q] = a.diag[q] = a.tpos[q] = -1;
    int fmt = 0;
    if (cls_full(F)) {
        fmt = 3;
        a.cls = F.cls + F.cls_lead; a.ctab = F.ctab;
    } else if (F.sdia) {
        fmt = 2;
        a.dvals = F.dvals; a.wu = F.wu; a.mlead = F.mlead;
    } else if (F.coded) {
        fmt = 1;
        a.vals = F.vals; a.codes = F.codes;
        for (int q = 0; q < K; ++q) {
            const auto it = std::find(F.h_offsets.begin(), F.h_offsets.end(), (int)a.flin[q]);
            if (it != F.h_offsets.end()) a.code[q] = (int)(it - F.h_offsets.begin());
        }
    } else {
        a.vals = F.vals; a.cols = F.cols;
    }
    if (fmt >= 2)
        for (int q = 0; q < K; ++q) {
            const int64_t o = std::llabs(a.flin[q]);
            for (int t = 0; t < 8 && a.diag[q] < 0; ++t)
                if ((t == 0 && o == 0) || (t > 0 && o != 0 && F.up[t] == o)) a.diag[q] = t;
            if (a.diag[q] >= 0) a.tpos[q] = 3 + (a.flin[q] < 0 ? -a.diag[q] : a.diag[q]);
        }
    Level& C = c->L[level - 1];
    LevelBuild build(c, C);
    MG_TRY(setup_geometry(c, C, level - 1, F.N / 2));
    if (!C.replicated) return fail("Galerkin coarse levels need a whole coarse level");
    const int64_t n = C.n_global, nnz = n * K;
    DevTemp d_ptr, d_idx, d_val;
    MG_TRY(d_ptr.alloc((size_t)(n + 1) * 8));
    MG_TRY(d_idx.alloc((size_t)nnz * 4));
    MG_TRY(d_val.alloc((size_t)nnz * 8));
    a.gc = C.g;
    a.indptr = d_ptr.as<int64_t>(); a.indices = d_idx.as<int>(); a.data = d_val.as<double>();
    a.flag = reinterpret_cast<int*>(c->partials.get());
    HIP_TRY(hipMemsetAsync(a.flag, 0, sizeof(int), c->stream));
    const dim3 grid = grid3(C.g, C.g.nk);
    int rc = 0;
    with_int_else<2, 3>(c->dim, [&](auto dim) { rc = launch_galerkin<decltype(dim)::value>(c, fmt, a, grid); });
    MG_TRY(rc);
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, a.flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (flag) return fail("a Galerkin entry falls outside the coarse Kuhn pattern");
    MG_TRY(build_level_from_csr(c, level - 1, C, n, nnz, d_ptr.p, 1, d_idx.as<const int32_t>(),
                                d_val.as<const double>(), nullptr, 1, true, nullptr, 0, true));
    return build.done();
}

}  // namespace

int mg_set_level_csr(mg_handle c, int level, int N, int64_t n_rows, int64_t nnz, const void* indptr, int indptr_is_64,
                     const int32_t* indices, const double* data, const int64_t* grid_index, int prune_zeros) {
    MG_TRY(check_level(c, level, false));
    if (!indptr || !indices || !data) return fail("null CSR arrays");
    if (n_rows <= 0 || nnz < 0) return fail("bad matrix dimensions");
    MG_TRY(check_csr(n_rows, n_rows, nnz, indptr, indptr_is_64, indices, false));      // (grid and flat levels alike)
    HIP_TRY(hipSetDevice(c->device));
    Level& L = c->L[level];
    LevelBuild build(c, L);
    MG_TRY(setup_geometry(c, L, level, N, n_rows));
    if (n_rows != L.n_global)
        return fail("matrix has " + std::to_string(n_rows) + " rows, grid has " + std::to_string(L.n_global));
    MG_TRY(build_level_from_csr(c, level, L, n_rows, nnz, indptr, indptr_is_64, indices, data, grid_index, prune_zeros));
    return build.done();
}

int mg_csr_check(int64_t n_rows, int64_t n_cols, int64_t nnz, const void* indptr, int indptr_is_64, const int32_t* indices,
                 int allow_duplicates) {
    return check_csr(n_rows, n_cols, nnz, indptr, indptr_is_64, indices, allow_duplicates != 0);
}

int mg_level_slab(mg_handle c, int level, int N, int64_t* row0, int64_t* n_local, int64_t* halo_lo, int64_t* halo_hi) {
    MG_TRY(check_level(c, level, false));
    if (N <= 0) return fail("elements_per_dim must be positive");
    Level tmp;
    MG_TRY(setup_geometry(c, tmp, level, N));
    if (row0) *row0 = tmp.row0;
    if (n_local) *n_local = tmp.nloc;
    // (what the rows may couple to: "halo_planes" planes, however many the vectors have room for)
    if (halo_lo) *halo_lo = tmp.halo_lo ? (int64_t)c->halo_planes * tmp.g.plane : 0;
    if (halo_hi) *halo_hi = tmp.halo_hi ? (int64_t)c->halo_planes * tmp.g.plane : 0;
    return 0;
}

int mg_set_level_csr_local(mg_handle c, int level, int N, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* indptr,
                           int indptr_is_64, const int32_t* indices, const double* data, const int64_t* col_nodes,
                           const int64_t* grid_index, int prune_zeros) {
    MG_TRY(check_level(c, level, false));
    if (!indptr || !indices || !data || !col_nodes) return fail("null CSR arrays");
    if (N <= 0 || n_rows <= 0 || n_cols < n_rows || nnz < 0) return fail("bad matrix dimensions");
    MG_TRY(check_csr(n_rows, n_cols, nnz, indptr, indptr_is_64, indices, false));
    HIP_TRY(hipSetDevice(c->device));
    Level& L = c->L[level];
    LevelBuild build(c, L);
    MG_TRY(setup_geometry(c, L, level, N));
    if (n_rows != L.nloc)
        return fail("the rank owns " + std::to_string(L.nloc) + " rows of this level (mg_level_slab), " + std::to_string(n_rows) +
                    " were handed over");
    MG_TRY(build_level_from_csr(c, level, L, n_rows, nnz, indptr, indptr_is_64, indices, data, grid_index, prune_zeros, true,
                                col_nodes, n_cols));
    return build.done();
}

int mg_set_level_grid(mg_handle c, int level, int N, int64_t n_rows, const int64_t* grid_index) {
    MG_TRY(check_level(c, level, false));
    if (N < 0) return fail("elements_per_dim must be >= 0");
    HIP_TRY(hipSetDevice(c->device));
    Level& L = c->L[level];
    LevelBuild build(c, L);
    MG_TRY(setup_geometry(c, L, level, N, n_rows));
    if (n_rows != L.n_global)
        return fail("vector has " + std::to_string(n_rows) + " entries, grid has " + std::to_string(L.n_global));
    MG_TRY(upload_permutation(c, L, grid_index, n_rows));
    MG_TRY(finish_level(c, L));
    return build.done();
}

int mg_galerkin_level(mg_handle c, int level) {
    MG_TRY(check_level(c, level));
    HIP_TRY(hipSetDevice(c->device));
    return galerkin_level(c, level);
}

int mg_galerkin_hierarchy(mg_handle c, int top_level) {
    MG_TRY(check_level(c, top_level));
    HIP_TRY(hipSetDevice(c->device));
    for (int l = top_level; l >= 1; --l) MG_TRY(galerkin_level(c, l));
    return 0;
}

int mg_gen_poisson_level(mg_handle c, int level, int N, int prune_zeros) {
    MG_TRY(check_level(c, level, false));
    if (N <= 0) return fail("elements_per_dim must be positive");
    HIP_TRY(hipSetDevice(c->device));
    GenArgs a = gen_args(c, N, prune_zeros);
    a.odd = c->gen_odd_rows;
    a.w = c->dim == 2 ? 1.0 : a.h;
    a.diag = c->dim == 2 ? 4.0 : 6.0 * a.h;
    return gen_stored_level(c, level, N, a.W, [&](const Level& L, dim3 grid, unsigned long long* counts) {
        const dim3 blk(kPlaneBlock);
        a.g = L.g;
        with_int_else<4, 1, 2>(L.R, [&](auto r) { hipLaunchKernelGGL(gen_poisson<decltype(r)::value>, grid, blk, 0, c->stream, a, L.vals, L.cols, L.dinv, L.f.rows, counts); });
    });
}

int mg_gen_lattice_level(mg_handle c, int level, int N, int width, const int* count, const int* offsets, const double* values,
                         const double* load) {
    MG_TRY(check_level(c, level, false));
    if (N <= 0 || (N & 1)) return fail("lattice levels need an even, positive number of lattice steps per dimension");
    if (!count || !offsets || !values || !load) return fail("null stencil tables");
    if (width < 1 || width > LAT_MAX) return fail("stencil width out of range");
    if (c->comm.active() && c->halo_planes < 2)
        return fail("lattice levels reach two planes: set mg_set_tuning(\"halo_planes\", 2) before mg_set_comm / level set-up");
    for (int p = 0; p < 8; ++p)
        if (count[p] < 0 || count[p] > width) return fail("a class has more entries than the stated width");
    HIP_TRY(hipSetDevice(c->device));
    DevTemp d_count, d_off, d_val, d_load;
    MG_TRY(d_count.alloc(8 * sizeof(int)));
    MG_TRY(d_off.alloc((size_t)8 * LAT_MAX * 3 * sizeof(int)));
    MG_TRY(d_val.alloc((size_t)8 * LAT_MAX * sizeof(double)));
    MG_TRY(d_load.alloc(8 * sizeof(double)));
    HIP_TRY(hipMemcpy(d_count.p, count, 8 * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_off.p, offsets, (size_t)8 * LAT_MAX * 3 * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_val.p, values, (size_t)8 * LAT_MAX * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_load.p, load, 8 * sizeof(double), hipMemcpyHostToDevice));
    LatticeArgs a{};
    a.N = N; a.dim = c->dim; a.W = width;
    a.count = d_count.as<const int>(); a.off = d_off.as<const int>();
    a.val = d_val.as<const double>(); a.load = d_load.as<const double>();
    return gen_stored_level(c, level, N, width, [&](const Level& L, dim3 grid, unsigned long long* counts) {
        const dim3 blk(kPlaneBlock);
        a.g = L.g;
        with_int_else<4, 1, 2>(L.R, [&](auto r) { hipLaunchKernelGGL(gen_lattice<decltype(r)::value>, grid, blk, 0, c->stream, a, L.vals, L.cols, L.dinv, L.f.rows, counts); });
    });
}

namespace {

// cell planes [kc0, kc1) along the slab axis that the interior rows of a level's owned planes read (kappa of the cells
// on both sides of every owned node plane)
void diffusion_planes(const Level& L, int* kc0, int* kc1) {
    *kc0 = std::max(L.g.k0 - 1, 0);
    *kc1 = std::min(L.g.k0 + L.g.nk, L.N);
}

int64_t cell_plane(const mg_context* c, int N) { return c->dim == 3 ? (int64_t)N * N : (int64_t)N; }

// the first entry of the device kappa (global cell index base + q) that is not a positive finite double, as an error
int check_kappa(mg_context* c, const double* d_kappa, int64_t n, int64_t base, int N) {
    DevTemp d_first;
    MG_TRY(d_first.alloc(sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(d_first.p, 0xff, sizeof(unsigned long long), c->stream));
    const unsigned nb = (unsigned)std::max<int64_t>(1, std::min<int64_t>(8192, (n + 255) / 256));
    hipLaunchKernelGGL(kappa_check, dim3(nb), dim3(256), 0, c->stream, d_kappa, n, base,
                       d_first.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    unsigned long long first = 0;
    HIP_TRY(hipMemcpyAsync(&first, d_first.p, sizeof(first), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (first == ~0ull) return 0;
    double x = 0.0;
    HIP_TRY(hipMemcpy(&x, d_kappa + (first - base), sizeof(double), hipMemcpyDeviceToHost));
    const int64_t q = (int64_t)first;
    std::string cell = "(" + std::to_string(q % N) + ", ";
    cell += c->dim == 3 ? std::to_string((q / N) % N) + ", " + std::to_string(q / ((int64_t)N * N)) : std::to_string(q / N);
    char val[40];
    snprintf(val, sizeof(val), "%.17g", x);
    return fail("kappa must be positive and finite: cell " + cell + ") = index " + std::to_string(q) + " holds " + val);
}

// the stored level from a device kappa holding cell planes [kc0, ...); d_sigma: the level's N^3 reaction cells or null;
// rw: the level's Robin fields
int gen_diffusion_level(mg_context* c, int level, int N, const double* d_kappa, int kc0, int prune_zeros, const double* d_sigma,
                        const RobinWalk& rw) {
    DiffusionArgs d{};
    d.ga = gen_args(c, N, prune_zeros);
    d.kappa = d_kappa;
    d.kc0 = kc0;
    MG_TRY(face_set_handle(c, "mg_gen_diffusion_level"));
    DevTemp rdiag;                              // nodal R(sigma) [+ B(alpha)]: read by the generating kernel and not kept
    if (d_sigma || rw.faces) {
        MG_TRY(rdiag.alloc((size_t)(N + 1) * (N + 1) * (N + 1) * 8));
        MG_TRY(launch_nodal_diag(c, d_sigma, rw, rdiag.as<double>(), N));
        d.react = rdiag.as<const double>();
    }
    const int faces = c->diffusion_faces;       // (not the default: a 3-D whole handle, so L.g is the whole grid)
    MG_TRY(gen_stored_level(c, level, N, d.ga.W, [&](const Level& L, dim3 grid, unsigned long long* counts) {
        const dim3 blk(kPlaneBlock);
        d.ga.g = L.g;
        d.box = free_box(faces, L.g.nx, L.g.ny, L.g.nz);
        with_int_else<4, 1, 2>(L.R, [&](auto r) { hipLaunchKernelGGL(gen_diffusion<decltype(r)::value>, grid, blk, 0, c->stream, d, L.vals, L.cols, L.dinv, L.f.rows, counts); });
    }));
    c->L[level].faces = faces;
    c->L[level].react = d_sigma != nullptr;
    c->L[level].robin = rw.faces;
    return 0;
}

}  // namespace

int mg_gen_diffusion_level(mg_handle c, int level, int N, const double* kappa, int prune_zeros) {
    MG_TRY(check_level(c, level, false));
    if (N <= 0) return fail("elements_per_dim must be positive");
    if (!kappa) return fail("null kappa");
    HIP_TRY(hipSetDevice(c->device));
    MG_TRY(reaction_handle(c, "mg_gen_diffusion_level", N));
    MG_TRY(robin_handle(c, "mg_gen_diffusion_level", N));
    Level geo;                                   // checked before the level is touched: a refusal leaves it as it was
    MG_TRY(setup_geometry(c, geo, level, N));
    int kc0 = 0, kc1 = 0;
    diffusion_planes(geo, &kc0, &kc1);
    const int64_t cp = cell_plane(c, N), n = (int64_t)(kc1 - kc0) * cp;
    DevTemp d_kappa;
    MG_TRY(d_kappa.alloc((size_t)n * 8));
    HIP_TRY(hipMemcpy(d_kappa.p, kappa + (size_t)kc0 * cp, (size_t)n * 8, hipMemcpyHostToDevice));
    MG_TRY(check_kappa(c, d_kappa.as<const double>(), n, (int64_t)kc0 * cp, N));
    return gen_diffusion_level(c, level, N, d_kappa.as<const double>(), kc0, prune_zeros, c->sigma, RobinWalk(c));
}

namespace {

// F of a matrix-free level from its kappa, and once more as the level's true right-hand side where it keeps one; allocates
// nothing (mg_refresh_diffusion_hierarchy relies on that)
int fill_rhs_mf(mg_context* c, Level& L, const double* d_kappa) {
    MG_TRY(launch_diffusion_rhs(c, L, d_kappa, L.f.rows, nullptr));
    if (L.ftrue.raw) HIP_TRY(hipMemcpyAsync(L.ftrue.base, L.f.base, (size_t)L.xlen * 8, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

// the matrix-free level from a whole device kappa (N^3 cells, n of them), which the level takes over on success; d_sigma:
// the level's N^3 reaction cells or null -- the level keeps their nodal R(sigma), not the cells; rw: the level's Robin
// fields, whose B(alpha) is folded into that nodal vector (R + B, or B alone)
int gen_diffusion_level_mf(mg_context* c, int level, int N, DevTemp& kappa, int64_t n, const double* d_sigma, const RobinWalk& rw) {
    const double* const d_kappa = kappa.as<const double>();
    Level& L = c->L[level];
    LevelBuild build(c, L);
    MG_TRY(setup_geometry(c, L, level, N));
    L.W = 7;
    L.R = c->rows_per_lane;         // (the slice count is what callers of launch_ell take a whole level's range from)
    L.nslices = (L.nloc + (int64_t)WAVE * L.R - 1) / ((int64_t)WAVE * L.R);
    MG_TRY(alloc_level_vectors(c, L));
    if (level + 1 < c->nlev) MG_TRY(vec_alloc(c, L, &L.ftrue));     // (the true right-hand side for mg_fmg, as on stored levels)
    L.faces = c->diffusion_faces;
    if (d_sigma || rw.faces) {
        MG_TRY(L.rdiag.alloc(c, (size_t)L.n_global));
        MG_TRY(launch_nodal_diag(c, d_sigma, rw, L.rdiag, N));
    }
    L.react = d_sigma != nullptr;
    L.robin = rw.faces;
    MG_TRY(fill_rhs_mf(c, L, d_kappa));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // what the stored level would report: one diagonal entry per row and two entries per pair of free axis neighbours (the
    // default set: seven per interior row less the columns on the boundary, one per boundary row)
    const FreeBox box = level_box(L, L.faces);
    const int64_t m[3] = {box.hi[0] - box.lo[0] + 1, box.hi[1] - box.lo[1] + 1, box.hi[2] - box.lo[2] + 1};
    L.nnz_stored = L.nnz_nonzero = (unsigned long long)(L.n_global + 2 * ((m[0] - 1) * m[1] * m[2] + m[0] * (m[1] - 1) * m[2] + m[0] * m[1] * (m[2] - 1)));
    L.rep_sym = 1;
    L.rb_ok = false;
    L.mf = true;
    L.kappa.adopt(c, kappa.release<double>(), (size_t)n);
    L.set = true;
    L.has_matrix = true;
    return build.done();
}

int mf_refusals(mg_context* c, const std::string& who) {
    MG_TRY(face_set_handle(c, who));
    if (c->dim != 3) return fail(who + ": matrix-free diffusion levels are 3-D only (this handle is 2-D)");
    if (c->comm.active()) return fail(who + ": matrix-free diffusion levels need a whole (not slab) handle");
    return 0;
}

}  // namespace

int mg_gen_diffusion_level_mf(mg_handle c, int level, int N, const double* kappa) {
    MG_TRY(check_level(c, level, false));
    MG_TRY(mf_refusals(c, "mg_gen_diffusion_level_mf"));
    if (level == 0)
        return fail("mg_gen_diffusion_level_mf: level 0 is the coarsest level, which the direct solve factorises and the coarse "
                    "CG reads row by row: it needs stored rows (mg_gen_diffusion_level)");
    if (N <= 0) return fail("elements_per_dim must be positive");
    if (!kappa) return fail("null kappa");
    HIP_TRY(hipSetDevice(c->device));
    MG_TRY(reaction_handle(c, "mg_gen_diffusion_level_mf", N));
    MG_TRY(robin_handle(c, "mg_gen_diffusion_level_mf", N));
    Level geo;                                   // checked before the level is touched: a refusal leaves it as it was
    MG_TRY(setup_geometry(c, geo, level, N));
    const int64_t n = cell_plane(c, N) * N;
    DevTemp d_kappa;
    MG_TRY(d_kappa.alloc((size_t)n * 8));
    HIP_TRY(hipMemcpy(d_kappa.p, kappa, (size_t)n * 8, hipMemcpyHostToDevice));
    MG_TRY(check_kappa(c, d_kappa.as<const double>(), n, 0, N));
    return gen_diffusion_level_mf(c, level, N, d_kappa, n, c->sigma, RobinWalk(c));
}

namespace {

// one pass over a level's device kappa (mg_diffusion_kappa.hip.h): the kappa of the Nc^dim cells of the level below and,
// where fine_out is not null, the level's own copy
int launch_kappa_ingest(mg_context* c, const double* fine, double* fine_out, double* coarse, int Nc, int averaging) {
    const int64_t nc = cell_plane(c, Nc) * Nc;
    const unsigned nb = (unsigned)std::max<int64_t>(1, std::min<int64_t>(2048, (nc + KI_BLOCK - 1) / KI_BLOCK));
    const int vec = ((reinterpret_cast<uintptr_t>(fine) | reinterpret_cast<uintptr_t>(fine_out)) & 15) == 0 ? 1 : 0;
    const int harmonic = averaging == MG_KAPPA_HARMONIC ? 1 : 0;
    if (c->dim == 3)
        hipLaunchKernelGGL(kappa_ingest<3>, dim3(nb), dim3(KI_BLOCK), 0, c->stream, fine, fine_out, coarse, Nc, harmonic, vec);
    else
        hipLaunchKernelGGL(kappa_ingest<2>, dim3(nb), dim3(KI_BLOCK), 0, c->stream, fine, fine_out, coarse, Nc, harmonic, vec);
    HIP_TRY(hipGetLastError());
    return 0;
}

// What the three generating hierarchy entries refuse alike (`matrix_free`: the call may make matrix-free levels), a top
// level whose geometry setup_geometry refuses last.  Only checks: nothing of the handle or the device is touched.
int hierarchy_refusals(mg_context* c, const std::string& who, int top_level, int N, int averaging, bool matrix_free) {
    if (matrix_free) MG_TRY(mf_refusals(c, who));
    if (N <= 0) return fail("elements_per_dim must be positive");
    if (averaging != MG_KAPPA_ARITHMETIC && averaging != MG_KAPPA_HARMONIC) return fail("unknown kappa averaging");
    if (c->comm.active())
        return fail(who + " needs a whole (not slab) handle: on slabs, call mg_gen_diffusion_level per level");
    if (N % (1 << top_level))
        return fail(who + " needs an even elements_per_dim on every level above level 0 (" + std::to_string(N) +
                    " is not N0 * 2^" + std::to_string(top_level) + ")");
    MG_TRY(reaction_handle(c, who, N));
    MG_TRY(robin_handle(c, who, N));
    Level geo;
    return setup_geometry(c, geo, top_level, N);
}

// Levels top_level .. 0 from the top level's kappa on the device, coarsened level by level; levels above level 0 with at
// least min_rows rows become matrix-free, the others are stored (generated before their kappa is coarsened and freed).
// `held` is `src` where the field is the walker's to give away or free -- a host entry's upload, and below the top level
// the coarsened field of the level above -- and empty where `src` is the caller's buffer, which is only read.  A
// matrix-free level takes a held field over as it is and gets its own copy of a borrowed one from the pass that coarsens
// it.  At most two kappa fields are alive at a time besides those the matrix-free levels keep.
// The handle's reaction field (mg_set_diffusion_reaction) walks beside kappa: borrowed on the top level, below it the
// arithmetic mean of the 2^3 children whatever `averaging` says (mass is additive), by the same pass; besides the handle's
// own, at most two sigma fields are alive at a time, and no level keeps one.  The Robin fields (mg_set_diffusion_robin)
// walk the same way, 2 x 2 children per face-cell (RobinWalk).
int gen_diffusion_hierarchy(mg_context* c, int top_level, int N, const double* src, DevTemp& held, int averaging,
                            int64_t min_rows) {
    MG_TRY(check_kappa(c, src, cell_plane(c, N) * N, 0, N));
    const double* ssrc = c->sigma;              // (hierarchy_refusals: of the top level's size)
    DevTemp sheld;
    RobinWalk rw(c);
    for (int l = top_level, Nl = N; l >= 0; --l, Nl /= 2) {
        const int64_t n = cell_plane(c, Nl) * Nl;
        const int64_t rows = c->dim == 3 ? ((int64_t)Nl + 1) * (Nl + 1) * (Nl + 1) : ((int64_t)Nl + 1) * (Nl + 1);
        const bool mf = l > 0 && rows >= min_rows;
        if (!mf) MG_TRY(gen_diffusion_level(c, l, Nl, src, 0, 1, ssrc, rw));
        DevTemp own, coarse, scoarse;
        if (mf && !held.p) MG_TRY(own.alloc((size_t)n * 8));       // (matrix-free levels are above level 0: the pass below copies)
        if (l > 0) {
            const int Nc = Nl / 2;
            MG_TRY(coarse.alloc((size_t)(cell_plane(c, Nc) * Nc) * 8));
            MG_TRY(launch_kappa_ingest(c, src, own.as<double>(), coarse.as<double>(), Nc, averaging));
            if (ssrc) {
                MG_TRY(scoarse.alloc((size_t)(cell_plane(c, Nc) * Nc) * 8));
                MG_TRY(launch_kappa_ingest(c, ssrc, nullptr, scoarse.as<double>(), Nc, MG_KAPPA_ARITHMETIC));
            }
            MG_TRY(rw.coarsen(c, Nc));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        if (mf) MG_TRY(gen_diffusion_level_mf(c, l, Nl, own.p ? own : held, n, ssrc, rw));
        if (l > 0) rw.descend();
        held = std::move(coarse);
        src = held.as<const double>();
        if (ssrc) {
            sheld = std::move(scoarse);
            ssrc = sheld.as<const double>();
        }
        c->L[l].diffusion_hierarchy = true;
    }
    return 0;
}

// the host entries: the top level's kappa is uploaded and the upload handed to the walker as its own
int gen_diffusion_hierarchy_host(mg_context* c, const std::string& who, int top_level, int N, const double* kappa_top,
                                 int averaging, bool matrix_free, int64_t min_rows) {
    MG_TRY(check_level(c, top_level, false));
    if (!kappa_top) return fail("null kappa");
    MG_TRY(hierarchy_refusals(c, who, top_level, N, averaging, matrix_free));
    HIP_TRY(hipSetDevice(c->device));
    const int64_t n = cell_plane(c, N) * N;
    DevTemp held;
    MG_TRY(held.alloc((size_t)n * 8));
    HIP_TRY(hipMemcpy(held.p, kappa_top, (size_t)n * 8, hipMemcpyHostToDevice));
    return gen_diffusion_hierarchy(c, top_level, N, held.as<const double>(), held, averaging, min_rows);
}

}  // namespace

int mg_gen_diffusion_hierarchy(mg_handle c, int top_level, int N, const double* kappa_top, int averaging) {
    return gen_diffusion_hierarchy_host(c, "mg_gen_diffusion_hierarchy", top_level, N, kappa_top, averaging, false, INT64_MAX);
}

int mg_gen_diffusion_hierarchy_mf(mg_handle c, int top_level, int N, const double* kappa_top, int averaging, int64_t min_rows) {
    return gen_diffusion_hierarchy_host(c, "mg_gen_diffusion_hierarchy_mf", top_level, N, kappa_top, averaging, true, min_rows);
}

int mg_gen_diffusion_hierarchy_device(mg_handle c, int top_level, int N, const double* kappa_dev, int averaging,
                                      int64_t mf_min_rows) {
    const std::string who = "mg_gen_diffusion_hierarchy_device";
    MG_TRY(check_level(c, top_level, false));
    HIP_TRY(hipSetDevice(c->device));
    MG_TRY(need_device_pointer(c, kappa_dev, who.c_str(), "kappa"));
    MG_TRY(hierarchy_refusals(c, who, top_level, N, averaging, mf_min_rows >= 0));
    DevTemp none;                               // the caller's buffer is borrowed: the walker holds nothing yet
    return gen_diffusion_hierarchy(c, top_level, N, kappa_dev, none, averaging, mf_min_rows >= 0 ? mf_min_rows : INT64_MAX);
}

int mg_refresh_diffusion_hierarchy(mg_handle c, int top_level, const double* kappa_dev, int averaging) {
    const std::string who = "mg_refresh_diffusion_hierarchy";
    MG_TRY(check_level(c, top_level, false));
    HIP_TRY(hipSetDevice(c->device));
    if (c->comm.active()) return fail(who + " needs a whole (not slab) handle");
    MG_TRY(need_device_pointer(c, kappa_dev, who.c_str(), "kappa"));
    if (averaging != MG_KAPPA_ARITHMETIC && averaging != MG_KAPPA_HARMONIC) return fail("unknown kappa averaging");
    for (int l = top_level; l >= 0; --l) {
        const Level& L = c->L[l];
        if (!L.set || !L.diffusion_hierarchy)
            return fail(who + ": level " + std::to_string(l) + (L.set ? " was not generated by a diffusion hierarchy call (levels set "
                        "from CSR, by mg_gen_poisson_level, by mg_galerkin_level or generated one by one cannot be refreshed)"
                        : " has not been set") + ": generate the hierarchy with mg_gen_diffusion_hierarchy[_mf | _device] first");
        if (l < top_level && 2 * L.N != c->L[l + 1].N)
            return fail(who + ": levels " + std::to_string(l + 1) + " and " + std::to_string(l) + " come from hierarchies of different "
                        "sizes (" + std::to_string(c->L[l + 1].N) + " and " + std::to_string(L.N) + " cells per dimension)");
        if (L.mf && (int64_t)L.kappa.count() != cell_plane(c, L.N) * L.N) return fail(who + ": level " + std::to_string(l) + " keeps a kappa of another size");
        if (L.faces != c->diffusion_faces)
            return fail(who + ": level " + std::to_string(l) + " was generated with the face set " + std::to_string(L.faces) +
                        ", the handle's is " + std::to_string(c->diffusion_faces) + " now (mg_set_diffusion_faces): generate the hierarchy again");
        if (L.react != (c->sigma.get() != nullptr))
            return fail(who + ": level " + std::to_string(l) + " was generated " + (L.react ? "with" : "without") + " a reaction term, the handle has " +
                        (c->sigma ? "a" : "no") + " reaction field now (mg_set_diffusion_reaction): generate the hierarchy again");
        if (L.robin != robin_faces(c))
            return fail(who + ": level " + std::to_string(l) + " was generated with Robin fields on the faces " + std::to_string(L.robin) +
                        ", the handle holds fields on the faces " + std::to_string(robin_faces(c)) + " now (mg_set_diffusion_robin): generate the hierarchy again");
    }
    const int N = c->L[top_level].N;
    MG_TRY(reaction_handle(c, who, N));
    MG_TRY(robin_handle(c, who, N));
    MG_TRY(check_kappa(c, kappa_dev, cell_plane(c, N) * N, 0, N));      // read-only: a refusal leaves the old hierarchy usable
    // whatever the old matrices fed goes: captured cycles, level 0's factorisation, every level's Chebyshev estimate
    ++c->epoch;
    drop_graphs(c);
    free_direct(c);
    for (int l = top_level; l >= 0; --l) { c->L[l].cheb_est_ok = false; c->L[l].cheb_lmax_est = 0.0; }
    // the walk of gen_diffusion_hierarchy with the split the levels have: a matrix-free level keeps its buffers, so the pass
    // above it coarsens straight into its kappa and nothing is allocated or freed for it
    const double* src = kappa_dev;
    DevTemp held;                               // src where it is a temporary: the coarsened field above a stored level
    const double* ssrc = c->sigma;              // the reaction field walks beside kappa; a matrix-free level's R(sigma) is rewritten in place
    DevTemp sheld;
    RobinWalk rw(c);                            // the Robin fields too: a matrix-free level's nodal vector is rewritten in place
    for (int l = top_level, Nl = N; l >= 0; --l, Nl /= 2) {
        Level& L = c->L[l];
        const bool mf = L.mf;
        if (!mf) {                              // stored: the level is rebuilt by the pipeline that made it
            MG_TRY(gen_diffusion_level(c, l, Nl, src, 0, 1, ssrc, rw));
            L.diffusion_hierarchy = true;
        } else if (ssrc || rw.faces) {
            MG_TRY(launch_nodal_diag(c, ssrc, rw, L.rdiag, Nl));
        }
        if (l > 0) MG_TRY(rw.coarsen(c, Nl / 2));
        DevTemp coarse, scoarse;
        if (l > 0 && ssrc) {
            MG_TRY(scoarse.alloc((size_t)(cell_plane(c, Nl / 2) * (Nl / 2)) * 8));
            MG_TRY(launch_kappa_ingest(c, ssrc, nullptr, scoarse.as<double>(), Nl / 2, MG_KAPPA_ARITHMETIC));
        }
        double* coarse_p = nullptr;
        if (l > 0) {
            const int Nc = Nl / 2;
            if (c->L[l - 1].mf) coarse_p = c->L[l - 1].kappa;
            else {
                MG_TRY(coarse.alloc((size_t)(cell_plane(c, Nc) * Nc) * 8));
                coarse_p = coarse.as<double>();
            }
            MG_TRY(launch_kappa_ingest(c, src, mf && src != L.kappa ? L.kappa.get() : nullptr, coarse_p, Nc, averaging));
        }
        if (mf) {                               // kappa overwritten in place; the vectors are those of a fresh level
            MG_TRY(fill_rhs_mf(c, L, L.kappa));
            HIP_TRY(hipMemsetAsync(L.v.raw, 0, (size_t)vec_total(L) * sizeof(double), c->stream));
            HIP_TRY(hipMemsetAsync(L.v2.raw, 0, (size_t)vec_total(L) * sizeof(double), c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (l > 0) rw.descend();
        held = std::move(coarse);
        src = coarse_p;
        if (ssrc) {
            sheld = std::move(scoarse);
            ssrc = sheld.as<const double>();
        }
    }
    return 0;
}

int mg_set_diffusion_faces(mg_handle c, int dirichlet_faces) {
    if (!c) return fail("null handle");
    const std::string who = "mg_set_diffusion_faces: ";
    if (dirichlet_faces < 0 || dirichlet_faces > MG_FACES_ALL)
        return fail(who + std::to_string(dirichlet_faces) + " is no face set (x- = 1, x+ = 2, y- = 4, y+ = 8, z- = 16, z+ = 32: 1..63)");
    if (dirichlet_faces == 0) return fail(who + "a face set of 0 leaves no Dirichlet face: the operator would be singular");
    if (dirichlet_faces != MG_FACES_ALL) {
        if (c->dim != 3) return fail(who + "no-flux faces are 3-D only (this handle is 2-D)");
        if (c->comm.active()) return fail(who + "no-flux faces need a whole (not slab) handle");
    }
    c->diffusion_faces = dirichlet_faces;
    return 0;
}

int mg_set_diffusion_insulated(mg_handle c) {
    if (!c) return fail("null handle");
    const std::string who = "mg_set_diffusion_insulated: ";
    if (c->dim != 3) return fail(who + "insulated bodies are 3-D only (this handle is 2-D)");
    if (c->comm.active()) return fail(who + "insulated bodies need a whole (not slab) handle");
    c->diffusion_faces = 0;
    return 0;
}

int mg_diffusion_nullspace(mg_handle c, int level, int* singular) {
    MG_TRY(check_level(c, level));
    if (!singular) return fail("null argument");
    *singular = cycle_singular(c, level) ? 1 : 0;
    return 0;
}

int mg_remove_mean(mg_handle c, double* x_dev, const double* w_dev, int64_t n, double* mean) {
    const std::string who = "mg_remove_mean";
    if (!c) return fail("null handle");
    if (n < 1) return fail(who + ": n must be positive");
    HIP_TRY(hipSetDevice(c->device));
    MG_TRY(need_device_pointer(c, x_dev, who.c_str(), "x_dev"));
    if (w_dev) MG_TRY(need_device_pointer(c, w_dev, who.c_str(), "w_dev"));
    if (reinterpret_cast<uintptr_t>(x_dev) % 16 || reinterpret_cast<uintptr_t>(w_dev) % 16)
        return fail(who + ": x_dev and w_dev must be 16-byte aligned");
    MG_TRY(ns_workspace(c, n));
    double denom = (double)n;
    const int64_t nb = ns_blocks(n);
    double* const part = c->ns_part;
    if (w_dev) {                                // the sum of the weights, by the same kernels
        hipLaunchKernelGGL(ns_partial, dim3((unsigned)nb), dim3(BLOCK), 0, c->stream, w_dev, (const double*)nullptr, n, part);
        hipLaunchKernelGGL(fcg_fold, dim3(1), dim3(BLOCK), 0, c->stream, (const double*)part, nb, 1, part + nb);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&denom, part + nb, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (!(denom > 0.0)) return fail(who + ": the weights do not sum to a positive number");
    }
    MG_TRY(ns_remove(c, x_dev, w_dev, nullptr, n, 1.0 / denom, c->scalars.get()));
    HIP_TRY(hipMemcpyAsync(c->h_scalars, c->scalars, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (mean) *mean = c->h_scalars[0];
    return 0;
}

int mg_diffusion_faces(mg_handle c, int* dirichlet_faces) {
    if (!c) return fail("null handle");
    if (!dirichlet_faces) return fail("null argument");
    *dirichlet_faces = c->diffusion_faces;
    return 0;
}

namespace {

// the first cell of the device sigma that is not a finite double >= 0, as an error (check_kappa's wording)
int check_sigma(mg_context* c, const std::string& who, const double* d_sigma, int64_t n, int N) {
    DevTemp d_first;
    MG_TRY(d_first.alloc(sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(d_first.p, 0xff, sizeof(unsigned long long), c->stream));
    const unsigned nb = (unsigned)std::max<int64_t>(1, std::min<int64_t>(8192, (n + 255) / 256));
    hipLaunchKernelGGL(sigma_check, dim3(nb), dim3(256), 0, c->stream, d_sigma, n, d_first.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    unsigned long long first = 0;
    HIP_TRY(hipMemcpyAsync(&first, d_first.p, sizeof(first), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (first == ~0ull) return 0;
    double x = 0.0;
    HIP_TRY(hipMemcpy(&x, d_sigma + first, sizeof(double), hipMemcpyDeviceToHost));
    const int64_t q = (int64_t)first;
    char val[40];
    snprintf(val, sizeof(val), "%.17g", x);
    return fail(who + ": sigma must be finite and not negative: cell (" + std::to_string(q % N) + ", " + std::to_string((q / N) % N) + ", " +
                std::to_string(q / ((int64_t)N * N)) + ") = index " + std::to_string(q) + " holds " + val);
}

// what both variants of mg_set_diffusion_reaction refuse before they look at the pointer
int reaction_refusals(mg_context* c, const std::string& who, int N) {
    if (c->dim != 3) return fail(who + ": the reaction term is 3-D only (this handle is 2-D)");
    if (c->comm.active()) return fail(who + ": the reaction term needs a whole (not slab) handle");
    if (N <= 0) return fail(who + ": elements_per_dim must be positive");
    return 0;
}

// the checked field becomes the handle's; until here the handle is as it was
int adopt_sigma(mg_context* c, const std::string& who, DevTemp& field, int N) {
    const int64_t n = (int64_t)N * N * N;
    MG_TRY(check_sigma(c, who, field.as<const double>(), n, N));
    c->sigma.adopt(c, field.release<double>(), (size_t)n);
    c->sigma_N = N;
    return 0;
}

}  // namespace

int mg_set_diffusion_reaction(mg_handle c, int N, const double* sigma_host) {
    if (!c) return fail("null handle");
    const std::string who = "mg_set_diffusion_reaction";
    if (!sigma_host) {
        c->sigma.reset();
        c->sigma_N = 0;
        return 0;
    }
    MG_TRY(reaction_refusals(c, who, N));
    HIP_TRY(hipSetDevice(c->device));
    hipPointerAttribute_t at{};
    const hipError_t e = hipPointerGetAttributes(&at, sigma_host);
    if (e != hipSuccess) (void)hipGetLastError();       // (an unregistered host pointer is an error of the query in some runtimes)
    if (e == hipSuccess && at.type == hipMemoryTypeDevice)
        return fail(who + ": sigma is not host memory (a device pointer? mg_set_diffusion_reaction_device takes those)");
    const size_t bytes = (size_t)N * N * N * 8;
    DevTemp field;
    MG_TRY(field.alloc(bytes));
    HIP_TRY(hipMemcpy(field.p, sigma_host, bytes, hipMemcpyHostToDevice));
    return adopt_sigma(c, who, field, N);
}

int mg_set_diffusion_reaction_device(mg_handle c, int N, const double* sigma_dev) {
    if (!c) return fail("null handle");
    const std::string who = "mg_set_diffusion_reaction_device";
    if (!sigma_dev) {
        c->sigma.reset();
        c->sigma_N = 0;
        return 0;
    }
    MG_TRY(reaction_refusals(c, who, N));
    HIP_TRY(hipSetDevice(c->device));
    MG_TRY(need_device_pointer(c, sigma_dev, who.c_str(), "sigma"));
    const size_t bytes = (size_t)N * N * N * 8;
    DevTemp field;
    MG_TRY(field.alloc(bytes));
    HIP_TRY(hipMemcpyAsync(field.p, sigma_dev, bytes, hipMemcpyDeviceToDevice, c->stream));
    return adopt_sigma(c, who, field, N);
}

int mg_diffusion_reaction(mg_handle c, int* on, int* elements_per_dim) {
    if (!c) return fail("null handle");
    if (on) *on = c->sigma ? 1 : 0;
    if (elements_per_dim) *elements_per_dim = c->sigma_N;
    return 0;
}

int mg_level_reaction(mg_handle c, int level, int* on) {
    MG_TRY(check_level(c, level));
    if (on) *on = c->L[level].react ? 1 : 0;
    return 0;
}

namespace {

// the bit number of a face that is exactly one bit of enum mg_face, -1 otherwise
int face_index(int face) {
    for (int f = 0; f < 6; ++f)
        if (face == 1 << f) return f;
    return -1;
}

int bad_face(const std::string& who, int face) {
    return fail(who + ": face = " + std::to_string(face) + " is not exactly one face (x- = 1, x+ = 2, y- = 4, y+ = 8, z- = 16, z+ = 32)");
}

// one Robin field into the handle: refusals, the copy, the check; until the last line the handle is as it was
int set_diffusion_robin(mg_context* c, const std::string& who, int N, int face, const double* alpha, bool device) {
    if (!c) return fail("null handle");
    const int fi = face_index(face);
    if (fi < 0) return bad_face(who, face);
    if (!alpha) {
        c->alpha[fi].reset();
        if (!robin_faces(c)) c->alpha_N = 0;
        return 0;
    }
    if (c->dim != 3) return fail(who + ": Robin faces are 3-D only (this handle is 2-D)");
    if (c->comm.active()) return fail(who + ": Robin faces need a whole (not slab) handle");
    if (N <= 0) return fail(who + ": elements_per_dim must be positive");
    if ((robin_faces(c) & ~face) && N != c->alpha_N)
        return fail(who + ": elements_per_dim = " + std::to_string(N) + ", the fields the handle holds on other faces have " +
                    std::to_string(c->alpha_N) + " face-cells per dimension: clear them first");
    HIP_TRY(hipSetDevice(c->device));
    const int64_t n = (int64_t)N * N;
    DevTemp field;
    if (device) {
        MG_TRY(need_device_pointer(c, alpha, who.c_str(), "alpha"));
        MG_TRY(field.alloc((size_t)n * 8));
        HIP_TRY(hipMemcpyAsync(field.p, alpha, (size_t)n * 8, hipMemcpyDeviceToDevice, c->stream));
    } else {
        hipPointerAttribute_t at{};
        const hipError_t e = hipPointerGetAttributes(&at, alpha);
        if (e != hipSuccess) (void)hipGetLastError();       // (an unregistered host pointer is an error of the query in some runtimes)
        if (e == hipSuccess && at.type == hipMemoryTypeDevice)
            return fail(who + ": alpha is not host memory (a device pointer? mg_set_diffusion_robin_device takes those)");
        MG_TRY(field.alloc((size_t)n * 8));
        HIP_TRY(hipMemcpy(field.p, alpha, (size_t)n * 8, hipMemcpyHostToDevice));
    }
    // the first face-cell that is not a finite double >= 0 (sigma_check: the same condition), as an error
    DevTemp d_first;
    MG_TRY(d_first.alloc(sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(d_first.p, 0xff, sizeof(unsigned long long), c->stream));
    const unsigned nb = (unsigned)std::max<int64_t>(1, std::min<int64_t>(8192, (n + 255) / 256));
    hipLaunchKernelGGL(sigma_check, dim3(nb), dim3(256), 0, c->stream, field.as<const double>(), n, d_first.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    unsigned long long first = 0;
    HIP_TRY(hipMemcpyAsync(&first, d_first.p, sizeof(first), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (first != ~0ull) {
        double x = 0.0;
        HIP_TRY(hipMemcpy(&x, field.as<const double>() + first, sizeof(double), hipMemcpyDeviceToHost));
        char val[40];
        snprintf(val, sizeof(val), "%.17g", x);
        return fail(who + ": alpha must be finite and not negative: face-cell (" + std::to_string((int64_t)first % N) + ", " +
                    std::to_string((int64_t)first / N) + ") of face " + std::to_string(face) + " = index " + std::to_string(first) + " holds " + val);
    }
    c->alpha[fi].adopt(c, field.release<double>(), (size_t)n);
    c->alpha_N = N;
    return 0;
}

}  // namespace

int mg_set_diffusion_robin(mg_handle c, int N, int face, const double* alpha_host) {
    return set_diffusion_robin(c, "mg_set_diffusion_robin", N, face, alpha_host, false);
}

int mg_set_diffusion_robin_device(mg_handle c, int N, int face, const double* alpha_dev) {
    return set_diffusion_robin(c, "mg_set_diffusion_robin_device", N, face, alpha_dev, true);
}

int mg_diffusion_robin(mg_handle c, int* faces, int* elements_per_dim) {
    if (!c) return fail("null handle");
    if (faces) *faces = robin_faces(c);
    if (elements_per_dim) *elements_per_dim = c->alpha_N;
    return 0;
}

int mg_level_robin(mg_handle c, int level, int* faces) {
    MG_TRY(check_level(c, level));
    if (faces) *faces = c->L[level].robin;
    return 0;
}

int mg_level_matrix_free(mg_handle c, int level, int* on, int64_t* kappa_bytes) {
    MG_TRY(check_level(c, level));
    const Level& L = c->L[level];
    if (on) *on = L.mf ? 1 : 0;
    if (kappa_bytes) *kappa_bytes = L.mf ? (int64_t)(L.kappa.count() * sizeof(double)) : 0;
    return 0;
}

int mg_jacobi_split(int device, int64_t n_rows, int64_t nnz, const void* indptr, int indptr_is_64,
                    const int32_t* indices, const double* data, double* dinv, double* scaled, unsigned char* keep) {
    if (!indptr || !indices || !data || !dinv || !scaled || !keep) return fail("null argument");
    // duplicates allowed: they sum, as in SciPy's A.diagonal() and A - D (the reference's getJacobiMatrices)
    MG_TRY(check_csr(n_rows, n_rows, nnz, indptr, indptr_is_64, indices, true));
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail("no HIP device visible: this library has no CPU path");
    HIP_TRY(hipSetDevice(device));
    DevTemp d_ptr, d_idx, d_val, d_dinv, d_scaled, d_keep;
    const size_t ptr_bytes = (size_t)(n_rows + 1) * (indptr_is_64 ? 8 : 4);
    MG_TRY(d_ptr.alloc(ptr_bytes));
    MG_TRY(d_idx.alloc((size_t)nnz * 4));
    MG_TRY(d_val.alloc((size_t)nnz * 8));
    MG_TRY(d_dinv.alloc((size_t)n_rows * 8));
    MG_TRY(d_scaled.alloc((size_t)nnz * 8));
    MG_TRY(d_keep.alloc((size_t)nnz));
    HIP_TRY(hipMemcpy(d_ptr.p, indptr, ptr_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_idx.p, indices, (size_t)nnz * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_val.p, data, (size_t)nnz * 8, hipMemcpyHostToDevice));
    CsrArgs a{};
    a.indptr = d_ptr.p; a.indptr64 = indptr_is_64; a.indices = d_idx.as<int>(); a.data = d_val.as<double>(); a.n = n_rows;
    hipLaunchKernelGGL(jacobi_split, dim3(blocks_for(n_rows, 256)), dim3(256), 0, 0, a, d_dinv.as<double>(), d_scaled.as<double>(),
                       d_keep.as<unsigned char>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(dinv, d_dinv.p, (size_t)n_rows * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(scaled, d_scaled.p, (size_t)nnz * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(keep, d_keep.p, (size_t)nnz, hipMemcpyDeviceToHost));
    return 0;
}

int mg_level_info(mg_handle c, int level, int64_t* n_global, int64_t* n_local, int64_t* row0, int64_t* nnz_stored,
                  int64_t* nnz_nonzero, int* ell_width, int* replicated, int* offset_codes) {
    MG_TRY(check_level(c, level));
    const Level& L = c->L[level];
    if (n_global) *n_global = L.n_global;
    if (n_local) *n_local = L.nloc;
    if (row0) *row0 = L.row0;
    if (nnz_stored) *nnz_stored = (int64_t)L.nnz_stored;
    if (nnz_nonzero) *nnz_nonzero = (int64_t)L.nnz_nonzero;
    if (ell_width) *ell_width = L.W;
    if (replicated) *replicated = L.replicated ? 1 : 0;
    if (offset_codes) *offset_codes = L.sdia ? -L.wu : (L.coded ? L.ntable : 0);
    return 0;
}

int mg_level_storage(mg_handle c, int level, int* symmetric, int64_t* first_asymmetric_row, int64_t* max_pair_ulps,
                     int* distinct_rows, int* ulps_used, int64_t* escape_rows) {
    MG_TRY(check_level(c, level));
    const Level& L = c->L[level];
    if (symmetric) *symmetric = L.rep_sym;
    if (first_asymmetric_row) *first_asymmetric_row = L.rep_first_asym;
    if (max_pair_ulps) *max_pair_ulps = L.rep_max_ulps;
    if (distinct_rows) *distinct_rows = L.rep_distinct;
    if (escape_rows) *escape_rows = L.cls_escape ? L.rep_escape : 0;
    if (ulps_used) *ulps_used = std::max(L.sdia ? (L.rep_sym_qbits ? 1 << L.rep_sym_qbits : 0) : 0, L.cls ? (L.rep_cls_qbits ? 1 << L.rep_cls_qbits : 0) : 0);
    return 0;
}

int mg_level_row_classes(mg_handle c, int level, int* classes) {
    MG_TRY(check_level(c, level));
    if (!classes) return fail("bad arguments");
    *classes = c->L[level].cls ? c->L[level].ncls : c->L[level].nscls;
    return 0;
}

int mg_set_vector(mg_handle c, int level, int which, const double* host) {
    MG_TRY(check_level(c, level));
    if (!host) return fail("null host vector");
    HIP_TRY(hipSetDevice(c->device));
    Level& L = c->L[level];
    DVector* v = pick(L, which);
    if (!v) return fail("unknown vector selector");
    MG_TRY(vec_alloc(c, L, v));
    return upload_vector(c, L, *v, host);
}

int mg_set_rhs_true(mg_handle c, int level, const double* host) {
    MG_TRY(check_level(c, level));
    if (!host) return fail("null host vector");
    HIP_TRY(hipSetDevice(c->device));
    Level& L = c->L[level];
    MG_TRY(vec_alloc(c, L, &L.ftrue));
    return upload_vector(c, L, L.ftrue, host);
}

int mg_get_vector(mg_handle c, int level, int which, double* host, int gather) {
    MG_TRY(check_level(c, level));
    if (!host) return fail("null host vector");
    HIP_TRY(hipSetDevice(c->device));
    Level& L = c->L[level];
    DVector* v = pick(L, which);
    if (!v || !v->raw) return fail("vector is not available on this level");
    MG_TRY(ensure_stage(c, L.n_global));
    ++c->downloads;
    const unsigned nb = (unsigned)std::min<int64_t>(4096, (L.n_global + 255) / 256);
    if (gather && is_slab(c, L)) {
        // all-gather slabs in lexicographic order inside a scratch vector, then permute
        DevBuf<double> full;
        MG_TRY(full.alloc(c, (size_t)L.n_global));
        HIP_TRY(hipMemcpyAsync(full + L.row0, v->rows, (size_t)L.nloc * 8, hipMemcpyDeviceToDevice, c->stream));
        MG_TRY(allgather_planes(c, L.splits, L.g.plane, full));
        hipLaunchKernelGGL(gather_out, dim3(nb), dim3(256), 0, c->stream, full, L.perm, L.n_global, (int64_t)0,
                           L.n_global, (int64_t)0, c->stage);
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(host, c->stage, (size_t)L.n_global * 8, hipMemcpyDeviceToHost));
        return 0;
    }
    if (is_slab(c, L)) {
        // owned rows only: pre-load the caller's buffer so untouched entries survive
        HIP_TRY(hipMemcpyAsync(c->stage, host, (size_t)L.n_global * 8, hipMemcpyHostToDevice, c->stream));
    }
    hipLaunchKernelGGL(gather_out, dim3(nb), dim3(256), 0, c->stream, v->base, L.perm, L.n_global, L.row0, L.nloc,
                       L.g.lead, c->stage);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host, c->stage, (size_t)L.n_global * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int mg_set_vector_device(mg_handle c, int level, int which, const double* dev) {
    if (!c) return fail("null handle");
    if (c->comm.active()) return fail("mg_set_vector_device needs a whole (not slab) handle");
    MG_TRY(check_level(c, level));
    HIP_TRY(hipSetDevice(c->device));
    MG_TRY(need_device_pointer(c, dev, "mg_set_vector_device", "the vector"));
    Level& L = c->L[level];
    DVector* v = pick(L, which);
    if (!v) return fail("unknown vector selector");
    MG_TRY(vec_alloc(c, L, v));
    const unsigned nb = (unsigned)std::min<int64_t>(4096, (L.n_global + 255) / 256);
    hipLaunchKernelGGL(scatter_in, dim3(nb), dim3(256), 0, c->stream, dev, L.perm, L.n_global, L.row0, L.g.lead, L.xlen, v->base);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int mg_get_vector_device(mg_handle c, int level, int which, double* dev) {
    if (!c) return fail("null handle");
    if (c->comm.active()) return fail("mg_get_vector_device needs a whole (not slab) handle");
    MG_TRY(check_level(c, level));
    HIP_TRY(hipSetDevice(c->device));
    MG_TRY(need_device_pointer(c, dev, "mg_get_vector_device", "the vector"));
    Level& L = c->L[level];
    DVector* v = pick(L, which);
    if (!v || !v->raw) return fail("vector is not available on this level");
    const unsigned nb = (unsigned)std::min<int64_t>(4096, (L.n_global + 255) / 256);
    hipLaunchKernelGGL(gather_out, dim3(nb), dim3(256), 0, c->stream, v->base, L.perm, L.n_global, L.row0, L.nloc, L.g.lead, dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// One input of a sensitivity or cell gradient entry, for the checks that pass before anything is launched: device memory of
// the handle's device (`optional`: or null) and, where `apart` is not null, no byte in common with the output, which other
// threads read while a thread writes its entries; `apart` is the reason appended to that refusal.
struct Operand { const char* name; const void* p; size_t bytes; bool optional; const char* apart; };

static int need_operands(mg_context* c, const char* who, std::initializer_list<Operand> in, const void* out, size_t out_bytes) {
    for (const Operand& o : in)
        if (o.p || !o.optional) MG_TRY(need_device_pointer(c, o.p, who, o.name));
    MG_TRY(need_device_pointer(c, out, who, "out"));
    for (const Operand& o : in)
        if (o.p && o.apart && overlaps(out, out_bytes, o.p, o.bytes)) return fail(std::string(who) + ": out overlaps " + o.name + o.apart);
    return 0;
}

static size_t node_bytes(const Level& L) { return (size_t)L.g.plane * (size_t)L.g.nz * 8; }
static size_t cell_bytes(const Level& L) { return (size_t)L.N * L.N * L.N * 8; }
static size_t face_cell_bytes(const Level& L) { return (size_t)L.N * L.N * 8; }

static int need_node_set(const char* who, const char* what, int value) {
    if (value != MG_NODES_INTERIOR && value != MG_NODES_ALL)
        return fail(std::string(who) + ": " + what + " = " + std::to_string(value) +
                    " is no node set (MG_NODES_INTERIOR = 0, MG_NODES_ALL = 1)");
    return 0;
}

// the two kappa sensitivities under the name of the entry called: the plain entries are the _ex forms with both node sets
// MG_NODES_INTERIOR
static int diffusion_dkappa(const char* who, mg_context* c, int level, const double* a_dev, int a_nodes, const double* b_dev, int b_nodes,
                            double* out_dev) {
    MG_TRY(need_dkappa_level(c, level, who));
    MG_TRY(need_node_set(who, "a_nodes", a_nodes));
    MG_TRY(need_node_set(who, "b_nodes", b_nodes));
    HIP_TRY(hipSetDevice(c->device));
    const Level& L = c->L[level];
    MG_TRY(need_operands(c, who, {{"a", a_dev, node_bytes(L), false, nullptr}, {"b", b_dev, node_bytes(L), false, nullptr}}, out_dev, cell_bytes(L)));
    MG_TRY(launch_dkappa(c, L, a_dev, b_dev, out_dev, c->dkappa_gather != 0, a_nodes == MG_NODES_ALL, b_nodes == MG_NODES_ALL));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

static int diffusion_apply_dkappa(const char* who, mg_context* c, int level, const double* dkappa_dev, const double* x_dev, int rows, int cols,
                                  double* out_dev) {
    MG_TRY(need_dkappa_level(c, level, who));
    MG_TRY(need_node_set(who, "rows", rows));
    MG_TRY(need_node_set(who, "cols", cols));
    HIP_TRY(hipSetDevice(c->device));
    const Level& L = c->L[level];
    // the march reads the neighbours of a row (and of a cell) while other workgroups write theirs
    MG_TRY(need_operands(c, who, {{"dkappa", dkappa_dev, cell_bytes(L), false, " (the march reads a row's cells)"},
                                  {"x", x_dev, node_bytes(L), false, " (the march reads a row's neighbours)"}}, out_dev, node_bytes(L)));
    MG_TRY(launch_apply_dkappa(c, L, dkappa_dev, x_dev, out_dev, rows == MG_NODES_ALL, cols == MG_NODES_ALL));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int mg_diffusion_dkappa(mg_handle c, int level, const double* a_dev, const double* b_dev, double* out_dev) {
    return diffusion_dkappa("mg_diffusion_dkappa", c, level, a_dev, MG_NODES_INTERIOR, b_dev, MG_NODES_INTERIOR, out_dev);
}

int mg_diffusion_dkappa_ex(mg_handle c, int level, const double* a_dev, int a_nodes, const double* b_dev, int b_nodes, double* out_dev) {
    return diffusion_dkappa("mg_diffusion_dkappa_ex", c, level, a_dev, a_nodes, b_dev, b_nodes, out_dev);
}

int mg_diffusion_apply_dkappa(mg_handle c, int level, const double* dkappa_dev, const double* x_dev, double* out_dev) {
    return diffusion_apply_dkappa("mg_diffusion_apply_dkappa", c, level, dkappa_dev, x_dev, MG_NODES_INTERIOR, MG_NODES_INTERIOR, out_dev);
}

int mg_diffusion_apply_dkappa_ex(mg_handle c, int level, const double* dkappa_dev, const double* x_dev, int rows, int cols,
                                 double* out_dev) {
    return diffusion_apply_dkappa("mg_diffusion_apply_dkappa_ex", c, level, dkappa_dev, x_dev, rows, cols, out_dev);
}

int mg_diffusion_dsigma(mg_handle c, int level, const double* a_dev, const double* b_dev, double* out_dev) {
    const char* who = "mg_diffusion_dsigma";
    MG_TRY(need_dkappa_level(c, level, who, "sigma"));
    HIP_TRY(hipSetDevice(c->device));
    const Level& L = c->L[level];
    MG_TRY(need_operands(c, who, {{"a", a_dev, node_bytes(L), false, ""}, {"b", b_dev, node_bytes(L), false, ""}}, out_dev, cell_bytes(L)));
    MG_TRY(launch_dsigma(c, L, a_dev, b_dev, out_dev));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int mg_diffusion_apply_dsigma(mg_handle c, int level, const double* dsigma_dev, const double* x_dev, double* out_dev) {
    const char* who = "mg_diffusion_apply_dsigma";
    MG_TRY(need_dkappa_level(c, level, who, "sigma"));
    HIP_TRY(hipSetDevice(c->device));
    const Level& L = c->L[level];
    MG_TRY(need_operands(c, who, {{"dsigma", dsigma_dev, cell_bytes(L), false, ""}, {"x", x_dev, node_bytes(L), false, ""}}, out_dev, node_bytes(L)));
    MG_TRY(launch_apply_dsigma(c, L, dsigma_dev, x_dev, out_dev));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// what the two Robin sensitivities refuse beyond the sigma entries: a face that is not one face or lies in the Dirichlet set
static int need_drobin_face(mg_context* c, const char* who, int face, int* fi) {
    *fi = face_index(face);
    if (*fi < 0) return bad_face(who, face);
    if (face & c->diffusion_faces)
        return fail(std::string(who) + ": face " + std::to_string(face) + " is a Dirichlet face of the handle's face set " +
                    std::to_string(c->diffusion_faces) + " (mg_set_diffusion_faces): it has no free node");
    return 0;
}

int mg_diffusion_drobin(mg_handle c, int level, int face, const double* a_dev, const double* b_dev, double* out_dev) {
    const char* who = "mg_diffusion_drobin";
    MG_TRY(need_dkappa_level(c, level, who, "Robin"));
    int fi = -1;
    MG_TRY(need_drobin_face(c, who, face, &fi));
    HIP_TRY(hipSetDevice(c->device));
    const Level& L = c->L[level];
    MG_TRY(need_operands(c, who, {{"a", a_dev, node_bytes(L), false, ""}, {"b", b_dev, node_bytes(L), false, ""}}, out_dev, face_cell_bytes(L)));
    MG_TRY(launch_drobin(c, L, fi, a_dev, b_dev, out_dev));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int mg_diffusion_apply_drobin(mg_handle c, int level, int face, const double* dalpha_dev, const double* x_dev, double* out_dev) {
    const char* who = "mg_diffusion_apply_drobin";
    MG_TRY(need_dkappa_level(c, level, who, "Robin"));
    int fi = -1;
    MG_TRY(need_drobin_face(c, who, face, &fi));
    HIP_TRY(hipSetDevice(c->device));
    const Level& L = c->L[level];
    MG_TRY(need_operands(c, who, {{"dalpha", dalpha_dev, face_cell_bytes(L), false, ""}, {"x", x_dev, node_bytes(L), false, ""}}, out_dev, node_bytes(L)));
    MG_TRY(launch_apply_drobin(c, L, fi, dalpha_dev, x_dev, out_dev));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// the cell gradient family: whole 3-D grid levels, refused by name otherwise
static int need_cell_grad_level(mg_context* c, int level, const char* who) {
    if (!c) return fail("null handle");
    if (c->dim != 3) return fail(std::string(who) + ": the cell gradient is 3-D only (this handle is 2-D)");
    if (c->comm.active()) return fail(std::string(who) + " needs a whole (not slab) handle");
    MG_TRY(check_level(c, level));
    if (c->L[level].flat) return fail(std::string(who) + ": level " + std::to_string(level) + " is flat (no grid): it has no cells");
    return 0;
}

int mg_diffusion_cell_gradient(mg_handle c, int level, const double* w_dev, const double* x_dev, double* out_dev) {
    const char* who = "mg_diffusion_cell_gradient";
    MG_TRY(need_cell_grad_level(c, level, who));
    HIP_TRY(hipSetDevice(c->device));
    const Level& L = c->L[level];
    MG_TRY(need_operands(c, who, {{"w", w_dev, cell_bytes(L), true, ""}, {"x", x_dev, node_bytes(L), false, ""}}, out_dev, 3 * cell_bytes(L)));
    MG_TRY(launch_cell_grad<CG_F>(c, L, w_dev, nullptr, x_dev, out_dev));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int mg_diffusion_cell_gradient_t(mg_handle c, int level, const double* w_dev, const double* p_dev, double* out_dev) {
    const char* who = "mg_diffusion_cell_gradient_t";
    MG_TRY(need_cell_grad_level(c, level, who));
    HIP_TRY(hipSetDevice(c->device));
    const Level& L = c->L[level];
    MG_TRY(need_operands(c, who, {{"w", w_dev, cell_bytes(L), true, ""}, {"p", p_dev, 3 * cell_bytes(L), false, ""}}, out_dev, node_bytes(L)));
    MG_TRY(launch_cell_grad_t(c, L, w_dev, p_dev, out_dev));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int mg_diffusion_cell_gradient_dot(mg_handle c, int level, const double* p_dev, const double* x_dev, double* out_dev) {
    const char* who = "mg_diffusion_cell_gradient_dot";
    MG_TRY(need_cell_grad_level(c, level, who));
    HIP_TRY(hipSetDevice(c->device));
    const Level& L = c->L[level];
    MG_TRY(need_operands(c, who, {{"p", p_dev, 3 * cell_bytes(L), false, ""}, {"x", x_dev, node_bytes(L), false, ""}}, out_dev, cell_bytes(L)));
    MG_TRY(launch_cell_grad<CG_C>(c, L, nullptr, p_dev, x_dev, out_dev));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// The point family (mg_diffusion_points.hip.h) on a whole 3-D grid level, every refusal with the entry's name: what the cell
// gradient family refuses, M < 1, and -- after one checking kernel -- a coordinate outside [0, 1], by the lowest offending point
// index (an integer min, as check_kappa).
static int need_point_level(mg_context* c, int level, const char* who) {
    const std::string w(who);
    if (!c) return fail(w + ": null handle");
    if (c->dim != 3) return fail(w + ": points are located on 3-D levels only (this handle is 2-D)");
    if (c->comm.active()) return fail(w + " needs a whole (not slab) handle");
    if (level < 0 || level >= c->nlev) return fail(w + ": level " + std::to_string(level) + " out of range");
    if (!c->L[level].set) return fail(w + ": level " + std::to_string(level) + " has not been set");
    if (c->L[level].flat) return fail(w + ": level " + std::to_string(level) + " is flat (no grid): it has no cells");
    return 0;
}

static int need_points(mg_context* c, const char* who, int64_t M, const double* pts) {
    DevTemp d_first;
    MG_TRY(d_first.alloc(sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(d_first.p, 0xff, sizeof(unsigned long long), c->stream));
    const unsigned nb = (unsigned)std::max<int64_t>(1, std::min<int64_t>(8192, (3 * M + 255) / 256));
    hipLaunchKernelGGL(pt_check, dim3(nb), dim3(256), 0, c->stream, pts, 3 * M, d_first.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    unsigned long long first = 0;
    HIP_TRY(hipMemcpyAsync(&first, d_first.p, sizeof(first), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (first == ~0ull) return 0;
    double x[3] = {0.0, 0.0, 0.0};
    HIP_TRY(hipMemcpy(x, pts + 3 * first, sizeof(x), hipMemcpyDeviceToHost));
    char val[120];
    snprintf(val, sizeof(val), "(%.17g, %.17g, %.17g)", x[0], x[1], x[2]);
    return fail(std::string(who) + ": a point must lie in the unit cube, every coordinate finite and in [0, 1]: point " +
                std::to_string(first) + " is " + val);
}

static int need_point_count(const char* who, int64_t M) {
    if (M < 1) return fail(std::string(who) + ": M = " + std::to_string(M) + " (at least one point is needed)");
    if (M > (int64_t)1 << 31) return fail(std::string(who) + ": M = " + std::to_string(M) + " is more than 2^31 points");
    return 0;
}

static PtArgs pt_args(const Level& L, int64_t M, const double* pts, const double* x, double* out, uint64_t* keys) {
    PtArgs a{};
    a.pts = pts; a.x = x; a.out = out; a.keys = keys;
    a.M = M; a.nx = L.g.nx; a.plane = L.g.plane; a.N = L.N;
    return a;
}

// S (GRAD false) or G (GRAD true) of the field x at the points
static int point_gather(mg_context* c, const bool GRAD, const char* who, int level, int64_t M, const double* pts, const double* x, double* out) {
    MG_TRY(need_point_level(c, level, who));
    MG_TRY(need_point_count(who, M));
    HIP_TRY(hipSetDevice(c->device));
    const Level& L = c->L[level];
    MG_TRY(need_operands(c, who, {{"pts", pts, (size_t)M * 24, false, ""}, {"x", x, node_bytes(L), false, ""}}, out,
                         (size_t)M * (GRAD ? 24 : 8)));
    MG_TRY(need_points(c, who, M, pts));
    const PtArgs a = pt_args(L, M, pts, x, out, nullptr);
    if (GRAD) hipLaunchKernelGGL(pt_gradient, dim3(blocks_for(M, PT_BLOCK)), dim3(PT_BLOCK), 0, c->stream, a);
    else hipLaunchKernelGGL(pt_sample, dim3(blocks_for(M, PT_BLOCK)), dim3(PT_BLOCK), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// S^T (GRAD false, in = w, M) or G^T (GRAD true, in = p, M x 3) onto the nodes: pairs, a stable sort by node, one add per run
static int point_scatter(mg_context* c, const bool GRAD, const char* who, int level, int64_t M, const double* pts, const double* in, double* out) {
    MG_TRY(need_point_level(c, level, who));
    MG_TRY(need_point_count(who, M));
    HIP_TRY(hipSetDevice(c->device));
    const Level& L = c->L[level];
    MG_TRY(need_operands(c, who, {{"pts", pts, (size_t)M * 24, false, ""}, {GRAD ? "p" : "w", in, (size_t)M * (GRAD ? 24 : 8), false, ""}},
                         out, node_bytes(L)));
    MG_TRY(need_points(c, who, M, pts));
    const size_t n = 4 * (size_t)M;
    const uint64_t nodes = (uint64_t)L.g.plane * (uint64_t)L.g.nz;
    unsigned bits = 1;                                      // the bits of the largest node id
    while (bits < 64 && ((nodes - 1) >> bits) != 0) ++bits;
    DevTemp keys_t, keys_s, vals_t, vals_s, sort_t;
    MG_TRY(keys_t.alloc(n * 8));
    MG_TRY(keys_s.alloc(n * 8));
    MG_TRY(vals_t.alloc(n * 8));
    MG_TRY(vals_s.alloc(n * 8));
    size_t sort_bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys_t.as<uint64_t>(), keys_s.as<uint64_t>(), vals_t.as<double>(),
                                      vals_s.as<double>(), n, 0u, bits, c->stream));
    MG_TRY(sort_t.alloc(sort_bytes));
    HIP_TRY(hipMemsetAsync(out, 0, node_bytes(L), c->stream));
    const PtArgs a = pt_args(L, M, pts, in, vals_t.as<double>(), keys_t.as<uint64_t>());
    if (GRAD) hipLaunchKernelGGL(pt_contrib<true>, dim3(blocks_for(M, PT_BLOCK)), dim3(PT_BLOCK), 0, c->stream, a);
    else hipLaunchKernelGGL(pt_contrib<false>, dim3(blocks_for(M, PT_BLOCK)), dim3(PT_BLOCK), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::radix_sort_pairs(sort_t.p, sort_bytes, keys_t.as<uint64_t>(), keys_s.as<uint64_t>(), vals_t.as<double>(),
                                      vals_s.as<double>(), n, 0u, bits, c->stream));
    hipLaunchKernelGGL(pt_run_sum, dim3(blocks_for((int64_t)n, PT_BLOCK)), dim3(PT_BLOCK), 0, c->stream, keys_s.as<const uint64_t>(),
                       vals_s.as<const double>(), (int64_t)n, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));              // the temporaries are freed on return
    return 0;
}

int mg_diffusion_point_sample(mg_handle c, int level, int64_t M, const double* pts_dev, const double* x_dev, double* out_dev) {
    return point_gather(c, false, "mg_diffusion_point_sample", level, M, pts_dev, x_dev, out_dev);
}

int mg_diffusion_point_load(mg_handle c, int level, int64_t M, const double* pts_dev, const double* w_dev, double* out_dev) {
    return point_scatter(c, false, "mg_diffusion_point_load", level, M, pts_dev, w_dev, out_dev);
}

int mg_diffusion_point_gradient(mg_handle c, int level, int64_t M, const double* pts_dev, const double* x_dev, double* out_dev) {
    return point_gather(c, true, "mg_diffusion_point_gradient", level, M, pts_dev, x_dev, out_dev);
}

int mg_diffusion_point_gradient_t(mg_handle c, int level, int64_t M, const double* pts_dev, const double* p_dev, double* out_dev) {
    return point_scatter(c, true, "mg_diffusion_point_gradient_t", level, M, pts_dev, p_dev, out_dev);
}

// ---- located point sets: checked, located and sorted once, then any number of lanes per call ------------------------------------
static PtArgs pt_set_locate_args(const mg_points& ps, const Level& L, uint64_t* keys) {
    return pt_args(L, ps.M, ps.pts, nullptr, nullptr, keys);
}

int mg_points_create(mg_handle c, int level, int64_t M, const double* pts_dev, mg_points_handle* out) {
    const char* who = "mg_points_create";
    if (out) *out = nullptr;
    MG_TRY(need_point_level(c, level, who));
    MG_TRY(need_point_count(who, M));
    if (!out) return fail(std::string(who) + ": null pointer (the set)");
    HIP_TRY(hipSetDevice(c->device));
    MG_TRY(need_device_pointer(c, pts_dev, who, "pts"));
    MG_TRY(need_points(c, who, M, pts_dev));
    const Level& L = c->L[level];
    std::unique_ptr<mg_points> owner(new mg_points());          // (a failure below leaves nothing behind)
    mg_points& ps = *owner;
    ps.level = level; ps.N = L.N; ps.M = M;
    const size_t n = 4 * (size_t)M;
    MG_TRY(ps.pts.alloc(c, 3 * (size_t)M));
    HIP_TRY(hipMemcpyAsync(ps.pts, pts_dev, (size_t)M * 24, hipMemcpyDeviceToDevice, c->stream));
    const uint64_t nodes = (uint64_t)L.g.plane * (uint64_t)L.g.nz;
    unsigned bits = 1;                                      // the bits of the largest node id, as point_scatter
    while (bits < 64 && ((nodes - 1) >> bits) != 0) ++bits;
    DevTemp keys_t, keys_s, slots_t, slots_s, sort_t, head_t, starts_t, count_t, select_t;
    MG_TRY(keys_t.alloc(n * 8));
    MG_TRY(keys_s.alloc(n * 8));
    MG_TRY(slots_t.alloc(n * 8));
    MG_TRY(slots_s.alloc(n * 8));
    MG_TRY(head_t.alloc(n));
    MG_TRY(starts_t.alloc((n + 1) * 8));
    MG_TRY(count_t.alloc(2 * sizeof(unsigned long long)));      // the number of runs; the longest run
    size_t sort_bytes = 0, select_bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys_t.as<uint64_t>(), keys_s.as<uint64_t>(), slots_t.as<uint64_t>(),
                                      slots_s.as<uint64_t>(), n, 0u, bits, c->stream));
    HIP_TRY(rocprim::select(nullptr, select_bytes, rocprim::counting_iterator<int64_t>(0), head_t.as<unsigned char>(), starts_t.as<int64_t>(),
                            count_t.as<unsigned long long>(), n, c->stream));
    MG_TRY(sort_t.alloc(sort_bytes));
    MG_TRY(select_t.alloc(select_bytes));
    MG_TRY(ps.rec.alloc(c, n));
    hipLaunchKernelGGL(pt_set_pairs, dim3(blocks_for(M, PT_BLOCK)), dim3(PT_BLOCK), 0, c->stream, pt_set_locate_args(ps, L, keys_t.as<uint64_t>()),
                       slots_t.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::radix_sort_pairs(sort_t.p, sort_bytes, keys_t.as<uint64_t>(), keys_s.as<uint64_t>(), slots_t.as<uint64_t>(),
                                      slots_s.as<uint64_t>(), n, 0u, bits, c->stream));
    hipLaunchKernelGGL(pt_set_records, dim3(blocks_for((int64_t)n, PT_BLOCK)), dim3(PT_BLOCK), 0, c->stream, pt_set_locate_args(ps, L, nullptr),
                       keys_s.as<const uint64_t>(), slots_s.as<const uint64_t>(), (int64_t)n, ps.rec.get(), head_t.as<unsigned char>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(count_t.p, 0, 2 * sizeof(unsigned long long), c->stream));
    HIP_TRY(rocprim::select(select_t.p, select_bytes, rocprim::counting_iterator<int64_t>(0), head_t.as<unsigned char>(), starts_t.as<int64_t>(),
                            count_t.as<unsigned long long>(), n, c->stream));
    unsigned long long counts[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(counts, count_t.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int64_t R = (int64_t)counts[0];
    if (R < 1 || (size_t)R > n) return fail(std::string(who) + ": the run count is inconsistent");
    ps.R = R;
    MG_TRY(ps.run_start.alloc(c, (size_t)R + 1));
    MG_TRY(ps.run_node.alloc(c, (size_t)R));
    HIP_TRY(hipMemcpyAsync(ps.run_start, starts_t.p, (size_t)R * 8, hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(pt_set_runs, dim3(blocks_for(R, PT_BLOCK)), dim3(PT_BLOCK), 0, c->stream, keys_s.as<const uint64_t>(), (int64_t)n, R,
                       ps.run_start.get(), ps.run_node.get(), count_t.as<unsigned long long>() + 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(counts + 1, count_t.as<unsigned long long>() + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));              // the temporaries are freed on return
    ps.longest = (int64_t)counts[1];
    c->point_sets.push_back(std::move(owner));
    *out = c->point_sets.back().get();
    return 0;
}

// the handle's own set behind `ps`, or null: nothing of `ps` is read before it is found in the list
static mg_points* own_point_set(mg_context* c, const mg_points* ps) {
    for (const auto& s : c->point_sets)
        if (s.get() == ps) return s.get();
    return nullptr;
}

static int need_point_set(mg_context* c, const mg_points* ps, const char* who) {
    const std::string w(who);
    if (!c) return fail(w + ": null handle");
    if (!ps) return fail(w + ": null point set");
    if (!own_point_set(c, ps))
        return fail(w + ": this is no live point set of this handle (destroyed already, or made by another handle)");
    return 0;
}

int mg_points_destroy(mg_handle c, mg_points_handle ps) {
    MG_TRY(need_point_set(c, ps, "mg_points_destroy"));
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (auto it = c->point_sets.begin(); it != c->point_sets.end(); ++it)
        if (it->get() == ps) { c->point_sets.erase(it); break; }
    return 0;
}

int mg_points_info(mg_handle c, mg_points_handle ps, int* level, int* N, int64_t* M, int64_t* runs, int64_t* longest_run, int64_t* bytes) {
    MG_TRY(need_point_set(c, ps, "mg_points_info"));
    if (level) *level = ps->level;
    if (N) *N = ps->N;
    if (M) *M = ps->M;
    if (runs) *runs = ps->R;
    if (longest_run) *longest_run = ps->longest;
    if (bytes) *bytes = ps->bytes();
    return 0;
}

// What the four batched entries refuse before anything is launched, and then their launches: the lanes in ascending groups of
// c->pt_group, the last group with what is left.  GATHER: S / G (in: nodes; out: M or 3 M); otherwise S^T / G^T (in: M or 3 M; out:
// nodes, zeroed on the stream first).
static int point_set_apply(mg_context* c, mg_points* ps, const bool GATHER, const bool GRAD, const char* who, const char* in_name, int nb,
                           const double* const* in, double* const* out) {
    const std::string w(who);
    MG_TRY(need_point_set(c, ps, who));
    const Level& L = c->L[ps->level];
    if (!L.set || L.flat || L.N != ps->N)
        return fail(w + ": level " + std::to_string(ps->level) + (L.set && !L.flat ? " has been set again with N = " + std::to_string(L.N)
                                                                                  : std::string(" is no longer a set grid level")) +
                    "; this set was located on N = " + std::to_string(ps->N) + " (make a new one)");
    if (nb < 1 || nb > MG_BATCH_MAX)
        return fail(w + ": nb = " + std::to_string(nb) + " is outside 1.." + std::to_string(MG_BATCH_MAX) + " (MG_BATCH_MAX)");
    if (!in || !out) return fail(w + ": null pointer array");
    HIP_TRY(hipSetDevice(c->device));
    const size_t per_point = (size_t)ps->M * (GRAD ? 24 : 8);
    const size_t in_bytes = GATHER ? node_bytes(L) : per_point, out_bytes = GATHER ? per_point : node_bytes(L);
    for (int b = 0; b < nb; ++b) {
        const std::string lane = "[" + std::to_string(b) + "]";
        MG_TRY(need_device_pointer(c, in[b], who, (in_name + lane).c_str()));
        MG_TRY(need_device_pointer(c, out[b], who, ("out" + lane).c_str()));
    }
    for (int b = 0; b < nb; ++b) {
        for (int q = 0; q < nb; ++q) {
            if (overlaps(out[b], out_bytes, in[q], in_bytes))
                return fail(w + ": out[" + std::to_string(b) + "] overlaps " + in_name + "[" + std::to_string(q) +
                            "]: every lane's output is memory of its own");
            if (q > b && overlaps(out[b], out_bytes, out[q], out_bytes))
                return fail(w + ": out[" + std::to_string(b) + "] overlaps out[" + std::to_string(q) + "]: every lane's output is memory of its own");
        }
    }
    if (!GATHER)
        for (int b = 0; b < nb; ++b) HIP_TRY(hipMemsetAsync(out[b], 0, out_bytes, c->stream));
    const int64_t threads = GATHER ? ps->M : ps->R;
    const dim3 grid(blocks_for(threads, PT_BLOCK)), blk(PT_BLOCK);
    for (int b0 = 0; b0 < nb; b0 += c->pt_group) {
        const int nv = std::min(c->pt_group, nb - b0);
        const bool known = with_int<1, 2, 3, 4, 5, 6, 7, 8>(nv, [&](auto n) {
            constexpr int NV = decltype(n)::value;
            PtSetArgs<NV> a{};
            a.pts = ps->pts; a.rec = ps->rec; a.run_start = ps->run_start; a.run_node = ps->run_node;
            a.M = ps->M; a.R = ps->R; a.nx = L.g.nx; a.plane = L.g.plane; a.N = L.N;
            for (int v = 0; v < NV; ++v) { a.in[v] = in[b0 + v]; a.out[v] = out[b0 + v]; }
            with_bool(GRAD, [&](auto g) {
                if (GATHER) hipLaunchKernelGGL((pt_set_gather<decltype(g)::value, NV>), grid, blk, 0, c->stream, a);
                else hipLaunchKernelGGL((pt_set_scatter<decltype(g)::value, NV>), grid, blk, 0, c->stream, a);
            });
        });
        if (!known) return fail(w + ": no kernel for a launch group of " + std::to_string(nv) + " lanes");
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int mg_points_sample(mg_handle c, mg_points_handle ps, int nb, const double* const* x_dev, double* const* out_dev) {
    return point_set_apply(c, ps, true, false, "mg_points_sample", "x", nb, x_dev, out_dev);
}

int mg_points_load(mg_handle c, mg_points_handle ps, int nb, const double* const* w_dev, double* const* out_dev) {
    return point_set_apply(c, ps, false, false, "mg_points_load", "w", nb, w_dev, out_dev);
}

int mg_points_gradient(mg_handle c, mg_points_handle ps, int nb, const double* const* x_dev, double* const* out_dev) {
    return point_set_apply(c, ps, true, true, "mg_points_gradient", "x", nb, x_dev, out_dev);
}

int mg_points_gradient_t(mg_handle c, mg_points_handle ps, int nb, const double* const* p_dev, double* const* out_dev) {
    return point_set_apply(c, ps, false, true, "mg_points_gradient_t", "p", nb, p_dev, out_dev);
}

int mg_zero_vector(mg_handle c, int level, int which) {
    MG_TRY(check_level(c, level));
    Level& L = c->L[level];
    DVector* v = pick(L, which);
    if (!v) return fail("unknown vector selector");
    MG_TRY(vec_alloc(c, L, v));
    return zero_vec(c, L, *v);
}

int mg_copy_vector(mg_handle c, int level, int dst_which, int src_which) {
    MG_TRY(check_level(c, level));
    Level& L = c->L[level];
    DVector* d = pick(L, dst_which);
    DVector* s = pick(L, src_which);
    if (!d || !s || !s->raw) return fail("bad vector selector");
    MG_TRY(vec_alloc(c, L, d));
    if (d->raw == s->raw) return 0;
    HIP_TRY(hipMemcpyAsync(d->base, s->base, (size_t)L.xlen * 8, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

int mg_smooth(mg_handle c, int level, int nw) {
    MG_TRY(need_matrix(c, level));
    if (nw < 0) return fail("nw must be >= 0");
    HIP_TRY(hipSetDevice(c->device));
    MG_TRY(exchange_halo(c, c->L[level], c->L[level].v));
    return smooth(c, level, nw);
}

int mg_smooth_split(mg_handle c, int level, int nw) {
    MG_TRY(need_matrix(c, level));
    if (nw < 0) return fail("nw must be >= 0");
    HIP_TRY(hipSetDevice(c->device));
    Level& L = c->L[level];
    if (is_slab(c, L)) return fail("mg_smooth_split is single-GPU only");
    if (!L.err.raw) return fail("MG_VEC_ERR must hold the diagonal of D^-1");
    const unsigned nb = (unsigned)std::min<int64_t>(2048, (L.nloc + 255) / 256);
    for (int s = 0; s < nw; ++s) {
        MG_TRY(launch_ell(c, L, level_op(L, MODE_SPMV)));
        hipLaunchKernelGGL(jacobi_split_combine, dim3(nb), dim3(256), 0, c->stream, L.v.rows, L.f.rows, L.err.rows,
                           L.v2.rows, L.v2.rows, L.nloc, c->omega);
        std::swap(L.v, L.v2);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int mg_residual(mg_handle c, int level) {
    MG_TRY(need_matrix(c, level));
    HIP_TRY(hipSetDevice(c->device));
    MG_TRY(exchange_halo(c, c->L[level], c->L[level].v));
    return residual(c, level);
}

int mg_restrict(mg_handle c, int level, int kind) {
    MG_TRY(check_level(c, level));
    if (level == 0) return fail("level 0 has no coarser level");
    MG_TRY(need_grid(c, level));
    MG_TRY(need_grid(c, level - 1));
    if (kind != MG_RESTRICT_INJECTION && kind != MG_RESTRICT_FULL_WEIGHTING && kind != MG_RESTRICT_TABLE &&
        kind != MG_RESTRICT_P1_TRANSPOSE)
        return fail("unknown restriction");
    HIP_TRY(hipSetDevice(c->device));
    return restrict_to(c, level, kind);
}

int mg_prolong(mg_handle c, int level, int add) {
    MG_TRY(check_level(c, level));
    if (level == 0) return fail("level 0 has no coarser level");
    MG_TRY(need_grid(c, level));
    MG_TRY(need_grid(c, level - 1));
    HIP_TRY(hipSetDevice(c->device));
    MG_TRY(exchange_halo(c, c->L[level - 1], c->L[level - 1].v));
    return prolong(c, level, add);
}

int mg_coarse_solve(mg_handle c, int* iterations, double* rel_residual) {
    MG_TRY(need_matrix(c, 0));
    HIP_TRY(hipSetDevice(c->device));
    return coarse_solve(c, iterations, rel_residual);
}

int mg_norm2(mg_handle c, int level, int which, double* out) {
    MG_TRY(check_level(c, level));
    if (!out) return fail("null output");
    HIP_TRY(hipSetDevice(c->device));
    Level& L = c->L[level];
    DVector* v = pick(L, which);
    if (!v || !v->raw) return fail("vector is not available on this level");
    return norm2(c, L, v->rows, out);
}

int mg_quadratic_form(mg_handle c, int level, int which, double* out) {
    MG_TRY(need_matrix(c, level));
    if (!out) return fail("null output");
    HIP_TRY(hipSetDevice(c->device));
    Level& L = c->L[level];
    DVector* v = pick(L, which);
    if (!v || !v->raw || v == &L.v2) return fail("vector is not available for a quadratic form");
    MG_TRY(exchange_halo(c, L, *v));
    const unsigned grid = L.mf ? mf_plan(c, L).grid : blocks_for(L.nslices, WAVES_PER_BLOCK);
    DevBuf<double> parts;
    MG_TRY(parts.alloc(c, grid));
    MG_TRY(launch_ell(c, L, {.mode = MODE_SPMV, .dot = true, .x_base = v->base, .out_rows = L.v2.rows, .partials = parts}));
    hipLaunchKernelGGL(reduce_partials, dim3(1), dim3(BLOCK), 0, c->stream, parts, (int)grid, c->scalars);
    if (!L.replicated) MG_TRY(allreduce_sum(c, c->scalars, 1));
    HIP_TRY(hipMemcpyAsync(c->h_scalars, c->scalars, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = c->h_scalars[0];
    return 0;
}

namespace {

__global__ void vec_diff(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out, int64_t n) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
        out[t] = a[t] - b[t];
}

// c->scalars[slot] = x^T M x with the handle's mass matrix (x: a vector of the mass matrix's level, halos valid)
int mass_form(mg_context* c, Level& L, DVector& x, int slot) {
    Level& M = c->mass;
    MG_TRY(vec_alloc(c, L, &c->mass_out));
    const unsigned nparts = blocks_for(M.nslices, WAVES_PER_BLOCK);
    if (nparts > 2 * kMaxParts) {
        // more partial sums than the handle's scratch holds: a buffer of its own for this call
        DevBuf<double> parts;
        MG_TRY(parts.alloc(c, nparts));
        unsigned grid = 0;
        MG_TRY(launch_ell(c, M, {.mode = MODE_SPMV, .dot = true, .x_base = x.base, .out_rows = c->mass_out.rows, .partials = parts, .grid_out = &grid}));
        hipLaunchKernelGGL(reduce_partials, dim3(1), dim3(BLOCK), 0, c->stream, parts, (int)grid, c->scalars + slot);
        if (hipStreamSynchronize(c->stream) != hipSuccess) return fail("mass_form: stream error");
    } else {
        unsigned grid = 0;
        MG_TRY(launch_ell(c, M, {.mode = MODE_SPMV, .dot = true, .x_base = x.base, .out_rows = c->mass_out.rows, .partials = c->partials,
                                 .grid_out = &grid}));
        hipLaunchKernelGGL(reduce_partials, dim3(1), dim3(BLOCK), 0, c->stream, c->partials, (int)grid, c->scalars + slot);
    }
    HIP_TRY(hipGetLastError());
    if (!L.replicated) MG_TRY(allreduce_sum(c, c->scalars + slot, 1));
    return 0;
}

// after a cycle on the top level: residual norm (and error norm) of the iterate in the chosen norm, one small
// device -> host copy for both
int fmg_norms(mg_context* c, int l, int norm, bool want_err, double* rn, double* en) {
    Level& L = c->L[l];
    MG_TRY(residual(c, l));
    if (norm == MG_NORM_MASS) {
        MG_TRY(exchange_halo(c, L, L.v2));
        MG_TRY(mass_form(c, L, L.v2, 0));
    } else {
        MG_TRY(dot_device(c, L, L.v2.rows, L.v2.rows, 0));
    }
    if (want_err) {
        MG_TRY(vec_alloc(c, L, &c->diff));
        const unsigned nb = (unsigned)std::min<int64_t>(4096, (L.nloc + 255) / 256);
        hipLaunchKernelGGL(vec_diff, dim3(nb), dim3(256), 0, c->stream, L.v.rows, c->uexact.rows, c->diff.rows, L.nloc);
        HIP_TRY(hipGetLastError());
        if (norm == MG_NORM_MASS) {
            MG_TRY(exchange_halo(c, L, c->diff));
            MG_TRY(mass_form(c, L, c->diff, 1));
        } else {
            MG_TRY(dot_device(c, L, c->diff.rows, c->diff.rows, 1));
        }
    }
    HIP_TRY(hipMemcpyAsync(c->h_scalars, c->scalars, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *rn = std::sqrt(std::max(0.0, c->h_scalars[0]));
    if (want_err) *en = std::sqrt(std::max(0.0, c->h_scalars[1]));
    return 0;
}

}  // namespace

int mg_set_mass_csr(mg_handle c, int level, int64_t n_rows, int64_t nnz, const void* indptr, int indptr_is_64,
                    const int32_t* indices, const double* data) {
    MG_TRY(check_level(c, level));
    MG_TRY(need_grid(c, level));
    if (!indptr || !indices || !data) return fail("null CSR arrays");
    if (n_rows <= 0 || nnz < 0) return fail("bad matrix dimensions");
    MG_TRY(check_csr(n_rows, n_rows, nnz, indptr, indptr_is_64, indices, false));
    HIP_TRY(hipSetDevice(c->device));
    Level& L = c->L[level];
    if (n_rows != L.n_global) return fail("mass matrix has " + std::to_string(n_rows) + " rows, level has " + std::to_string(L.n_global));
    Level& M = c->mass;
    vec_free(&c->mass_out);             // (sized for the level the previous mass matrix belonged to)
    LevelBuild build(c, M);
    c->mass_level = -1;
    MG_TRY(setup_geometry(c, M, level, L.N));
    if (L.perm) {                       // the level's DoF numbering
        MG_TRY(M.perm.alloc(c, (size_t)L.n_global));
        if (hipMemcpy(M.perm, L.perm, (size_t)L.n_global * sizeof(int), hipMemcpyDeviceToDevice) != hipSuccess)
            return fail("copy of the level's permutation failed");
    }
    // (level index 1: any level but the coarsest may use symmetric diagonal storage)
    MG_TRY(build_level_from_csr(c, 1, M, n_rows, nnz, indptr, indptr_is_64, indices, data, nullptr, 1, false));
    c->mass_level = level;
    return build.done();
}

int mg_set_exact(mg_handle c, int level, const double* host) {
    MG_TRY(check_level(c, level));
    if (!host) return fail("null host vector");
    HIP_TRY(hipSetDevice(c->device));
    Level& L = c->L[level];
    if (c->uexact_level != level) { vec_free(&c->uexact); vec_free(&c->diff); }
    MG_TRY(vec_alloc(c, L, &c->uexact));
    c->uexact_level = level;
    return upload_vector(c, L, c->uexact, host);
}

int mg_counters(mg_handle c, int64_t* uploads, int64_t* downloads, int64_t* graph_replays, int* graphs_cached) {
    if (!c) return fail("null handle");
    if (uploads) *uploads = c->uploads;
    if (downloads) *downloads = c->downloads;
    if (graph_replays) *graph_replays = c->graph_replays;
    if (graphs_cached) *graphs_cached = (int)c->graphs.size();
    return 0;
}

int mg_smoother_launches(mg_handle c, int level, int path, int64_t* launches, int64_t* sweeps, int64_t* tail_launches) {
    MG_TRY(check_level(c, level, false));
    if (path < 0 || path >= MG_PATH_COUNT) return fail("smoother path " + std::to_string(path) + " out of range");
    const auto& n = c->smoother_counts[(size_t)level][(size_t)path];
    if (launches) *launches = n.launches;
    if (sweeps) *sweeps = n.sweeps;
    if (tail_launches) *tail_launches = n.tail;
    return 0;
}

int mg_march_plan(mg_handle c, int level, int sweeps, int64_t* waves, int64_t* planes, int64_t* const_waves, int64_t* const_planes) {
    MG_TRY(check_level(c, level));
    const Level& L = c->L[level];
    int64_t* const out[4] = {waves, planes, const_waves, const_planes};
    for (int64_t* o : out)
        if (o) *o = 0;
    const int slot = march_plan_slot(c, L, sweeps);
    if (slot < 0 || !L.plan[slot].iv) return 0;
    const Level::MarchPlan& mp = L.plan[slot];
    if (waves) *waves = mp.waves[0];
    if (planes) *planes = mp.planes[0];
    if (const_waves) *const_waves = mp.waves[1];
    if (const_planes) *const_planes = mp.planes[1];
    return 0;
}

int mg_reset_smoother_launches(mg_handle c) {
    if (!c) return fail("null handle");
    for (auto& level : c->smoother_counts) level.fill({});
    return 0;
}

int mg_prepare_cycle(mg_handle c, int level) {
    MG_TRY(check_level(c, level));
    for (int l = 0; l <= level; ++l) {
        MG_TRY(need_matrix(c, l));
        if (level > 0) MG_TRY(need_grid(c, l));
    }
    HIP_TRY(hipSetDevice(c->device));
    MG_TRY(prepare_cycle(c, level));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int mg_vcycle(mg_handle c, int level, int ncycles, double* resid_l2) {
    MG_TRY(check_level(c, level));
    for (int l = 0; l <= level; ++l) {
        MG_TRY(need_matrix(c, l));
        if (level > 0) MG_TRY(need_grid(c, l));
    }
    MG_TRY(face_set_refusals(c, level));
    HIP_TRY(hipSetDevice(c->device));
    Level& L = c->L[level];
    MG_TRY(exchange_halo(c, L, L.v));
    for (int k = 0; k < ncycles; ++k) {
        MG_TRY(vcycle_graphed(c, level));
        if (resid_l2) {
            MG_TRY(residual(c, level));
            MG_TRY(norm2(c, L, L.v2.rows, &resid_l2[k]));
        }
    }
    return 0;
}

int mg_fmg_ex(mg_handle c, int top, int mu0, double tol, int max_cycles, int norm, double* resid_hist, double* err_hist,
              int* cycles_done) {
    MG_TRY(check_level(c, top));
    for (int l = 0; l <= top; ++l) {
        MG_TRY(need_matrix(c, l));
        if (top > 0) MG_TRY(need_grid(c, l));
    }
    if (norm != MG_NORM_L2 && norm != MG_NORM_MASS) return fail("unknown norm");
    if (norm == MG_NORM_MASS && c->mass_level != top) return fail("mg_fmg_ex: no mass matrix on the top level (mg_set_mass_csr)");
    if (err_hist && (!c->uexact.raw || c->uexact_level != top)) return fail("mg_fmg_ex: no exact solution on the top level (mg_set_exact)");
    MG_TRY(face_set_refusals(c, top));
    MG_TRY(singular_refusal(c, "mg_fmg", top));
    HIP_TRY(hipSetDevice(c->device));
    for (int l = 0; l < top; ++l) {
        Level& L = c->L[l];
        if (!L.ftrue.raw) return fail("mg_fmg needs the true right-hand side of level " + std::to_string(l));
        HIP_TRY(hipMemcpyAsync(L.f.base, L.ftrue.base, (size_t)L.xlen * 8, hipMemcpyDeviceToDevice, c->stream));
    }
    MG_TRY(coarse_solve(c, nullptr, nullptr));
    int done_cycles = 0;
    const bool norms = resid_hist != nullptr || err_hist != nullptr;
    for (int l = 1; l <= top; ++l) {
        Level& L = c->L[l];
        if (l < top)   // cycles on level l-1 consumed F[l-1..0]; F[l] is still the true right-hand side
            HIP_TRY(hipMemcpyAsync(L.f.base, L.ftrue.base, (size_t)L.xlen * 8, hipMemcpyDeviceToDevice, c->stream));
        // v_h = Interpolation(v_2h) (multigrid.py:283-284): interpolate into ERR, then copy to V
        MG_TRY(exchange_halo(c, c->L[l - 1], c->L[l - 1].v));
        MG_TRY(prolong(c, l, 0));
        HIP_TRY(hipMemcpyAsync(L.v.base, L.err.base, (size_t)L.xlen * 8, hipMemcpyDeviceToDevice, c->stream));
        MG_TRY(exchange_halo(c, L, L.v));
        const bool until_tol = l == top && tol > 0.0;
        const int ncyc = until_tol ? max_cycles : mu0;
        for (int k = 0; k < ncyc; ++k) {
            MG_TRY(vcycle_graphed(c, l));
            if (l < top) continue;
            ++done_cycles;
            if (!until_tol && !norms) continue;
            // residual (and error) of this cycle's iterate in the caller's norm (multigrid.py:291-295)
            double rn = 0.0, en = 0.0;
            MG_TRY(fmg_norms(c, l, norm, err_hist != nullptr, &rn, &en));
            if (resid_hist) resid_hist[k] = rn;
            if (err_hist) err_hist[k] = en;
            if (until_tol && rn <= tol) break;
        }
    }
    if (cycles_done) *cycles_done = done_cycles;
    return 0;
}

int mg_fmg(mg_handle c, int top, int mu0, double tol, int max_cycles, double* resid_l2, int* cycles_done) {
    return mg_fmg_ex(c, top, mu0, tol, max_cycles, MG_NORM_L2, resid_l2, nullptr, cycles_done);
}

int mg_pcg(mg_handle c, int level, double rtol, int max_iter, double* resid_hist, int* iterations) {
    MG_TRY(check_level(c, level));
    if (c->L[level].flat)
        return fail("mg_pcg: level " + std::to_string(level) + " is flat (no grid): there is no V-cycle to precondition with");
    if (level < 1) return fail("mg_pcg: level 0 is the coarsest level: the V-cycle preconditioner needs level >= 1");
    if (max_iter < 0) return fail("mg_pcg: max_iter must not be negative");
    for (int l = 0; l <= level; ++l) {
        MG_TRY(need_matrix(c, l));
        MG_TRY(need_grid(c, l));
    }
    MG_TRY(face_set_refusals(c, level));
    HIP_TRY(hipSetDevice(c->device));
    return fcg_solve(c, level, rtol, max_iter, resid_hist, iterations);
}

int mg_pcg_batch(mg_handle c, int level, int nb, const double* const* f_dev, double* const* x_dev, double rtol, int max_iter,
                 double* resid_hist, int* iterations) {
    const std::string who = "mg_pcg_batch";
    MG_TRY(batch_refusals(c, who, level, nb, f_dev, nullptr, x_dev, "f_dev", nullptr, "x_dev"));
    if (level < 1) return fail(who + ": level 0 is the coarsest level: the V-cycle preconditioner needs level >= 1");
    if (max_iter < 0) return fail(who + ": max_iter must not be negative");
    for (int l = 0; l <= level; ++l) {
        MG_TRY(need_matrix(c, l));
        MG_TRY(need_grid(c, l));
        if (c->L[l].mf && l >= 1 && (c->smoother == MG_SMOOTH_RBGS || c->smoother == MG_SMOOTH_MCGS))
            return fail(who + ": level " + std::to_string(l) + " is a matrix-free diffusion level: Gauss-Seidel smoothers (RBGS, MCGS) "
                        "need stored rows; use Jacobi or Chebyshev");
    }
    MG_TRY(face_set_refusals(c, level));
    MG_TRY(singular_refusal(c, who, level));
    // what mg_pcg refuses only where the cycle is prepared (the P1 stencil check, the colouring, the factorisation, the Chebyshev
    // interval) is refused here, with the handle's own vectors in place, before a lane is allocated or a vector overwritten
    MG_TRY(prepare_cycle(c, level));
    MG_TRY(ensure_lanes(c, nb, 0, level));
    Level& L = c->L[level];
    std::vector<int> all((size_t)nb);
    for (int b = 0; b < nb; ++b) all[(size_t)b] = b;
    BatchScope s(c, 0, level, nb);
    MG_TRY(s.each(all, [&](int b) -> int {
        MG_TRY(scatter_to(c, L, L.f, f_dev[b]));
        return scatter_to(c, L, L.v, x_dev[b]);
    }));
    MG_TRY(fcg_solve_batch(c, s, level, nb, rtol, max_iter, resid_hist, std::max(1, max_iter), iterations));
    MG_TRY(s.each(all, [&](int b) { return gather_from(c, L, L.v, x_dev[b]); }));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int mg_apply_batch(mg_handle c, int level, int op, int nb, const double* const* x_dev, const double* const* f_dev,
                   double* const* out_dev, double* dots) {
    const std::string who = "mg_apply_batch";
    if (op != MG_BATCH_JACOBI && op != MG_BATCH_RESIDUAL && op != MG_BATCH_SPMV) return fail(who + ": unknown operation " + std::to_string(op));
    const bool spmv = op == MG_BATCH_SPMV;
    MG_TRY(batch_refusals(c, who, level, nb, x_dev, spmv ? nullptr : f_dev, out_dev, "x_dev", spmv ? nullptr : "f_dev", "out_dev"));
    MG_TRY(need_matrix(c, level));
    if (dots && !spmv) return fail(who + ": dots are the SpMV's (x . A x)");
    if (op == MG_BATCH_JACOBI && c->smoother != MG_SMOOTH_JACOBI)
        return fail(who + ": MG_BATCH_JACOBI is a sweep of the Jacobi smoother; the handle's smoother is another one (mg_set_params)");
    MG_TRY(ensure_lanes(c, nb, level, level));       // (one level's operation: only that level's vectors)
    Level& L = c->L[level];
    std::vector<int> all((size_t)nb);
    for (int b = 0; b < nb; ++b) all[(size_t)b] = b;
    BatchScope s(c, level, level, nb);
    MG_TRY(s.each(all, [&](int b) -> int {
        if (!spmv) MG_TRY(scatter_to(c, L, L.f, f_dev[b]));
        return scatter_to(c, L, L.v, x_dev[b]);
    }));
    if (op == MG_BATCH_JACOBI) {
        MG_TRY(smooth_batch(c, s, level, 1, all));
        MG_TRY(s.each(all, [&](int b) { return gather_from(c, L, L.v, out_dev[b]); }));
    } else if (op == MG_BATCH_RESIDUAL) {
        MG_TRY(residual_batch(c, s, level, all));
        MG_TRY(s.each(all, [&](int b) { return gather_from(c, L, L.v2, out_dev[b]); }));
    } else {
        // out = A x into R; with dots the partial sums of x . A x, summed as mg_quadratic_form sums them
        const unsigned grid = L.mf ? mf_plan(c, L).grid : blocks_for(L.nslices, WAVES_PER_BLOCK);
        std::vector<DevBuf<double>> parts(dots ? (size_t)nb : 0);
        for (auto& p : parts) MG_TRY(p.alloc(c, grid));
        auto one = [&](int b) {
            return launch_ell(c, L, {.mode = MODE_SPMV, .dot = dots != nullptr, .x_base = L.v.base, .out_rows = L.v2.rows,
                                     .partials = dots ? parts[(size_t)b].get() : nullptr});
        };
        if (mf_fused(c, L, all.size())) {
            MG_TRY(mf_groups(c, s, L, MODE_SPMV, dots != nullptr, all,
                [&](int b, const double** x, const double**, double** out, double** pp) {
                    LaneLevel& v = s.at(b, level);
                    *x = v.v.base + L.g.lead; *out = v.v2.rows; *pp = dots ? parts[(size_t)b].get() : nullptr;
                },
                one, [](int, int) {}));
        } else {
            MG_TRY(s.each(all, one));
        }
        MG_TRY(s.each(all, [&](int b) -> int {
            MG_TRY(gather_from(c, L, L.v2, out_dev[b]));
            if (!dots) return 0;
            hipLaunchKernelGGL(reduce_partials, dim3(1), dim3(BLOCK), 0, c->stream, parts[(size_t)b].get(), (int)grid, c->scalars.get());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(c->h_scalars, c->scalars, sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            dots[b] = c->h_scalars[0];
            return 0;
        }));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int mg_batch_info(mg_handle c, int* lanes, int64_t* bytes) {
    if (!c) return fail("null handle");
    int64_t n = 0;
    for (const Lane& lane : c->lanes) n += lane_bytes(lane);
    if (lanes) *lanes = (int)c->lanes.size();
    if (bytes) *bytes = n;
    return 0;
}

int mg_release_batch(mg_handle c) {
    if (!c) return fail("null handle");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->lanes.clear();
    c->eigs = EigsWork{};
    return 0;
}

int mg_eigs(mg_handle c, int level, int k, int block, const double* rho_dev, double* const* x_dev, int warm, double rtol, int max_iter,
            double* lambda, double* resid, int* iterations, int* restarts) {
    const std::string who = "mg_eigs";
    if (!c) return fail("null handle");
    if (block < 1 || block > MG_EIGS_MAX)
        return fail(who + ": block = " + std::to_string(block) + " is outside 1.." + std::to_string(MG_EIGS_MAX) + " (MG_EIGS_MAX)");
    if (k < 1 || k > block) return fail(who + ": k = " + std::to_string(k) + " is outside 1..block = " + std::to_string(block));
    if (!(rtol > 0.0) && max_iter <= 0) return fail(who + ": rtol <= 0 and max_iter <= 0: nothing would stop the iteration");
    if (!lambda || !resid) return fail(who + ": null pointer (lambda, resid)");
    MG_TRY(batch_refusals(c, who, level, block, nullptr, nullptr, x_dev, nullptr, nullptr, "x_dev"));
    if (level < 1) return fail(who + ": level 0 is the coarsest level: the V-cycle preconditioner needs level >= 1");
    for (int l = 0; l <= level; ++l) {
        MG_TRY(need_matrix(c, l));
        MG_TRY(need_grid(c, l));
        if (c->L[l].mf && l >= 1 && (c->smoother == MG_SMOOTH_RBGS || c->smoother == MG_SMOOTH_MCGS))
            return fail(who + ": level " + std::to_string(l) + " is a matrix-free diffusion level: Gauss-Seidel smoothers (RBGS, MCGS) "
                        "need stored rows; use Jacobi or Chebyshev");
    }
    MG_TRY(face_set_refusals(c, level));
    MG_TRY(singular_refusal(c, who, level));
    const Level& L = c->L[level];
    const int64_t n1 = (int64_t)L.N + 1;
    if (L.N < 1 || L.n_global != n1 * n1 * n1 || L.g.lead != 0 || L.xlen != L.nloc)
        return fail(who + ": level " + std::to_string(level) + " is no whole grid of (N + 1)^3 nodes");
    if (rho_dev) {
        MG_TRY(need_device_pointer(c, rho_dev, who.c_str(), "rho_dev"));
        MG_TRY(check_rho(c, who, rho_dev, (int64_t)L.N * L.N * L.N, L.N));
    }
    MG_TRY(prepare_cycle(c, level));
    MG_TRY(ensure_lanes(c, block, 0, level));
    MG_TRY(ensure_eigs(c, level, block));
    BatchScope s(c, 0, level, block);
    return eigs_solve(c, s, level, k, block, rho_dev, x_dev, warm, rtol, max_iter, lambda, resid, iterations, restarts);
}

int mg_block_gram(mg_handle c, int level, int na, const double* const* a_dev, int nb, const double* const* b_dev, const double* d_dev,
                  double* out) {
    const std::string who = "mg_block_gram";
    MG_TRY(block_level_refusals(c, who, level));
    if (na < 1 || na > BC_MAX_IN || nb < 1 || nb > BC_MAX_IN)
        return fail(who + ": na = " + std::to_string(na) + ", nb = " + std::to_string(nb) + ": both must be in 1.." + std::to_string(BC_MAX_IN));
    if (!out) return fail(who + ": null pointer (out)");
    HIP_TRY(hipSetDevice(c->device));
    MG_TRY(block_pointer_refusals(c, who, na, a_dev, "a_dev"));
    MG_TRY(block_pointer_refusals(c, who, nb, b_dev, "b_dev"));
    if (d_dev) MG_TRY(block_pointer_refusals(c, who, 1, &d_dev, "d_dev"));
    const Level& L = c->L[level];
    bool sym = na == nb;
    for (int i = 0; sym && i < na; ++i) sym = a_dev[i] == b_dev[i];
    // (scratch of this call: freed on return, mg_memory_bytes is as before)
    EigsWork scratch;
    MG_TRY(ensure_block_scratch(c, L, scratch));
    GramBatch gb;
    MG_TRY(gram_enqueue(c, L, scratch, gb, out, nb, 0, 0, na, a_dev, nb, b_dev, d_dev, sym, false));
    return gram_collect(c, scratch, gb);
}

int mg_block_combine(mg_handle c, int level, int ns, const double* const* s_dev, int no, const double* coeff, double* const* out_dev) {
    const std::string who = "mg_block_combine";
    MG_TRY(block_level_refusals(c, who, level));
    if (ns < 1 || ns > BC_MAX_IN) return fail(who + ": ns = " + std::to_string(ns) + " is outside 1.." + std::to_string(BC_MAX_IN));
    if (no < 1 || no > BC_MAX_OUT) return fail(who + ": no = " + std::to_string(no) + " is outside 1.." + std::to_string(BC_MAX_OUT));
    if (!coeff) return fail(who + ": null pointer (coeff)");
    HIP_TRY(hipSetDevice(c->device));
    MG_TRY(block_pointer_refusals(c, who, ns, s_dev, "s_dev"));
    MG_TRY(block_pointer_refusals(c, who, no, out_dev, "out_dev"));
    const Level& L = c->L[level];
    const size_t len = (size_t)L.n_global * sizeof(double);
    for (int o = 0; o < no; ++o) {
        for (int q = 0; q < o; ++q)
            if (overlaps(out_dev[o], len, out_dev[q], len))
                return fail(who + ": out_dev[" + std::to_string(o) + "] overlaps out_dev[" + std::to_string(q) + "]");
        for (int i = 0; i < ns; ++i)
            if (out_dev[o] != s_dev[i] && overlaps(out_dev[o], len, s_dev[i], len))
                return fail(who + ": out_dev[" + std::to_string(o) + "] overlaps s_dev[" + std::to_string(i) + "] without being it: an output "
                            "may be one of the inputs, nothing in between");
    }
    MG_TRY(launch_block_combine(c, L, ns, s_dev, no, coeff, out_dev));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int mg_eigs_info(mg_handle c, int* block, int64_t* bytes) {
    if (!c) return fail("null handle");
    if (block) *block = c->eigs.block;
    if (bytes) *bytes = c->eigs.bytes();
    return 0;
}

int mg_release_eigs(mg_handle c) {
    if (!c) return fail("null handle");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->eigs = EigsWork{};
    return 0;
}

int mg_time_kernel(mg_handle c, const char* kernel, int level, int reps, double* avg_ms) {
    MG_TRY(need_matrix(c, level));
    if (!kernel || !avg_ms || reps < 1) return fail("bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    const std::string k(kernel);
    Level& L = c->L[level];
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    HIP_TRY(hipEventCreate(&ev.e0));
    HIP_TRY(hipEventCreate(&ev.e1));
    const hipEvent_t e0 = ev.e0, e1 = ev.e1;
    DevTemp ki_src, ki_coarse;      // "kappa_ingest": a copy of the level's kappa to read, a coarse field to write
    // "diffusion_mf[:jacobi|:residual|:spmv|:chebyshev]": the matrix-free march in one mode, i.e. that kernel on a matrix-free level
    // (timed as the operation `op` of that name, on a level that must be matrix-free)
    // "diffusion_mf_batch<NV>:jacobi|residual|spmv": one fused launch of the march over NV vectors -- V, F, R and scratch copies
    // of them for the other vectors (uncounted, freed on return)
    if (k.rfind("diffusion_mf_batch", 0) == 0) {
        if (!L.mf) return fail("level is not a matrix-free diffusion level");
        const int nv = k.size() > 18 ? k[18] - '0' : 0;
        const std::string mode = k.size() > 19 ? k.substr(19) : "";
        const int m = mode == ":jacobi" ? MODE_JACOBI : mode == ":residual" ? MODE_RESIDUAL : mode == ":spmv" ? MODE_SPMV : -1;
        if (nv < 2 || nv > MF_BATCH_MAX || m < 0) return fail("unknown kernel " + k);
        DevTemp scratch[3 * MF_BATCH_MAX];
        const double *x[MF_BATCH_MAX] = {L.v.rows}, *f[MF_BATCH_MAX] = {L.f.rows};
        double* out[MF_BATCH_MAX] = {L.v2.rows};
        const size_t total = (size_t)vec_total(L) * sizeof(double), off = (size_t)(vec_front(L) + L.g.lead);
        const DVector* src[3] = {&L.v, &L.f, &L.v2};
        for (int v = 1; v < nv; ++v) {
            double* p[3];
            for (int q = 0; q < 3; ++q) {
                MG_TRY(scratch[3 * v + q].alloc(total));
                HIP_TRY(hipMemcpyAsync(scratch[3 * v + q].p, src[q]->raw, total, hipMemcpyDeviceToDevice, c->stream));
                p[q] = scratch[3 * v + q].as<double>() + off;
            }
            x[v] = p[0]; f[v] = p[1]; out[v] = p[2];
        }
        MG_TRY(launch_diffusion_mf_batch(c, L, m, false, nv, x, f, out, nullptr));      // warm-up
        HIP_TRY(hipEventRecord(e0, c->stream));
        for (int r = 0; r < reps; ++r) MG_TRY(launch_diffusion_mf_batch(c, L, m, false, nv, x, f, out, nullptr));
        HIP_TRY(hipEventRecord(e1, c->stream));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        *avg_ms = (double)ms / reps;
        return 0;
    }
    // the cell gradient family (mg_diffusion_flux.hip.h) with w = F[:N^3], x = V and p = (V, F, V)[:N^3] per component in a scratch
    // of 3 N^3 (uncounted, freed on return): "cell_grad" = F(w, x), "cell_grad_nw" = F(null, x), into a scratch whose first entries
    // (as many as R holds) are copied to R after the timed region; "cell_grad_dot" = C(p, x) into R[:N^3]; "cell_grad_t" =
    // F^T(w, p) into R
    if (k.rfind("cell_grad", 0) == 0) {
        MG_TRY(need_cell_grad_level(c, level, "mg_time_kernel"));
        const bool f_form = k == "cell_grad" || k == "cell_grad_nw", c_form = k == "cell_grad_dot", t_form = k == "cell_grad_t";
        if (!(f_form || c_form || t_form)) return fail("unknown kernel " + k);
        MG_TRY(vec_alloc(c, L, &L.v)); MG_TRY(vec_alloc(c, L, &L.f)); MG_TRY(vec_alloc(c, L, &L.v2));
        const size_t cells = (size_t)L.N * L.N * L.N;
        DevTemp three;
        MG_TRY(three.alloc(3 * cells * sizeof(double)));
        double* t3 = three.as<double>();
        const double* w = k == "cell_grad_nw" ? nullptr : L.f.rows;
        if (!f_form) {
            const double* src[3] = {L.v.rows, L.f.rows, L.v.rows};
            for (int d = 0; d < 3; ++d)
                HIP_TRY(hipMemcpyAsync(t3 + d * cells, src[d], cells * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        }
        auto run = [&]() -> int {
            if (f_form) return launch_cell_grad<CG_F>(c, L, w, nullptr, L.v.rows, t3);
            if (c_form) return launch_cell_grad<CG_C>(c, L, nullptr, t3, L.v.rows, L.v2.rows);
            return launch_cell_grad_t(c, L, w, t3, L.v2.rows);
        };
        MG_TRY(run());      // warm-up
        HIP_TRY(hipEventRecord(e0, c->stream));
        for (int r = 0; r < reps; ++r) MG_TRY(run());
        HIP_TRY(hipEventRecord(e1, c->stream));
        if (f_form)
            HIP_TRY(hipMemcpyAsync(L.v2.rows, t3, std::min((size_t)L.n_global, 3 * cells) * sizeof(double), hipMemcpyDeviceToDevice,
                                   c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        *avg_ms = (double)ms / reps;
        return 0;
    }
    const bool mf_key = k.rfind("diffusion_mf", 0) == 0;
    const std::string mf_mode = !mf_key ? "" : k.size() > 12 ? k.substr(12) : ":jacobi";
    const std::string op = !mf_key ? k : mf_mode[0] == ':' ? mf_mode.substr(1) : "";
    // one step with x_{k-1} (the scalars of step 1 of a degree-2 polynomial on the level's interval)
    auto cheb_step = [&]() -> int {
        double lo = 0.0, hi = 0.0, al[2], be[2];
        MG_TRY(cheb_interval(c, level, &lo, &hi));
        cheb_steps(lo, hi, 2, al, be);
        EllRequest step = level_op(L, MODE_CHEB);
        step.alpha = al[1]; step.beta = be[1];
        return launch_ell(c, L, step);
    };
    auto once = [&]() -> int {
        if (mf_key && !L.mf) return fail("level is not a matrix-free diffusion level");
        if (op == "jacobi") return launch_ell(c, L, level_op(L, MODE_JACOBI));
        if (op == "chebyshev") return cheb_step();
        if (op == "spmv") return launch_ell(c, L, level_op(L, MODE_SPMV));
        if (op == "residual") return residual(c, level);
        if (mf_key) return fail("unknown mode of diffusion_mf: " + mf_mode);
        // "jacobi2": only where mg_smooth itself pairs sweeps on this level; "jacobi2!": wherever the kernel applies
        if (k == "jacobi2" || k == "jacobi2!") {
            if (!fused_sweeps_ok(c, L, k == "jacobi2!")) return fail("level does not use the two-sweep kernel");
            const J2Plan plan = jacobi2_plan(c, L, false, 0);
            return launch_jacobi2(c, L, plan, 0, 1, plan.nseg, L.v.rows, L.f.rows, L.v2.rows);
        }
        if (k.rfind("jacobik3", 0) == 0) {     // K = fuse_k sweeps per pass on a whole class-coded 3-D level ("!": wherever it applies)
            const bool forced = k.find(":form") != std::string::npos;
            if (!sweepsk_ok(c, L, forced || k.find('!') != std::string::npos)) return fail("level does not use the K-sweep pass");
            c->timing_force_form = forced ? k.back() - '0' : -1;
            const bool slab = is_slab(c, L);
            if (slab && L.cls_halo != 1) return fail("the slab's class halos are not built yet (first smoother call)");
            const int rc = launch_jacobikc(c, L, slab ? std::min(std::min(c->fuse_k, 5), L.hd) : sweepsk_max(c, L), L.v.rows, L.f.rows, L.v2.rows);
            c->timing_force_form = -1;
            return rc;
        }
        if (k == "jacobiblk" || k == "jacobiblk!") {      // K sweeps per launch on resident blocks ("!": whatever the level's size)
            const int keep = c->fuse_block;
            if (k.back() == '!') c->fuse_block = 2;
            const bool ok = block_sweeps_ok(c, L);
            c->fuse_block = keep;
            if (!ok) return fail("level does not use the block pass");
            const JBPlan plan = block_plan(c, L);
            return launch_jacobi_block(c, L, plan.K, plan.EZ, L.v.rows, L.f.rows, L.v2.rows);
        }
        if (k == "jacobi_small") {           // all mu1 sweeps of a small level in one launch
            if (!small_level_ok(c, L) || c->mu1 < 2) return fail("level does not use the one-launch smoother");
            return launch_jacobi_small(c, L, c->mu1, L.v.rows, L.f.rows, L.v2.rows);
        }
        if (k == "lattice") {              // one Jacobi launch of the lattice plane march, an error where the level does not use it
            if (!(L.coded && L.scls && c->class_sweeps && lat_march_ok(c, L))) return fail("level does not use the lattice march");
            return launch_lat_march(c, L, MODE_JACOBI, L.v.rows, L.f.rows, L.v2.rows, 0, 0.0, 0.0);
        }
        if (k == "jacobik") {
            if (!sweeps2d_ok(c, L)) return fail("level does not use the K-sweep 2-D kernel");
            return launch_jacobik(c, L, c->fuse_2d_k, L.v.rows, L.f.rows, L.v2.rows);
        }
        if (k == "gs") {            // one full Gauss-Seidel sweep (all colours) with the configured colouring
            if (c->smoother == MG_SMOOTH_JACOBI) return fail("the configured smoother is Jacobi");
            return smooth(c, level, 1);
        }
        // d(v^T A f) / d kappa: the plane march / one thread per cell, into MG_VEC_R (":all": both vectors with their boundary entries)
        if (k == "dkappa" || k == "dkappa_gather" || k == "dkappa:all") {
            MG_TRY(need_dkappa_level(c, level, "mg_time_kernel"));
            MG_TRY(vec_alloc(c, L, &L.v)); MG_TRY(vec_alloc(c, L, &L.f)); MG_TRY(vec_alloc(c, L, &L.v2));
            const bool all = k == "dkappa:all";
            return launch_dkappa(c, L, L.v.rows, L.f.rows, L.v2.rows, k == "dkappa_gather", all, all);
        }
        // (dA/dkappa . f[:N^3]) v: the SpMV march with kappa := the direction, into MG_VEC_R (":all": every row and column of A^)
        if (k == "apply_dkappa" || k == "apply_dkappa:all") {
            MG_TRY(need_dkappa_level(c, level, "mg_time_kernel"));
            MG_TRY(vec_alloc(c, L, &L.v)); MG_TRY(vec_alloc(c, L, &L.f)); MG_TRY(vec_alloc(c, L, &L.v2));
            const bool all = k == "apply_dkappa:all";
            return launch_apply_dkappa(c, L, L.f.rows, L.v.rows, L.v2.rows, all, all);
        }
        // the sigma sensitivities: D_sigma(v, f) into MG_VEC_R[:N^3] / T_sigma(f[:N^3], v) into MG_VEC_R
        if (k == "dsigma" || k == "apply_dsigma") {
            MG_TRY(need_dkappa_level(c, level, "mg_time_kernel", "sigma"));
            MG_TRY(vec_alloc(c, L, &L.v)); MG_TRY(vec_alloc(c, L, &L.f)); MG_TRY(vec_alloc(c, L, &L.v2));
            return k == "dsigma" ? launch_dsigma(c, L, L.v.rows, L.f.rows, L.v2.rows) : launch_apply_dsigma(c, L, L.f.rows, L.v.rows, L.v2.rows);
        }
        // the Robin sensitivities of face z+: D(v, f) into MG_VEC_R[:N^2] / T(f[:N^2], v) into MG_VEC_R
        if (k == "drobin" || k == "apply_drobin") {
            MG_TRY(need_dkappa_level(c, level, "mg_time_kernel", "Robin"));
            int fi = -1;
            MG_TRY(need_drobin_face(c, "mg_time_kernel", MG_FACE_ZHI, &fi));
            MG_TRY(vec_alloc(c, L, &L.v)); MG_TRY(vec_alloc(c, L, &L.f)); MG_TRY(vec_alloc(c, L, &L.v2));
            return k == "drobin" ? launch_drobin(c, L, fi, L.v.rows, L.f.rows, L.v2.rows) : launch_apply_drobin(c, L, fi, L.f.rows, L.v.rows, L.v2.rows);
        }
        if (k == "kappa_ingest") {  // the copy and the coarsening in one pass, from a scratch copy of kappa back into the level's own
            if (!L.mf) return fail("level is not a matrix-free diffusion level");
            if (!ki_src.p) {
                MG_TRY(ki_src.alloc(L.kappa.count() * 8));
                MG_TRY(ki_coarse.alloc((L.kappa.count() / 8) * 8));
                HIP_TRY(hipMemcpyAsync(ki_src.p, L.kappa, L.kappa.count() * 8, hipMemcpyDeviceToDevice, c->stream));
            }
            return launch_kappa_ingest(c, ki_src.as<const double>(), L.kappa, ki_coarse.as<double>(), L.N / 2,
                                       MG_KAPPA_ARITHMETIC);
        }
        if (k == "restrict") return level > 0 ? restrict_to(c, level, c->restriction) : fail("level 0");
        if (k == "prolong") return level > 0 ? prolong(c, level, 1) : fail("level 0");
        if (k == "norm2") return dot_device(c, L, L.v.rows, L.v.rows, 1);
        return fail("unknown kernel " + k);
    };
    // (its launches are not the smoother's: mg_smoother_launches stays as it was, "gs" included)
    const auto counts = c->smoother_counts;
    auto timed = [&]() -> int {
        MG_TRY(once());   // warm-up
        HIP_TRY(hipEventRecord(e0, c->stream));
        for (int r = 0; r < reps; ++r) MG_TRY(once());
        HIP_TRY(hipEventRecord(e1, c->stream));
        return 0;
    };
    const int rc = timed();
    c->smoother_counts = counts;
    MG_TRY(rc);
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = (double)ms / reps;
    return 0;
}

int mg_sync(mg_handle c) {
    if (!c) return fail("null handle");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int mg_memory_bytes(mg_handle c, int64_t* bytes) {
    if (!c || !bytes) return fail("bad arguments");
    *bytes = c->bytes;
    return 0;
}

}  // extern "C"
