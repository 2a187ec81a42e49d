// K weighted-Jacobi sweeps in one pass over HBM (K = 3, 4, 5) on class-coded 3-D seven-point levels.
//
// multigrid.py:223-228 runs mu = 50 identical sweeps in a row.  The two-sweep pass (mg_jacobi2.hip.h) already streams
// its 25 bytes per row at the rate the memory system gives a plane march, so the only lever left is bytes per SWEEP:
// here a workgroup carries K sweeps through the planes at once and a pass costs one read of x, f and the class byte
// and one write of the result per K sweeps (plus the tile rims, which grow with K: a tile loads EX x (EY + 2) cells of
// a plane and stores (EX - 2K) x (EY - 2K + 2)).
//
// The march.  "Level" t is the iterate after t sweeps (level 0 = x).  A thread owns NC cells of the tile; at step k
// the workgroup FINISHES plane k+K-t of level t for t = 1 .. K (level K of plane k is the result) and STARTS the plane
// above it.  A row's sum is accumulated in the order of the one-sweep kernels, -P, -nx, -1, 0, +1, +nx, +P:
//   phase A  (registers only)  the level-(t-1) value of plane k+K-t+1 has just been finished (or, level 0, arrived
//            from memory): it is the missing +P term of level t in plane k+K-t, whose result is thereby complete --
//            and in turn the missing term of level t+1 one plane below: the K finishes chain through registers.  The
//            value a cell relaxes (its own previous-level value, the diagonal operand) is read back from the cell's own
//            slot of the level's LDS image, which then takes the new plane.  The next plane's sum starts with its -P
//            term, that same read-back value.
//   barrier
//   phase B  the in-plane terms (-nx, -1, 0, +1, +nx) of the planes started in phase A.  A thread reads its own cells'
//            values back from the images and the line below / above its lines; the -1 / +1 neighbours are its own
//            values of the neighbouring lanes (DPP wave rotates: a tile line is the 64 lanes of one wave), the +-nx
//            neighbours between a thread's own lines are its own registers.
//   barrier
// so per cell and level there are K partial sums in registers and ONE plane image in LDS -- K (EY+2) x EX images in
// all --, not three planes of every level, and per cell, level and step the LDS sees one write and three reads.  f is
// needed by every level of a plane: a ring of K values per cell, the newest arriving from memory a step before its first use; class bytes are packed four cells to a register.  The
// loads of plane k+K+1 are issued right after phase A has consumed plane k+K's registers and are in flight through
// phase B and both barriers.
// A wave whose cells of the planes k .. k+K all carry the level's most frequent class (the interior stencil), in a
// step whose planes all exist, runs straight-line code with the entries in scalar registers; other waves (next to the
// boundary, first / last planes) take the general path: per cell group either the scalar entries or the class table.
// On whole levels the steps of the straight-line forms are known before the launch (the march plan, jk3_plan below): a wave
// inside a planned run of planes loads and inspects no classes at all.
// Everything is done in ROW space like the other passes (cell <-> row whether or not it wraps around a grid line; rows
// outside the level are zeros at every level), with the same fma chain and the same IEEE division as sdia_cls_body:
// bit-identical to K single sweeps.  Out-of-grid cells that the tile clamps (lines beyond ny + 1 or below -2, cells
// past the end of a grid line) hold finite, wrong values; they reach grid rows only through couplings that do not
// exist (stored zeros), so no result depends on them.
//
// Tile shapes ("fuse_k_shape"; all are 64 cells wide, a wave owns LPW whole lines and a thread NC = LPW cells, one per line):
//   1  64 x 48, 12 waves x 4 lines          jk3_body<K, 12, 4>       also levels of more than 64 classes, and K = 2 on slabs
//   4  64 x 24,  8 waves x 3 lines          jk3_body<K, 8, 3>        two workgroups per CU, 64 table rows ("fuse_k_small_tiles")
//   7  64 x 32, 16 waves x 2 lines          jk3_body<K, 16, 2>       three and four sweeps per pass; with ESC, levels with escape rows
//   8  shape 7 with one barrier per step    jk3_body<K, 16, 2, .., B1>   five sweeps per pass; slabs
//   9  64 x 36, rim waves                   jk3_rim_body<5>          five sweeps per pass on the large whole levels
// (128-cell lines, -1 / +1 neighbours through LDS, a second register set for the arriving plane and the 64 x 24 / 64 x 48
// tiles by 4, 6 and 16 waves were measured slower and are gone: DESIGN.md, "Tile shape".)
//
// Slabs: with K halo planes of x (and K - 1 of f and the classes) on either side a rank relaxes level t on the planes
// [-(K-t), nz + (K-t)) of its neighbours too (plo / phi), so K sweeps need ONE exchange and no boundary chain.
#pragma once
#include "mg_jacobi2.hip.h"
#include <type_traits>

namespace mgk {

struct JK3Args {
    const double* x;            // row-based source iterate, zero slack (vec_reach) on both sides
    const double* f;            // row-based
    double* out;                // row-based, != x
    const unsigned char* cls;   // class of row r is cls[r + clead]
    const double* ctab;         // ctab[class][CLS_W]: the row's seven entries in column order
    int64_t clead, P;
    int ncls, cmain;
    double cm[8];               // entries of the most frequent class (scalar registers)
    double omega;
    int nx, ny, nz;             // nz: owned planes
    int plo, phi;               // halo planes below / above whose rows exist on a neighbour (0: the level ends here)
    // work items: tiles x plane segments of `seglen` planes; the launch covers the planes [za0, za1) and then [zb0, zb1)
    // (slabs: the planes the neighbours wait for in one launch, the rest in another; whole levels: [0, nz) and nothing)
    int ntx, nty, seglen, za0, za1, zb0, zb1;
    // ... and so that the last round of workgroups is not a nearly empty one, the tiles from `ta` on (fewer than there are
    // CUs; plane range a only) are cut into shorter segments of `seglen_b` planes and come last
    int ta, seglen_b;
    unsigned nitems, xcd_chunk;
    int nt_store;               // 1: non-temporal stores of the result
    // rows of class CLS_ESCAPE (mg_jacobi2.hip.h): read from the symmetric diagonal storage, slices of 1 << sshift rows
    int escape;                 // 1: the level has such rows
    const double* dvals;
    int64_t mlead;
    int sshift;
    int force_form;             // -1; timing experiments (mg_time_kernel only, results are wrong): every step in form 0 / 1 / 2
    // march plan (jk3_plan): per (tile, wave) the planes [p0, p1) in which all the wave's cells carry class `cmain` and the
    // planes [q0, q1) in which every one of them keeps its class, four ints; null: no plan, every step loads and inspects
    // its classes (slabs, levels with escape rows, other tile shapes)
    const int* plan;
};

// Where a tile cell's double lies, as a byte offset from `base of the plane - bias` (>> 3: where its class byte lies from
// jk3_class_base): lines clamped to [-2, ny + 1], cells past the end of their grid line to the cell behind it.  The march
// and the plan (jk3_plan) both take their class addresses from these two functions, so the plan speaks about exactly the
// bytes whose loads it replaces.
__device__ __forceinline__ unsigned jk3_cell_offset(int line, int col, int nx, int ny, int tx0, int xcl, int bias) {
    return 8u * (unsigned)(min(max(line, -2), ny + 1) * nx + tx0 + min(col, xcl) + bias);
}
__device__ __forceinline__ const unsigned char* jk3_class_base(const unsigned char* cls, int64_t clead, int bias) {
    return cls + clead - bias;
}

// Rows of class CLS_ESCAPE (levels with more than 255 distinct rows, mg_jacobi2.hip.h): when a plane arrives, every lane
// that holds such a row fetches its seven entries from the symmetric diagonal storage into a row of a POOL behind the
// class table -- rows handed out in turn, workgroup-wide, through an LDS counter -- and goes on with the pool row's number
// as the cell's class: the general form of the step then finds the entries where it finds those of any class.  A pool row
// is needed for the K + 1 steps its plane stays in the ring; the host checks (jk3_escape_window) that no tile ever takes
// more than jk3_pool(K) rows within K + 2 consecutive planes before it lets a level use the march.
// (a power of two that fits next to the K plane images of the 64 x 32 tiles: 64 KB, 32 KB with five images)
constexpr int jk3_pool(int K) { return K >= 5 ? 512 : 1024; }

// (TR: rows of the class table kept in LDS -- 256, or 64 for the shapes that run two workgroups per CU)
template <int K, int NW, int LPW, int TR> constexpr size_t jk3_lds_doubles() {
    return TR * CLS_W + (size_t)K * (NW * LPW + 2) * 64 + 2 * (64 + 2);
}
// One barrier per step (tile shape 8, `B1`): level 0 is not kept in LDS at all -- a wave has x of its own lines in registers
// and loads the line above and the line below them too (lines its neighbour waves load in the same step: they come from
// the caches) --, and the images of levels 1 .. K-1 are double-buffered by the parity of the step.  Phase A of step k
// writes parity k & 1 and reads its own slots of parity (k - 1) & 1; phase B reads parity k & 1, so the barrier behind
// phase B goes: the next write of a parity that phase B(k) reads is phase A(k + 2), and the barrier in front of phase
// B(k + 1) lies between them.  Images of EY lines, stride EY + 1: the zero lines between them (and before the first) are
// the line below and above the tile of every level >= 1 (those rows were always outside the level's valid region).
//   [zero] [level 1, parity 0] [zero] [level 2, parity 0] [zero] ... [level K-1, parity 1] [zero]
template <int K, int NW, int LPW, int TR> constexpr size_t jk3b_lds_doubles() {
    return TR * CLS_W + (size_t)(2 * (K - 1) * (NW * LPW + 1) + 1) * 64;
}
template <int K, int NW, int LPW, int TR> constexpr size_t jk3b_lds_bytes() {
    return sizeof(double) * jk3b_lds_doubles<K, NW, LPW, TR>();
}

template <int K, int NW, int LPW, int TR, bool ESC = false> constexpr size_t jk3_lds_bytes() {
    constexpr size_t base = jk3_lds_doubles<K, NW, LPW, TR>();
    return sizeof(double) * (ESC ? (base + CLS_W - 1) / CLS_W * CLS_W + (size_t)(jk3_pool(K) + 1) * CLS_W : base);
}

// (jk3_from_west / jk3_from_east -- the value of the lane next door through DPP -- live in mg_jacobi2.hip.h)

// Level caps.  Level t is valid on the tile lines [t - 1, EY - t] only (level 0 has the halo lines -1 and EY too, the result
// exists on [K - 1, EY - K]), so the highest level a line takes part in is cap(ey) = min(ey + 1, EY - ey, K): whatever is
// computed above it reaches no result.  A line belongs to one wave, so the caps of a wave's lines are the same for all its
// lanes and fixed for the launch: the straight-line forms of a step exist once per KIND of wave -- the waves whose lines
// all have cap K (`jk3_caps<K, EY, -1>`) and one kind for each wave that has a line with a lower cap (E0: its first line).
template <int K, int EY, int E0> struct jk3_caps {
    static constexpr int of(int l) {      // of the wave's line l
        if (E0 < 0) return K;
        const int ey = E0 + l, a = ey + 1 < EY - ey ? ey + 1 : EY - ey;
        return a < K ? a : K;
    }
};

template <int K, int NW, int LPW, int TR, bool ESC = false, bool B1 = false>
__device__ __forceinline__ void jk3_body(const JK3Args& a) {
    constexpr int EX = 64, EY = NW * LPW, NC = LPW, IMG = (EY + 2) * EX;
    // (B1) image stride and parity stride, in doubles
    constexpr int IS = (EY + 1) * EX, PS = (K - 1) * IS;
    static_assert(!B1 || !ESC, "one barrier per step: no escape rows");
    // classes in the ring: a byte per cell, four cells to a register -- sixteen bits where pool rows are classes too
    constexpr int CBITS = ESC ? 16 : 8, CPR = 32 / CBITS, CW = (NC + CPR - 1) / CPR;
    constexpr unsigned CMASK = (1u << CBITS) - 1u;
    constexpr int DYN0 = (int)((jk3_lds_doubles<K, NW, LPW, TR>() + CLS_W - 1) / CLS_W);   // the pool's first row, counted from sT
    static_assert(CLS_W == 8, "table rows of eight doubles");
    constexpr int WI = EX - 2 * K, HY = EY - 2 * K + 2;       // cells per line / lines of a tile that get all K sweeps
    static_assert(NC * (K + 1) <= 64, "the fast-path flags live in one scalar register pair");
    static_assert(WI > 0 && HY > 0, "tile too small for K sweeps");
    extern __shared__ double j2_smem[];
    double* const sT = j2_smem;                               // 256 x 8   entries of the row classes, [7] = omega / diagonal
    double* const sI = sT + TR * CLS_W + (EX + 2);           // K x (EY+2) x EX   one plane of level t, origin (0,-1)
                                                              // (B1: see jk3b_lds_doubles; addressed from j2_smem)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));

    unsigned id;
    {
        const unsigned b = blockIdx.x, xcd = b & 7u, j = b >> 3, ch = a.xcd_chunk;
        id = ((j / ch) * 8u + xcd) * ch + (j % ch);
    }
    if (id >= a.nitems) return;
    const unsigned ntile = (unsigned)(a.ntx * a.nty);
    const int nsa = (a.za1 - a.za0 + a.seglen - 1) / a.seglen;
    const int nsb = (a.zb1 - a.zb0 + a.seglen - 1) / a.seglen;
    const unsigned items_a = (unsigned)a.ta * (unsigned)(nsa + max(nsb, 0));
    unsigned tt;
    int z0, z1;
    if (id < items_a) {
        const int seg = (int)(id / (unsigned)a.ta);
        tt = id % (unsigned)a.ta;
        z0 = seg < nsa ? a.za0 + seg * a.seglen : a.zb0 + (seg - nsa) * a.seglen;
        z1 = min(seg < nsa ? a.za1 : a.zb1, z0 + a.seglen);
    } else {
        const unsigned j = id - items_a, tb = ntile - (unsigned)a.ta;
        tt = (unsigned)a.ta + j % tb;
        z0 = a.za0 + (int)(j / tb) * a.seglen_b;
        z1 = min(a.za1, z0 + a.seglen_b);
    }
    const int tiy = (int)(tt / (unsigned)a.ntx), tix = (int)(tt % (unsigned)a.ntx);
    if (z1 <= z0) return;
    const int tx0 = tix * WI - K, ty0 = tiy * HY - (K - 1);   // grid position of cell (0, 0)

    {
        const int nt = a.ncls * CLS_W;
        for (int i = threadIdx.x; i < nt; i += NW * WAVE) {
            double v = a.ctab[i];
            if ((i & (CLS_W - 1)) == CLS_W - 1) {
                const double d = a.ctab[i - 4];
                v = a.omega * (1.0 / (d != 0.0 ? d : 1.0));
            }
            sT[i] = v;
        }
        constexpr int NZ = B1 ? (2 * (K - 1) * (EY + 1) + 1) * EX : K * IMG + 2 * (EX + 2);
        for (int i = threadIdx.x; i < NZ; i += NW * WAVE) sT[TR * CLS_W + i] = 0.0;
    }
    unsigned* const esc_count = reinterpret_cast<unsigned*>(sT + (size_t)CLS_W * (DYN0 + jk3_pool(K)));   // (ESC) pool rows handed out so far
    if constexpr (ESC) {
        if (threadIdx.x == 0) *esc_count = 0u;
    }
    const double m0 = a.cm[0], m1 = a.cm[1], m2 = a.cm[2], m3 = a.cm[3], m4 = a.cm[4], m5 = a.cm[5], m6 = a.cm[6];
    const double mcf = a.omega * (1.0 / (m3 != 0.0 ? m3 : 1.0));
    const int cmain = a.cmain;

    // cell c of this thread: ex = lane, ey = wave*LPW + c
    const int ey0 = wave * LPW;
    const int lw0 = (ey0 + 1) * EX + lane;
    auto lwof = [&](int c) -> int { return c * EX; };      // cell c relative to cell 0
    // cell 0 in the images 0, 1 / 2, 3 / 4: one address register per pair, so that every LDS access of the march is
    // `register + 16-bit immediate` (the images span more than 64 KB; left alone the compiler keeps an address per
    // cell and image)
    int ibase[(K + 1) / 2];     // (element offsets from sI; the pin keeps the compiler from folding them back into one per access)
#pragma unroll
    for (int q = 0; q < (K + 1) / 2; ++q) {
        ibase[q] = 2 * q * IMG + lw0;
        asm volatile("" : "+v"(ibase[q]));
    }
    auto image = [&](int t) -> double* { return sI + ibase[t >> 1] + (t & 1) * IMG; };  // level t's plane, at cell 0
    // (B1) level t >= 1 of the step's parity (bcur) or of the step before (bprev), at cell 0: one address register each,
    // set per step, at the wave's line -1 of level 1 -- every access of a step is `register + 16-bit immediate`
    int bcur = 0, bprev = 0;
    auto limg = [&](int base, int t) -> double* { return j2_smem + base + (t - 1) * IS + EX; };
    double XP[B1 ? NC : 1];     // (B1) x of the plane before the newest, own cells: the value level 1 relaxes
    double hS, hN;              // (B1) x of the line below / above this wave's lines, of the newest plane
    unsigned inT = 0;           // bit c: this lane's cell c gets all K sweeps and lies on the grid
    const int64_t rb0 = (int64_t)(ty0 + ey0) * a.nx + (tx0 + lane);
    auto rowof = [&](int c) -> int64_t { return rb0 + (int64_t)c * a.nx; };
    // the row of cell c in plane p exists  <=>  the level's plane range holds p + sh(c), sh = -1, 0, +1 (two bits per cell)
    unsigned shw = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int ex = lane, ey = ey0 + c;
        if (ex >= K && ex < EX - K && ey >= K - 1 && ey <= EY - K && tx0 + ex < a.nx && ty0 + ey < a.ny) inT |= 1u << c;
        const int64_t r = rowof(c);
        shw |= (r < 0 ? 0u : (r >= a.P ? 2u : 1u)) << (2 * c);
    }
    auto shof = [&](int c) -> int { return (int)((shw >> (2 * c)) & 3u) - 1; };
    // (ESC) bit c: cell c is a stand-in -- its line or its place in the line is clamped (see `eo`), it reads another cell's
    // row and no result depends on it: if that row is an escape row, the cell goes on as class 0 and takes no pool row
    unsigned standin = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int line = ty0 + ey0 + c;
        if (lane > a.nx + 1 - tx0 || line < -2 || line > a.ny + 1) standin |= 1u << c;
    }
    const bool wlo = wave == 0, whi = wave == NW - 1;
    // Level caps (jk3_caps) on the 64 x 32 tiles of sixteen waves, two lines each (tile shapes 7 and 8): the first two and the
    // last two waves have lines with a cap below K (K = 3: the first and the last).  A cell with cap m < K computes the levels
    // 1 .. m, still hands its level-m value to the image -- the line next to it, whose cap is m + 1, reads it as its -nx / +nx
    // term -- and does nothing above: those partial sums and image slots keep their zeros and nothing reads them.
    constexpr bool CAPS = B1 && NW == 16 && LPW == 2 && K >= 3;
    using caps_all = jk3_caps<K, EY, -1>;
    using caps_w0 = jk3_caps<K, EY, 0>;
    using caps_w1 = jk3_caps<K, EY, LPW>;
    using caps_w2 = jk3_caps<K, EY, EY - 2 * LPW>;
    using caps_w3 = jk3_caps<K, EY, EY - LPW>;
    constexpr bool CAPS1 = CAPS && (caps_w1::of(0) < K || caps_w1::of(LPW - 1) < K);
    constexpr bool CAPS2 = CAPS && (caps_w2::of(0) < K || caps_w2::of(LPW - 1) < K);
    // 0: all lines have cap K (one compare and a branch not taken in front of each phase); 1 .. 4: the waves above
    const int wkind = !CAPS ? 0 : wave == 0 ? 1 : wave == NW - 1 ? 4 : (CAPS1 && wave == 1) ? 2 : (CAPS2 && wave == NW - 2) ? 3 : 0;
    auto by_caps = [&](auto&& fn) __attribute__((always_inline)) {
        if constexpr (CAPS) {
            if (__builtin_expect(wkind != 0, 0)) {
                if (wkind == 1) fn(caps_w0{});
                else if (wkind == 4) fn(caps_w3{});
                else if constexpr (CAPS1 && CAPS2) {
                    if (wkind == 2) fn(caps_w1{});
                    else fn(caps_w2{});
                }
                return;
            }
        }
        fn(caps_all{});
    };
    // (general form: the same caps at run time, one scalar register per cell, compared where a level is reached -- the pin
    //  keeps the compiler from holding every comparison's outcome in a register pair for the whole march)
    auto cap_of = [&](int c) -> int {
        if constexpr (!CAPS) return K;
        const int ey = ey0 + c;
        int cap = min(min(ey + 1, EY - ey), K);
        asm volatile("" : "+v"(cap));
        return __builtin_amdgcn_readfirstlane(cap);
    };

    // Addresses: `uniform base of the plane + a byte offset fixed for the whole march` (see j2c_body).  Lines are
    // clamped to [-2, ny + 1], cells past the end of their grid line to the cell behind it, planes to the slack planes.
    const int bias = 2 * a.nx + K + 2;
    const int xcl = a.nx + 1 - tx0;
    unsigned eo[NC];            // byte offsets of the cells' doubles (>> 3: of their class bytes)
#pragma unroll
    for (int c = 0; c < NC; ++c) eo[c] = jk3_cell_offset(ty0 + ey0 + c, lane, a.nx, a.ny, tx0, xcl, bias);
    // ... of the line above the tile (the last wave loads it) / below it (the first wave)
    const int above = min(ty0 + EY, a.ny + 1), below = max(ty0 - 1, -2);
    const unsigned eor = 8u * (unsigned)(bias + tx0 + min(lane, xcl) + (wlo ? below : above) * a.nx);
    unsigned eos = 0, eon = 0;  // (B1) the lines below / above the wave's, clamped like `eo`
    if constexpr (B1) {
        eos = jk3_cell_offset(ty0 + ey0 - 1, lane, a.nx, a.ny, tx0, xcl, bias);
        eon = jk3_cell_offset(ty0 + ey0 + LPW, lane, a.nx, a.ny, tx0, xcl, bias);
    }
    const unsigned char* const clsb = jk3_class_base(a.cls, a.clead, bias);
    const double* const xb0 = a.x - bias;
    const double* const fb0 = a.f - bias;
    auto sbase = [](const void* p) -> gcptr_t {
        const unsigned long long u = (unsigned long long)p;
        const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u);
        const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
        return (gcptr_t)(((unsigned long long)hi << 32) | lo);
    };
    // (the pins keep the 32-bit offsets from being widened once and for all outside the loop: `scalar base + 32-bit
    //  register offset` is an addressing mode, a 64-bit register pair per cell is not)
    auto ldd = [](gcptr_t b, unsigned e8) -> double {
        asm volatile("" : "+v"(e8));
        return *(const __attribute__((address_space(1))) double*)(b + e8);
    };
    // (the class byte arrives as the low byte of an unaligned 32-bit load and is masked where it is first used: a byte
    //  load is masked by the compiler right behind the load -- which makes every wave wait for the loads it has just issued)
    typedef unsigned int __attribute__((aligned(1))) u32_unaligned_t;
    auto ldc = [](gcptr_t b, unsigned e8) -> int {
        unsigned e = e8 >> 3;
        asm volatile("" : "+v"(e));
        return (int)*(const __attribute__((address_space(1))) u32_unaligned_t*)(b + e);
    };
    const int pmin = -a.plo - 1, pmax = a.nz + a.phi;

    // Planned steps (march plan).  On a whole level (plo = phi = 0) the step k takes one of the straight-line forms when
    //   k >= 1 and k + K + 1 < nz      every row the step touches exists (planes k-1 .. k+K+1 through sh), and
    //   form 0:  fast == ALLFAST       all 64 x NC class bytes of the ring's planes k .. k+K are `cmain`, or else
    //   form 1:  `same`                every cell's class byte is the same in the ring's planes k .. k+K.
    // The plan gives the wave two runs of planes: [p0, p1), all class bytes are cmain, and [q0, q1), every cell's class byte
    // is the same in all planes of the run (the two are equal or disjoint: a run of cmain planes is a run of constant
    // classes, and the longest of either kind is kept).  The third / fourth line holds when r0 <= k and k + K <= r1 - 1
    // for the run [r0, r1).  A segment's ring holds real planes from its step z0 - K on (the K steps before it run on the
    // zeros the ring starts with and take the form those give), so the steps
    //   [klo, khi) = [max(r0, 1, z0 - K), min(r1 - K, nz - K - 1))
    // are steps to which today's test gives form 0 (run p) or, since a constant class that is not cmain everywhere fails
    // the form-0 test, form 1 (run q), known without looking at a class: they load no classes, move no ring and decide
    // nothing.  A segment uses the run that gives it more such steps.  Step k's loads bring the plane that step k + 1
    // consumes, so the class loads stop with the loads for step klo and resume with those for step khi.  Step klo - 1
    // exists and is an ordinary one; it leaves the classes of the plane klo in cw[0], where form 1 reads them and where
    // they stay.  In step khi the ring's planes khi .. khi+K-1 (all below r1) get those classes and their flags, as
    // today's path would hold them, and the plane khi + K arrives from memory.
    constexpr bool PLANNED = !ESC && NW == 16 && LPW == 2 && K >= 3;    // tile shapes 7 and 8
    int klo = 0x7fffffff, khi = 0x7fffffff, kform = 0;
    if constexpr (PLANNED) {
        if (a.plan) {
            const int* const pw = a.plan + 4 * ((int)tt * NW + wave);
            const int top = a.nz - K - 1;
            const int lo0 = max(max(pw[0], 1), z0 - K), hi0 = min(pw[1] - K, top);
            const int lo1 = max(max(pw[2], 1), z0 - K), hi1 = min(pw[3] - K, top);
            const int n0 = min(hi0, z1) - lo0, n1 = min(hi1, z1) - lo1;
            if (n0 > 0 && n0 >= n1) {
                klo = __builtin_amdgcn_readfirstlane(lo0);
                khi = __builtin_amdgcn_readfirstlane(hi0);
            } else if (n1 > 0) {
                klo = __builtin_amdgcn_readfirstlane(lo1);
                khi = __builtin_amdgcn_readfirstlane(hi1);
                kform = 1;
            }
        }
    }
    auto interior_step = [&](int k) -> bool { return PLANNED && k >= klo && k < khi; };

    // registers per cell: K partial sums; f of the planes k .. k+K-1; x, f and the class of the plane that arrives
    double acc[K][NC], fr[K][NC];
    // x and the classes of the plane that arrives, own cells; (first / last wave) x of the line below / above the tile
    double X[NC], hy = 0.0;
    int C[NC];
    unsigned cw[K + 1][CW];     // class bytes of the planes k .. k+K, four cells to a register
    unsigned long long fast = 0;        // wave-uniform; bit j*NC + c: all 64 cells c of plane k+j are of class cmain
    constexpr unsigned long long ALLFAST = (NC * (K + 1) == 64) ? ~0ull : ((1ull << (NC * (K + 1))) - 1ull);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int t = 0; t < K; ++t) acc[t][c] = fr[t][c] = 0.0;
        X[c] = 0.0;
        C[c] = 0;
    }
#pragma unroll
    for (int j = 0; j <= K; ++j)
#pragma unroll
        for (int q = 0; q < CW; ++q) cw[j][q] = 0u;
    hS = hN = 0.0;
#pragma unroll
    for (int c = 0; c < (B1 ? NC : 1); ++c) XP[c] = 0.0;   // (level 0 below the first plane: the zeros of the image it replaces)

    // Loads are issued in slices, slice i of n between the pieces of phase B: issued in one burst (14 per wave, all twelve
    // waves at the same point of the step) they keep every wave at the vector-memory issue port in front of the barrier
    // while nothing computes -- measured: the burst added its whole issue time to the step.
    // Slice i: x and the classes of its cells of `plane` into X and C (the y ring with the last slice), f of the
    // plane `fplane` into the slot of the ring that has just become free (a step needs it one step after x of that plane).
    // (`noc`, wave-uniform: the step that consumes the plane is an interior one -- no class loads)
    auto load_slice = [&](const int i, const int n, const int plane, const int fplane, const bool noc) __attribute__((always_inline)) {
        const int64_t o = (int64_t)min(max(plane, pmin), pmax) * a.P;
        const gcptr_t cb = sbase(clsb + o);
        const gcptr_t xb = sbase(xb0 + o);
        const gcptr_t fb = sbase(fb0 + (int64_t)min(max(fplane, pmin), pmax) * a.P);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if ((c * n) / NC != i) continue;
            X[c] = ldd(xb, eo[c]);
            if (!noc) C[c] = ldc(cb, eo[c]);
            fr[K - 1][c] = ldd(fb, eo[c]);
        }
        if constexpr (B1) {
            if (i == n - 1) { hS = ldd(xb, eos); hN = ldd(xb, eon); }
        } else if (i == n - 1 && (wlo || whi)) {
            hy = ldd(xb, eor);
        }
    };
    auto cls_of = [&](int j, int c) -> int { return (int)((cw[j][c / CPR] >> (CBITS * (c % CPR))) & CMASK); };
    // (general form: extracted anew at every use -- kept, the table addresses of all cells and ring planes cost 20 registers)
    auto cls_now = [&](int j, int c) -> int {
        unsigned w = cw[j][c / CPR];
        asm volatile("" : "+v"(w));
        return (int)((w >> (CBITS * (c % CPR))) & CMASK);
    };
    int k_plane = 0;            // the step: plane whose result it stores, whether it stores, the plane's base in `out`
    bool k_store = false;
    __attribute__((address_space(1))) char* k_out = nullptr;
    // (a cell that stores is not clamped: its byte offset is its row's)
    auto store = [&](int c, double v) {
        unsigned e8 = eo[c];
        asm volatile("" : "+v"(e8));
        // (the result is next read a whole pass later: stored past the caches, it leaves the L2 to the tile rims)
        if (a.nt_store) __builtin_nontemporal_store(v, (__attribute__((address_space(1))) double*)(k_out + e8));
        else *(__attribute__((address_space(1))) double*)(k_out + e8) = v;
    };
    // plane range of level t (rows outside it are zeros)
    int lo_t[K + 1], n_t[K + 1];
#pragma unroll
    for (int t = 1; t <= K; ++t) {
        lo_t[t] = -min(a.plo, K - t);
        n_t[t] = a.nz + min(a.phi, K - t) - lo_t[t];
    }

    // ---- the three forms of a step (chosen per wave and step; all of them read and write the images alike) ----
    // Straight-line form.  COL = false: every cell has the interior stencil, entries in scalar registers.  COL = true:
    // a cell's class is the same in all planes of the ring -- it depends on the lane (tile columns along the x boundary) and / or
    // on the cell's grid line (tile rows along the y boundary), away from the first and last planes: the entries of each cell's
    // row come from the class table once per cell and phase.  (Until the y boundary took this form too its tiles ran the
    // general one, 1.6 x slower -- and on a level with one round of workgroups, 257^3, the slowest tiles ARE the launch.)
    auto phase_a_fast = [&](auto col_tag, auto caps) __attribute__((always_inline)) {
        constexpr bool COL = decltype(col_tag)::value;
        using CAP = decltype(caps);
#pragma unroll
        for (int c = 0; c < NC; ++c) {      // (cell c lies on the wave's line c)
            const int iw = lwof(c);
            double k0 = m0, k6 = m6, kcf = mcf;
            if constexpr (COL) {
                const dvec2_t* const tr = reinterpret_cast<const dvec2_t*>(sT + CLS_W * cls_of(0, c));
                const dvec2_t t01 = tr[0], t67 = tr[3];
                k0 = t01.x; k6 = t67.x; kcf = t67.y;
            }
            double nw = X[c];
#pragma unroll
            for (int t = 1; t <= K; ++t) {
                if (t > CAP::of(c)) {       // (above the line's cap: its last level goes to the image, nothing else)
                    if (t == CAP::of(c) + 1) (B1 ? limg(bcur, t - 1) : image(t - 1))[iw] = nw;
                    continue;
                }
                if constexpr (B1) {
                    const double wd = t == 1 ? XP[c] : limg(bprev, t - 1)[iw];
                    const double s = fma(k6, nw, acc[t - 1][c]);      // +P
                    const double o = wd + kcf * (fr[K - t][c] - s);
                    acc[t - 1][c] = fma(k0, wd, 0.0);                 // -P of the plane above
                    if (t > 1) limg(bcur, t - 1)[iw] = nw;
                    nw = o;
                    continue;
                }
                double* const img = image(t - 1);
                const double wd = img[iw];
                const double s = fma(k6, nw, acc[t - 1][c]);      // +P
                const double o = wd + kcf * (fr[K - t][c] - s);
                acc[t - 1][c] = fma(k0, wd, 0.0);                 // -P of the plane above
                img[iw] = nw;
                nw = o;
            }
            if (CAP::of(c) == K && k_store && (inT >> c & 1u)) store(c, nw);
        }
    };
    // (phase B comes in K pieces, one per level, so that the loads can go out in COMMON code between them: a load issued
    //  inside the branches of the three forms makes the compiler spill hundreds of registers)
    auto phase_b_fast = [&](auto col_tag, auto caps, const int t) __attribute__((always_inline)) {
        constexpr bool COL = decltype(col_tag)::value;
        using CAP = decltype(caps);
        const double* const img = B1 ? limg(bcur, t > 1 ? t - 1 : 1) : image(t - 1);
        double v[LPW], ys, yn;      // level t-1 on the wave's lines, the line below and the line above them
        if (B1 && t == 1) {         // (level 0: registers)
            ys = hS; yn = hN;
#pragma unroll
            for (int l = 0; l < LPW; ++l) v[l] = X[l];
        } else {
            ys = img[-EX]; yn = img[LPW * EX];
#pragma unroll
            for (int l = 0; l < LPW; ++l) v[l] = img[l * EX];
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (t > CAP::of(c)) continue;       // (the line has no level t: the reads only it needed go with it)
            const double yw = jk3_from_west(v[c]), ye = jk3_from_east(v[c]);
            double k1 = m1, k2 = m2, k3 = m3, k4 = m4, k5 = m5;
            if constexpr (COL) {
                const dvec2_t* const tr = reinterpret_cast<const dvec2_t*>(sT + CLS_W * cls_of(0, c));
                const dvec2_t t01 = tr[0], t23 = tr[1], t45 = tr[2];
                k1 = t01.y; k2 = t23.x; k3 = t23.y; k4 = t45.x; k5 = t45.y;
            }
            double s = acc[t - 1][c];
            s = fma(k1, c > 0 ? v[c > 0 ? c - 1 : 0] : ys, s);
            s = fma(k2, yw, s);
            s = fma(k3, v[c], s);
            s = fma(k4, ye, s);
            s = fma(k5, c + 1 < LPW ? v[c + 1 < LPW ? c + 1 : c] : yn, s);
            acc[t - 1][c] = s;
        }
    };
    // General form: every cell's entries from the class table, rows outside the level masked to zero.
    auto phase_a_general = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int iw = lwof(c);
            double nw = X[c];
            int pc = k_plane + shof(c);
            asm volatile("" : "+v"(pc));            // (one register per cell and step, not one per cell and level for the whole march)
            const int cap = cap_of(c);
#pragma unroll
            for (int t = 1; t <= K; ++t) {
                const int j = K - t;                                  // ring index of the plane being finished
                double* const img = B1 ? limg(bcur, t > 1 ? t - 1 : 1) : image(t - 1);
                if (CAPS && t > cap) {
                    if (t == cap + 1) img[iw] = nw;
                    continue;
                }
                const double wd = B1 ? (t == 1 ? XP[B1 ? c : 0] : limg(bprev, t - 1)[iw]) : img[iw];
                const dvec2_t t67 = reinterpret_cast<const dvec2_t*>(sT + CLS_W * cls_now(j, c))[3];
                const dvec2_t t01 = reinterpret_cast<const dvec2_t*>(sT + CLS_W * cls_now(j + 1, c))[0];
                const double s = fma(t67.x, nw, acc[t - 1][c]);
                double o = wd + t67.y * (fr[j][c] - s);
                o = (unsigned)(pc + j - lo_t[t]) < (unsigned)n_t[t] ? o : 0.0;
                acc[t - 1][c] = fma(t01.x, wd, 0.0);
                if (!B1 || t > 1) img[iw] = nw;
                nw = o;
                __builtin_amdgcn_sched_barrier(0);      // (rare path: one cell and level at a time keeps it out of the
                                                        //  register budget of the straight-line forms)
            }
            if (k_store && (inT >> c & 1u)) store(c, nw);
        }
    };
    auto phase_b_general = [&](const int t) __attribute__((always_inline)) {
        // (B1, level 0: the -1 / +1 neighbours through DPP as in the straight-line form, all cells' before the first use)
        double x0w[B1 ? NC : 1], x0e[B1 ? NC : 1];
        if constexpr (B1) {
            if (t == 1) {
#pragma unroll
                for (int c = 0; c < NC; ++c) { x0w[c] = jk3_from_west(X[c]); x0e[c] = jk3_from_east(X[c]); }
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (CAPS && t > cap_of(c)) continue;
            const int iw = lwof(c);
            double ys, yw, yd, ye, yn;
            if (B1 && t == 1) {
                ys = c > 0 ? X[c > 0 ? c - 1 : c] : hS;
                yw = x0w[B1 ? c : 0]; yd = X[c]; ye = x0e[B1 ? c : 0];
                yn = c + 1 < LPW ? X[c + 1 < LPW ? c + 1 : c] : hN;
            } else {
                const double* const img = B1 ? limg(bcur, t > 1 ? t - 1 : 1) : image(t - 1);
                ys = img[iw - EX]; yw = img[iw - 1]; yd = img[iw]; ye = img[iw + 1]; yn = img[iw + EX];
            }
            const dvec2_t* const tr = reinterpret_cast<const dvec2_t*>(sT + CLS_W * cls_now(K - t, c));
            const dvec2_t t01 = tr[0], t23 = tr[1], t45 = tr[2];
            double s = acc[t - 1][c];
            s = fma(t01.y, ys, s);
            s = fma(t23.x, yw, s);
            s = fma(t23.y, yd, s);
            s = fma(t45.x, ye, s);
            s = fma(t45.y, yn, s);
            acc[t - 1][c] = s;
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // One step: `X, C, hy` hold plane k+K (arrived).  When phase A has consumed them, the loads of plane k+K+1 go out into the
    // same registers and are in flight through phase B.
    auto step = [&](const int k) __attribute__((always_inline)) {
        k_plane = k; k_store = k >= z0;
        if constexpr (B1) {
            bcur = TR * CLS_W + ey0 * EX + lane + (k & 1) * PS;
            bprev = TR * CLS_W + ey0 * EX + lane + ((k + 1) & 1) * PS;
            asm volatile("" : "+v"(bcur));
            asm volatile("" : "+v"(bprev));
        }
        {
            const unsigned long long u = (unsigned long long)(a.out - bias + (int64_t)k * a.P);
            const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u);
            const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
            k_out = (__attribute__((address_space(1))) char*)(((unsigned long long)hi << 32) | lo);
        }
        // ---- the plane k+K has arrived: its classes join the ring ----
        // (the loaded values are first touched HERE: left alone the compiler masks the class bytes right behind their
        //  loads, a step early, and every wave then waits for its loads before the barrier instead of computing)
#pragma unroll
        for (int c = 0; c < NC; ++c) asm volatile("" : "+v"(X[c]));
        const bool interior = interior_step(k);     // (wave-uniform, from scalar registers)
        if constexpr (PLANNED) {
            if (k == khi) {     // the first step behind the planned ones: the ring as today's path would hold it
                unsigned m = 0;
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    if (__builtin_amdgcn_readfirstlane((int)(__ballot(cls_of(0, c) != cmain) == 0ull))) m |= 1u << c;
                fast = 0;
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    fast |= (unsigned long long)m << (j * NC);
#pragma unroll
                    for (int q = 0; q < CW; ++q) cw[j][q] = cw[0][q];
                }
            }
        }
        int form = kform;
        if (!interior) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                asm volatile("" : "+v"(C[c]));
                C[c] &= 255;
            }
            if constexpr (ESC) {
                // rows of class CLS_ESCAPE: their entries into pool rows, the pool row as the cell's class (see jk3_pool)
                if (a.escape) {
                    const int64_t mp = (int64_t)min(max(k + K, pmin), pmax) * a.P - bias + a.mlead;
                    const int sh = a.sshift;
                    const double* const dv = a.dvals;
                    auto at = [&](int64_t m, int slot) -> double { return dv[((((m >> sh) << 2) + slot) << sh) + (m & (((int64_t)1 << sh) - 1))]; };
                    // (one counter update per wave and plane; the loads of all its cells in flight together)
                    unsigned long long em[NC];
                    unsigned total = 0u;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        if (C[c] == CLS_ESCAPE && (standin >> c & 1u)) C[c] = 0;
                        em[c] = __ballot(C[c] == CLS_ESCAPE);
                        total += (unsigned)__popcll(em[c]);
                    }
                    if (total != 0u) {
                        unsigned b0 = 0u;
                        if (lane == 0) b0 = atomicAdd(esc_count, total);
                        b0 = (unsigned)__builtin_amdgcn_readfirstlane((int)b0);
                        double e[NC][7];
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            if (C[c] == CLS_ESCAPE) {
                                const int64_t m = mp + (int64_t)(eo[c] >> 3);
                                e[c][0] = at(m - a.P, 3); e[c][1] = at(m - a.nx, 2); e[c][2] = at(m - 1, 1);
                                e[c][3] = at(m, 0); e[c][4] = at(m, 1); e[c][5] = at(m, 2); e[c][6] = at(m, 3);
                            }
                        }
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            if (C[c] == CLS_ESCAPE) {
                                const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(em[c] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)em[c], 0u));
                                const int row = DYN0 + (int)((b0 + below) & (unsigned)(jk3_pool(K) - 1));
                                double* const tr = sT + CLS_W * row;
#pragma unroll
                                for (int i = 0; i < 7; ++i) tr[i] = e[c][i];
                                tr[7] = a.omega * (1.0 / (e[c][3] != 0.0 ? e[c][3] : 1.0));
                                C[c] = row;
                            }
                            b0 += (unsigned)__popcll(em[c]);
                        }
                    }
                }
            }
            {
                unsigned m = 0;
#pragma unroll
                for (int q = 0; q < CW; ++q) cw[K][q] = 0u;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    cw[K][c / CPR] |= (unsigned)C[c] << (CBITS * (c % CPR));
                    if (__builtin_amdgcn_readfirstlane((int)(__ballot(C[c] != cmain) == 0ull))) m |= 1u << c;
                }
                fast |= (unsigned long long)m << (K * NC);
            }
            // which form: 0 = interior stencil everywhere in this wave's cells of the planes k .. k+K, 1 = every cell's class the
            // same in all those planes -- both only where every row the step touches exists (planes k-1 .. k+K+1 through sh) or lies on a
            // neighbouring slab (there a level's values beyond its plane range are wrong instead of zero, and reach no
            // result) --, 2 = general
            form = 2;
            if ((a.plo > 0 || k >= 1) && (a.phi > 0 || k + K + 1 < a.nz)) {
                if (fast == ALLFAST) {
                    form = 0;
                } else {
                    bool same = true;
#pragma unroll
                    for (int j = 0; j <= K; ++j)
#pragma unroll
                        for (int c = 0; c < NC; ++c) same = same && cls_of(j, c) == cls_of(0, c);
                    if (__builtin_amdgcn_readfirstlane((int)(__ballot(!same) == 0ull))) form = 1;
                }
            }
        }
        if (a.force_form >= 0) form = a.force_form;
        // ---- phase A: finish plane k+K-t of level t, t = 1 .. K; start the plane above it ----
        if constexpr (CAPS) {
            if (form == 0) by_caps([&](auto caps) __attribute__((always_inline)) { phase_a_fast(std::false_type{}, caps); });
            else if (form == 1) by_caps([&](auto caps) __attribute__((always_inline)) { phase_a_fast(std::true_type{}, caps); });
            else phase_a_general();
        } else {
            if (form == 0) phase_a_fast(std::false_type{}, caps_all{});
            else if (form == 1) phase_a_fast(std::true_type{}, caps_all{});
            else phase_a_general();
        }
        if constexpr (B1) {
#pragma unroll
            for (int c = 0; c < NC; ++c) XP[c] = X[c];
        } else if (wlo || whi) {
            image(0)[wlo ? -EX : LPW * EX] = hy;
        }
        // ---- the rings move on; the next loads go out ----
#pragma unroll
        for (int c = 0; c < NC; ++c) {
#pragma unroll
            for (int j = 0; j + 1 < K; ++j) fr[j][c] = fr[j + 1][c];
            asm volatile("" : "+v"(fr[K - 2][c]));
        }
        if (!interior) {
#pragma unroll
            for (int j = 0; j < K; ++j)
#pragma unroll
                for (int q = 0; q < CW; ++q) cw[j][q] = cw[j + 1][q];
            fast >>= NC;
        }
        __syncthreads();
        // ---- phase B: the in-plane terms of the planes started above (ring index K - t of the moved ring); the next
        //      loads go out between its pieces ----
        auto issue = [&](const int i, const int n) __attribute__((always_inline)) {
            __builtin_amdgcn_sched_barrier(0);
            load_slice(i, n, k + K + 1, k + K, interior_step(k + 1));
            __builtin_amdgcn_sched_barrier(0);
        };
#pragma unroll
        for (int t = 1; t <= K; ++t) {
            if constexpr (CAPS) {
                if (form == 0) by_caps([&](auto caps) __attribute__((always_inline)) { phase_b_fast(std::false_type{}, caps, t); });
                else if (form == 1) by_caps([&](auto caps) __attribute__((always_inline)) { phase_b_fast(std::true_type{}, caps, t); });
                else phase_b_general(t);
            } else {
                if (form == 0) phase_b_fast(std::false_type{}, caps_all{}, t);
                else if (form == 1) phase_b_fast(std::true_type{}, caps_all{}, t);
                else phase_b_general(t);
            }
            issue(t - 1, K);
        }
        if constexpr (!B1) __syncthreads();
    };

    load_slice(0, 1, z0 - K, z0 - K - 1, false);
    __syncthreads();

    for (int k = z0 - 2 * K; k < z1; ++k) step(k);
}

// WPE: waves per SIMD the register budget is set for (12-wave workgroups: 3, one per CU; 6- and 8-wave workgroups: 3 / 4,
// two per CU, so that one workgroup's waves run while the other's wait at a barrier)
template <int K, int NW, int LPW, int WPE, int TR>
__global__ __attribute__((amdgpu_flat_work_group_size(NW * WAVE, NW * WAVE), amdgpu_waves_per_eu(WPE, WPE)))
void sdia_jacobikc(JK3Args a) {
    jk3_body<K, NW, LPW, TR>(a);
}

// (its own symbol for the finest level, so that profiler summaries list the dominant launches apart)
template <int K, int NW, int LPW, int WPE, int TR>
__global__ __attribute__((amdgpu_flat_work_group_size(NW * WAVE, NW * WAVE), amdgpu_waves_per_eu(WPE, WPE)))
void sdia_jacobikc_finest(JK3Args a) {
    jk3_body<K, NW, LPW, TR>(a);
}

// tile shape 8: one barrier per step (see jk3b_lds_doubles)
template <int K, int NW, int LPW, int WPE, int TR>
__global__ __attribute__((amdgpu_flat_work_group_size(NW * WAVE, NW * WAVE), amdgpu_waves_per_eu(WPE, WPE)))
void sdia_jacobikc_b1(JK3Args a) {
    jk3_body<K, NW, LPW, TR, false, true>(a);
}
template <int K, int NW, int LPW, int WPE, int TR>
__global__ __attribute__((amdgpu_flat_work_group_size(NW * WAVE, NW * WAVE), amdgpu_waves_per_eu(WPE, WPE)))
void sdia_jacobikc_finest_b1(JK3Args a) {
    jk3_body<K, NW, LPW, TR, false, true>(a);
}

// (levels with rows of class CLS_ESCAPE)
template <int K, int NW, int LPW, int WPE, int TR>
__global__ __attribute__((amdgpu_flat_work_group_size(NW * WAVE, NW * WAVE), amdgpu_waves_per_eu(WPE, WPE)))
void sdia_jacobikc_escape(JK3Args a) {
    jk3_body<K, NW, LPW, TR, true>(a);
}

// Rim waves (tile shape 9).  On the 64 x 32 tiles of shape 8 the lines 0 .. K-2 and EY-K+1 .. EY-1 carry the halo levels (caps
// 1 .. K-1, jk3_caps) and store nothing; two waves on either side own them, two lines each, and compute 3 and 7 line-levels a
// step (K = 5) where the other twelve compute 10 -- the step is as long as its full-cap waves make it, so two waves' worth of
// its time buys no result line.  Here ONE wave on either side owns all K - 1 rim lines (caps 1 + 2 + .. + K-1 = K (K-1) / 2
// line-levels: as many as the K line-levels of each of an interior wave's two lines when K = 5), and the fourteen waves between
// them own two full-cap lines each: EY = 2 (K - 1) + 28 lines, of which HY = 28 get all K sweeps.  Everything else is shape
// 8's: one barrier per step, level 0 in registers, the images double-buffered by parity, DPP neighbours, march plans.
// The line map: which lines a wave owns.  The march, the plan (jk3_plan_rim) and the host's tile counts all read it.
template <int K> struct jk3_rim_map {
    static constexpr int NW = 16, RL = K - 1;               // waves; lines of a rim wave
    static constexpr int NLM = RL > 2 ? RL : 2;             // the most lines a wave owns
    static constexpr int EY = 2 * RL + 2 * (NW - 2), HY = EY - 2 * K + 2, WI = 64 - 2 * K;
    static constexpr int first(int wave) { return wave == 0 ? 0 : wave == NW - 1 ? EY - RL : RL + 2 * (wave - 1); }
    static constexpr int lines(int wave) { return wave == 0 || wave == NW - 1 ? RL : 2; }
};
// ... and the kinds of wave: 0 = two lines of cap K, 1 = wave 0 (caps 1 .. K-1), 2 = the last wave (caps K-1 .. 1).  A kind is
// a type: the march runs one plane loop per kind, chosen once per wave, so that the registers of a loop are those of its kind
// (K (K-1) / 2 partial sums and ring values of f on a rim wave, not K for each of its K - 1 lines).
template <int K, int KIND> struct jk3_rim_kind {
    static constexpr int NL = KIND == 0 ? 2 : K - 1;
    static constexpr int cap(int l) { return KIND == 0 ? K : KIND == 1 ? l + 1 : K - 1 - l; }
};

template <int K, int TR> constexpr size_t jk3r_lds_bytes() {
    return sizeof(double) * (TR * CLS_W + (size_t)(2 * (K - 1) * (jk3_rim_map<K>::EY + 1) + 1) * 64);
}

// EARLY ("fuse_k_load_early"): false = the loads of the next plane go out in K slices, one behind each piece of phase B; true =
// each goes out as soon as its register is free -- f and, off plan, the classes behind the ring shift in front of the barrier,
// x of the wave's lines and of the lines below / above them in one group behind piece 1 of phase B.
template <int K, int TR, bool EARLY = false>
__device__ __forceinline__ void jk3_rim_body(const JK3Args& a) {
    using MAP = jk3_rim_map<K>;
    constexpr int EX = 64, NW = MAP::NW, EY = MAP::EY, NCM = MAP::NLM, WI = MAP::WI, HY = MAP::HY;
    constexpr int IS = (EY + 1) * EX, PS = (K - 1) * IS;      // image stride and parity stride, in doubles (jk3b_lds_doubles)
    static_assert(CLS_W == 8, "table rows of eight doubles");
    static_assert(K >= 3 && NCM <= 4, "a wave's class bytes of a plane live in one register");
    static_assert(NCM * (K + 1) <= 64, "the fast-path flags live in one scalar register pair");
    static_assert(8 * ((K - 2) * IS + (NCM + 1) * EX) < 65536, "every LDS access of a step is `register + 16-bit immediate`");
    extern __shared__ double j2_smem[];
    double* const sT = j2_smem;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));

    unsigned id;
    {
        const unsigned b = blockIdx.x, xcd = b & 7u, j = b >> 3, ch = a.xcd_chunk;
        id = ((j / ch) * 8u + xcd) * ch + (j % ch);
    }
    if (id >= a.nitems) return;
    const unsigned ntile = (unsigned)(a.ntx * a.nty);
    const int nsa = (a.za1 - a.za0 + a.seglen - 1) / a.seglen;
    const int nsb = (a.zb1 - a.zb0 + a.seglen - 1) / a.seglen;
    const unsigned items_a = (unsigned)a.ta * (unsigned)(nsa + max(nsb, 0));
    unsigned tt;
    int z0, z1;
    if (id < items_a) {
        const int seg = (int)(id / (unsigned)a.ta);
        tt = id % (unsigned)a.ta;
        z0 = seg < nsa ? a.za0 + seg * a.seglen : a.zb0 + (seg - nsa) * a.seglen;
        z1 = min(seg < nsa ? a.za1 : a.zb1, z0 + a.seglen);
    } else {
        const unsigned j = id - items_a, tb = ntile - (unsigned)a.ta;
        tt = (unsigned)a.ta + j % tb;
        z0 = a.za0 + (int)(j / tb) * a.seglen_b;
        z1 = min(a.za1, z0 + a.seglen_b);
    }
    const int tiy = (int)(tt / (unsigned)a.ntx), tix = (int)(tt % (unsigned)a.ntx);
    if (z1 <= z0) return;
    const int tx0 = tix * WI - K, ty0 = tiy * HY - (K - 1);   // grid position of cell (0, 0)

    {
        const int nt = a.ncls * CLS_W;
        for (int i = threadIdx.x; i < nt; i += NW * WAVE) {
            double v = a.ctab[i];
            if ((i & (CLS_W - 1)) == CLS_W - 1) {
                const double d = a.ctab[i - 4];
                v = a.omega * (1.0 / (d != 0.0 ? d : 1.0));
            }
            sT[i] = v;
        }
        constexpr int NZ = (2 * (K - 1) * (EY + 1) + 1) * EX;
        for (int i = threadIdx.x; i < NZ; i += NW * WAVE) sT[TR * CLS_W + i] = 0.0;
    }
    const double m0 = a.cm[0], m1 = a.cm[1], m2 = a.cm[2], m3 = a.cm[3], m4 = a.cm[4], m5 = a.cm[5], m6 = a.cm[6];
    const double mcf = a.omega * (1.0 / (m3 != 0.0 ? m3 : 1.0));
    const int cmain = a.cmain;

    // cell l of this thread: ex = lane, ey = ey0 + l, l < the lines of the wave's kind (what is set up for the cells beyond
    // them, on the fourteen waves with two lines, is never used)
    const int ey0 = MAP::first(wave);
    const int wkind = wave == 0 ? 1 : wave == NW - 1 ? 2 : 0;
    int bcur = 0, bprev = 0;    // level 1 of the step's parity / of the step before, at the line below the wave's first (see jk3_body)
    // ... of parity 0; the one register the march keeps of the lane (the table and a line are multiples of 64 doubles: the
    // lane is its low six bits)
    int lbase = TR * CLS_W + ey0 * EX + lane;
    asm volatile("" : "+v"(lbase));
    auto limg = [&](int base, int t) -> double* { return j2_smem + base + (t - 1) * IS + EX; };
    unsigned inT = 0;           // bit l: this lane's cell l gets all K sweeps and lies on the grid
#pragma unroll
    for (int l = 0; l < NCM; ++l) {
        const int ey = ey0 + l;
        if (lane >= K && lane < EX - K && ey >= K - 1 && ey <= EY - K && tx0 + lane < a.nx && ty0 + ey < a.ny) inT |= 1u << l;
    }
    // the row of cell l in plane p exists  <=>  the level holds plane p + sh(l), sh = -1, 0, +1 (general form only: worked out
    // where it is used, from scalars and the lane, instead of living in a register through the march)
    auto shof = [&](int l) -> int {
        const int64_t r = (int64_t)(ty0 + ey0 + l) * a.nx + (tx0 + (lbase & 63));
        return r < 0 ? -1 : (r >= a.P ? 1 : 0);
    };

    const int bias = 2 * a.nx + K + 2;
    const int xcl = a.nx + 1 - tx0;
    unsigned eo[NCM];           // byte offsets of the cells' doubles (>> 3: of their class bytes)
#pragma unroll
    for (int l = 0; l < NCM; ++l) {
        eo[l] = jk3_cell_offset(ty0 + ey0 + l, lane, a.nx, a.ny, tx0, xcl, bias);
        asm volatile("" : "+v"(eo[l]));     // (one register per cell: left alone the compiler keeps the class byte's offset too)
    }
    // the lines below / above the wave's
    const unsigned eos = jk3_cell_offset(ty0 + ey0 - 1, lane, a.nx, a.ny, tx0, xcl, bias);
    const unsigned eon = jk3_cell_offset(ty0 + ey0 + MAP::lines(wave), lane, a.nx, a.ny, tx0, xcl, bias);
    const unsigned char* const clsb = jk3_class_base(a.cls, a.clead, bias);
    const double* const xb0 = a.x - bias;
    const double* const fb0 = a.f - bias;
    auto sbase = [](const void* p) -> gcptr_t {
        const unsigned long long u = (unsigned long long)p;
        const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u);
        const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
        return (gcptr_t)(((unsigned long long)hi << 32) | lo);
    };
    auto ldd = [](gcptr_t b, unsigned e8) -> double {
        asm volatile("" : "+v"(e8));
        return *(const __attribute__((address_space(1))) double*)(b + e8);
    };
    typedef unsigned int __attribute__((aligned(1))) u32_unaligned_t;
    auto ldc = [](gcptr_t b, unsigned e8) -> int {
        unsigned e = e8 >> 3;
        asm volatile("" : "+v"(e));
        return (int)*(const __attribute__((address_space(1))) u32_unaligned_t*)(b + e);
    };
    const int pmin = -a.plo - 1, pmax = a.nz + a.phi;

    // planned steps: see jk3_body
    int klo = 0x7fffffff, khi = 0x7fffffff, kform = 0;
    if (a.plan) {
        const int* const pw = a.plan + 4 * ((int)tt * NW + wave);
        const int top = a.nz - K - 1;
        const int lo0 = max(max(pw[0], 1), z0 - K), hi0 = min(pw[1] - K, top);
        const int lo1 = max(max(pw[2], 1), z0 - K), hi1 = min(pw[3] - K, top);
        const int n0 = min(hi0, z1) - lo0, n1 = min(hi1, z1) - lo1;
        if (n0 > 0 && n0 >= n1) {
            klo = __builtin_amdgcn_readfirstlane(lo0);
            khi = __builtin_amdgcn_readfirstlane(hi0);
        } else if (n1 > 0) {
            klo = __builtin_amdgcn_readfirstlane(lo1);
            khi = __builtin_amdgcn_readfirstlane(hi1);
            kform = 1;
        }
    }
    auto interior_step = [&](int k) -> bool { return k >= klo && k < khi; };

    // registers per cell: partial sums and f of the levels up to the line's cap; x (X: the plane that arrives, XP: the one
    // before), the class of the plane that arrives; per wave x of the lines below / above its lines
    double acc[K][NCM], fr[K][NCM], X[NCM], XP[NCM], hS = 0.0, hN = 0.0;
    int C[NCM];
    unsigned cw[K + 1];         // class bytes of the planes k .. k+K, a byte per cell
    unsigned long long fast = 0;        // wave-uniform; bit j*NL + l: all 64 cells l of plane k+j are of class cmain
#pragma unroll
    for (int l = 0; l < NCM; ++l) {
#pragma unroll
        for (int t = 0; t < K; ++t) acc[t][l] = fr[t][l] = 0.0;
        X[l] = XP[l] = 0.0;
        C[l] = 0;
    }
#pragma unroll
    for (int j = 0; j <= K; ++j) cw[j] = 0u;

    // slice i of n of the loads of a step (see jk3_body): x and, off plan, the classes of `plane`, f of `fplane`
    auto load_slice = [&](auto kind, const int i, const int n, const int plane, const int fplane, const bool noc) __attribute__((always_inline)) {
        constexpr int NL = decltype(kind)::NL;
        const int64_t o = (int64_t)min(max(plane, pmin), pmax) * a.P;
        const gcptr_t cb = sbase(clsb + o);
        const gcptr_t xb = sbase(xb0 + o);
        const gcptr_t fb = sbase(fb0 + (int64_t)min(max(fplane, pmin), pmax) * a.P);
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if ((l * n) / NL != i) continue;
            X[l] = ldd(xb, eo[l]);
            if (!noc) C[l] = ldc(cb, eo[l]);
            fr[K - 1][l] = ldd(fb, eo[l]);
        }
        if (i == n - 1) { hS = ldd(xb, eos); hN = ldd(xb, eon); }
    };
    // ... the same loads by the register they need (EARLY): f of `fplane` and, off plan, the classes of `plane`; x of `plane`
    auto load_f_classes = [&](auto kind, const int plane, const int fplane, const bool noc) __attribute__((always_inline)) {
        constexpr int NL = decltype(kind)::NL;
        const gcptr_t cb = sbase(clsb + (int64_t)min(max(plane, pmin), pmax) * a.P);
        const gcptr_t fb = sbase(fb0 + (int64_t)min(max(fplane, pmin), pmax) * a.P);
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (!noc) C[l] = ldc(cb, eo[l]);
            fr[K - 1][l] = ldd(fb, eo[l]);
        }
    };
    auto load_x = [&](auto kind, const int plane) __attribute__((always_inline)) {
        constexpr int NL = decltype(kind)::NL;
        const gcptr_t xb = sbase(xb0 + (int64_t)min(max(plane, pmin), pmax) * a.P);
#pragma unroll
        for (int l = 0; l < NL; ++l) X[l] = ldd(xb, eo[l]);
        hS = ldd(xb, eos);
        hN = ldd(xb, eon);
    };
    auto cls_of = [&](int j, int l) -> int { return (int)((cw[j] >> (8 * l)) & 255u); };
    auto cls_now = [&](int j, int l) -> int {       // (general form: extracted anew at every use)
        unsigned w = cw[j];
        asm volatile("" : "+v"(w));
        return (int)((w >> (8 * l)) & 255u);
    };
    int k_plane = 0;
    bool k_store = false;
    __attribute__((address_space(1))) char* k_out = nullptr;
    auto store = [&](int l, double v) {
        unsigned e8 = eo[l];
        asm volatile("" : "+v"(e8));
        if (a.nt_store) __builtin_nontemporal_store(v, (__attribute__((address_space(1))) double*)(k_out + e8));
        else *(__attribute__((address_space(1))) double*)(k_out + e8) = v;
    };
    int lo_t[K + 1], n_t[K + 1];
#pragma unroll
    for (int t = 1; t <= K; ++t) {
        lo_t[t] = -min(a.plo, K - t);
        n_t[t] = a.nz + min(a.phi, K - t) - lo_t[t];
    }

    // ---- the three forms of a step, as in jk3_body (B1), over the lines and caps of the wave's kind ----
    auto phase_a_fast = [&](auto col_tag, auto kind) __attribute__((always_inline)) {
        constexpr bool COL = decltype(col_tag)::value;
        using KD = decltype(kind);
#pragma unroll
        for (int l = 0; l < KD::NL; ++l) {
            const int iw = l * EX;
            double k0 = m0, k6 = m6, kcf = mcf;
            if constexpr (COL) {
                const dvec2_t* const tr = reinterpret_cast<const dvec2_t*>(sT + CLS_W * cls_of(0, l));
                const dvec2_t t01 = tr[0], t67 = tr[3];
                k0 = t01.x; k6 = t67.x; kcf = t67.y;
            }
            double nw = X[l];
#pragma unroll
            for (int t = 1; t <= K; ++t) {
                if (t > KD::cap(l)) {           // (above the line's cap: its last level goes to the image, nothing else)
                    if (t == KD::cap(l) + 1) limg(bcur, t - 1)[iw] = nw;
                    continue;
                }
                const double wd = t == 1 ? XP[l] : limg(bprev, t - 1)[iw];
                const double s = fma(k6, nw, acc[t - 1][l]);      // +P
                const double o = wd + kcf * (fr[K - t][l] - s);
                acc[t - 1][l] = fma(k0, wd, 0.0);                 // -P of the plane above
                if (t > 1) limg(bcur, t - 1)[iw] = nw;
                nw = o;
            }
            if (KD::cap(l) == K && k_store && (inT >> l & 1u)) store(l, nw);
        }
    };
    auto phase_b_fast = [&](auto col_tag, auto kind, const int t) __attribute__((always_inline)) {
        constexpr bool COL = decltype(col_tag)::value;
        using KD = decltype(kind);
        constexpr int NL = KD::NL;
        const double* const img = limg(bcur, t > 1 ? t - 1 : 1);
        double v[NL], ys, yn;
        if (t == 1) {           // (level 0: registers)
            ys = hS;
#pragma unroll
            for (int l = 0; l < NL; ++l) v[l] = X[l];
            yn = hN;
        } else {
            ys = img[-EX];
#pragma unroll
            for (int l = 0; l < NL; ++l) v[l] = img[l * EX];
            yn = img[NL * EX];
        }
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (t > KD::cap(l)) continue;       // (the line has no level t: the reads only it needed go with it)
            const double yw = jk3_from_west(v[l]), ye = jk3_from_east(v[l]);
            double k1 = m1, k2 = m2, k3 = m3, k4 = m4, k5 = m5;
            if constexpr (COL) {
                const dvec2_t* const tr = reinterpret_cast<const dvec2_t*>(sT + CLS_W * cls_of(0, l));
                const dvec2_t t01 = tr[0], t23 = tr[1], t45 = tr[2];
                k1 = t01.y; k2 = t23.x; k3 = t23.y; k4 = t45.x; k5 = t45.y;
            }
            double s = acc[t - 1][l];
            s = fma(k1, l > 0 ? v[l > 0 ? l - 1 : 0] : ys, s);
            s = fma(k2, yw, s);
            s = fma(k3, v[l], s);
            s = fma(k4, ye, s);
            s = fma(k5, l + 1 < NL ? v[l + 1 < NL ? l + 1 : l] : yn, s);
            acc[t - 1][l] = s;
        }
    };
    // General form: every cell's entries from the class table, rows outside the level masked to zero.
    auto phase_a_general = [&](auto kind) __attribute__((always_inline)) {
        using KD = decltype(kind);
#pragma unroll
        for (int l = 0; l < KD::NL; ++l) {
            const int iw = l * EX;
            double nw = X[l];
            int pc = k_plane + shof(l);
            asm volatile("" : "+v"(pc));
#pragma unroll
            for (int t = 1; t <= K; ++t) {
                const int j = K - t;                                  // ring index of the plane being finished
                double* const img = limg(bcur, t > 1 ? t - 1 : 1);
                if (t > KD::cap(l)) {
                    if (t == KD::cap(l) + 1) img[iw] = nw;
                    continue;
                }
                const double wd = t == 1 ? XP[l] : limg(bprev, t - 1)[iw];
                const dvec2_t t67 = reinterpret_cast<const dvec2_t*>(sT + CLS_W * cls_now(j, l))[3];
                const dvec2_t t01 = reinterpret_cast<const dvec2_t*>(sT + CLS_W * cls_now(j + 1, l))[0];
                const double s = fma(t67.x, nw, acc[t - 1][l]);
                double o = wd + t67.y * (fr[j][l] - s);
                o = (unsigned)(pc + j - lo_t[t]) < (unsigned)n_t[t] ? o : 0.0;
                acc[t - 1][l] = fma(t01.x, wd, 0.0);
                if (t > 1) img[iw] = nw;
                nw = o;
                __builtin_amdgcn_sched_barrier(0);      // (rare path: one cell and level at a time)
            }
            if (KD::cap(l) == K && k_store && (inT >> l & 1u)) store(l, nw);
        }
    };
    auto phase_b_general = [&](auto kind, const int t) __attribute__((always_inline)) {
        using KD = decltype(kind);
        constexpr int NL = KD::NL;
        double x0w[NL], x0e[NL];        // (level 0: the -1 / +1 neighbours through DPP, all cells' before the first use)
        if (t == 1) {
#pragma unroll
            for (int l = 0; l < NL; ++l) { x0w[l] = jk3_from_west(X[l]); x0e[l] = jk3_from_east(X[l]); }
        }
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (t > KD::cap(l)) continue;
            const int iw = l * EX;
            double ys, yw, yd, ye, yn;
            if (t == 1) {
                ys = l > 0 ? X[l > 0 ? l - 1 : l] : hS;
                yw = x0w[l]; yd = X[l]; ye = x0e[l];
                yn = l + 1 < NL ? X[l + 1 < NL ? l + 1 : l] : hN;
            } else {
                const double* const img = limg(bcur, t - 1);
                ys = img[iw - EX]; yw = img[iw - 1]; yd = img[iw]; ye = img[iw + 1]; yn = img[iw + EX];
            }
            const dvec2_t* const tr = reinterpret_cast<const dvec2_t*>(sT + CLS_W * cls_now(K - t, l));
            const dvec2_t t01 = tr[0], t23 = tr[1], t45 = tr[2];
            double s = acc[t - 1][l];
            s = fma(t01.y, ys, s);
            s = fma(t23.x, yw, s);
            s = fma(t23.y, yd, s);
            s = fma(t45.x, ye, s);
            s = fma(t45.y, yn, s);
            acc[t - 1][l] = s;
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // One step (jk3_body, B1): `X, C, hS, hN` hold plane k+K; the loads of plane k+K+1 go out between the pieces of phase B.
    auto step = [&](auto kind, const int k) __attribute__((always_inline)) {
        using KD = decltype(kind);
        constexpr int NL = KD::NL;
        constexpr unsigned long long ALLFAST = (1ull << (NL * (K + 1))) - 1ull;
        k_plane = k; k_store = k >= z0;
        bcur = lbase + (k & 1) * PS;
        bprev = lbase + ((k + 1) & 1) * PS;
        asm volatile("" : "+v"(bcur));
        asm volatile("" : "+v"(bprev));
        {
            const unsigned long long u = (unsigned long long)(a.out - bias + (int64_t)k * a.P);
            const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u);
            const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
            k_out = (__attribute__((address_space(1))) char*)(((unsigned long long)hi << 32) | lo);
        }
        // ---- the plane k+K has arrived: its classes join the ring (the loaded values are first touched here) ----
#pragma unroll
        for (int l = 0; l < NL; ++l) asm volatile("" : "+v"(X[l]));
        const bool interior = interior_step(k);     // (wave-uniform, from scalar registers)
        if (k == khi) {         // the first step behind the planned ones: the ring as the unplanned path would hold it
            unsigned m = 0;
#pragma unroll
            for (int l = 0; l < NL; ++l)
                if (__builtin_amdgcn_readfirstlane((int)(__ballot(cls_of(0, l) != cmain) == 0ull))) m |= 1u << l;
            fast = 0;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                fast |= (unsigned long long)m << (j * NL);
                cw[j] = cw[0];
            }
        }
        int form = kform;
        if (!interior) {
            unsigned m = 0;
            cw[K] = 0u;
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                asm volatile("" : "+v"(C[l]));
                C[l] &= 255;
                cw[K] |= (unsigned)C[l] << (8 * l);
                if (__builtin_amdgcn_readfirstlane((int)(__ballot(C[l] != cmain) == 0ull))) m |= 1u << l;
            }
            fast |= (unsigned long long)m << (K * NL);
            // which form (jk3_body): 0 = interior stencil in all the wave's cells of the planes k .. k+K, 1 = every cell's class
            // the same in those planes -- both only where every row the step touches exists --, 2 = general
            form = 2;
            if ((a.plo > 0 || k >= 1) && (a.phi > 0 || k + K + 1 < a.nz)) {
                if (fast == ALLFAST) {
                    form = 0;
                } else {
                    bool same = true;
#pragma unroll
                    for (int j = 1; j <= K; ++j) same = same && cw[j] == cw[0];
                    if (__builtin_amdgcn_readfirstlane((int)(__ballot(!same) == 0ull))) form = 1;
                }
            }
        }
        if (a.force_form >= 0) form = a.force_form;
        // ---- phase A: finish plane k+K-t of level t, t = 1 .. cap; start the plane above it ----
        if (form == 0) phase_a_fast(std::false_type{}, kind);
        else if (form == 1) phase_a_fast(std::true_type{}, kind);
        else phase_a_general(kind);
#pragma unroll
        for (int l = 0; l < NL; ++l) XP[l] = X[l];
        // ---- the rings move on; the next loads go out ----
#pragma unroll
        for (int l = 0; l < NL; ++l) {
#pragma unroll
            for (int j = 0; j + 1 < K; ++j) fr[j][l] = fr[j + 1][l];
            if (KD::cap(l) >= 2) asm volatile("" : "+v"(fr[K - 2][l]));
        }
        if (!interior) {
#pragma unroll
            for (int j = 0; j < K; ++j) cw[j] = cw[j + 1];
            fast >>= NL;
        }
        if constexpr (EARLY) {  // (f's newest ring slot and the class registers are free from here on)
            __builtin_amdgcn_sched_barrier(0);
            load_f_classes(kind, k + K + 1, k + K, interior_step(k + 1));
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        // ---- phase B: the in-plane terms of the planes started above; the next loads go out between its pieces (EARLY: x
        // behind the first, which is the last to read plane k+K's) ----
#pragma unroll
        for (int t = 1; t <= K; ++t) {
            if (form == 0) phase_b_fast(std::false_type{}, kind, t);
            else if (form == 1) phase_b_fast(std::true_type{}, kind, t);
            else phase_b_general(kind, t);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (!EARLY) load_slice(kind, t - 1, K, k + K + 1, k + K, interior_step(k + 1));
            else if (t == 1) load_x(kind, k + K + 1);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // one plane loop per kind of wave; every wave passes the same barriers, one before the first step and one in each
    auto march = [&](auto kind) __attribute__((always_inline)) {
        load_slice(kind, 0, 1, z0 - K, z0 - K - 1, false);
        __syncthreads();
        for (int k = z0 - 2 * K; k < z1; ++k) step(kind, k);
    };
    if (wkind == 0) march(jk3_rim_kind<K, 0>{});
    else if (wkind == 1) march(jk3_rim_kind<K, 1>{});
    else march(jk3_rim_kind<K, 2>{});
}

// tile shape 9: rim waves (64 x 36 tiles for K = 5, 28 result lines)
template <int K, int TR>
__global__ __attribute__((amdgpu_flat_work_group_size(16 * WAVE, 16 * WAVE), amdgpu_waves_per_eu(4, 4)))
void sdia_jacobikc_rim(JK3Args a) {
    jk3_rim_body<K, TR>(a);
}
template <int K, int TR>
__global__ __attribute__((amdgpu_flat_work_group_size(16 * WAVE, 16 * WAVE), amdgpu_waves_per_eu(4, 4)))
void sdia_jacobikc_finest_rim(JK3Args a) {
    jk3_rim_body<K, TR>(a);
}
// ... with the next plane's loads issued as early as their registers are free (jk3_rim_body, EARLY)
template <int K, int TR>
__global__ __attribute__((amdgpu_flat_work_group_size(16 * WAVE, 16 * WAVE), amdgpu_waves_per_eu(4, 4)))
void sdia_jacobikc_rim_early(JK3Args a) {
    jk3_rim_body<K, TR, true>(a);
}
template <int K, int TR>
__global__ __attribute__((amdgpu_flat_work_group_size(16 * WAVE, 16 * WAVE), amdgpu_waves_per_eu(4, 4)))
void sdia_jacobikc_finest_rim_early(JK3Args a) {
    jk3_rim_body<K, TR, true>(a);
}

// The most pool rows any tile of the march <K, NW, LPW> takes within K + 2 consecutive planes: one workgroup per tile
// counts the cells of class CLS_ESCAPE plane by plane -- the tile's cells at the very rows the march reads their classes
// from, but for the clamped ones (`standin` there) -- and keeps the largest sum over a window of planes.
struct JK3WindowArgs {
    const unsigned char* cls;
    int64_t clead, P;
    int nx, ny, nz, ntx, nty;
    unsigned* most;
};

template <int K, int NW, int LPW>
__global__ __launch_bounds__(256) void jk3_escape_window(JK3WindowArgs a) {
    constexpr int EX = 64, EY = NW * LPW, WI = EX - 2 * K, HY = EY - 2 * K + 2, W = K + 2;
    __shared__ unsigned s_ring[W], s_plane;
    const int tiy = (int)(blockIdx.x / (unsigned)a.ntx), tix = (int)(blockIdx.x % (unsigned)a.ntx);
    const int tx0 = tix * WI - K, ty0 = tiy * HY - (K - 1), xcl = a.nx + 1 - tx0;
    unsigned win = 0u, best = 0u;
    for (int p = 0; p < a.nz; ++p) {
        if (threadIdx.x == 0) s_plane = 0u;
        __syncthreads();
        unsigned n = 0u;
        for (int i = threadIdx.x; i < EX * EY; i += 256) {
            const int ex = i % EX, line = ty0 + i / EX;
            if (ex > xcl || line < -2 || line > a.ny + 1) continue;
            const int64_t row = (int64_t)p * a.P + (int64_t)line * a.nx + tx0 + ex;
            n += a.cls[a.clead + row] == CLS_ESCAPE ? 1u : 0u;
        }
        if (n) atomicAdd(&s_plane, n);
        __syncthreads();
        if (threadIdx.x == 0) {
            win += s_plane - (p >= W ? s_ring[p % W] : 0u);
            s_ring[p % W] = s_plane;
            best = max(best, win);
        }
    }
    if (threadIdx.x == 0 && best) atomicMax(a.most, best);
}

// The march plan of a whole level for the tiles of the march <K, NW, LPW>: one workgroup per tile, shaped like the
// march's, walks the planes; every wave looks at the class bytes the march's wave would load for the plane (the same
// offsets, jk3_cell_offset / jk3_class_base) and keeps two runs of consecutive planes, the longest of their kind and the
// first of equally long ones (r0 = r1 = 0: none):
//   [p0, p1)  all of them are `cmain`                                   (form 0 of the march's steps)
//   [q0, q1)  every one of them is what it was in the plane before      (form 1)
// plan[4 * (tile * NW + wave) + 0 .. 3] = p0, p1, q0, q1.  The classes belong to the matrix: built once per level, tile
// shape and K, dropped when the level's classes change.
struct JK3PlanArgs {
    const unsigned char* cls;
    int64_t clead, P;
    int nx, ny, nz, ntx, nty, cmain;
    int* plan;
};

// (the walk over the planes: `eo` the wave's cells as the march addresses them, `pw` where its four ints go)
template <int NC>
__device__ __forceinline__ void jk3_plan_walk(const JK3PlanArgs& a, const unsigned char* const clsb, const unsigned (&eo)[NC], int* const pw) {
    constexpr int U = 4;        // planes whose bytes are in flight together
    const int lane = threadIdx.x & 63;
    int p0 = 0, p1 = 0, prun = 0;       // the best run of cmain planes; where the present one starts
    int q0 = 0, q1 = 0, qrun = 0;       // ... of planes with the classes of the plane before
    int prev[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) prev[c] = -1;
    for (int pb = 0; pb < a.nz; pb += U) {
        int cl[U][NC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned char* const cb = clsb + (int64_t)min(pb + u, a.nz - 1) * a.P;
#pragma unroll
            for (int c = 0; c < NC; ++c) cl[u][c] = cb[eo[c] >> 3];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = pb + u;
            if (p >= a.nz) break;
            bool all = true, same = true;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                all = all && cl[u][c] == a.cmain;
                same = same && cl[u][c] == prev[c];
                prev[c] = cl[u][c];
            }
            if (__ballot(!all) != 0ull) {
                if (p - prun > p1 - p0) { p0 = prun; p1 = p; }
                prun = p + 1;
            }
            if (__ballot(!same) != 0ull) {          // (the plane starts a run of its own)
                if (p - qrun > q1 - q0) { q0 = qrun; q1 = p; }
                qrun = p;
            }
        }
    }
    if (a.nz - prun > p1 - p0) { p0 = prun; p1 = a.nz; }
    if (a.nz - qrun > q1 - q0) { q0 = qrun; q1 = a.nz; }
    if (lane == 0) { pw[0] = p0; pw[1] = p1; pw[2] = q0; pw[3] = q1; }
}

template <int K, int NW, int LPW>
__global__ __launch_bounds__(NW * WAVE) void jk3_plan(JK3PlanArgs a) {
    constexpr int EX = 64, EY = NW * LPW, NC = LPW, WI = EX - 2 * K, HY = EY - 2 * K + 2;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned tt = blockIdx.x;
    const int tiy = (int)(tt / (unsigned)a.ntx), tix = (int)(tt % (unsigned)a.ntx);
    const int tx0 = tix * WI - K, ty0 = tiy * HY - (K - 1);
    const int ey0 = wave * LPW, bias = 2 * a.nx + K + 2, xcl = a.nx + 1 - tx0;
    unsigned eo[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) eo[c] = jk3_cell_offset(ty0 + ey0 + c, lane, a.nx, a.ny, tx0, xcl, bias);
    jk3_plan_walk<NC>(a, jk3_class_base(a.cls, a.clead, bias), eo, a.plan + 4 * ((int)tt * NW + wave));
}

// ... for the tiles of shape 9 (jk3_rim_map): a wave with fewer lines than the longest looks at its last line again
template <int K>
__global__ __launch_bounds__(16 * WAVE) void jk3_plan_rim(JK3PlanArgs a) {
    using MAP = jk3_rim_map<K>;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned tt = blockIdx.x;
    const int tiy = (int)(tt / (unsigned)a.ntx), tix = (int)(tt % (unsigned)a.ntx);
    const int tx0 = tix * MAP::WI - K, ty0 = tiy * MAP::HY - (K - 1);
    const int ey0 = MAP::first(wave), nl = MAP::lines(wave), bias = 2 * a.nx + K + 2, xcl = a.nx + 1 - tx0;
    unsigned eo[MAP::NLM];
#pragma unroll
    for (int l = 0; l < MAP::NLM; ++l) eo[l] = jk3_cell_offset(ty0 + ey0 + min(l, nl - 1), lane, a.nx, a.ny, tx0, xcl, bias);
    jk3_plan_walk<MAP::NLM>(a, jk3_class_base(a.cls, a.clead, bias), eo, a.plan + 4 * ((int)tt * MAP::NW + wave));
}

}  // namespace mgk
