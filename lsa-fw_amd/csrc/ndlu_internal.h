// Nested-dissection multifrontal LU on the device: what ndlu.hip (set-up, cache, C-ABI), ndlu_factor.hip (numeric
// factorisation) and ndlu_sweeps.hip (solves) share -- device records, the host tables of a factorisation, constants.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <new>
#include <string>

#include "lsa_internal.h"
#include "nd_internal.h"

int k_allgather_inplace(lsa_ctx* ctx, void* vec, size_t bytes_per_rank);  // comm.hip

constexpr int kRT = 32;      // front rows per solve tile
constexpr int kSweepWide = 512;  // upward 8-row tiles (64 lanes per row pair) only on levels with a pivot block at least this wide (nd_setup_levels)
constexpr int kCH = 1024;    // vector entries staged in LDS per pass of a solve tile
constexpr int kGT = 64;      // GEMM tile edge
constexpr int kNB = 32;      // pivot columns per block of the Gauss-Jordan inversion (ndlu_factor.hip)
constexpr int kSB = 128;     // ... per super-block of the tournament path (nd_gj_update_kernel)
constexpr int kTRmin = 256;  // tournament pivoting, smallest first-round chunk: sizes the candidate buffers
constexpr int kNdBatchMax = 16;  // most problems of one batched solve (lsa_ndlu_solve_batch): the capacity of NdSweepPtrs there
static_assert(kNdBatchMax == kKrylovGroupMax, "a lockstep round hands all its problems to one batched sweep");
constexpr int kMCH = 256;        // vector entries per column staged in LDS per pass of a multi-column solve tile (ndlu_multi.hip)
constexpr int kNdMultiMax = 8;   // most columns of one pass of lsa_ndlu_solve_multi (real vectors; complex ones: 4 -- nd_multi_cap): 16 KB of LDS (transposed: 32 KB)

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline size_t esize(int dtype) { return dtype == LSA_C128 ? 16 : 8; }

struct NdNodeDev {
    int64_t front_off;  // scalars into the working arena (f x f, row-major) while the node's chunk is being factored
    int64_t lfac_off;   // packed factors: [F11^-1; -F21 F11^-1], f x m row-major
    int64_t ufac_off;   // packed factors: F11^-1 F12, m x b row-major
    int64_t upd_off;    // the node's update matrix (b x b, row-major) in the update arena
    int64_t u_off;      // into the update-vector / boundary-vector buffers (b entries)
    int64_t ge_off;     // into gell (nchild * f entries)
    int64_t acc_off;    // upward sweep: this node's slot rows (nchild x f entries, row c written by child c), or -1: pull through gell
    int64_t pacc_off;   // upward sweep: this node's slot row in its parent's accumulation buffer, or -1: writes its update vector
    int32_t idx_off;    // into idx (f entries)
    int32_t cmap_off;   // into cmap (b entries)
    int32_t piv_off;    // into ipiv / rowq (m entries)
    int32_t own0;       // first own unknown when the vectors are in elimination order
    int32_t m, f, parent;
    int32_t nchild;     // rows of the node's gather table
    // distributed top nodes (NdSymbolic: kind 4): this rank's slice of the boundary rows / of the own rows of U.  Everywhere else
    // brow0 = 0, brow = f - m, orow0 = 0, orows = m.  The working front of a node is (m + brow) x f, its packed L (m + brow) x m,
    // its packed U orows x (f - m), its update matrix brow x (f - m).
    int32_t brow0, brow, orow0, orows;
    int32_t flags;      // bit 0: distributed node (its downward pushes are done by nd_dist_unpack_kernel, after the exchange of its own rows)
    int32_t pad0;
    int64_t xg_base, xg_stride;  // distributed node: own row j lies at xg_base + (j / s) * xg_stride + j % s of the own-row exchange buffer, s = ceil(m / ranks)
    int64_t inv_off;    // distributed node: the whole inverse of its pivot block in the working arena while the node is factored (-1: the
                        // first m rows of the packed L are the inverse)
};
static_assert(sizeof(NdNodeDev) == 144, "node record layout");

// what the sweeps read of a node (in level order: one record per workgroup and launch, loaded first thing -- kept at 96 bytes)
struct NdSweepNode {
    int64_t lfac_off, ufac_off, u_off, ge_off, acc_off, pacc_off;
    int32_t idx_off, cmap_off, own0, m, f, nchild;
    int32_t brow0, brow, orow0, orows, flags, pad0;
    NdSweepNode() = default;
    explicit NdSweepNode(const NdNodeDev& n)
        : lfac_off(n.lfac_off), ufac_off(n.ufac_off), u_off(n.u_off), ge_off(n.ge_off), acc_off(n.acc_off), pacc_off(n.pacc_off), idx_off(n.idx_off),
          cmap_off(n.cmap_off), own0(n.own0), m(n.m), f(n.f), nchild(n.nchild), brow0(n.brow0), brow(n.brow), orow0(n.orow0), orows(n.orows),
          flags(n.flags), pad0(0) {}
};
static_assert(sizeof(NdSweepNode) == 96, "sweep record layout");

struct TileList {
    int64_t off = 0;  // pairs of int32 into the tile buffer
    int32_t count = 0;
};

// factorisation work unit: nodes of ONE tree level whose working fronts share the arena
struct NdChunk {
    int32_t node_begin = 0, node_count = 0, max_m = 0, max_f = 0;  // range of the chunk-ordered node list (own size descending)
    std::vector<int32_t> sorted_m;
    int64_t work_entries = 0;             // sum of f^2: scalars of the arena this chunk uses
    int64_t asm_begin = 0, asm_count = 0;  // its range of the assembly lists
    TileList unperm, gemm[3], save;
    std::vector<TileList> ext;  // one per child rank
    bool exchange_before = false;  // subtree-parallel: the ranks' subtree-root update matrices are all-gathered before this chunk
    // distributed top nodes in this chunk: their children's update matrices arrive in row chunks through the staging buffer, one
    // in-place all-gather per step; slot r of a step holds rows [row0, row0 + nrows) of child `child` (a node id; nrows = 0: empty)
    struct XPiece {
        int32_t child = -1, row0 = 0, nrows = 0;
    };
    std::vector<std::vector<XPiece>> xsteps;  // [step][rank]
};

// one launch of each sweep: the nodes of a tree level
struct NdLevel {
    int32_t node_begin = 0, node_count = 0, max_m = 0, max_f = 0;
    int32_t fwd_tiles = 0, bwd_tiles = 0;  // grid.y of the sweep kernels: tiles of the tallest node (0 = nothing to do)
    int32_t sweep_rows = 32;               // rows per upward-sweep tile: 32; 8 on levels with few tiles and wide pivot blocks; 128 on thin levels
    int32_t bwd_rows = 32;                 // rows per downward-sweep tile: 32; 8 on levels with few tiles
    // distributed top nodes of the level: their range of the list d_dist_nodes, the level's exchange regions (entries per rank)
    int32_t dist_begin = 0, dist_count = 0, dist_children = 0, dist_rows = 0;  // ... most children / most entries (own rows, a child's boundary) of one of them
    int64_t ux_base = 0, ux_slot = 0, xg_base = 0, xg_slot = 0;
};

// ---- the top of the forest as ONE assembled inverse.  The root R (no boundary) and its children c, when they are the two
// highest levels, are three dependent launches that each do almost nothing: children upward, root, children downward.  With
//     v_c = rhs[own_c] + (what c's children pushed onto c's own positions)
//     z_R = rhs[own_R] + sum over c of (what c's children pushed onto c's boundary positions, scattered by cmap_c)
// those three steps are [x_c...; x_R] = T [v_c...; z_R] with the dense s x s matrix (s = m_R + sum m_c)
//     T[R, R] = inv_R                    T[R, c] =  inv_R[:, cmap_c] s1_c            (s1_c = -F21 inv_c: boundary rows of L_c)
//     T[c, R] = -U_c inv_R[cmap_c, :]    T[c, d] = [c == d] inv_c + T[c, R][:, cmap_d] s1_d
// i.e. the exact inverse of the top Schur complement, ASSEMBLED from blocks the factorisation of the unmerged forest leaves
// (nd_top_gemm_kernel, two launches per factorisation) instead of being eliminated as one wide pivot block.  One launch
// (nd_top_kernel) then replaces the three; the transposed sweeps keep reading the unmerged blocks.
constexpr int kTopChildren = 8;  // most children of the root the merged top takes
struct NdTopNode {
    int64_t acc_off, ge_off;  // the node's slot rows (what ITS children pushed) and gather rows
    int32_t own0, m, f, nchild;
    int32_t off, pad0;        // its first unknown in the order of the top: children in rank order, then the root
};
struct NdTop {
    int32_t s, nchild;
    NdTopNode node[kTopChildren + 1];  // the root's children, then the root
};

// one product of the assembly: C = D + sign * A B over tiles of 32 x 32, with A's columns or B's rows picked through a
// boundary map (cmap of a child: positions in the root's front)
struct NdTopJob {
    int64_t a_off, b_off, c_off, d_off;  // A in lfac / ufac / T (a_src 0 / 1 / 2), B and D in lfac (d_off < 0: none), C in T
    int32_t M, N, K, lda, ldb, ldd;
    int32_t a_src, gather;               // gather 1: A's column k is acol[k]; 2: B's row k is brow[k]; the map at cmap + map_off
    int32_t map_off, negate;
};
static_assert(sizeof(NdTopJob) == 72, "assembly job layout");

struct lsa_ndlu {
    lsa_ctx* ctx = nullptr;
    NdSymbolic S;
    int dtype = LSA_C128;
    bool ordered = false;           // the matrix came in elimination order: own unknown r of a node is own0 + r
    std::vector<NdChunk> chunks;    // factorisation order
    std::vector<NdLevel> levels;    // sweep order
    NdNodeDev* d_nodes = nullptr;                        // by node id (factorisation, exchange kernels of the sweeps)
    NdSweepNode *d_lnodes = nullptr, *d_lnodes_bwd = nullptr;  // in lvl_nodes order: the sweeps' records (downwards a distributed node appears as its slice of own rows)
    int32_t *d_dist_nodes = nullptr, *d_child_ptr = nullptr, *d_child_idx = nullptr;  // distributed nodes by level; children of every node
    void *d_xstage = nullptr, *d_xg = nullptr;          // staging of update rows on their way to distributed parents; own-row exchange buffer of the sweeps
    // transposed sweeps with distributed nodes (built by the first adjoint solve): per sweep record its offset in a rank's slot of the
    // partial-sum buffer (-1: not distributed), the buffer (nranks slots of tg_slot_max vector scalars), the slot size of every level
    int64_t* d_tgoff = nullptr;
    void* d_tg = nullptr;
    std::vector<int64_t> tg_slot;
    int64_t tg_slot_max = 0;
    int64_t xstage_slot = 0;                            // scalars per rank of d_xstage
    std::vector<int64_t> h_upd_off, h_lfac_off;         // per node: its update matrix in the update arena, its packed L (host copies of the plan)
    int64_t chunk_node_upd_off(int32_t t) const { return h_upd_off[(size_t)t]; }
    int32_t* d_gell = nullptr;
    int32_t *d_idx = nullptr, *d_cmap = nullptr, *d_tiles = nullptr, *d_chunk_nodes = nullptr;
    int64_t* d_asm_dst = nullptr;
    int32_t* d_asm_src = nullptr;
    int64_t asm_count = 0;
    int32_t *d_ipiv = nullptr, *d_rowq = nullptr, *d_flag = nullptr, *d_xflag = nullptr;
    unsigned long long* d_maxabs = nullptr;
    void *d_lfac = nullptr, *d_ufac = nullptr;  // packed factors (resident)
    void *d_work = nullptr, *d_upd = nullptr;   // working fronts of one chunk; live update matrices
    void *d_ubuf = nullptr, *d_xb = nullptr, *d_acc = nullptr;  // sweeps: update vectors (pull form), boundary vectors, slot rows (push form)
    void *d_tmp = nullptr, *d_ybuf = nullptr;
    int64_t lfac_entries = 0, ufac_entries = 0, work_entries = 0, upd_entries = 0, acc_entries = 0;
    int64_t xupd_slot = 0;                     // subtree-parallel: scalars per rank in the exchange region at the start of the update arena
    int32_t *d_cand[2] = {nullptr, nullptr};  // tournament pivoting: candidate rows, two buffers used in turn
    void* d_dinv = nullptr;                    // ... the inverted pivot tile of every node of the chunk being eliminated
    int32_t tp_min = 1 << 30;                  // chunks whose tallest pivot block has at least this many rows use it
    int32_t sb_min = 1 << 30;                  // ... and from this many rows on, with super-blocks of kSB columns (nd_gj_update_kernel)
    int32_t sb_cols = 128;                     // columns of a super-block (kSB; LSA_ND_SB_COLS, a multiple of 64, for measurements)
    int32_t ycap = 32;                         // rows of d_ybuf per unknown: kNB, or sb_cols when a chunk works in super-blocks
    int32_t gj_panel = 0;                      // LSA_ND_GJ_PANEL: 0 = regrouped launches, panel width by instance; 16 = 16-column panels up to 512 rows; 8 = the earlier launch sequence
    int32_t factor_launches = 0;               // kernel launches of the last numeric factorisation
    hipStream_t side = nullptr;                // ... the next block's tournament runs here, under the current block's update
    hipEvent_t ev_panel = nullptr, ev_pivots = nullptr;
    double seconds_analyse = 0.0, seconds_numeric = 0.0;
    int32_t solve_launches = 0;
    // the root and its children as one assembled inverse (nd_top_kernel): top.s = 0 where the forest is not eligible
    NdTop top = {};
    int32_t top_level = -1;                    // the root's level; the level below it has no launch of its own
    NdTop* d_top_rec = nullptr;                // `top` in device memory: a multi-column launch for a batch of sets has no room for it in its arguments
    void* d_top = nullptr;                     // T, top.s^2 scalars of the factor type, assembled by every numeric factorisation
    int32_t* d_top_icmap = nullptr;            // per child of the root, per own row of the root: its position in the child's boundary, or -1
    NdTopJob* d_top_jobs = nullptr;
    int32_t* d_top_tiles = nullptr;            // (job, tile) pairs of the two assembly launches
    int32_t top_tiles[2] = {0, 0};
    int64_t top_replaced_entries = 0;          // factor scalars the sweeps no longer read
    int acc_vbytes = 0;  // scalar size of the vectors the slot rows were last used with (their never-written entries must read zero)
    // lsa_ndlu_solve_multi: the sweep buffers of the columns of a pass beyond the first (which uses the buffers above), made by the
    // first multi-column solve, as many as fitted; what the last such solve used (lsa_ndlu_multi_info)
    struct MultiColumn {
        void *ubuf = nullptr, *xb = nullptr, *acc = nullptr, *tmp = nullptr;
        int acc_vbytes = 0;
    };
    std::vector<MultiColumn> multi;
    void* multi_stage = nullptr;     // the copy of an aliased block's columns for one pass of the forward block solves (counted in multi_bytes)
    int64_t multi_stage_bytes = 0;
    bool multi_full = false;     // an allocation failed: no further columns are tried
    int64_t multi_bytes = 0;
    int32_t multi_passes = 0;    // passes of two columns or more of the last solve of several columns (written by ndlu_solve_run, and by the column-by-column loop of lsa_ndlu_solve_multi)
    int32_t multi_width = 0;     // ... and its widest pass (1: column by column; 0: none yet)
    bool multi_transposed = false;  // lsa_ndlu_set_multi_transposed: block solves with trans != 0 run in wide passes too
};

template <typename U>
int upload(lsa_ctx* ctx, const std::vector<U>& h, U** d) {
    const size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(U);
    LSA_HIP_ALLOC(ctx, hipMalloc((void**)d, bytes));
    if (!h.empty()) LSA_HIP_CHECK(ctx, hipMemcpy(*d, h.data(), h.size() * sizeof(U), hipMemcpyHostToDevice));
    return LSA_OK;
}

// ndlu_factor.hip: the numeric factorisation of C on the analysis and buffers of f (factor type f->dtype)
int ndlu_numeric(lsa_ctx* ctx, lsa_ndlu* f, const lsa_mat* C);
// ---- solves on the factors, on device pointers, queued on the context's stream and not synchronised.
// ndlu_sweeps.hip: x = C^-1 b, and x = C^-T b (conj == 0) or C^-H b (real factors: the transposed solve); b == x is allowed.  The two
// calls of a Krylov step; every other form is a request.
int ndlu_solve_dev(lsa_ctx* ctx, lsa_ndlu* f, int vdtype, const void* b, void* x);
int ndlu_solve_adjoint_dev(lsa_ctx* ctx, lsa_ndlu* f, int conj, int vdtype, const void* b, void* x);
// whether g can run in a batch with f
bool nd_batch_compatible(const lsa_ndlu* f, const lsa_ndlu* g);

// One request for every form of the solve: X[z][:, q] = op(C_z)^-1 B[z][:, q] for q < nrhs on the factor sets f[z], z < J, with op
// by trans (0: C, 1: C^T, 2: C^H).  Column q of a set lies at B[z] + q ldb and X[z] + q ldx scalars of vdtype; the sets share ldb and
// ldx, several sets may read one B, and B[z] == X[z] (with ldb == ldx) is allowed.
//   sets = false: one factorisation (J = 1) on the sweeps' instances of capacity one, the only form for a forest cut over ranks or
//                 with distributed nodes, and then for one column only;
//   sets = true:  J <= kNdBatchMax factorisations that nd_batch_compatible passed, on the instances of capacity kNdBatchMax whatever J:
//                 one launch per level and direction for all of them.
// One column runs the single-column sweeps.  More run in passes of up to kNdMultiMax (complex vectors: 4) columns that share every
// factor load (ndlu_multi.hip), a last odd column through the single-column sweeps again; every column of every set has the bits
// ndlu_solve_dev or ndlu_solve_adjoint_dev give for it.
struct NdSolve {
    int32_t J;
    lsa_ndlu* const* f;
    bool sets;
    int trans, vdtype;
    int32_t nrhs;
    const void* const* B;
    int64_t ldb;
    void* const* X;
    int64_t ldx;
    const char* who;  // the entry's name for messages
};
// what a request ran as: its passes of two or more columns and the widest pass (one column: 0 and 1)
struct NdSolveInfo {
    int32_t passes, width;
};
// ndlu_multi.hip: runs the request; never writes to the caller's pointer arrays.  A request of several columns leaves its pass count and
// widest pass in multi_passes and multi_width of every set, one of a single column leaves them alone.  `who` prefixes every message:
// the C entry's name, or the name of the solver that built the request.
int ndlu_solve_run(lsa_ctx* ctx, const NdSolve& rq, NdSolveInfo* info = nullptr);
int ndlu_solve_column(lsa_ctx* ctx, const NdSolve& rq, const void* const* b, void* const* x);  // ndlu_sweeps.hip: its single-column part
void ndlu_multi_free(lsa_ndlu* f);
