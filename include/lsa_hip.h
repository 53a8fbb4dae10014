/* liblsa_hip.so -- C-ABI of the MI355X-native shift-invert eigen path for LSA-FW.
 *
 * The reference (ferdean/lsa-fw) has no native code of its own: the hot path is one Python call,
 *     Solver/eigen.py:136  ->  Solver/utils.py:270  ->  SLEPc.EPS.solve()
 * and every numeric step runs inside petsc4py/slepc4py.  This header is therefore the interface a
 * maintainer binds *instead of* slepc4py for that path (ctypes stub: INTEGRATION.md).  Each entry point
 * names the petsc4py/slepc4py call site in the reference it stands in for.
 *
 * Conventions
 *   - every function returns an int status: LSA_OK (0) or a negative lsa_status; no exception and no HIP
 *     error crosses the boundary; lsa_last_error(ctx) gives the text of the last failure;
 *   - host buffers are owned by the caller and only read/written during the call; device memory is owned
 *     by the library behind opaque handles and released by the matching *_destroy;
 *   - complex values are interleaved (re, im) doubles; CSR uses int32 row pointers / column indices,
 *     columns sorted inside each row, explicit zeros allowed, a structurally present diagonal is required
 *     for factorisation;
 *   - a context is bound to one GPU and one HIP stream and is not thread-safe.
 */
#ifndef LSA_HIP_H
#define LSA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { LSA_F64 = 0, LSA_C128 = 1 } lsa_dtype;

typedef enum {
    LSA_OK = 0,
    LSA_ERR_ARG = -1,        /* bad argument / shape / dtype            -> Python ValueError  (Solver/eigen.py:79-87) */
    LSA_ERR_HIP = -2,        /* HIP runtime failure (OOM, launch, ...)  -> RuntimeError                                 */
    LSA_ERR_ZERO_PIVOT = -3, /* factorisation hit a zero pivot          -> RuntimeError (tests/unit/Solver/test_eigen.py:272-281) */
    LSA_ERR_DIVERGED = -4,   /* inner solve did not reach rtol          -> RuntimeError (Solver/eigen2.py:179-181) */
    LSA_ERR_NONFINITE = -5,  /* NaN/Inf produced                        -> RuntimeError (Solver/eigen2.py:186-189) */
    LSA_ERR_TIMEOUT = -6,    /* a bounded device-side wait expired      -> RuntimeError                                 */
    LSA_ERR_COMM = -7,       /* RCCL failure                            -> RuntimeError                                 */
    LSA_ERR_OOM = -8         /* device memory exhausted (the only failure a factorisation may answer by a leaner method) */
} lsa_status;

typedef struct lsa_ctx lsa_ctx;
typedef struct lsa_mat lsa_mat;   /* CSR matrix on the device             (PETSc.Mat AIJ, FEM/utils.py:104)  */
typedef struct lsa_vec lsa_vec;   /* dense vector on the device           (PETSc.Vec,      FEM/utils.py:662)  */
typedef struct lsa_ilu lsa_ilu;   /* ILU(k) factors + triangular schedule (PETSc.PC ILU,   Solver/utils.py:261-266) */
typedef struct lsa_op lsa_op;     /* shift-invert operator (C^-1 M)       (SLEPc.ST SINVERT, Solver/utils.py:256-259) */
typedef struct lsa_krylov lsa_krylov; /* Arnoldi basis + recurrences      (SLEPc.BV + EPS Krylov-Schur, Solver/utils.py:270) */

/* counters filled by the solvers (all cumulative since creation of the object they belong to) */
typedef struct {
    int64_t op_applies;      /* shift-invert applies (outer Arnoldi steps)           */
    int64_t gmres_iters;     /* inner GMRES iterations                                */
    int64_t spmv_calls;      /* SpMV launches                                         */
    int64_t sptrsv_calls;    /* triangular-solve launches (L and U counted apart)     */
    double last_rel_res;     /* relative residual estimate of the last inner solve    */
    double max_rel_res;      /* worst one seen                                        */
    double seconds_factor;   /* wall seconds spent in symbolic + numeric factorisation */
    double seconds_solve;    /* wall seconds spent inside lsa_op_apply / lsa_krylov_extend / lsa_lanczos_extend, failed calls included */
    int32_t stagnated_solves; /* inner solves accepted at a stagnated true residual in (10 rtol, 1000 rtol]: the caller warns */
    int32_t pc_fallback;     /* 1 if the exact LU did not fit the device memory and ILU(k) + GMRES took its place */
    int32_t backward_accepted; /* direct solves whose ||b - C x|| / ||b|| missed rtol but whose backward error
                                  ||b - C x|| / (||C||_F ||x||) is <= 1e-12: shifts next to an eigenvalue */
    int32_t analysis_reused; /* 1 if the exact LU found its pattern-only analysis prepared (lsa_ndlu_prepare) or cached in the context */
    int32_t refined_solves;  /* direct solves that took a step of iterative refinement x += C^-1 (b - C x) because the first
                                answer missed rtol (Solver/eigen2.py:178-189 checks the same residual) */
    int32_t reserved0;
} lsa_stats;

/* ---- context ------------------------------------------------------------------------------------ */
int lsa_ctx_create(int device, lsa_ctx **out);
void lsa_ctx_destroy(lsa_ctx *ctx);
const char *lsa_last_error(const lsa_ctx *ctx);
int lsa_ctx_synchronize(lsa_ctx *ctx);
/* free and total bytes of the context's device memory right now (hipMemGetInfo) */
int lsa_ctx_mem_info(lsa_ctx *ctx, int64_t *free_bytes, int64_t *total_bytes);
/* name of the GPU architecture the context runs on, e.g. "gfx950" */
const char *lsa_ctx_arch(const lsa_ctx *ctx);

/* ---- vectors ------------------------------------------------------------------------------------ */
int lsa_vec_create(lsa_ctx *ctx, int64_t n, int dtype, lsa_vec **out);
void lsa_vec_destroy(lsa_vec *v);
int lsa_vec_upload(lsa_ctx *ctx, lsa_vec *v, const void *host);
int lsa_vec_download(lsa_ctx *ctx, const lsa_vec *v, void *host);

/* ---- CSR matrices: iPETScMatrix.from_matrix / as_scipy_array (FEM/utils.py:183-220,585-588) -------- */
int lsa_csr_upload(lsa_ctx *ctx, int32_t n, int64_t nnz, const int32_t *rowptr, const int32_t *col,
                   const void *val, int dtype, lsa_mat **out);
void lsa_mat_destroy(lsa_mat *m);
int lsa_mat_download_values(lsa_ctx *ctx, const lsa_mat *m, void *host_val);
/* C = alpha*A + beta*B on one shared sparsity pattern: MatDuplicate + MatAXPY of ST sinvert
 * (explicit in Solver/eigen2.py:110-111).  alpha/beta are (re, im); out_dtype LSA_F64 needs real inputs
 * and zero imaginary parts.  LIFETIME: the result BORROWS A's device index arrays (row pointers, columns) and only owns
 * its values: A must outlive it (destroy the result first).  The Python binding keeps A alive for that reason. */
int lsa_csr_axpby(lsa_ctx *ctx, const lsa_mat *A, const lsa_mat *B, const double alpha[2], const double beta[2],
                  int out_dtype, lsa_mat **out);
/* W = diag(left) M diag(right) on M's pattern: the windowed mass matrices behind the forcing and response windows of the resolvent
 * and transient-growth analyses (Q = D M D).  M is real (LSA_F64), square and whole (no shard, no row view); left and right are
 * host vectors of n doubles in M's row numbering, right == NULL means right = left.  The values are (left[i] * M_ij) * right[j], two
 * roundings in that order -- the order scipy.sparse.diags(l) @ M @ diags(r) rounds in -- so a window of ones gives M's values bit
 * for bit.  LIFETIME: like the result of lsa_csr_axpby, out BORROWS M's index arrays, host pattern and the row groups / compressed
 * indices of its SpMV (8 bytes per entry of its own; lsa_spmv takes the same kernel form for it as for M): M must outlive it.
 * LSA_ERR_ARG, naming the function, for a complex M, a shard or row view, or a non-finite entry of left or right. */
int lsa_csr_window(lsa_ctx *ctx, const lsa_mat *M, const double *left, const double *right, lsa_mat **out);
/* y = A x: MatMult (Solver/eigen2.py:174).  Real matrix with complex vectors is supported. */
int lsa_spmv(lsa_ctx *ctx, const lsa_mat *A, const lsa_vec *x, lsa_vec *y);
/* y = A^T x or A^H x (conj != 0) without a second copy of the values: a transposed INDEX (row pointers, rows, positions of the
 * values) is built once per pattern and shared by the matrices of that pattern; additions in a fixed order.  The adjoint
 * eigenproblem of Sensitivity/__init__.py:47-57,247-248 */
int lsa_spmv_transpose(lsa_ctx *ctx, const lsa_mat *A, int conj, const lsa_vec *x, lsa_vec *y);
/* y[z] = A_z^T x[z] or A_z^H x[z] (conj != 0), z < J <= 16, in ONE launch for matrices of one pattern (the C_k = A - z_k M built on
 * A's index arrays by lsa_csr_axpby, or equal host patterns), one shape and one dtype, on the transposed index they share; vectors
 * of one dtype, no y[z] among the inputs or twice.  Every output's entries are summed by the same 16 lanes in the same order as in
 * lsa_spmv_transpose: each y[z] holds exactly its bits.  LSA_ERR_ARG, naming what differs, for anything else. */
int lsa_spmv_transpose_batch(lsa_ctx *ctx, int32_t J, const lsa_mat *const *A, int conj, const lsa_vec *const *x, lsa_vec *const *y);
/* y[z] = A_z x[z], z < J <= 16, in ONE launch for whole square matrices of one pattern, one shape and one dtype (the same matrix may
 * stand in several slots: Q x_k for all members of a lockstep group); vectors of one dtype, no y[z] among the inputs or twice.  Each
 * problem walks its rows through the kernel body lsa_spmv runs for this pattern and these scalar types (sub-wave rows, compressed
 * indices or row groups), so each y[z] holds exactly lsa_spmv's bits.  LSA_ERR_ARG, naming what differs, for anything else. */
int lsa_spmv_batch(lsa_ctx *ctx, int32_t J, const lsa_mat *const *A, const lsa_vec *const *x, lsa_vec *const *y);
/* Which kernel lsa_spmv launches for this matrix and vector type (template arguments included) and the bytes that
 * kernel moves per launch: values + column indices (2-byte offsets from the row's first column when the compressed form
 * is in use) + row pointers + one read of x and one write of y.  The numerator of an HBM-roofline fraction.  The name is that
 * of the launch: the XCD forms are named only where they run (8 x 64 row groups, 8 x 256 / lanes rows), the non-temporal
 * instances carry their fourth argument. */
int lsa_spmv_info(lsa_ctx *ctx, const lsa_mat *A, int xdtype, char *kernel, int32_t kernel_len, int64_t *bytes_moved);
/* Launch y = A x `iters` times back to back on the context's stream, bracketed by HIP events on that
 * stream; *avg_ms = mean duration of one launch.  This is the measurement bench.py's roofline uses. */
int lsa_spmv_time(lsa_ctx *ctx, const lsa_mat *A, const lsa_vec *x, lsa_vec *y, int iters, double *avg_ms);

/* ---- ILU(k): PC ILU of the ST's KSP (Solver/utils.py:261-266, PreconditionerType.ILU) ------------ */
/* levels = level of fill (0 = ILU(0)); pivots with |u_ii| < shift_tol are replaced by shift_tol*sign
 * (PETSc -pc_factor_shift_type nonzero); shift_tol = 0 makes a zero pivot an error.  Symbolic analysis
 * and the dependency schedule are computed on the host, the numeric factorisation on the device. */
int lsa_ilu_create(lsa_ctx *ctx, const lsa_mat *C, int levels, double shift_tol, lsa_ilu **out);
void lsa_ilu_destroy(lsa_ilu *pc);
/* Triangular-solve algorithm: 0 = one launch per dependency level, 1 = sync-free (one launch, row hand-offs through
 * the solution vector), 2 = blocked (diagonal blocks of block_size rows inverted into dense triangles on the device,
 * 2 launches per block replayed from a hipGraph).  lsa_ilu_create picks 2 for narrow dependency DAGs (2D FEM) when
 * the 2 * n * block_size scalars fit, else 1.  All three give the same solve up to summation order. */
int lsa_ilu_set_algorithm(lsa_ctx *ctx, lsa_ilu *pc, int algo, int32_t block_size);
/* which: 0 = x = L^-1 b (unit lower), 1 = x = U^-1 b, 2 = x = U^-1 L^-1 b (MatSolve) */
int lsa_ilu_solve(lsa_ctx *ctx, lsa_ilu *pc, int which, const lsa_vec *b, lsa_vec *x);
/* `iters` back-to-back solves bracketed by HIP events on the context's stream; *avg_ms = mean per solve */
int lsa_ilu_solve_time(lsa_ctx *ctx, lsa_ilu *pc, int which, const lsa_vec *b, lsa_vec *x, int iters, double *avg_ms);
/* introspection for tests: nnz of the factor pattern, number of dependency levels (lower, upper),
 * number of shifted pivots */
int lsa_ilu_info(const lsa_ilu *pc, int64_t *nnz, int32_t *levels_lower, int32_t *levels_upper, int32_t *nshift);
/* copy the factor out (CSR, L strictly below the diagonal with unit diagonal implied, U on and above) */
int lsa_ilu_download(lsa_ctx *ctx, const lsa_ilu *pc, int32_t *rowptr, int32_t *col, void *val);

/* ---- nested-dissection multifrontal LU: PC LU of the ST's KSP (.examples/eigenvalues.py:100;
 * Sensitivity/__init__.py:182,260) ---------------------------------------------------------------------------------------
 * The sparse direct solver PETSc's PC LU stands for, rebuilt for the device: elimination forest of dense fronts from a
 * nested dissection of the pattern's graph, every front's pivot block inverted explicitly, so that a solve is two sweeps
 * over the tree levels with one dense mat-vec per node and sweep.  C may be in any order (the dissection is internal). */
typedef struct lsa_nd_sym lsa_nd_sym;  /* analysis of a pattern (host only)  */
typedef struct lsa_ndlu lsa_ndlu;      /* factorisation resident in HBM      */
/* Host-only analysis of a square CSR pattern (no GPU needed): ordering, elimination forest, front index lists.
 * leaf_size <= 0 picks 128 unknowns per leaf subdomain.  constraint: NULL, or n flags marking the unknowns whose diagonal
 * is numerically zero (the pressure rows of a saddle-point matrix): they are eliminated after all their neighbours, which
 * keeps every pivot block non-singular.  The handle is returned on failure too (for lsa_nd_sym_error). */
int lsa_nd_analyse(int32_t n, const int32_t *rowptr, const int32_t *col, int32_t leaf_size, const int8_t *constraint, lsa_nd_sym **out);
/* Ordering only: the dissection's elimination order and forest, without the index tables.  lsa_nd_sym_export then fills
 * perm, node_start, parent and level (front_size = own size, idx untouched).  A caller that permutes its matrices by perm
 * and hands the forest back (first = node_start[t], size = node_start[t + 1] - node_start[t]: lsa_ndlu_prepare_tree) runs the
 * whole iteration in the elimination order: a node's own unknowns are contiguous in every vector, and the sweeps of the
 * factorisation address them without index lists. */
int lsa_nd_order(int32_t n, const int32_t *rowptr, const int32_t *col, int32_t leaf_size, const int8_t *constraint, lsa_nd_sym **out);
/* The same analysis for a tree the caller provides, optionally localised for one rank of a subtree-parallel
 * factorisation.  Node t owns the matrix indices [first[t], first[t] + size[t]) (nodes in any order in which parent[] can be
 * looked up; -1 = root); owner[t] (NULL on one rank) = the rank whose subtree the node belongs to, -1 = the replicated top
 * of the tree.  Rows that belong to no node must be empty (padding of the sharded block layout).  The tables then hold
 * this rank's own nodes, the top, and the other ranks' subtree roots as childless "ghost" nodes. */
int lsa_nd_analyse_tree(int32_t n, const int32_t *rowptr, const int32_t *col, int32_t ntree, const int32_t *first, const int32_t *size,
                        const int32_t *parent, const int32_t *owner, int32_t rank, int32_t nranks, lsa_nd_sym **out);
const char *lsa_nd_sym_error(const lsa_nd_sym *h);
void lsa_nd_sym_destroy(lsa_nd_sym *h);
/* tree nodes, tree levels, largest front, total length of the front index lists, scalars one solve reads (sum of
 * m^2 + 2 m b over the nodes), scalars of all fronts (sum of f^2), multiply-adds of the numeric factorisation */
int lsa_nd_sym_info(const lsa_nd_sym *h, int32_t *ntree, int32_t *nlevels, int32_t *max_front, int64_t *index_entries,
                    int64_t *factor_entries, int64_t *front_entries, double *flops);
/* Device memory of a factorisation of this analysis, in bytes, before any GPU is touched (what lsa_ndlu_create will allocate;
 * scalar_bytes 8 or 16; work_budget_bytes: what the working fronts of one chunk may take, <= 0: a whole level): out[0] packed
 * factors sum(m^2 + 2 m b), out[1] working arena, out[2] update arena (out[3] of it: the exchange region of a forest cut over
 * ranks), out[4] sweep buffers, out[5] number of chunks, out[6] the largest front, out[7] index tables.  Optional per-node
 * copies of the plan (tests): upd_off[ntree], work_off[ntree] (scalars), chunk_of[ntree] (-1: not factored here). */
int lsa_nd_sym_memory(const lsa_nd_sym *h, int32_t scalar_bytes, int64_t work_budget_bytes, int64_t *out, int64_t *upd_off, int64_t *work_off,
                      int32_t *chunk_of);
/* copies of the analysis (any pointer may be NULL): perm[n] (elimination order -> original index), node_start[ntree + 1],
 * parent[ntree] (-1 = root), level[ntree], front_size[ntree], idx[index_entries] (front index lists, original numbering) */
int lsa_nd_sym_export(const lsa_nd_sym *h, int32_t *perm, int32_t *node_start, int32_t *parent, int32_t *level, int32_t *front_size,
                      int32_t *idx);
/* the index tables the device kernels walk, for tests: cmap[sum b] (position of each boundary unknown in the parent's
 * front), gptr[sum (f + 1)] / gidx[sum b] (gather lists of the upward sweep), asm_dst[nnz] (front-buffer slot of every
 * matrix entry), lvl_ptr[nlevels + 1] / lvl_nodes[ntree] (nodes by level) */
int lsa_nd_sym_export_tables(const lsa_nd_sym *h, int32_t *cmap, int32_t *gptr, int32_t *gidx, int64_t *asm_dst, int32_t *lvl_ptr,
                             int32_t *lvl_nodes);
/* per kept node: kind[ntree] (1 = factored on this rank, 2 = replicated top, 3 = another rank's subtree root, 4 = distributed
 * top node, see lsa_nd_sym_export_top), front_off /
 * u_off[ntree + 1] (offsets into the front / update-vector buffers; the subtree roots lie in per-rank slots at the start),
 * asm_src[scalars[3]] (matrix entry of every assembly slot), children_ptr[ntree + 1] / children_idx; scalars[6] = front
 * slot, update-vector slot, first replicated work level, assembly entries, ranks, rank */
int lsa_nd_sym_export_dist(const lsa_nd_sym *h, int32_t *kind, int64_t *front_off, int64_t *u_off, int32_t *asm_src, int32_t *children_ptr,
                           int32_t *children_idx, int64_t *scalars);
/* DISTRIBUTED top nodes (owner -2 in the forest handed to lsa_nd_analyse_tree; kind 4): every rank keeps the pivot block whole
 * and its own equal slice of the boundary rows (working front (m + brow) x f, update matrix brow x b, packed L (m + brow) x m)
 * and of the own rows of U (orows x b).  Per kept node: owner[ntree] (rank, -1 replicated top, -2 distributed top), rows[4 ntree]
 * = (brow0, brow, orow0, orows), exch[4 ntree] = (ux_base, ux_stride, xg_base, xg_stride): where the node's update entries and
 * finished own rows lie in the sweeps' per-level exchange regions (entry k of rank k / s's slot: base + (k / s) stride + k % s,
 * s = ceil(count / ranks)); totals[2] = entries of the update-vector buffer, of the own-row exchange buffer */
int lsa_nd_sym_export_top(const lsa_nd_sym *h, int32_t *owner, int32_t *rows, int64_t *exch, int64_t *totals);
/* Analysis (from C's host copy of the pattern; reused from the context when the last destroyed or prepared factorisation
 * had the same pattern) + numeric factorisation on the device.  If a pivot block comes out singular and C has zero
 * diagonal entries, the analysis is redone once with those unknowns as constraints.  LSA_ERR_ZERO_PIVOT when a pivot block
 * is singular to 1e-15 max|C| after that, LSA_ERR_OOM when the fronts do not fit. */
int lsa_ndlu_create(lsa_ctx *ctx, const lsa_mat *C, int32_t leaf_size, lsa_ndlu **out);
/* Analysis only, parked in the context: the pattern of P (any matrix with C's pattern, e.g. A) and the scalar type the
 * factors will have.  The next lsa_ndlu_create on that pattern then runs the numeric phase alone.  Lets a caller keep
 * the pattern-only work out of a timed solve (the Python layer calls it from prepare()).  constraint: as for
 * lsa_nd_analyse (NULL: none). */
int lsa_ndlu_prepare(lsa_ctx *ctx, const lsa_mat *P, int dtype, int32_t leaf_size, const int8_t *constraint);
/* The same with the caller's forest (arguments as for lsa_nd_analyse_tree on one rank; normally the forest of lsa_nd_order on
 * the matrix permuted by its perm). */
int lsa_ndlu_prepare_tree(lsa_ctx *ctx, const lsa_mat *P, int dtype, int32_t ntree, const int32_t *first, const int32_t *size,
                          const int32_t *parent);
/* Subtree-parallel form (one process per GPU, after lsa_comm_init*): every rank holds the whole matrix C and calls this with
 * the same forest (arguments as for lsa_nd_analyse_tree; the context's rank selects the localisation).  A rank factors
 * the subtrees it owns; the subtree roots' fronts are exchanged by one in-place all-gather; the top of the forest
 * (owner -1) is then factored redundantly by every rank.  A solve exchanges the subtree roots' update vectors (a few KB)
 * between the upward sweep over the own subtrees and the replicated top; it returns the entries of x that belong to this
 * rank's subtrees and to the top (the caller's all-gather of x completes it).  Failures are agreed on collectively. */
int lsa_ndlu_create_tree(lsa_ctx *ctx, const lsa_mat *C, int32_t ntree, const int32_t *first, const int32_t *size, const int32_t *parent,
                         const int32_t *owner, lsa_ndlu **out);
/* new values on the analysed pattern (a shift sweep: .examples/eigenvalues.py:97-108) */
int lsa_ndlu_refactor(lsa_ctx *ctx, lsa_ndlu *f, const lsa_mat *C);
void lsa_ndlu_destroy(lsa_ndlu *f);
/* x = C^-1 b */
int lsa_ndlu_solve(lsa_ctx *ctx, lsa_ndlu *f, const lsa_vec *b, lsa_vec *x);
/* x[z] = C_z^-1 b[z], z < J <= 16, for J factorisations of one analysis (one pattern, made by lsa_ndlu_create or
 * lsa_ndlu_create_tree in this context on one rank): one launch per tree level and direction for the whole batch, and each x[z]
 * holds exactly the bits lsa_ndlu_solve(f[z], b[z]) gives.  Factorisations of different analyses, or two problems sharing a
 * factorisation or an output: LSA_ERR_ARG. */
int lsa_ndlu_solve_batch(lsa_ctx *ctx, int32_t J, lsa_ndlu *const *f, const lsa_vec *const *b, lsa_vec *const *x);
/* x = C^-T b (conj = 0) or C^-H b (conj != 0) on the same factors: the sweeps of the transposed forest.  The adjoint
 * eigenproblem (Sensitivity/__init__.py:47-57,247-287 forms A^H, M^H explicitly and factorises again) needs no second
 * factorisation and no transposed matrix. */
int lsa_ndlu_solve_adjoint(lsa_ctx *ctx, lsa_ndlu *f, int conj, const lsa_vec *b, lsa_vec *x);
/* x[z] = C_z^-T b[z] (conj = 0) or C_z^-H b[z] (conj != 0), z < J <= 16, under the rules of lsa_ndlu_solve_batch (factorisations of
 * one analysis on one rank, vectors of one dtype, no shared factorisation or output: LSA_ERR_ARG otherwise): the transposed sweeps
 * of the whole batch in one launch per tree level and direction, and each x[z] holds exactly the bits
 * lsa_ndlu_solve_adjoint(f[z], conj, b[z]) gives.  b[z] == x[z] solves in place; several problems may read one b. */
int lsa_ndlu_solve_batch_adjoint(lsa_ctx *ctx, int32_t J, lsa_ndlu *const *f, int conj, const lsa_vec *const *b, lsa_vec *const *x);
int lsa_ndlu_solve_time(lsa_ctx *ctx, lsa_ndlu *f, const lsa_vec *b, lsa_vec *x, int iters, double *avg_ms);
/* X[:, q] = op(C)^-1 B[:, q], q < nrhs, on ONE factorisation: PETSc MatMatSolve / KSPMatSolve (the reference reaches them through
 * the kept KSP of iKSP, Solver/utils.py:331-419, one right-hand side at a time).  trans: 0 = C^-1, 1 = C^-T, 2 = C^-H.  B and X are
 * column-major blocks: column q starts at q * ld scalars, ld >= n, each vector at least ld (nrhs - 1) + n long.  B == X with
 * ldb == ldx solves in place; any other overlap, nrhs < 1, ld < n, a short block, mixed vector dtypes, complex factors with real
 * vectors: LSA_ERR_ARG.  For trans = 0 on one rank the columns go through the sweeps in passes of up to 8 (real vectors) or 4
 * (complex vectors) that read every factor scalar once per pass (lsa_ndlu_multi_info); so do the transposed systems once
 * lsa_ndlu_set_multi_transposed switched that on for the factorisation (off by default: they run column by column, as a
 * forest cut over ranks always does).  Either
 * way column q holds exactly the bits lsa_ndlu_solve / lsa_ndlu_solve_adjoint gives for it.  nrhs = 1 is lsa_ndlu_solve.  The
 * sweep buffers of the further columns of a pass are made by the first call and released with the factorisation; where they
 * do not fit, the passes get narrower, down to column by column. */
int lsa_ndlu_solve_multi(lsa_ctx *ctx, lsa_ndlu *f, int trans, int32_t nrhs, const lsa_vec *B, int64_t ldb, lsa_vec *X, int64_t ldx);
/* `iters` such block solves back to back (B and X apart), bracketed by HIP events on the context's stream; *avg_ms = mean per
 * block solve (KSPMatSolve timed as lsa_ndlu_solve_time times KSPSolve) */
int lsa_ndlu_solve_multi_time(lsa_ctx *ctx, lsa_ndlu *f, int trans, int32_t nrhs, const lsa_vec *B, int64_t ldb, lsa_vec *X, int64_t ldx,
                              int iters, double *avg_ms);
/* on != 0: lsa_ndlu_solve_multi and lsa_ndlu_solve_multi_time with trans != 0 carry the columns of a pass through one launch per
 * tree level and direction of the transposed sweeps, as trans = 0 does (one rank, no distributed node; same passes, same bits per
 * column).  The default is off. */
int lsa_ndlu_set_multi_transposed(lsa_ctx *ctx, lsa_ndlu *f, int on);
/* what the last lsa_ndlu_solve_multi on f used, in either direction (the work MatMatSolve hides): width = columns of its widest
 * pass (1: column by column, 0: none yet), extra_bytes = device memory of the per-column sweep buffers, launches_per_pass = dependent launches of
 * one pass (those of one lsa_ndlu_solve) */
int lsa_ndlu_multi_info(const lsa_ndlu *f, int32_t *width, int64_t *extra_bytes, int32_t *launches_per_pass);
/* X[z][:, q] = C_z^-1 B[z][:, q], z < J <= 16, q < nrhs: the block solve of lsa_ndlu_solve_multi on J factorisations of one analysis,
 * every launch of the sweeps carrying all columns of a pass for all J of them.  The rules of lsa_ndlu_solve_batch hold for the
 * factorisations (one analysis, one rank, no distributed node, vectors of one dtype) and those of lsa_ndlu_solve_multi for the
 * blocks, which share ldb and ldx (ld >= n, each vector at least ld (nrhs - 1) + n long, complex factors need complex vectors).
 * B[z] == X[z] with ldb == ldx solves in place; several sets may read ONE B (the region eigensolver's case); two sets sharing a
 * factorisation or an X, or any other overlap: LSA_ERR_ARG.  trans must be 0 (LSA_ERR_ARG otherwise): the transposed form is an
 * entry of its own, lsa_ndlu_solve_multi_batch_adjoint.
 * Column q of set z holds exactly the bits lsa_ndlu_solve(f[z], .) gives for it.  The pass width is the smallest every set has
 * sweep buffers for; a last single column goes through the sweeps of lsa_ndlu_solve_batch, and nrhs = 1 is that call. */
int lsa_ndlu_solve_multi_batch(lsa_ctx *ctx, int32_t J, lsa_ndlu *const *f, int trans, int32_t nrhs, const lsa_vec *const *B, int64_t ldb,
                               lsa_vec *const *X, int64_t ldx);
/* `iters` such block solves back to back (every B[z] apart from every X[z]), timed as lsa_ndlu_solve_multi_time; *avg_ms = mean per
 * block solve of all J sets */
int lsa_ndlu_solve_multi_batch_time(lsa_ctx *ctx, int32_t J, lsa_ndlu *const *f, int trans, int32_t nrhs, const lsa_vec *const *B,
                                    int64_t ldb, lsa_vec *const *X, int64_t ldx, int iters, double *avg_ms);
/* X[z][:, q] = C_z^-T B[z][:, q] (conj = 0) or C_z^-H B[z][:, q] (conj != 0), z < J <= 16, q < nrhs: the transposed block solve on J
 * factorisations of one analysis, every launch of the transposed sweeps carrying all columns of a pass for all J of them -- what a
 * left (adjoint) phase of the region eigensolver needs on the factor sets of its nodes.  The rules are those of
 * lsa_ndlu_solve_multi_batch, word for word: one analysis, one rank, no distributed node, vectors of one dtype; the blocks share ldb
 * and ldx; several sets may read ONE B; B[z] == X[z] with ldb == ldx solves in place; two sets sharing a factorisation or an X, or
 * any other overlap: LSA_ERR_ARG, X untouched.  Passes of 8, 4 or 2 real or 4 or 2 complex columns, the widest every set has sweep
 * buffers for; a last single column goes through the sweeps of lsa_ndlu_solve_batch_adjoint, and nrhs = 1 is that call.  Column q of
 * set z holds exactly the bits lsa_ndlu_solve_adjoint(f[z], conj, .) gives for it.  Independent of lsa_ndlu_set_multi_transposed
 * (that switch belongs to lsa_ndlu_solve_multi). */
int lsa_ndlu_solve_multi_batch_adjoint(lsa_ctx *ctx, int32_t J, lsa_ndlu *const *f, int conj, int32_t nrhs, const lsa_vec *const *B,
                                       int64_t ldb, lsa_vec *const *X, int64_t ldx);
/* `iters` such block solves back to back (every B[z] apart from every X[z]), timed as lsa_ndlu_solve_multi_batch_time */
int lsa_ndlu_solve_multi_batch_adjoint_time(lsa_ctx *ctx, int32_t J, lsa_ndlu *const *f, int conj, int32_t nrhs, const lsa_vec *const *B,
                                            int64_t ldb, lsa_vec *const *X, int64_t ldx, int iters, double *avg_ms);
/* Inertia (numbers of negative, zero, positive eigenvalues) of a REAL SYMMETRIC C from its factorisation: what SLEPc's spectrum
 * slicing takes from the symmetric-indefinite factorisation behind EPS.setInterval / EPS_ALL (Solver/utils.py:248-254: the
 * number of eigenvalues of a definite pencil below sigma is the number of negative eigenvalues of A - sigma M).  Sum over the
 * tree nodes of the inertia of their pivot blocks, each evaluated on the host (O(m^3)): for the Hermitian problems of the
 * interval sweep.  Real factors on one rank only; the symmetry of C is the caller's statement. */
int lsa_ndlu_inertia(lsa_ctx *ctx, lsa_ndlu *f, int64_t *negative, int64_t *zero, int64_t *positive);
/* out[8] as lsa_nd_sym_memory fills it, for the analysis the context holds prepared (after lsa_ndlu_prepare / _prepare_tree, or
 * parked by the last lsa_ndlu_destroy) with its own scalar type: what the next factorisation on it allocates.  LSA_ERR_ARG when
 * the context holds none. */
int lsa_ndlu_prepared_memory(lsa_ctx *ctx, int64_t *out);
/* front_entries: scalars of the device buffers (packed factors + the working fronts of one chunk + the update arena);
 * apply_bytes: algorithmic bytes of one solve (every factor scalar once + the vectors); apply_launches: dependent
 * launches of one solve (two per tree level, less one: the roots have no downward step); factor_launches: kernel
 * launches of the last numeric factorisation, counted on the host */
int lsa_ndlu_info(const lsa_ndlu *f, int32_t *ntree, int32_t *nlevels, int32_t *max_front, int64_t *factor_entries,
                  int64_t *front_entries, int64_t *apply_bytes, int32_t *apply_launches, double *seconds_analyse,
                  double *seconds_numeric, int32_t *factor_launches);
/* level `level` (0 = leaves) of f's sweeps, one launch upwards and one downwards: its nodes, its widest pivot block, the rows
 * of a tile of the upward and of the downward launch (8: 64 lanes along a row pair, 32: 16 lanes, 128: 4 lanes) and the tiles
 * of its tallest node in each (the launches' grid.y; 0: no launch).  LSA_ERR_ARG beyond the last level. */
int lsa_ndlu_sweep_level(const lsa_ndlu *f, int32_t level, int32_t *nodes, int32_t *max_pivot, int32_t *fwd_rows, int32_t *bwd_rows,
                         int32_t *fwd_tiles, int32_t *bwd_tiles);

/* ---- GMRES: KSPSolve of the ST (reference default PREONLY+LU; north star: GMRES+ILU) ----------------- */
/* right-preconditioned restarted GMRES with CGS2; pc may be NULL.  x holds the initial guess on entry
 * when use_x0 != 0.  Returns LSA_ERR_DIVERGED if rtol is not reached within maxit iterations.  min(restart, maxit) is
 * at most 1024 for complex and 2048 for real vectors (what the basis product handles): LSA_ERR_ARG beyond. */
int lsa_gmres(lsa_ctx *ctx, const lsa_mat *C, lsa_ilu *pc, const lsa_vec *b, lsa_vec *x, int use_x0, double rtol,
              int restart, int maxit, int32_t *iters, double *rel_res);

/* ---- shift-invert operator: ST SINVERT (Solver/utils.py:244-266; Solver/eigen2.py:109-201) ---------- */
typedef struct {
    int32_t ilu_levels;   /* level of fill of the preconditioner (default 0)                  */
    double ilu_shift;     /* pivot shift tolerance (0 = zero pivot is an error)              */
    double ksp_rtol;      /* inner GMRES relative tolerance                                  */
    int32_t ksp_restart;  /* GMRES restart length                                            */
    int32_t ksp_maxit;    /* GMRES iteration cap                                             */
    int32_t pc_type;      /* 0 = none, 1 = ILU(k), 2 = exact LU (nested-dissection multifrontal; falls back to ILU(k) + GMRES only
                             when it runs out of device memory).  (3, round 1's banded block LU, is a cross-check library now.) */
    double antishift[2];  /* mode 2 only: nu of the Cayley transform (re, im); SLEPc's default is nu = sigma */
} lsa_op_options;

/* Builds C = A - sigma*M (complex if sigma has an imaginary part or A/M are complex), factors it, and
 * allocates the inner-solver workspace.  M may be NULL (standard problem, M = I).
 * mode: 0 = shift-invert  y = (A - sigma M)^-1 M x     (iSTType.SINVERT)
 *       1 = shift         y = M^-1 (A - sigma M) x     (iSTType.SHIFT; M = NULL gives y = (A - sigma I) x)
 *       2 = Cayley        y = (A - sigma M)^-1 (A + nu M) x   (iSTType.CAYLEY, nu = opts->antishift) */
int lsa_op_create(lsa_ctx *ctx, const lsa_mat *A, const lsa_mat *M, const double sigma[2], int mode,
                  const lsa_op_options *opts, lsa_op **out);
void lsa_op_destroy(lsa_op *op);
int lsa_op_apply(lsa_ctx *ctx, lsa_op *op, const lsa_vec *x, lsa_vec *y);
int lsa_op_stats(const lsa_op *op, lsa_stats *out);
/* Adjoint form of a shift-invert operator on the SAME factors: y = Kfac^-H Kmul^H x = (A - sigma M)^-H M^H x, the operator of
 * the adjoint eigenproblem (A^H, M^H) at the target conj(sigma) (Sensitivity/__init__.py:230-311, which forms the two
 * transposes and factorises again).  Transposed sweeps of the nested-dissection LU, transposed SpMV; one rank, or the
 * subtree-parallel layout of lsa_op_create_dist (same exchanges as the forward solve; the transposed products use the whole
 * matrices every rank holds). */
/* (A change of direction also clears the operator's "solves carry a refinement step" state: the other direction's solves decide
 * that for themselves, as those of a new operator do.) */
int lsa_op_set_adjoint(lsa_ctx *ctx, lsa_op *op, int on);
/* Projected operator  y = P Kfac^-1 Kmul x  with P = diag(keep): keep[i] in {0, 1}, host array of n doubles (NULL
 * removes the projection).  Stands in for the velocity-subspace projection of ArpackEigenSolver's matvec
 * (Solver/eigen2.py:164-201: pressure dofs zeroed before and after the inner solve); the input side of the
 * projection is the caller's: Krylov vectors are outputs of this operator, the start vector is masked on the host. */
int lsa_op_set_projection(lsa_ctx *ctx, lsa_op *op, const double *keep);

/* ---- Krylov basis: BV + Arnoldi recurrences of EPS Krylov-Schur (SLEPc.EPS.solve, Solver/utils.py:270) -- */
/* Basis of up to ncv+1 complex vectors of length n, resident in HBM, column-major.  ncv <= 1024 (the basis product of
 * lsa_krylov_restart / lsa_krylov_ritz_vectors keeps a tile of the small matrix in 64 KB of LDS): LSA_ERR_ARG beyond. */
int lsa_krylov_create(lsa_ctx *ctx, lsa_op *op, int32_t ncv, lsa_krylov **out);
void lsa_krylov_destroy(lsa_krylov *k);
/* perm[i] = the caller's index of row i of the basis (the solve runs in a permuted numbering): lsa_krylov_ritz_vectors then
 * returns its vectors in the caller's numbering, rows scattered on the device.  NULL removes it. */
int lsa_krylov_set_row_permutation(lsa_ctx *ctx, lsa_krylov *k, const int32_t *perm);
/* v_0 = v / ||v||  (host complex vector of length n) */
/* (A start vector begins a new run on the workspace: the pipelined step path is armed again, whatever an earlier run on the
 * same workspace found out about its inner solves.  lsa_krylov_inject with j = 0 is this call.) */
int lsa_krylov_set_start(lsa_ctx *ctx, lsa_krylov *k, const void *host_v);
/* v_j = host vector orthonormalised (CGS2) against v_0..v_{j-1}: used to continue after an exact breakdown
 * (invariant subspace found, e.g. repeated eigenvalues) with a fresh direction; j = 0 equals set_start. */
int lsa_krylov_inject(lsa_ctx *ctx, lsa_krylov *k, int32_t j, const void *host_v);
/* Arnoldi steps j = j0 .. j1-1:  w = OP v_j;  CGS2 against v_0..v_j;  v_{j+1} = w/||w||.
 * H is the caller's (ncv+1) x ncv column-major complex Hessenberg; columns j0..j1-1 are written.
 * Returns LSA_OK and *breakdown = step index if ||w|| underflowed (invariant subspace), else -1. */
int lsa_krylov_extend(lsa_ctx *ctx, lsa_krylov *k, int32_t j0, int32_t j1, void *H, int32_t ldh, int32_t *breakdown);
/* Krylov-Schur truncation: V[:, 0:knew] = V[:, 0:m] Q (Q is m x knew column-major complex on the host)
 * and V[:, knew] = V[:, m]. */
int lsa_krylov_restart(lsa_ctx *ctx, lsa_krylov *k, int32_t m, int32_t knew, const void *Q, int32_t ldq);
/* X = V[:, 0:m] Y, Y m x nvec on the host; X (n x nvec column-major complex) is written to the host.  normalise: 0 = as they
 * are; bit 0 = each column scaled to unit 2-norm (SLEPc convention, Solver/utils.py:309); bit 1 = and rotated to a canonical
 * phase (its entry of largest magnitude real and positive: a real eigenvector comes out real, the test the reference's real
 * build makes at Solver/utils.py:280-291), with the 2-norms of the columns' imaginary parts kept for lsa_krylov_imag_norms. */
int lsa_krylov_ritz_vectors(lsa_ctx *ctx, lsa_krylov *k, int32_t m, int32_t nvec, const void *Y, int32_t ldy,
                            int normalise, void *X);
/* 2-norms of the imaginary parts of the columns of the last lsa_krylov_ritz_vectors call with normalise bit 1 (nvec <= its nvec) */
int lsa_krylov_imag_norms(const lsa_krylov *k, int32_t nvec, double *out);
/* residual check of Solver/eigen2.py:48-56 on the device:
 * res[i] = ||A x_i - lam_i M x_i|| / (||A x_i|| + |lam_i| ||M x_i|| + 1e-16), X on the host (n x nvec). */
int lsa_eig_residuals(lsa_ctx *ctx, const lsa_mat *A, const lsa_mat *M, int32_t nvec, const void *lam, const void *X,
                      double *res);
/* pairing of left and right eigenvectors, SLEPc's EPSGetLeftEigenvector convention a^H A = lam a^H M and the products the
 * reference forms to scale its adjoint mode (Sensitivity/__init__.py:281-287), on the device: X, Z on the host (n x nvec complex,
 * column-major), G[i + j*nvec] = z_i^H M x_j, norm_z[j] = ||z_j||, norm_mx[j] = ||M x_j||.  M == NULL: the identity (n says how
 * long the vectors are; with M it must be M's size).  The products M x_j are those of lsa_spmv, every sum is a fixed-order
 * two-stage reduction: two calls return the same bits. */
int lsa_eig_biorth(lsa_ctx *ctx, const lsa_mat *M, int64_t n, int32_t nvec, const void *X, const void *Z, void *G,
                   double *norm_z, double *norm_mx);

/* ---- the whole eigen-solve behind one call: SLEPc.EPS.solve() (Solver/utils.py:268-270) ------------------------------------------
 * Krylov-Schur outer iteration (SLEPc's default EPS: expand to ncv vectors, Schur form of the projected matrix with the wanted
 * Ritz values first, residual estimates |b^H y|, relative convergence test EPS_CONV_REL, restart with nconv + (m - nconv)/2
 * vectors) with the dense ncv x ncv algebra done by the library itself on the host (in-tree complex QR algorithm: no LAPACK
 * is needed by a consumer of this header).  lsa_hip/krylov_schur.py is the same loop in Python over LAPACK, kept as the test
 * double and for `which` policies that need callbacks. */
typedef enum {  /* EPSWhich on the eigenvalues lambda of the pencil (iEpsWhich, Solver/utils.py:152-187) */
    LSA_WHICH_LARGEST_MAGNITUDE = 1,
    LSA_WHICH_LARGEST_REAL = 3,
    LSA_WHICH_SMALLEST_REAL = 4,
    LSA_WHICH_LARGEST_IMAGINARY = 5,
    LSA_WHICH_SMALLEST_IMAGINARY = 6,
    LSA_WHICH_TARGET_MAGNITUDE = 7,
    LSA_WHICH_TARGET_REAL = 8,
    LSA_WHICH_TARGET_IMAGINARY = 9
} lsa_which;
typedef struct {
    int32_t nev;            /* eigenpairs wanted                                                                       */
    int32_t max_restarts;   /* EPS max_it                                                                              */
    double tol;             /* relative tolerance on the residual estimate of a Ritz pair                             */
    int32_t which;          /* lsa_which                                                                               */
    int32_t transform;      /* how a Ritz value theta of the operator maps to lambda: 0 = sigma + 1/theta (shift-invert),
                               1 = theta + sigma (shift), 2 = (sigma theta + nu) / (theta - 1) (Cayley)               */
    double sigma[2];        /* the operator's shift                                                                    */
    double antishift[2];    /* nu of the Cayley transform                                                              */
    double target[2];       /* target of the TARGET_* policies                                                         */
    uint64_t seed;          /* of the start vector (when v0 is NULL) and of the fresh directions after a breakdown     */
    double keep_fraction;   /* share of the unconverged part of the basis kept at a restart (0.5)                      */
} lsa_ks_options;
typedef struct {
    int32_t nconv;          /* converged pairs (may exceed nev, like EPS.getConverged())                               */
    int32_t nout;           /* pairs written: min(nconv, max_out)                                                      */
    int32_t restarts;
    int32_t pad;
    int64_t op_applies;
    double next_unconverged; /* relative residual estimate of the first pair that missed the tolerance                 */
    double seconds_expand;   /* wall time inside the Arnoldi expansions (device work + waiting for it)                 */
    double seconds_dense;    /* ... in the host's dense algebra on the projected matrix (Schur forms, reordering)      */
    double seconds_restart;  /* ... in the basis updates V <- V Q and the final Ritz vectors                           */
} lsa_ks_result;
/* n and ncv of a basis */
int lsa_krylov_shape(const lsa_krylov *k, int64_t *n, int32_t *ncv);
/* rows of a matrix handle (local rows of a shard) */
int64_t lsa_mat_rows(const lsa_mat *m);
/* The outer iteration on an existing basis (any operator: shift-invert, shift, Cayley, projected, adjoint, sharded).
 * v0: host start vector (n complex) or NULL (random from opts->seed); mask: NULL or n 0/1 doubles applied to every injected
 * vector (projected operators, padding of the sharded layout).  Outputs, wanted first: theta_out / lambda_out[max_out]
 * (complex), X_out (n x max_out complex column-major, unit 2-norm, canonical phase; NULL: no vectors), est_out[max_out]
 * relative residual estimates.  Returns LSA_OK also when fewer than nev pairs converged in max_restarts (see result). */
int lsa_krylov_solve(lsa_ctx *ctx, lsa_krylov *k, const lsa_ks_options *opts, const void *v0, const double *mask, int32_t max_out,
                     void *theta_out, void *lambda_out, void *X_out, double *est_out, lsa_ks_result *result);
/* The same iteration for J problems of one group at once (1 <= J <= 16): workspaces of one context with one n and one ncv, no
 * two of them sharing a workspace or an operator.  Problems whose Arnoldi steps run the pipelined DCGS2 tail form on factors of
 * one LU analysis advance in lockstep: a round queues one step of each such problem as ONE batched sweep pair and ONE batched
 * reduction, update and tail launch, and one read-back covers up to 16 rounds of all of them; Schur forms, convergence tests and
 * restarts run per problem on the host.  A problem whose steps take another form (or change form on the way: a missed
 * ksp_rtol, a breakdown) runs them through the code of lsa_krylov_solve, and every problem returns exactly the bits of its own
 * lsa_krylov_solve.  (The tail form needs a complex C = A - sigma M: the problems of a group with a REAL shift on real
 * matrices never advance in lockstep; all their steps run through the solo code inside this call.)  Every array argument has J entries (v0, X_out, est_out and their entries may be NULL as in the solo call);
 * status[z] is the problem's own return code -- a failing problem does not stop the others, its error text names it -- and the
 * call returns the first non-zero status (LSA_ERR_ARG at once for a bad group, with status untouched). */
typedef struct {
    int64_t rounds;               /* lockstep rounds queued                                                                 */
    int64_t launches;             /* kernel launches of those rounds: products, sweeps, reduction, update, tail             */
    int64_t periods;              /* read-backs of lockstep rounds (one synchronisation each)                               */
    double launches_per_round;    /* launches / rounds                                                                      */
    int64_t lockstep_steps[16];   /* per problem: Arnoldi steps accepted from lockstep rounds                               */
    int64_t solo_steps[16];       /* per problem: Arnoldi steps that ran alone (lsa_krylov_solve's code)                    */
} lsa_ks_batch_info;
int lsa_krylov_solve_batch(lsa_ctx *ctx, int32_t J, lsa_krylov *const *k, const lsa_ks_options *const *opts, const void *const *v0,
                           int32_t max_out, void *const *theta_out, void *const *lambda_out, void *const *X_out, double *const *est_out,
                           lsa_ks_result *results, int32_t *status, lsa_ks_batch_info *info);
/* Eigenpairs of A x = lambda M x nearest sigma in ONE call: builds and factors A - sigma M (lsa_op_create, mode 0), allocates
 * the basis, iterates, writes the pairs and releases everything.  ncv <= 0: max(2 nev, nev + 15) (SLEPc's default).  row_perm:
 * NULL, or perm[i] = the caller's index of row i (the matrices were uploaded in a permuted order, e.g. that of lsa_nd_order):
 * the vectors come back in the caller's numbering.  stats: NULL or the operator's counters. */
int lsa_eigs_sinvert(lsa_ctx *ctx, const lsa_mat *A, const lsa_mat *M, const double sigma[2], int32_t nev, int32_t ncv, double tol,
                     int32_t max_restarts, const lsa_op_options *opts, const void *v0, const int32_t *row_perm, int32_t max_out,
                     void *lambda_out, void *X_out, double *est_out, lsa_ks_result *result, lsa_stats *stats);
/* The dense kernels of that iteration, for tests (host only; complex column-major):
 *   lsa_dense_schur: A = Q T Q^H, T (upper triangular) over A, Q written; LSA_ERR_DIVERGED if the QR algorithm stalls
 *   lsa_dense_schur_reorder: the diagonal entries with select[k] != 0 move to the leading block (orders kept), T and Q updated
 *   lsa_dense_tri_eigenvectors: right eigenvectors of the upper triangular T, unit 2-norm columns of S */
int lsa_dense_schur(int32_t n, void *A, int32_t lda, void *Q, int32_t ldq);
/* Inertia of a dense real symmetric matrix (column-major, both triangles read and symmetrised; host only): Bunch-Kaufman diagonal
 * pivoting; pivots below tol_rel * max|A| count as zero.  The building block of lsa_ndlu_inertia. */
int lsa_dense_sym_inertia(int32_t n, const double *A, int32_t lda, double tol_rel, int64_t *negative, int64_t *zero, int64_t *positive);
int lsa_dense_schur_reorder(int32_t n, void *T, int32_t ldt, void *Q, int32_t ldq, const int32_t *select, int32_t *nselected);
int lsa_dense_tri_eigenvectors(int32_t n, const void *T, int32_t ldt, void *S, int32_t lds);

/* ---- symmetric-definite problems: SLEPc EPS Krylov-Schur, symmetric variant with B-inner product (EPS_GHEP / EPS_HEP,
 * Solver/utils.py:244-270 with iEpsProblemType.GHEP; Elasticity/utils.py:141-155) -------------------------------------------------
 * Thick-restart Lanczos for OP = (K - sigma M)^-1 M, sigma real, which is self-adjoint in the M-inner product.  Everything on the
 * device is float64: a real basis V with V^T M V = I, a real symmetric projected matrix, real eigenvalues, M-orthonormal vectors.
 * The operator handle is the one of the general path (lsa_op_create, mode 0); its factors must be real and exact (pc_type 2). */
typedef struct lsa_lanczos lsa_lanczos;   /* SLEPc EPS Krylov-Schur, symmetric variant with B-inner product (GHEP) */
/* Basis of ncv + 1 real vectors (SLEPc.BV with BVSetMatrix(M)).  LSA_ERR_ARG unless the operator is shift-invert with real
 * exact factors, forward, unprojected, on one rank. */
int lsa_lanczos_create(lsa_ctx *ctx, lsa_op *op, int32_t ncv, lsa_lanczos **out);
void lsa_lanczos_destroy(lsa_lanczos *l);
/* as lsa_krylov_set_row_permutation: the vectors of lsa_lanczos_solve leave in the caller's numbering */
int lsa_lanczos_set_row_permutation(lsa_ctx *ctx, lsa_lanczos *l, const int32_t *perm);
/* v_0 = v / sqrt(v^T M v) (host real vector of length n), M-normalised on the device (BVInsertVec + BVNormColumn);
 * LSA_ERR_ARG when v^T M v is not positive */
int lsa_lanczos_set_start(lsa_ctx *ctx, lsa_lanczos *l, const double *host_v);
/* Lanczos steps j = j0 .. j1-1 (EPSFullLanczos / BVOrthogonalize with the B-inner product): w = OP v_j, two passes of classical
 * Gram-Schmidt against v_0..v_j in the M-inner product, v_{j+1} = w / beta_j.  T is the caller's (ncv+1) x ncv column-major real
 * matrix (ldt >= j1 + 1): T[j, j] = alpha_j, T[j+1, j] = beta_j and, for j + 1 < ncv, T[j, j+1] = beta_j are written; every other
 * entry is the caller's.  *breakdown = step index if beta_j vanished (invariant subspace), else -1.  LSA_ERR_ARG when w^T M w is
 * not positive (M is not positive definite on the Krylov space), LSA_ERR_DIVERGED when an inner solve misses the operator's
 * ksp_rtol after one refinement step. */
int lsa_lanczos_extend(lsa_ctx *ctx, lsa_lanczos *l, int32_t j0, int32_t j1, double *T, int32_t ldt, int32_t *breakdown);
/* the first ncols columns of the basis, in the basis' own row numbering (n x ncols column-major on the host); for tests (BVGetColumn) */
int lsa_lanczos_basis(lsa_ctx *ctx, const lsa_lanczos *l, int32_t ncols, double *host_V);
/* The whole iteration (SLEPc.EPS.solve() with EPS_GHEP): expand to ncv vectors, eigen-decomposition of the projected matrix
 * (lsa_dense_syev), Ritz values ranked by opts->which on lambda = sigma + 1/theta, residual estimates |beta y_mi| / |theta_i|
 * against opts->tol, thick restart with nconv + (m - nconv) keep_fraction vectors.  opts->transform must be 0 and the imaginary
 * parts of sigma and target 0.  v0: host start vector (n doubles) or NULL (random from opts->seed).  Outputs, wanted first:
 * theta_out / lambda_out[max_out] (real), X_out (n x max_out real column-major, x^T M x = 1, the entry of largest magnitude
 * positive; NULL: no vectors), est_out[max_out].  Returns LSA_OK also when fewer than nev pairs converged (see result). */
int lsa_lanczos_solve(lsa_ctx *ctx, lsa_lanczos *l, const lsa_ks_options *opts, const double *v0, int32_t max_out,
                      double *theta_out, double *lambda_out, double *X_out, double *est_out, lsa_ks_result *result);
/* The dense kernel of that iteration (host only; LAPACK's dsyev, which SLEPc's DS of type HEP calls): real symmetric A (n x n
 * column-major, lower triangle read), eigenvalues ascending in w, orthonormal eigenvectors over A.  Householder
 * tridiagonalisation + implicit QL.  LSA_ERR_DIVERGED if the QL iteration stalls. */
int lsa_dense_syev(int32_t n, double *A, int32_t lda, double *w);

/* ---- resolvent (input-output) analysis: optimal gains, responses and forcings of M q' = A q + M f at a frequency omega -------------
 * With R = (i omega M - A)^-1 the gains sigma_1 >= sigma_2 >= ... are the maxima of ||q||_M / ||f||_M over q = R M f; sigma_j^2
 * are the largest eigenvalues of W = R M R^H M = C^-1 M C^-H M, C = A - i omega M, which is self-adjoint and non-negative in the
 * M-(semi-)inner product.  The iteration is the thick-restart Lanczos of lsa_lanczos_* with a complex basis, V^H M V = I, and the
 * same real symmetric projected matrix; both inner solves of a step run on ONE factorisation of C.  The operator handle is the
 * one of the general path: lsa_op_create, mode 0, sigma = (0, omega), pc_type 2, M real symmetric positive semidefinite. */
typedef struct lsa_resolvent lsa_resolvent;
/* Basis of ncv + 1 complex vectors.  LSA_ERR_ARG, with a message that names the condition, unless the operator is shift-invert
 * (mode 0) with M, M real, exact factors (real for omega = 0, else complex), forward, unprojected, on one rank. */
int lsa_resolvent_create(lsa_ctx *ctx, lsa_op *op, int32_t ncv, lsa_resolvent **out);
void lsa_resolvent_destroy(lsa_resolvent *r);
/* as lsa_krylov_set_row_permutation: the vectors of lsa_resolvent_solve leave in the caller's numbering */
int lsa_resolvent_set_row_permutation(lsa_ctx *ctx, lsa_resolvent *r, const int32_t *perm);
/* on != 0: the forcings of lsa_resolvent_solve send their adjoint solves through ONE block solve on the factors (the wide passes of
 * lsa_ndlu_solve_multi with trans = 2), each checked as before from one read-back; from the first column that misses ksp_rtol on
 * the columns finish one by one with the refinement step.  Gains, forcings and the solve counts are those of the default (off),
 * bit for bit.  The block's 2 nvec work vectors are made by the first such call; where they do not fit, the columns run one by one. */
int lsa_resolvent_set_block_forcings(lsa_ctx *ctx, lsa_resolvent *r, int on);
/* Forcing weight Qf and response weight Qq in place of M (NULL: M): real symmetric positive semidefinite n x n matrices of any
 * pattern, e.g. the windowed D M D of lsa_csr_window.  The response is q = R Qf f (the weak form: the forcing enters through its own
 * mass matrix), the gains are the maxima of ||q||_Qq / ||f||_Qf, and sigma_j^2 are the non-zero eigenvalues of
 * W = C^-1 Qf C^-H Qq, self-adjoint in the Qq-semi-inner product: no inverse of a weight appears and a step has the launches it had
 * (rhs = Qq v, tm = Qf z, t = Qq w).  The basis and the responses are Qq-orthonormal, the forcings f_j = -C^-H Qq q_j / sigma_j are
 * Qf-orthonormal (only Qf f_j is determined).  The matrices are BORROWED: they must outlive the handle.  The call begins anew as
 * lsa_growth_set_steps does: no right-hand side is left over, and lsa_resolvent_set_start (or lsa_resolvent_solve) must follow.
 * With no weights set every call returns the bits it returned before weights existed.  LSA_ERR_ARG, naming the function, for a
 * complex matrix or one of another size. */
int lsa_resolvent_set_weights(lsa_ctx *ctx, lsa_resolvent *r, const lsa_mat *Qf, const lsa_mat *Qq);
/* v_0 = v / sqrt(v^H Qq v) (host complex vector of length n; Qq = M unless lsa_resolvent_set_weights gave another), normalised on
 * the device; LSA_ERR_ARG when v^H Qq v is not positive */
int lsa_resolvent_set_start(lsa_ctx *ctx, lsa_resolvent *r, const void *host_v);
/* Lanczos steps j = j0 .. j1-1 on W: z = C^-H M v_j, w = C^-1 M z, two passes of classical Gram-Schmidt against v_0..v_j in the
 * M-inner product, v_{j+1} = w / beta_j.  T is the caller's (ncv+1) x ncv column-major REAL matrix (ldt >= j1 + 1), written as by
 * lsa_lanczos_extend: alpha_j = Re v_j^H M W v_j (the imaginary part is rounding and is dropped), beta_j > 0.  Both solves are
 * checked against the operator's ksp_rtol, each direction with its own refinement step once one of its solves missed it;
 * LSA_ERR_DIVERGED when a solve misses it after that step, LSA_ERR_ARG when w^H M w is negative.  For tests. */
int lsa_resolvent_extend(lsa_ctx *ctx, lsa_resolvent *r, int32_t j0, int32_t j1, double *T, int32_t ldt, int32_t *breakdown);
/* the first ncols columns of the basis, in the basis' own row numbering (n x ncols complex column-major on the host); for tests */
int lsa_resolvent_basis(lsa_ctx *ctx, const lsa_resolvent *r, int32_t ncols, void *host_V);
/* The whole iteration, through the loop of lsa_lanczos_solve: Ritz values ranked largest first, accepted on |beta y_mi| / theta_i <=
 * opts->tol; of opts only nev, max_restarts, tol, seed and keep_fraction are read.  v0: host start vector (n complex) or NULL
 * (random from opts->seed).  Outputs, largest gain first: theta_out[max_out] = sigma_j^2, gain_out[max_out] = sigma_j, Q_out the
 * responses (n x max_out complex column-major, q_j^H M q_k = delta_jk, the entry of largest magnitude real positive; NULL: none),
 * F_out the forcings f_j = R^H M q_j / sigma_j (same shape, f_j^H M f_k = delta_jk, R M f_j = sigma_j q_j; one checked adjoint
 * solve each after convergence; needs Q_out; NULL: none), est_out[max_out].  counts (NULL or 4 entries): accepted adjoint and
 * forward solves of this handle so far, and how many of each carried the refinement step.  Returns LSA_OK also when fewer than nev
 * gains converged (see result).  Under lsa_resolvent_set_weights read Qq for M in Q_out's norms and Qf in F_out's, and R Qf f_j =
 * sigma_j q_j.  The shift of the operator may be any complex number: sigma = (beta, omega) gives the discounted resolvent
 * ((beta + i omega) M - A)^-1, and 1 / sigma_1 at a point z is the epsilon-level of the energy-norm pseudospectrum there. */
int lsa_resolvent_solve(lsa_ctx *ctx, lsa_resolvent *r, const lsa_ks_options *opts, const void *v0, int32_t max_out, double *theta_out,
                        double *gain_out, void *Q_out, void *F_out, double *est_out, lsa_ks_result *result, int64_t *counts);
/* ---- lockstep sweeps: up to 16 frequencies of one sweep advance together ------------------------------------------------------------
 * lsa_resolvent_extend for the active members of a group (active NULL: all), member z from its own j0[z] to the common j1 into its own
 * T[z].  Members whose factors are complex and of one LU analysis (the pattern-only phase redone on the lead's analysis), whose step
 * runs the fused kernels (LSA_LANCZOS_FUSED) and whose refinement steps are off advance in ROUNDS: one step of every member that
 * still has one as ONE launch per launch of a solo step -- the adjoint sweeps of all factor sets, C_k^H z_k (the batched transposed
 * product), Q_f z_k (lsa_spmv_batch's kernel), the forward sweeps, C_k w_k, then per Gram-Schmidt pass the Q_q product, the batched
 * reduction and the batched update, the last product and reduction and the batched tail -- and ONE copy of all members' slots behind
 * ONE synchronisation.  The number of basis columns is per member; a member at j1 waits.  A member outside the set (real factors, another
 * analysis, refinement on), or one whose solve misses ksp_rtol in a round, runs its steps through lsa_resolvent_extend's code inside
 * this call.  Every member is left with exactly the bits of its own lsa_resolvent_extend.  status[z] / breakdown[z] per member: a
 * failing member does not stop the others, its text names it; the call returns the first non-zero status.  LSA_ERR_ARG at once, with
 * a text, for J outside [1, 16], a null handle, a handle or an operator given twice, handles of another context, differing n or ncv,
 * or weights on more than one pattern.  For tests. */
int lsa_resolvent_extend_batch(lsa_ctx *ctx, int32_t J, lsa_resolvent *const *r, const uint8_t *active, const int32_t *j0, int32_t j1,
                               double *const *T, int32_t ldt, int32_t *breakdown, int32_t *status);
/* lsa_resolvent_solve for J members of a group: the expansions through the rounds above, Ritz values, convergence tests and restarts
 * per member on the host; nev, tol and max_restarts may differ between the members.  A member that converges or exhausts its restarts
 * forms its responses and forcings on its own factor set (lsa_resolvent_set_block_forcings honoured) and leaves while the rest go on.
 * Every array argument has J entries (v0, Q_out, F_out, est_out and their entries may be NULL as in the solo call; counts: NULL or
 * 4 J entries); every member returns exactly the bits of its own lsa_resolvent_solve.  info (NULL or the record of
 * lsa_krylov_solve_batch): rounds, launches, read-backs, and per member the steps accepted from rounds and the steps that ran alone,
 * whose sum is the member's operator applies.  Errors as lsa_resolvent_extend_batch, and F_out[z] without Q_out[z]. */
int lsa_resolvent_solve_batch(lsa_ctx *ctx, int32_t J, lsa_resolvent *const *r, const lsa_ks_options *const *opts, const void *const *v0,
                              int32_t max_out, double *const *theta_out, double *const *gain_out, void *const *Q_out, void *const *F_out,
                              double *const *est_out, lsa_ks_result *results, int64_t *counts, int32_t *status, lsa_ks_batch_info *info);

/* ---- transient growth: optimal energy gains and initial conditions of M q' = A q over a finite horizon ---------------------------
 * One implicit-Euler step (M - dt A) q+ = M q is q+ = -sigma C^-1 M q with C = A - sigma M, sigma = 1 / dt; over N steps the propagator
 * is Phi = (-sigma C^-1 M)^N and its adjoint in the M-inner product Phi+ = (-sigma C^-T M)^N, on the same factors.  The gains
 * G_1 >= G_2 >= ... = max ||q(N dt)||_M^2 / ||q(0)||_M^2 are the largest eigenvalues of W = Phi+ Phi: the thick-restart Lanczos iteration
 * of lsa_lanczos_* with a real M-orthonormal basis and a march of 2N solves on ONE factorisation of C behind every step.  The
 * operator handle is the one of the general path: lsa_op_create, mode 0, sigma = (1 / dt, 0), pc_type 2, A and M real, M symmetric
 * positive semidefinite. */
typedef struct lsa_growth lsa_growth;
/* Basis of ncv + 1 real vectors for horizons of nsteps >= 1 steps.  keep: host array of n doubles in {0, 1}, or NULL for all ones:
 * rows with 0 (constrained dofs, each decoupled in row and column of A and M) are left out of the flow -- every right-hand side of
 * the march and every start vector is multiplied by it.  LSA_ERR_ARG, with a message that names the condition, unless the operator
 * is shift-invert (mode 0) with M, M real, real exact factors, forward, unprojected, on one rank, at a real positive shift. */
int lsa_growth_create(lsa_ctx *ctx, lsa_op *op, int32_t ncv, int32_t nsteps, const double *keep, lsa_growth **out);
void lsa_growth_destroy(lsa_growth *g);
/* as lsa_krylov_set_row_permutation: the vectors of lsa_growth_solve leave in the caller's numbering (keep and the start vectors
 * are in the basis' own) */
int lsa_growth_set_row_permutation(lsa_ctx *ctx, lsa_growth *g, const int32_t *perm);
/* another horizon on the same handle and factors; what follows gives the bytes a new handle with this nsteps gives */
int lsa_growth_set_steps(lsa_ctx *ctx, lsa_growth *g, int32_t nsteps);
/* The time-stepping scheme behind the march.  LSA_GROWTH_EULER (what a new handle has): implicit Euler as above, first order in dt.
 * LSA_GROWTH_SDIRK2: the L-stable, stiffly accurate two-stage singly diagonally implicit Runge-Kutta method with gamma = 1 - 1/sqrt(2),
 * second order in dt.  Both of its stages solve with M - gamma dt A, so the library takes sigma from the operator as before and the
 * time step it stands for is dt = 1 / (gamma sigma): the caller builds the operator at sigma = 1 / (gamma dt).  With S = -sigma C^-1 M one
 * time step is Phi_1 = S (a S + b I), a = 1 + sqrt(2), b = -sqrt(2), and its M-adjoint the same with C^-T: every time step is two
 * solves (lsa_growth_extend: 2N forward and 2N transposed per step; lsa_growth_solve's final march: 2N per vector, energy_out at the
 * second stage of each time step), each of them checked as under Euler.  Like lsa_growth_set_steps it begins anew: what follows
 * gives the bytes a new handle set to this scheme gives.  LSA_ERR_ARG, naming the scheme, for any other code. */
enum { LSA_GROWTH_EULER = 0, LSA_GROWTH_SDIRK2 = 1 };
int lsa_growth_set_scheme(lsa_ctx *ctx, lsa_growth *g, int32_t scheme);
/* Response weight Q (NULL: M; real symmetric positive semidefinite, n x n, any pattern; BORROWED: it outlives the handle): the gains
 * become the maxima of ||q(T)||_Q^2 / ||q(0)||_M^2, the largest eigenvalues of W = M^-1 Phi^T Q Phi.  No inverse appears: the march of a
 * step turns around on -sigma keep (.) (Q x) instead of -sigma keep (.) (M x) after its last forward solve (index N - 1, N = stages *
 * nsteps; log entry N - 1 then holds the windowed energy at T); nothing else in the march changes, under either scheme.  The basis
 * and the initial conditions stay M-orthonormal.  Begins anew like lsa_growth_set_scheme.  LSA_ERR_ARG, naming the function, for a
 * complex matrix or one of another size.  (An initial-condition weight would need Q^-1 and is not built.) */
int lsa_growth_set_response_weight(lsa_ctx *ctx, lsa_growth *g, const lsa_mat *Q);
/* out[j] = (Phi q0_j)^T Q (Phi q0_j), j < nvec, of the responses the last lsa_growth_solve marched (one more product and dot per mode
 * in its final marches); with no response weight the M-energy at T, energy_out[j (N + 1) + N].  LSA_ERR_ARG when nvec exceeds what
 * that call marched. */
int lsa_growth_response_energy(lsa_ctx *ctx, const lsa_growth *g, int32_t nvec, double *out);
/* v_0 = keep (.) v, M-normalised on the device (host vector of length n); LSA_ERR_ARG when its M-norm is not positive */
int lsa_growth_set_start(lsa_ctx *ctx, lsa_growth *g, const double *host_v);
/* Lanczos steps j = j0 .. j1-1 on W: N forward and N transposed solves, each followed by a product with M, the mask and the factor
 * -sigma; then the reorthogonalisation and tail of lsa_lanczos_extend.  T as there ((ncv+1) x ncv column-major, ldt >= j1 + 1).
 * Every solve of the march is checked against the operator's ksp_rtol -- the last one in the step's first reduction, the others
 * through a device log read back with the step's slot: one host synchronisation per step -- each direction with its own refinement
 * step once one of its solves missed; LSA_ERR_DIVERGED (naming direction, march index and step) when a solve misses after it. */
int lsa_growth_extend(lsa_ctx *ctx, lsa_growth *g, int32_t j0, int32_t j1, double *T, int32_t ldt, int32_t *breakdown);
/* the first ncols columns of the basis, in the basis' own row numbering (n x ncols column-major on the host); for tests */
int lsa_growth_basis(lsa_ctx *ctx, const lsa_growth *g, int32_t ncols, double *host_V);
/* The whole iteration, through the loop of lsa_lanczos_solve: Ritz values ranked largest first, accepted on |beta y_mi| / theta_i <=
 * opts->tol; of opts only nev, max_restarts, tol, seed and keep_fraction are read.  v0: host start vector (n doubles) or NULL (random
 * from opts->seed).  Outputs, largest gain first: theta_out[max_out] = gain_out[max_out] = G_j; Q0_out the optimal initial conditions
 * (n x max_out column-major, M-orthonormal, zero on masked rows, the entry of largest magnitude positive; NULL: none); QT_out the
 * responses Phi q0_j, not normalised (same shape; needs Q0_out; NULL: none); energy_out[j (N + 1) + s] = ||Phi_s q0_j||_M^2 for
 * s = 0..N (needs Q0_out; NULL: none) -- responses and energies from one more forward march of N checked solves per vector;
 * est_out[max_out].  counts (NULL or 4 entries): accepted forward and transposed solves of this handle so far, and how many of
 * each carried the refinement step.  Returns LSA_OK also when fewer than nev gains converged (see result).  Under a response weight
 * (lsa_growth_set_response_weight) gain_out holds the weighted gains, energy_out stays the whole-domain M-energy curve, and
 * lsa_growth_response_energy gives the weighted energy at T. */
int lsa_growth_solve(lsa_ctx *ctx, lsa_growth *g, const lsa_ks_options *opts, const double *v0, int32_t max_out, double *theta_out,
                     double *gain_out, double *Q0_out, double *QT_out, double *energy_out, double *est_out, lsa_ks_result *result,
                     int64_t *counts);

/* ---- region eigensolver: all eigenvalues inside a contour, with a count (what SLEPc answers with EPSCISS and an RG region; the
 * reference's door to it is iEpsSolver.set_interval_complex, Solver/utils.py:252-254) ------------------------------------------------
 * Contour-integral (FEAST-type) subspace iteration for A x = lambda M x on an ellipse with centre c and semi-axes rx, ry: nodes
 * z_k = c + rx cos t_k + i ry sin t_k, t_k = 2 pi (k + 1/2) / N (none on the real axis), weights w_k = (ry cos t_k + i rx sin t_k) / N.
 * One iteration on the n x L complex block Y: B = M Y; Q = -sum_k w_k C_k^-1 B with C_k = A - z_k M factorised by the
 * nested-dissection LU on ONE ordering and ONE pattern-only analysis (block solves in lsa_ndlu_solve_multi's passes); U = Q
 * orthonormalised twice through its Gram matrix (directions below 1e-14 of the largest Gram eigenvalue are dropped: the rank may
 * shrink); Ritz pairs of (U^H A U, U^H M U); residuals ||A x - lam M x|| / (||A x|| + |lam| ||M x||).  It stops when every Ritz
 * value inside the ellipse has a residual <= tol (with none inside: from the second iteration on), or at max_it.  Every sum runs in a fixed order without atomics: two runs return
 * the same bits, and so do kept and refactorised factor sets.
 * The spectrum must not crowd the subspace: the iteration contracts like the quadrature's filter at the (L+1)-th nearest eigenvalue,
 * so L has to exceed the count inside generously (dense spectra: by half as much again or more); `complete` says whether it did. */
/* The two building blocks on lsa_vec blocks.  Blocks are column-major in ONE complex128 vector each: column c starts at c * ld
 * scalars, ld >= n, the vector at least ld (cols - 1) + n long; anything else is LSA_ERR_ARG. */
/* Y[:, 0:ncols] = A X[:, 0:ncols]: MatMatMult on a dense block.  A whole square matrix (no row shard), float64 or complex128; X and Y
 * apart.  Every pass of up to 8 columns reads A's indices and values once.  The sums are not in lsa_spmv's order: column c need not
 * hold lsa_spmv's bits. */
int lsa_spmm(lsa_ctx *ctx, const lsa_mat *A, int32_t ncols, const lsa_vec *X, int64_t ldx, lsa_vec *Y, int64_t ldy);
/* Y[:, 0:ncols] = A^T X[:, 0:ncols] (conj = 0) or A^H X[:, 0:ncols] (conj != 0): MatTransposeMatMult on a dense block, under the block
 * rules of lsa_spmm.  It runs in pull form on the transposed index the matrices of one pattern share (built by the first transposed
 * product): no atomics, every output's entries added in a fixed order, every pass of up to 8 columns reading the index and the values
 * once.  Like lsa_spmm it need not reproduce lsa_spmv_transpose's bits. */
int lsa_spmm_transpose(lsa_ctx *ctx, const lsa_mat *A, int conj, int32_t ncols, const lsa_vec *X, int64_t ldx, lsa_vec *Y, int64_t ldy);
/* G = U^H W over the first n rows: U has p columns, W has q, 1 <= p, q <= 128; G is the caller's p x q column-major complex host
 * array.  Per-workgroup partial sums, then one finishing pass in chunk order; synchronises.  U and W one and the same block
 * (same vector, ld and column count): the diagonal is returned exactly real. */
int lsa_block_gram(lsa_ctx *ctx, int64_t n, int32_t p, const lsa_vec *U, int64_t ldu, int32_t q, const lsa_vec *W, int64_t ldw, void *G);
typedef struct lsa_contour lsa_contour;
/* what the left phases of a handle did, booked apart from lsa_contour_info / lsa_contour_batch_info (which a left phase leaves as they were) */
typedef struct {
    int32_t solves;            /* lsa_contour_solve_left calls so far                                                     */
    int32_t iterations;        /* their iterations                                                                        */
    int64_t block_solves;      /* column solves with C_k^H accepted                                                       */
    int64_t refined_solves;    /* ... of them with the refinement step                                                    */
    int64_t backward_accepted; /* ... accepted on the backward error                                                      */
    int64_t groups;            /* as lsa_contour_batch_stats, the left phases only                                        */
    int64_t batched_columns;
    int64_t serial_columns;
    double seconds_factor;     /* refactorisations during the left phases (one set refactorised node by node)            */
    double seconds_solve;
    double seconds_product;
    double seconds_gram;
    double seconds_dense;
} lsa_contour_left_stats;
typedef struct {
    int32_t iterations;        /* iterations run                                                                          */
    int32_t rank;              /* columns of the last orthonormal basis (<= subspace)                                     */
    int32_t inside;            /* Ritz values inside the ellipse in the last iteration                                    */
    int32_t converged_inside;  /* ... of them with residual <= tol                                                        */
    int32_t complete;          /* 1: stopped because all inside had converged AND inside < rank (spare directions left)   */
    int32_t nout;              /* pairs written: min(inside, max_out)                                                     */
    double estimate;           /* Re sum_j y_j^H q_j / L at iteration 0: stochastic estimate of the count inside (sizing) */
    int64_t block_solves;      /* accepted column solves (nodes x columns x iterations)                                   */
    int64_t refined_solves;    /* ... that carried the refinement step                                                    */
    int64_t backward_accepted; /* ... accepted on the backward error                                                      */
    double worst_rel_res;      /* worst ||b - C_k x|| / ||b|| of an accepted column solve                                 */
} lsa_contour_result;
typedef struct {
    int32_t kept;              /* 1: N factor sets alive; 0: one set refactorised node by node in every iteration          */
    int32_t nodes;
    int64_t bytes;             /* device bytes of the six n x L blocks, the N value arrays of C_k and the small buffers
                                  (the factor sets: lsa_ndlu_info / lsa_ndlu_prepared_memory)                              */
    double seconds_factor;     /* building C_k, factorising (creation) and refactorising (solves)                          */
    double seconds_solve;      /* block solves with their checks and refinement steps                                      */
    double seconds_product;    /* M Y, A U, M U, the Ritz blocks and their residual sums                                   */
    double seconds_gram;       /* Gram matrices and basis updates                                                          */
    double seconds_dense;      /* host: Hermitian eigen-decompositions, the reduced problem                                */
    lsa_stats solver;          /* counters of the column solves (op_applies, refined_solves, backward_accepted, max_rel_res, ...) */
} lsa_contour_stats;
/* A, M: the pencil on one shared pattern (M real), both outliving the handle.  Builds C_k = A - z_k M for the N nodes and
 * factorises: keep_factors != 0 keeps N factor sets (every set after the first redoes the pattern-only phase from the first one's
 * forest), 0 keeps one and refactorises it node by node in every iteration; both return the same bits.  The first set takes the
 * analysis the context holds prepared (lsa_ndlu_prepare / lsa_ndlu_prepare_tree with LSA_C128).  ksp_rtol: what every column of
 * every block solve must reach (||b - C_k x|| <= ksp_rtol ||b||; one refinement step on a miss, kept for that node from then on;
 * then a backward error <= 1e-12 ||C_k||_F ||x||; else LSA_ERR_DIVERGED naming node and column).  LSA_ERR_ARG, naming the condition:
 * several ranks, a missing or complex M, nodes < 4 or odd, subspace < 2, > 128 or > n, radii not positive.  A node on an eigenvalue:
 * LSA_ERR_ZERO_PIVOT with the node's index in the message. */
int lsa_contour_create(lsa_ctx *ctx, const lsa_mat *A, const lsa_mat *M, int32_t nodes, const double centre[2], const double radii[2],
                       int32_t subspace, int keep_factors, double ksp_rtol, lsa_contour **out);
void lsa_contour_destroy(lsa_contour *h);
/* as lsa_krylov_set_row_permutation: the vectors of lsa_contour_solve leave in the caller's numbering (Y0 is in the matrices' own) */
int lsa_contour_set_row_permutation(lsa_ctx *ctx, lsa_contour *h, const int32_t *perm);
/* The iteration from the start block Y0 (host, n x subspace complex column-major).  Outputs: the Ritz pairs INSIDE the ellipse of the
 * last iteration, nearest the centre (in the ellipse's metric) first: lam_out[max_out] complex, X_out (n x max_out complex
 * column-major, unit 2-norm, canonical phase, the caller's row numbering; NULL: none), res_out[max_out].  LSA_OK also when the
 * iteration ended at max_it or with a full subspace (see result->complete). */
int lsa_contour_solve(lsa_ctx *ctx, lsa_contour *h, double tol, int32_t max_it, const void *Y0_host, int32_t max_out, void *lam_out,
                      void *X_out, double *res_out, lsa_contour_result *result);
int lsa_contour_info(const lsa_contour *h, lsa_contour_stats *out);
/* on != 0: an iteration solves the block B = M Y on the nodes in lockstep -- the nodes that do not carry the refinement step in runs
 * of at most 16 factor sets of one analysis, each run one lsa_ndlu_solve_multi_batch from the shared B -- and then checks and
 * accumulates node by node in node order as before.  A node that carries the refinement step, or has a column that misses ksp_rtol,
 * goes through the node-by-node solve (which solves again to the same bits, then refines), so results, verdicts, counters and
 * error texts are those of the default, byte for byte.  Needs keep_factors (LSA_ERR_ARG without) and one n x subspace solution
 * block per node: nodes * n * subspace * 16 bytes, counted into lsa_contour_stats.bytes (LSA_ERR_OOM with the bytes needed and free
 * where they do not fit; the switch then stays off).  on = 0 releases the blocks.  Off by default. */
int lsa_contour_set_batch_nodes(lsa_ctx *ctx, lsa_contour *h, int on);
typedef struct {
    int32_t enabled;           /* 1: lsa_contour_set_batch_nodes is on                                                     */
    int32_t pad0;
    int64_t groups;            /* batched groups launched: multi-column passes of lsa_ndlu_solve_multi_batch, per run of nodes */
    int64_t batched_columns;   /* column solves (node x column) done in those                                              */
    int64_t serial_columns;    /* column solves done node by node (repeated ones of a fall-back included)                  */
} lsa_contour_batch_stats;
int lsa_contour_batch_info(const lsa_contour *h, lsa_contour_batch_stats *out);
/* The left phase on the same handle and the same factor sets: the iteration of lsa_contour_solve on the adjoint pencil (A^H, M^H),
 * whose node matrices on the conjugate contour are C_k^H -- no factorisation, no analysis, no new device memory.  One iteration on the
 * block Y: B = M^H Y (lsa_spmm_transpose's kernel); Q = -sum_k conj(w_k) C_k^-H B (the transposed block sweeps; under
 * lsa_contour_set_batch_nodes runs of up to 16 sets through those of lsa_ndlu_solve_multi_batch_adjoint); U = Q orthonormalised
 * twice; Ritz pairs (mu, s) of (U^H A^H U, U^H M^H U), residual ||A^H w - mu M^H w|| / (||A^H w|| + |mu| ||M^H w||), inside when
 * conj(mu) lies in the ellipse.  Every column solve is checked against C_k^H x as the right phase checks against C_k x, with the
 * nodes' adjoint refinement flags.  Stopping rule, `complete`, `estimate`, counters, output order and canonical phase are those of
 * lsa_contour_solve; lam_out holds lambda = conj(mu), the values in the caller's region, W_out the left eigenvectors
 * (w^H A = lambda w^H M).  Kept, refactorised and lockstep factor sets return the same bytes.  The handle's own books
 * (lsa_contour_info, lsa_contour_batch_info) are left as they were: the left phases' go to lsa_contour_left_info. */
int lsa_contour_solve_left(lsa_ctx *ctx, lsa_contour *h, double tol, int32_t max_it, const void *Y0_host, int32_t max_out, void *lam_out,
                           void *W_out, double *res_out, lsa_contour_result *result);
int lsa_contour_left_info(const lsa_contour *h, lsa_contour_left_stats *out);

/* ---- stochastic forcing: EOFs and stochastic optimals of M q' = A q + f on a frequency quadrature ----------------------------------
 * Under forcing that is white in time with spatial covariance weight Q_f, the response covariance of a stable (A, M) is
 * P = (1 / 2 pi) int R Q_f R^H d omega with R(z) = (z M - A)^-1.  The variance carried by a structure, measured in Q_q, is an
 * eigenvalue of P Q_q = (1 / 2 pi) int W(i omega) d omega with W(z) = C^-1 Q_f C^-H Q_q, C = A - z M: the step of lsa_resolvent_*.  For
 * real A, M, W(conj z) = conj W(z), so the integral over the whole axis is the real operator
 *     S = (1 / pi) sum_k w_k Re W(z_k)     over nodes z_k = beta + i omega_k, omega_k >= 0, weights w_k > 0,
 * self-adjoint in the Q_q-semi-inner product: a real thick-restart Lanczos iteration (lsa_lanczos_*' basis and loop) with N kept
 * factorisations of A - z_k M behind every step.  The results are those of the QUADRATURE operator S the caller gives: whether N
 * nodes resolve the integral is the caller's to check (sharp resonances need many nodes, or a discount beta > 0, which smooths the
 * integrand as it does for the resolvent). */
/* Y[:, k] = (A - z_k M) X[:, k] for k < nodes in ONE launch: A, M real on one shared pattern (whole square matrices), shifts[2 k],
 * shifts[2 k + 1] = Re, Im z_k on the host, X and Y complex128 vectors of at least n * nodes entries holding n x nodes column-major
 * blocks (leading dimension n), apart.  Every non-zero's column index and two real values are read once for up to 16 columns.  The
 * entries of a row are strided over 8 lanes, each adding its own in order, then a fixed tree: the same bits on every call.
 * The check product of the forward solves of a stochastic-forcing step; exported for tests. */
int lsa_shifted_spmm(lsa_ctx *ctx, const lsa_mat *A, const lsa_mat *M, int32_t nodes, const double *shifts, const lsa_vec *X, lsa_vec *Y);
/* Y[:, c] = (A - z_c M)^H X[:, c] for c < nodes in ONE launch, on the transposed index of the shared pattern (built on first use, as
 * for lsa_spmv_transpose); arguments, checks and messages as lsa_shifted_spmm.  Every non-zero's row index, source position and two
 * real values are read once for up to 16 columns; the entries of an output row are strided over 8 lanes, each adding its own in
 * order, then a fixed tree: the same bits on every call, not those of lsa_spmv_transpose (another summation order).  The check
 * product of the adjoint block solves of lsa_stochastic_trace; exported for tests. */
int lsa_shifted_spmm_transpose(lsa_ctx *ctx, const lsa_mat *A, const lsa_mat *M, int32_t nodes, const double *shifts, const lsa_vec *X, lsa_vec *Y);
typedef struct lsa_stochastic lsa_stochastic;
typedef struct {
    int32_t nodes;
    int32_t kind;              /* 0: EOFs, 1: stochastic optimals                                                          */
    int64_t bytes;             /* device bytes: the N value arrays of C_k, the N factor sets, the n x N blocks, the basis   */
    double seconds_factor;     /* building C_k and factorising (creation)                                                  */
    double seconds_solve;      /* device seconds of the sweeps of all steps and applies (HIP events around the phases)      */
    double seconds_product;    /* device seconds of their check products, weight products, sums and the accumulation       */
    double seconds_dense;      /* host seconds of the loop's dense eigen-solves (lsa_stochastic_solve)                      */
    lsa_stats solver;          /* counters of the inner solves (op_applies, refined_solves, backward_accepted, max_rel_res) */
    int32_t batch_adjoint;     /* lsa_stochastic_set_batch_adjoint is on                                                    */
    int64_t adjoint_batches;   /* grouped calls of the batched transposed sweeps with more than one set, since creation     */
    int64_t forward_batches;   /* ... and of the batched forward sweeps                                                     */
    double seconds_solve_adjoint;   /* the adjoint sweeps' share of seconds_solve                                           */
    double seconds_product_adjoint; /* the adjoint check products' share of seconds_product                                 */
} lsa_stochastic_stats;
/* A, M: real (LSA_F64) whole square matrices on one shared pattern, both outliving the handle.  shifts[2 nodes]: the nodes z_k (re,
 * im pairs); weights[nodes]: w_k > 0.  Builds C_k = A - z_k M and keeps nodes factor sets alive on one ordering and one pattern-only
 * analysis, as lsa_contour_create does with keep_factors (the first takes the analysis the context holds prepared, LSA_C128), and a
 * real basis of ncv + 1 vectors.  ksp_rtol: what each of the 2 nodes solves of a step must reach.  LSA_ERR_ARG, naming the
 * condition: a complex A or M, patterns that differ, a context of several ranks, nodes < 1, a weight that is not positive and finite,
 * ncv < 1 or > n.  LSA_ERR_OOM before factorising (before the second set where the context holds no prepared analysis), with the
 * bytes needed and the bytes available in the message, when nodes factor sets (the figures of lsa_ndlu_prepared_memory) exceed 0.8
 * of the free device memory.  A node on an eigenvalue: LSA_ERR_ZERO_PIVOT with the node's index in the message. */
int lsa_stochastic_create(lsa_ctx *ctx, const lsa_mat *A, const lsa_mat *M, int32_t nodes, const double *shifts, const double *weights, int32_t ncv,
                          double ksp_rtol, lsa_stochastic **out);
void lsa_stochastic_destroy(lsa_stochastic *h);
/* as lsa_krylov_set_row_permutation: the vectors of lsa_stochastic_solve leave in the caller's numbering (start vectors and
 * lsa_stochastic_apply are in the matrices' own) */
int lsa_stochastic_set_row_permutation(lsa_ctx *ctx, lsa_stochastic *h, const int32_t *perm);
/* Forcing weight Qf and response weight Qq in place of M (NULL: M; real symmetric positive semidefinite, n x n, any pattern; BORROWED:
 * they outlive the handle), as lsa_resolvent_set_weights: W(z) = C^-1 Qf C^-H Qq.  No inverse of a weight appears.  Begins anew: the
 * refinement steps are off again and a start vector must follow.  LSA_ERR_ARG, naming the weight, for a complex matrix or one of
 * another size. */
int lsa_stochastic_set_weights(lsa_ctx *ctx, lsa_stochastic *h, const lsa_mat *Qf, const lsa_mat *Qq);
/* kind 0 (what a new handle has), EOFs: S above, Qq the inner product -- per node z = C^-H (Qq v), tm = Qf z, w = C^-1 tm.  kind 1,
 * stochastic optimals: S' = (1 / pi) sum_k w_k Re(C_k^-H Qq C_k^-1 Qf), Qf the inner product: the same step with the two solves and the
 * two weights swapped.  Begins anew like lsa_stochastic_set_weights.  LSA_ERR_ARG for any other code. */
int lsa_stochastic_set_kind(lsa_ctx *ctx, lsa_stochastic *h, int32_t kind);
/* on != 0: the forward solves of a step (the second ones of kind 0, the first ones of kind 1) go through the batched sweeps of
 * lsa_ndlu_solve_batch, in groups of at most 16 factor sets of one analysis; a node that carries the refinement step runs alone.  The
 * results are those of the default, bit for bit.  Off by default.  (The adjoint solves have a switch of their own:
 * lsa_stochastic_set_batch_adjoint.) */
int lsa_stochastic_set_batch_forward(lsa_ctx *ctx, lsa_stochastic *h, int on);
/* on != 0: the adjoint solves of a step (the first ones of kind 0, the second ones of kind 1) go through the batched transposed
 * sweeps of lsa_ndlu_solve_batch_adjoint, in groups of at most 16 factor sets of one analysis -- a node that carries the refinement
 * step runs alone --, and their check products C_k^H z_k through lsa_spmv_transpose_batch in groups of 16.  The log, the verdicts
 * and every result are those of the default, bit for bit.  Off by default; does not begin the iteration anew. */
int lsa_stochastic_set_batch_adjoint(lsa_ctx *ctx, lsa_stochastic *h, int on);
/* on != 0: every solve of every node carries the refinement step from the start (for tests: at small sizes no solve misses ksp_rtol) */
int lsa_stochastic_set_refinement(lsa_ctx *ctx, lsa_stochastic *h, int on);
/* One operator apply on a host vector in the matrices' own numbering: host_y = S host_v (kind 1: S'), each of its 2 nodes solves
 * checked as in a step, and node_terms[k] = (w_k / pi) Re((Q v)^T w_k), node k's share of v^T Q S v (Q the kind's inner product; NULL:
 * none).  For tests and for the frequency spectrum of a mode. */
int lsa_stochastic_apply(lsa_ctx *ctx, lsa_stochastic *h, const double *host_v, double *host_y, double *node_terms);
/* The whole iteration, through the loop of lsa_lanczos_solve: Ritz values ranked largest first, accepted on |beta y_mi| / theta_i <=
 * opts->tol; of opts only nev, max_restarts, tol, seed and keep_fraction are read.  v0: host start vector (n doubles) or NULL (random
 * from opts->seed).  Outputs, largest first: theta_out[max_out] the variances, X_out the modes (n x max_out column-major, real,
 * orthonormal in the kind's weight, the entry of largest magnitude positive, the caller's row numbering; NULL: none),
 * est_out[max_out].  counts (NULL or 4 entries): accepted adjoint and forward solves of this handle so far, and how many of each
 * carried the refinement step.  Every one of the 2 nodes solves of a step is checked against ksp_rtol from a device log that travels
 * with the step's one read-back, by the rule of lsa_lanczos_extend: within tolerance, else a refinement step for that node and
 * direction from then on with the step done again, else a backward error within 1e-12 ||C_k||_F ||x||, else LSA_ERR_DIVERGED naming
 * node and direction.  Returns LSA_OK also when fewer than nev values converged (see result). */
int lsa_stochastic_solve(lsa_ctx *ctx, lsa_stochastic *h, const lsa_ks_options *opts, const double *v0, int32_t max_out, double *theta_out,
                         double *X_out, double *est_out, lsa_ks_result *result, int64_t *counts);
int lsa_stochastic_info(const lsa_stochastic *h, lsa_stochastic_stats *out);
/* ---- the trace of the quadrature operator by block probes: tr S = sum of ALL variances, the total the leading ones are a share of.
 * For a real probe z, z^T S z is unbiased for tr S when E[z z^T] = I, and with two solves of ONE direction
 *     z^T S  z = (1 / pi) sum_k w_k Re[(C_k^-H z)^H Qf (C_k^-H Qq z)]     (kind 0: adjoint solves only)
 *     z^T S' z = (1 / pi) sum_k w_k Re[(C_k^-1 z)^H Qq (C_k^-1 Qf z)]     (kind 1: forward solves only)
 * so a probe is two independent columns, z and Q z (Q the kind's weight), shared by all nodes: no dependent second solve.  With
 * ndeflate modes U of the handle's kind, orthonormal in Q, the second column is Q p with p = z - U (U^T Q z), and
 * tr S = sum_j theta_j + E[z^T S p]: the probes resolve only the remainder. */
typedef struct {
    int64_t solves_adjoint;    /* accepted adjoint solves (kind 0: 2 nodes nprobes)                                         */
    int64_t solves_forward;    /* accepted forward solves (kind 1)                                                          */
    int64_t refined_solves;    /* ... of either direction that carried the refinement step                                  */
    int64_t batches;           /* batches of probes queued, those done again after a missed solve included                  */
    int64_t grouped_sweeps;    /* block solves on more than one factor set in one sweep                                     */
    int32_t widest_pass;       /* most columns that shared the factor loads of a sweep (complex vectors: 4)                 */
    int32_t batch;             /* probes per batch, as given or chosen                                                      */
    double seconds_solve;      /* device seconds of the sweeps (HIP events around the phases)                               */
    double seconds_product;    /* ... of the probes, the deflation, the check products and the weight products              */
    double seconds_forms;      /* ... of the forms and check sums                                                           */
    int64_t bytes;             /* device bytes the call held beside the handle's                                            */
} lsa_stochastic_trace_stats;
/* forms[r] = z_r^T S p_r (kind 1: S') for r < nprobes, and node_terms[k nprobes + r] = node k's share (w_k / pi) Re(...) of it
 * (NULL: none); forms[r] is the sum of its column of node_terms in node order, on the host.  probes: n x nprobes real, column-major,
 * the caller's row numbering (lsa_stochastic_set_row_permutation), or NULL: Rademacher probes from `seed`, those of
 * lsa_stochastic_probes.  U: n x ndeflate real in the caller's numbering, the modes lsa_stochastic_solve gave for the handle's kind
 * and weights (ndeflate = 0: none; at most 128).  Per batch of `batch` probes (0: 8, or fewer where the n x 2 batch nodes complex
 * blocks exceed 0.8 of the free device memory) the call queues the probes, the deflation, one block solve of 2 batch columns per
 * run of at most 16 factor sets from ONE right-hand block, the check products of all columns in one launch, the weight product and
 * the forms, then reads 7 doubles per (node, probe) back behind ONE synchronisation.  Every one of the 2 nodes nprobes solves is
 * judged as a step's are: within ksp_rtol, else that node and direction carry the refinement step from then on (the node's block
 * then runs alone with a block refinement step behind it) and the batch is done again, else a backward error within 1e-12 ||C_k||_F
 * ||x||, else LSA_ERR_DIVERGED naming node, direction and probe.  Every column holds the bits of its solo sweep and every sum runs
 * in a fixed order: the results do not depend on `batch`, and two calls give the same bits.  The Lanczos basis is neither read nor
 * disturbed: the call may come before or after lsa_stochastic_solve.  LSA_ERR_ARG, naming the condition: nprobes < 1, ndeflate < 0
 * or > 128, ndeflate > 0 with U NULL, batch < 0, a U whose Gram matrix U^T Q U (summed on the device, before any solve) is further
 * from I than 1e-6 in an entry.  LSA_ERR_OOM with the bytes needed and available where a given batch, or one probe, does not fit. */
int lsa_stochastic_trace(lsa_ctx *ctx, lsa_stochastic *h, int32_t nprobes, uint64_t seed, const double *probes, int32_t ndeflate, const double *U,
                         int32_t batch, double *forms, double *node_terms, lsa_stochastic_trace_stats *stats);
/* The generator of lsa_stochastic_trace alone: Z_host (n x nprobes, column-major, the caller's numbering) = the Rademacher probes of
 * `seed`.  With mix(x) = splitmix64's output function (x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) 0xBF58476D1CE4E5B9; x = (x ^ x >> 27)
 * 0x94D049BB133111EB; x ^ x >> 31, all modulo 2^64): Z[i, p] = +1 where the top bit of mix(mix(mix(seed) + p) + i) is 0, else -1,
 * i the CALLER's row: a pure function of (seed, p, i), whatever the permutation, the batch width or the probes of a launch. */
int lsa_stochastic_probes(lsa_ctx *ctx, lsa_stochastic *h, int32_t nprobes, uint64_t seed, double *Z_host);

/* ---- MatrixMarket reader (host only): the A.mtx / M.mtx stage boundary --------------------------------------------
 * Stands in for scipy.io.mmread + the per-entry setValue loop of iPETScMatrix.from_path / from_matrix
 * (FEM/utils.py:143-147,208-215).  Coordinate format; general / symmetric / hermitian / skew-symmetric; real / integer /
 * complex / pattern; explicit zeros kept, duplicates summed, columns sorted.  Needs no GPU. */
typedef struct lsa_mm lsa_mm;
int lsa_mm_open(const char *path, lsa_mm **out, int32_t *nrows, int32_t *ncols, int64_t *nnz, int *is_complex);
int lsa_mm_read_csr(const lsa_mm *h, int32_t *rowptr, int32_t *col, void *val);
const char *lsa_mm_error(const lsa_mm *h);
void lsa_mm_close(lsa_mm *h);

/* ---- multi-GPU (one process per GPU; rows of C, M and the factors are sharded, the basis replicated) ---- */
/* RCCL bootstrap: rank 0 calls lsa_comm_unique_id, the launcher broadcasts the 128 bytes (e.g. with
 * torch.distributed), every rank then calls lsa_comm_init. */
int lsa_comm_unique_id(void *id128);
int lsa_comm_init(lsa_ctx *ctx, int nranks, int rank, const void *id128);
/* The same layout with a host-staged exchange instead of RCCL: the library copies this rank's block to a host buffer of
 * nranks * bytes_per_rank bytes (block r at r * bytes_per_rank), calls fn, which must fill the other ranks' blocks
 * (returning 0), and copies the buffer back to the device.  For tests and rehearsals with several ranks on ONE GPU (RCCL
 * refuses two ranks on a device) and for launchers whose only transport is a host one (torch.distributed over gloo). */
typedef int (*lsa_host_allgather_fn)(void *host_buf, int64_t bytes_per_rank, void *user);
int lsa_comm_init_host(lsa_ctx *ctx, int nranks, int rank, lsa_host_allgather_fn fn, void *user);
/* all-gathers issued on this context and the bytes this rank received through them */
int lsa_comm_stats(const lsa_ctx *ctx, int64_t *calls, int64_t *bytes_received);
/* The RCCL plumbing exercised with ONE rank (what a one-GPU box can run): open the library, unique id, a communicator of
 * one rank on the context's device, one in-place ncclAllGather of `bytes` bytes on the context's stream, compare, destroy.
 * Leaves the context's own communicator untouched.  LSA_OK, or LSA_ERR_COMM with the failing step in lsa_last_error. */
int lsa_comm_selftest(lsa_ctx *ctx, int64_t bytes);
/* Row-block shard of a global CSR: this rank owns rows [row0, row1); x and y of lsa_spmv stay global-length
 * and replicated, each rank computes its rows and the blocks are exchanged with ncclAllGather.
 * Padded block layout: the global index space is nranks equal blocks of B_pad = n_global / nranks slots, rank r owns
 * [r*B_pad, r*B_pad + rows_r); the unused tail of a block is padding (zero in every vector, referenced by no column),
 * so the all-gather moves equal counts.  Column indices are expressed in this padded space. */
int lsa_csr_upload_shard(lsa_ctx *ctx, int32_t n_global, int32_t row0, int32_t row1, int64_t nnz_local,
                         const int32_t *rowptr_local, const int32_t *col, const void *val, int dtype, lsa_mat **out);
/* Shift-invert operator on row shards (PETSc's parallel default bjacobi + ilu): A_rows / M_rows are this
 * rank's shards (lsa_csr_upload_shard), A_diag / M_diag its square diagonal blocks in local numbering
 * (lsa_csr_upload).  C's rows and the ILU(k) of C's diagonal block stay on the rank; every SpMV and every
 * preconditioner apply ends with one in-place all-gather; the Krylov bases are replicated, so dot products need no
 * collective and the Hessenberg matrices are bit-identical on every rank. */
int lsa_op_create_sharded(lsa_ctx *ctx, const lsa_mat *A_rows, const lsa_mat *M_rows, const lsa_mat *A_diag,
                          const lsa_mat *M_diag, const double sigma[2], int mode, const lsa_op_options *opts, lsa_op **out);

/* Shift-invert operator of the subtree-parallel layout: every rank holds the WHOLE matrices A, M in the padded block layout
 * (n_pad x n_pad, empty padding rows) and the forest of lsa_ndlu_create_tree, and solves with the subtree-parallel exact LU
 * (own subtrees, one small all-gather, replicated top, all-gather of the solution): no inner iteration.  The sparse products
 * run on the whole matrix on every rank when the pattern has at most 60 entries per row (cheaper than an exchange: two
 * collectives per operator apply), on the rank's rows [row0, row1) followed by an all-gather otherwise (four).  mode 0 or
 * 2, opts->pc_type 2. */
int lsa_op_create_dist(lsa_ctx *ctx, const lsa_mat *A, const lsa_mat *M, int32_t row0, int32_t row1, int32_t ntree, const int32_t *first,
                       const int32_t *size, const int32_t *parent, const int32_t *owner, const double sigma[2], int mode,
                       const lsa_op_options *opts, lsa_op **out);

#ifdef __cplusplus
}
#endif
#endif /* LSA_HIP_H */
