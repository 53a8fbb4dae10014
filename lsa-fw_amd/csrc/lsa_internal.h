// Internal declarations shared by the translation units of liblsa_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/lsa_hip.h"

// ---- scalar helpers ---------------------------------------------------------------------------------
struct cplx {
    double re, im;
};
static_assert(sizeof(cplx) == 16, "complex128 layout");

__host__ __device__ inline cplx make_cplx(double r, double i) { return cplx{r, i}; }

template <typename T>
struct scalar_traits;
template <>
struct scalar_traits<double> {
    static constexpr int dtype = LSA_F64;
    __host__ __device__ static double zero() { return 0.0; }
};
template <>
struct scalar_traits<cplx> {
    static constexpr int dtype = LSA_C128;
    __host__ __device__ static cplx zero() { return cplx{0.0, 0.0}; }
};

// acc += a * b for every (matrix scalar, vector scalar) pair the path needs
__host__ __device__ inline void fma_acc(double& acc, double a, double b) { acc = fma(a, b, acc); }
__host__ __device__ inline void fma_acc(cplx& acc, double a, cplx b) {
    acc.re = fma(a, b.re, acc.re);
    acc.im = fma(a, b.im, acc.im);
}
__host__ __device__ inline void fma_acc(cplx& acc, cplx a, cplx b) {
    acc.re = fma(a.re, b.re, acc.re);
    acc.re = fma(-a.im, b.im, acc.re);
    acc.im = fma(a.re, b.im, acc.im);
    acc.im = fma(a.im, b.re, acc.im);
}
// acc += conj(a) * b
__host__ __device__ inline void fma_conj_acc(double& acc, double a, double b) { acc = fma(a, b, acc); }
__host__ __device__ inline void fma_conj_acc(cplx& acc, cplx a, cplx b) {
    acc.re = fma(a.re, b.re, acc.re);
    acc.re = fma(a.im, b.im, acc.re);
    acc.im = fma(a.re, b.im, acc.im);
    acc.im = fma(-a.im, b.re, acc.im);
}
__host__ __device__ inline double s_mul(double a, double b) { return a * b; }
__host__ __device__ inline cplx s_mul(double a, cplx b) { return cplx{a * b.re, a * b.im}; }
__host__ __device__ inline cplx s_mul(cplx a, cplx b) { return cplx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__host__ __device__ inline double s_add(double a, double b) { return a + b; }
__host__ __device__ inline cplx s_add(cplx a, cplx b) { return cplx{a.re + b.re, a.im + b.im}; }
__host__ __device__ inline double s_sub(double a, double b) { return a - b; }
__host__ __device__ inline cplx s_sub(cplx a, cplx b) { return cplx{a.re - b.re, a.im - b.im}; }
__host__ __device__ inline double s_conj(double a) { return a; }
__host__ __device__ inline cplx s_conj(cplx a) { return cplx{a.re, -a.im}; }
__host__ __device__ inline double s_abs2(double a) { return a * a; }
__host__ __device__ inline double s_abs2(cplx a) { return a.re * a.re + a.im * a.im; }
__host__ __device__ inline double s_inv(double a) { return 1.0 / a; }
__host__ __device__ inline cplx s_inv(cplx a) {
    // Smith's algorithm: no overflow for large / tiny pivots
    if (fabs(a.re) >= fabs(a.im)) {
        double r = a.im / a.re, d = a.re + a.im * r;
        return cplx{1.0 / d, -r / d};
    }
    double r = a.re / a.im, d = a.re * r + a.im;
    return cplx{r / d, -1.0 / d};
}
__host__ __device__ inline cplx to_cplx(double a) { return cplx{a, 0.0}; }
__host__ __device__ inline cplx to_cplx(cplx a) { return a; }
__host__ __device__ inline void s_from(double& out, double re, double) { out = re; }
__host__ __device__ inline void s_from(cplx& out, double re, double im) { out = cplx{re, im}; }
// a complex entry moved as one 16-byte access (cplx itself is only 8-byte aligned: two 8-byte accesses otherwise), for arrays that are
// 16-byte aligned: hipMalloc, columns of 16 n bytes, offsets in whole complex numbers (the complex step kernels of lanczos.hip, resolvent.hip)
typedef double rz_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ cplx rz_ld(const cplx* p) {
    const rz_d2 v = *reinterpret_cast<const rz_d2*>(p);
    return cplx{v.x, v.y};
}
__device__ __forceinline__ void rz_st(cplx* p, cplx v) {
    rz_d2 o;
    o.x = v.re;
    o.y = v.im;
    *reinterpret_cast<rz_d2*>(p) = o;
}

// ---- objects behind the opaque handles ----------------------------------------------------------------
struct lsa_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    std::string arch;
    int num_cu = 256;
    // pinned host scratch for small device->host reads (Hessenberg columns, flags)
    void* pinned = nullptr;
    size_t pinned_bytes = 0;
    // device scratch for reductions
    void* dscratch = nullptr;
    size_t dscratch_bytes = 0;
    // RCCL (multi-GPU); null when single-process
    void* comm = nullptr;
    int nranks = 1, rank = 0;
    // host-staged transport (tests and rehearsals on one GPU; RCCL refuses two ranks on one device)
    lsa_host_allgather_fn host_gather = nullptr;
    void* host_gather_user = nullptr;
    void* comm_stage = nullptr;
    size_t comm_stage_bytes = 0;
    int64_t comm_calls = 0, comm_bytes = 0;  // all-gathers issued, bytes received by this rank
    // the last destroyed nested-dissection LU (analysis + tables + buffers), reused when the next one has the same pattern and
    // shape: a shift sweep refactorises the same pattern once per sigma (.examples/eigenvalues.py:97-108)
    struct lsa_ndlu* nd_cache = nullptr;
    struct lsa_krylov* krylov_cache = nullptr;  // the last destroyed Krylov workspace (two bases, work vectors), reused by the next of the same shape
};
extern "C" void lsa_ndlu_drop_cache(lsa_ctx* ctx);  // ndlu.hip
extern "C" void lsa_krylov_drop_cache(lsa_ctx* ctx);  // solver.hip

struct lsa_vec {
    lsa_ctx* ctx;
    int64_t n;
    int dtype;
    void* d;
};

// immutable host array of int32 shared by reference count
struct SharedInts {
    std::shared_ptr<const std::vector<int32_t>> p;
    const int32_t* data() const { return p ? p->data() : nullptr; }
    size_t size() const { return p ? p->size() : 0; }
    const int32_t& operator[](size_t i) const { return (*p)[i]; }
    const std::vector<int32_t>& vec() const {
        static const std::vector<int32_t> none;
        return p ? *p : none;
    }
    void assign(const int32_t* b, const int32_t* e) { p = std::make_shared<const std::vector<int32_t>>(b, e); }
    bool same_object(const SharedInts& o) const { return p == o.p; }
    bool operator==(const SharedInts& o) const { return p == o.p || vec() == o.vec(); }
    bool operator!=(const SharedInts& o) const { return !(*this == o); }
};

// The transpose of a pattern in pull form (built on first use of the transposed product, shared by the matrices of one pattern):
// output c sums the entries q in [rp[c], rp[c + 1]): the value at position src[q] of the CSR arrays times x[ci[q]].
struct TransposeIndex {
    int32_t *rp = nullptr, *ci = nullptr, *src = nullptr;  // device: ncols + 1, nnz, nnz
    int32_t ncols = 0;
    int64_t nnz = 0;
    ~TransposeIndex() {
        for (void* p : {(void*)rp, (void*)ci, (void*)src})
            if (p) (void)hipFree(p);
    }
};

struct PatternShared {  // what the matrices of one pattern build once and share (a slot, so that whoever builds it first fills it for all)
    std::shared_ptr<TransposeIndex> tr;
};

struct lsa_mat {
    lsa_ctx* ctx;
    int32_t n;        // rows held locally
    int32_t ncols;    // global column count
    int32_t row0;     // first global row of this shard (0 when unsharded)
    int64_t nnz;
    int dtype;
    int32_t* rp;      // device, n+1
    int32_t* ci;      // device, nnz
    void* val;        // device, nnz
    bool owns_index;  // false when the index arrays are shared with another matrix
    bool owns_values = true;  // false for a row view (mat_row_view): every device array belongs to the viewed matrix
    // host copy of the pattern (analysis phases): shared, not copied, between the matrices that have one pattern (A, M and the
    // C = A - sigma M built for every solve), together with its hash (nd_pattern_hash, computed on first use: the cache of the
    // nested-dissection LU is matched by it once per solve -- hashing 15 M indices anew took 18 ms of a 0.36 s solve)
    mutable SharedInts h_rp, h_ci;
    mutable std::shared_ptr<uint64_t> h_hash;
    mutable std::shared_ptr<PatternShared> h_shared;  // (shared like the hash: A, M and every C = A - sigma M built on their pattern)
    // compressed column indices for the SpMV (built on first use): col = cbase[row] + ci16[p] when every row spans
    // fewer than 65 536 columns (banded FEM matrices do); ci16_state: 0 = not tried, 1 = available, -1 = does not fit
    mutable uint16_t* ci16 = nullptr;
    mutable int32_t* cbase = nullptr;
    mutable int ci16_state = 0;
    // row groups for the SpMV (built on first use): consecutive rows with one and the same column pattern (the unknowns of
    // a mesh node) share their column indices and their gathers of x; grp_start holds (first row, rows, first entry, entries per row) of
    // group g (at most 4).  grp_state: 0 = not tried, 1 = available, -1 = not worth it (mean group size < 1.5)
    mutable int32_t* grp_start = nullptr;
    mutable int32_t ngroups = 0;
    mutable int grp_state = 0;
    bool owns_extras = true;  // false when ci16 / cbase / grp_start are borrowed from the matrix whose pattern this one shares
};

int lsa_set_error(lsa_ctx* ctx, int code, const char* fmt, ...);
// rows [r0, r1) of a square matrix as a shard (n = r1 - r0, row0 = r0): borrows every array, must not outlive `full`
lsa_mat* mat_row_view(const lsa_mat* full, int32_t r0, int32_t r1);
void comm_release(lsa_ctx* ctx);  // comm.hip
int k_agree_status(lsa_ctx* ctx, int rc);  // comm.hip: collective agreement on a status (returns rc on one rank)
int k_agree_min_i64(lsa_ctx* ctx, int64_t* value);  // comm.hip: the smallest of the ranks' values (collective)
int k_agree_in_step(lsa_ctx* ctx, const char* where);  // comm.hip: error on every rank unless all ranks have made the same number of exchanges (collective)
int lsa_ensure_scratch(lsa_ctx* ctx, size_t dbytes, size_t hbytes);
// an on/off LSA_* switch of the environment: unset -> dflt, else whether its value reads as a non-zero integer
inline bool env_flag(const char* name, bool dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) != 0 : dflt;
}
// after a kernel launch: the launch's own error, if any, as the library's status
inline int lsa_check_launch(lsa_ctx* ctx, const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lsa_set_error(ctx, LSA_ERR_HIP, "%s: kernel launch failed: %s", what, hipGetErrorString(e));
    return LSA_OK;
}
// k_multi_dot's row chunks, which the fused reductions of lanczos.hip and growth.hip keep for the sake of its bits: at most 2048 of
// them, whole multiples of 256 rows, at least 512 rows.  Returns the number of chunks (= partial sums per coefficient).
constexpr int kDotMaxChunks = 2048;
inline int dot_chunks(int64_t n, int64_t* rows_per_chunk) {
    int64_t rows = ((n + kDotMaxChunks - 1) / kDotMaxChunks + 255) / 256 * 256;
    rows = std::max<int64_t>(rows, 512);
    *rows_per_chunk = rows;
    return (int)std::max<int64_t>((n + rows - 1) / rows, 1);
}

#define LSA_HIP_CHECK(ctx, expr)                                                                         \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess)                                                                            \
            return lsa_set_error((ctx), LSA_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                 __FILE__, __LINE__);                                                    \
    } while (0)

// allocations: out of memory is its own status (callers may fall back to a leaner method; nothing else may)
#define LSA_HIP_ALLOC(ctx, expr)                                                                                    \
    do {                                                                                                            \
        hipError_t _e = (expr);                                                                                     \
        if (_e != hipSuccess) {                                                                                     \
            (void)hipGetLastError();                                                                                \
            return lsa_set_error((ctx), _e == hipErrorOutOfMemory ? LSA_ERR_OOM : LSA_ERR_HIP, "%s failed: %s (%s:%d)", #expr, \
                                 hipGetErrorString(_e), __FILE__, __LINE__);                                        \
        }                                                                                                           \
    } while (0)

#define LSA_CHECK(expr)            \
    do {                           \
        int _rc = (expr);          \
        if (_rc != LSA_OK) return _rc; \
    } while (0)

// the timed entries (lsa_*_time): `run` queued once beforehand if `warm` (what a first call builds stays outside the measurement),
// then iters times between the context's two events; the mean milliseconds of one run
template <typename F>
int lsa_time_runs(lsa_ctx* ctx, bool warm, int iters, double* avg_ms, F&& run) {
    if (warm) LSA_CHECK(run());
    LSA_HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for (int i = 0; i < iters; ++i) LSA_CHECK(run());
    LSA_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    LSA_HIP_CHECK(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    LSA_HIP_CHECK(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *avg_ms = (double)ms / iters;
    return LSA_OK;
}

// problems of one lockstep group (lsa_krylov_solve_batch): the capacity of the batched DCGS2 argument records (blas.hip), of the
// batched sweeps (kNdBatchMax, ndlu_internal.h: asserted equal there) and of the per-problem arrays of lsa_ks_batch_info
constexpr int kKrylovGroupMax = 16;

// ---- kernels launched across translation units --------------------------------------------------------
// (all launch on ctx->stream and return LSA_OK or a status)

// y = A x                       (spmv.hip)
int k_spmv(lsa_ctx* ctx, const lsa_mat* A, int xdtype, const void* x, void* y);
int k_spmv_transpose(lsa_ctx* ctx, const lsa_mat* A, int conj, int xdtype, const void* x, void* y);
// the transposed index of the pattern of a whole square A, built on first use and shared by the matrices of the pattern
int k_transpose_index(lsa_ctx* ctx, const lsa_mat* A, const TransposeIndex** out);
// ys[z] = mats[z]^T xs[z] (conj != 0: ^H), z < J <= 16, in one launch on the transposed index of one pattern; each ys[z] holds
// k_spmv_transpose's bits.  LSA_ERR_ARG naming what differs unless n, ncols, nnz and dtype agree and the matrices share the pattern
// object or their index arrays, or have equal host patterns
int k_spmv_transpose_batch(lsa_ctx* ctx, int32_t J, const lsa_mat* const* mats, int conj, int xdtype, const void* const* xs, void* const* ys);
// ys[z] = mats[z] xs[z], z < J <= 16, in one launch on the index arrays of one pattern (whole square matrices; the same matrix may
// stand in several slots); each ys[z] holds k_spmv's bits.  LSA_ERR_ARG naming what differs, as k_spmv_transpose_batch
int k_spmv_batch(lsa_ctx* ctx, int32_t J, const lsa_mat* const* mats, int xdtype, const void* const* xs, void* const* ys);
// `to` has `from`'s pattern and scalar type (lsa_csr_window): it borrows the row groups and compressed indices k_spmv uses for `from`
// (built here where `from` has not met a product yet), so that both take one kernel form; owns_extras = false, `from` outlives `to`
void spmv_share_extras(const lsa_mat* from, lsa_mat* to);

// Block kernels of the region eigensolver (contour.hip): complex128 column-major blocks, column c at c * ld, ld >= n
// Y[:, 0:ncols] = A X[:, 0:ncols] for a whole square A (f64 or c128), in passes of 8 columns that read A once each; not k_spmv's bits
int k_spmm(lsa_ctx* ctx, const lsa_mat* A, int32_t ncols, const void* X, int64_t ldx, void* Y, int64_t ldy);
// Y[:, 0:ncols] = A^T X[:, 0:ncols] (conj != 0: A^H), the same passes on the pattern's transposed index: no atomics, a fixed summation
// order; not k_spmv_transpose's bits
int k_spmm_transpose(lsa_ctx* ctx, const lsa_mat* A, int conj, int32_t ncols, const void* X, int64_t ldx, void* Y, int64_t ldy);
// G_host (p x q column-major) = U^H W over n rows, p, q <= 128: fixed-order two-stage sums; synchronises.  U == W (one block): real diagonal
int k_block_gram(lsa_ctx* ctx, int64_t n, int32_t p, const void* U, int64_t ldu, int32_t q, const void* W, int64_t ldw, void* G_host);

// Z = Mh^-1 Ah for r x r complex host matrices (column-major, ld r) by LU with partial pivoting, both overwritten (dense.hip); false: singular
bool dense_lu_solve(int32_t r, void* Mh, void* Ah);

// BLAS-1 / tall-skinny kernels (blas.hip); T selected by dtype
int k_copy(lsa_ctx* ctx, int dtype, int64_t n, const void* x, void* y);
int k_set_zero(lsa_ctx* ctx, int dtype, int64_t n, void* x);
// y += alpha x
int k_axpy(lsa_ctx* ctx, int dtype, int64_t n, const double alpha[2], const void* x, void* y);
// h[c] = sum_i conj(V[i,c]) w[i], c < j   -> device array h (same dtype); V column-major with leading dim ldv
int k_multi_dot(lsa_ctx* ctx, int dtype, int64_t n, int j, const void* V, int64_t ldv, const void* w, void* h_dev);
// w -= V h, and nrm2_dev[0] = ||w||^2 afterwards when nrm2_dev != null
int k_multi_axpy_dot(lsa_ctx* ctx, int dtype, int64_t n, int j, const void* V, int64_t ldv, const void* h1_dev, void* w, void* h2_dev);
int k_multi_axpy(lsa_ctx* ctx, int dtype, int64_t n, int j, const void* V, int64_t ldv, const void* h_dev, void* w,
                 double* nrm2_dev);
// columns of X: canonical phase (largest entry real positive), unit norm when `unit`; imag2_dev[c] = sum Im(X[:, c])^2
int k_columns_canonical(lsa_ctx* ctx, int64_t n, int ncols, void* X, int64_t ldx, int unit, double* imag2_dev);
// nrm2_dev[0] = ||x||^2
int k_nrm2(lsa_ctx* ctx, int dtype, int64_t n, const void* x, double* nrm2_dev);
// nrm2_dev[0] = ||x||^2, nrm2_dev[1] = ||y||^2 in one pass over both (fixed-order two-stage sums)
int k_pair_nrm2(lsa_ctx* ctx, int dtype, int64_t n, const void* x, const void* y, double* nrm2_dev);
int k_mask(lsa_ctx* ctx, int dtype, int64_t n, const double* keep_dev, void* y);
int k_residual_norms(lsa_ctx* ctx, int dtype, int64_t n, const void* b, const void* z, void* w, double* nrm2_dev);
// y = x / sqrt(nrm2_dev[0])   (no host round trip)
int k_scale_by_inv_norm(lsa_ctx* ctx, int dtype, int64_t n, const void* x, const double* nrm2_dev, void* y);
// hsum[c] += hadd[c] (c < j) and hsum[j] = sqrt(nrm2[0])  -- assembles one Hessenberg column on the device
int k_hess_column(lsa_ctx* ctx, int dtype, int j, const void* h1, const void* h2, const double* nrm2_dev, void* hout);
// CGS2 + normalisation of one Arnoldi step in five launches, the inner solve's residual check folded in (blas.hip); returns 1
// (nothing launched) for shapes it does not handle
size_t k_cgs2_fused_work_bytes(lsa_ctx* ctx, int64_t n, int jmax);
int k_cgs2_fused(lsa_ctx* ctx, int dtype, int64_t n, int j, const void* V, int64_t ldv, void* w, void* vnext, void* hcol_dev, void* work,
                 const void* chk_b, const void* chk_z, double* chk_out);
// The same CGS2 for an Arnoldi step of OP = C^-1 M whose matrices share their index arrays, in five launches that leave y alone
// and end with ONE kernel that normalises (v_next = w / ||w||, Hessenberg column), multiplies t <- M v_next for the next step
// and checks this step's inner solve (|t - C y|^2, |t|^2 per workgroup into tail_part, summed by k_cgs2_tail_checks): 18
// launches per step instead of 20.  The two products are bit for bit those of k_spmv.  Complex vectors only.
bool k_cgs2_tail_fits(lsa_ctx* ctx, int64_t n, int jmax, const lsa_mat* M, const lsa_mat* C);
int k_cgs2_tail_parts(int64_t n);  // workgroups of the tail kernel = (|t - C y|^2, |t|^2) pairs per step
int k_cgs2_fused_tail(lsa_ctx* ctx, int64_t n, int j, const void* V, int64_t ldv, const void* y, void* w, void* vnext, void* hcol_dev, void* work,
                      const lsa_mat* M, const lsa_mat* C, void* t, double* tail_part);
int k_cgs2_tail_checks(lsa_ctx* ctx, int nslots, int nparts, const double* tail_parts, double* checks);
// DCGS2 (delayed reorthogonalisation) of a pipelined Arnoldi step in the fused workspace, complex vectors: one reduction and one
// update (k_dcgs2_step: V[:, j] projected twice and normalised in place, y projected once into V[:, j+1], the step's a, b, nu, c
// into its slot of 2 lds + 4 entries; y == nullptr: the flush, V[:, j] only), then either the tail (k_dcgs2_tail: t <- M V[:, j+1]
// and the check pairs, as k_cgs2_fused_tail) or k_dcgs2_norm; both leave the provisional ||V[:, j+1]|| at slot[2 lds + 2].
// first != 0: V[:, j] is final already.  Fits for bases of up to ncv + 1 vectors with ncv + 1 <= 128 (n <= 262 k).
bool k_dcgs2_fits(int64_t n, int ncv);
int k_dcgs2_step(lsa_ctx* ctx, int64_t n, int j, void* V, int64_t ldv, const void* y, int first, void* slot, int lds, void* work,
                 const void* chk_b, const void* chk_z, double* chk_out);
int k_dcgs2_norm(lsa_ctx* ctx, int64_t n, void* work, void* slot, int lds);
int k_dcgs2_tail(lsa_ctx* ctx, int64_t n, int j, const void* V, int64_t ldv, const void* y, void* work, const lsa_mat* M, const lsa_mat* C, void* t,
                 double* tail_part, void* slot, int lds);
// The batched forms of a tail-form DCGS2 step, for the rounds of a lockstep group (lsa_krylov_solve_batch): J <= 16 problems of
// one n, each at its own step j[z], in two launches (reduction, update) and one (tail); per problem the bits of k_dcgs2_step and
// k_dcgs2_tail.  work[z]: the problem's fused workspace.
int k_dcgs2_step_batch(lsa_ctx* ctx, int J, int64_t n, const int32_t* j, void* const* V, int64_t ldv, const void* const* y, const int32_t* first,
                       void* const* slot, int lds, void* const* work);
int k_dcgs2_tail_batch(lsa_ctx* ctx, int J, int64_t n, const int32_t* j, void* const* V, int64_t ldv, const void* const* y, void* const* work,
                       const lsa_mat* const* M, const lsa_mat* const* C, void* const* t, double* const* tail_part, void* const* slot, int lds);
int k_spmv_plain_subwave_lanes(const lsa_mat* A);  // spmv.hip
// Out[:, 0:k] = V[:, 0:m] Q   (Q m x k column-major on the device, ldq); m <= k_basis_gemm_max_cols(dtype), LSA_ERR_ARG beyond
int k_basis_gemm_max_cols(int dtype);
int k_basis_gemm(lsa_ctx* ctx, int dtype, int64_t n, int m, int k, const void* V, int64_t ldv, const void* Q, int ldq,
                 void* Out, int64_t ldo);
// Out[perm[i], c] = In[i, c] for the columns c < ncols (both n x ncols, leading dimension n)
int k_scatter_rows(lsa_ctx* ctx, int dtype, int64_t n, int ncols, const int32_t* perm, const void* In, void* Out);

// ---- what the basis handles lsa_krylov (solver.hip) and lsa_lanczos (lanczos.hip) and their owners share (solver.hip) ------
// *row_perm <- a device copy of perm after checking that it permutes 0..n-1 (null: dropped); who: the caller's name for the message
int basis_upload_row_permutation(lsa_ctx* ctx, const char* who, int64_t n, const int32_t* perm, int32_t** row_perm);
// Out[:, 0:k] = V[:, 0:m] Q for a host matrix Q (m x k, leading dimension ldq; V and Out: n): packed densely into the pinned
// scratch (kept pinned_extra bytes longer for the caller), uploaded to qdev, k_basis_gemm
int basis_times_host_matrix(lsa_ctx* ctx, int dtype, int64_t n, int m, int k, const void* V, const void* Q, int ldq, void* qdev, void* Out,
                            size_t pinned_extra);
// device columns (n x ncols, leading dimension n) to the host in the caller's numbering: scattered through row_perm (null: as they
// are) into *xtmp, which is made on first use with room for xtmp_cols columns; synchronises
int basis_columns_to_host(lsa_ctx* ctx, int dtype, int64_t n, int ncols, const int32_t* row_perm, const void* dev, void** xtmp, int xtmp_cols, void* host);
// The direct inner solve of a Krylov step, queued without a read-back: y = C^-1 rhs, z = C y and, with refine, one step of
// iterative refinement (r = rhs - z, z = C^-1 r, y += z, z = C y; the two sums of that residual pass land in norms[0..2]).  C is
// the operator's factorised matrix with its exact LU, rows and exchanges as the operator has them; the caller judges rhs - z.
// direction: -1 the operator's own (lsa_op_set_adjoint), 0 C^-1, 1 C^-H on the same factors (one rank), whatever the operator's is.
int direct_solve_enqueue(lsa_ctx* ctx, lsa_op* op, int dtype, const void* rhs, void* y, void* z, void* r, bool refine, double* norms,
                         int direction = -1);
// books one accepted direct solve of relative residual res / bnorm: `products` sparse products besides the refinement's one
void stats_book_direct_solve(lsa_stats* st, int products, bool refine, double res, double bnorm);

// ---- the solo solve loop's queueing ahead (solver.hip; LSA_KRYLOV_PREAPPLY), driven by lsa_krylov_solve (dense.hip) -----------
// armed: a full expansion queues the operator apply of its final vector V[:, ncv] behind its flush; krylov_preapply(m) queues it
// where that has not happened (both only where the plan is the pipelined DCGS2 tail form).  The restart hands it to the first step
// of the next expansion, which then starts at its orthogonalisation; whatever else comes first drops it.
void krylov_arm_preapply(lsa_krylov* k, bool on);
int krylov_preapply(lsa_ctx* ctx, lsa_krylov* k, int32_t m);
// lsa_krylov_restart without its wait for the stream where the next expansion is pipelined (its read-back reports a failure)
int krylov_restart_queued(lsa_ctx* ctx, lsa_krylov* k, int32_t m, int32_t knew, const void* Q, int32_t ldq);

// ---- the lockstep expansion of a group of problems (solver.hip), driven by lsa_krylov_solve_batch (dense.hip) ---------------
struct KrylovGroupBuf {  // the group's slots, checks and check pairs: cell (round s, problem z) at s J + z
    int32_t J, slots, nparts;
    void* Hdev;
    double *checks, *tail_parts;
};
// argument errors of a group: null or foreign workspaces, other shapes, shared workspaces or operators
int krylov_group_check(lsa_ctx* ctx, int32_t J, lsa_krylov* const* ks);
int krylov_group_alloc(lsa_ctx* ctx, int32_t J, lsa_krylov* const* ks, KrylovGroupBuf* gb);
void krylov_group_free(KrylovGroupBuf* gb);
// lsa_krylov_extend(ks[z], j0[z], j1, Hs[z], ldh) for every active problem z, in lockstep where the plans allow; status[z] and
// breakdown[z] per problem (an error stops that problem alone; its text, naming the problem, goes to errs[z]); info: counters, or null
int krylov_extend_batch(lsa_ctx* ctx, KrylovGroupBuf* gb, lsa_krylov* const* ks, const uint8_t* active, const int32_t* j0, int32_t j1, void* const* Hs,
                        int32_t ldh, int32_t* breakdown, int32_t* status, std::string* errs, lsa_ks_batch_info* info);
// puts "problem z: " in front of the context's error text
void lsa_name_problem(lsa_ctx* ctx, int32_t z);

// ---- what the Lanczos iteration (lanczos.hip) needs of a shift-invert operator (solver.hip) -------------------------------
struct lsa_ndlu;
struct lsa_op_parts {
    int64_t n;
    const lsa_mat *Kmul, *Kfac;  // y = Kfac^-1 (Kmul x); Kmul null: standard problem
    lsa_ndlu* nd;                // exact LU of Kfac, or null
    bool plain;                  // forward, unprojected, whole on this rank
    bool shift_invert, adjoint, projected, one_rank;  // what `plain` is made of, for callers that say which one is missing
    double ksp_rtol;
    double normF;                // ||Kfac||_F (0: unknown): the scale of the backward-error judgement of a direct solve
    double sigma[2];             // the shift the operator was built at
    bool* refine;                // the operator's flag: solves carry one step of iterative refinement
    lsa_stats* st;
};
int lsa_op_get_parts(lsa_op* op, lsa_op_parts* out);
// The library's judgement of a direct solve x of right-hand side b (res = |b - C x|): within ksp_rtol, or, after the refinement step,
// a backward error within 1e-12 ||C||_F -- |b - C x| cannot go below eps ||C|| |x|, whatever the solver.  0: accepted (*backward says
// by which rule), 1: again with the refinement step switched on, -1: diverged.  normF: ||C||_F (0: unknown).
inline int direct_solve_verdict(double ksp_rtol, double normF, bool refine, double res, double bnorm, double xnorm, bool* backward) {
    *backward = refine && res > ksp_rtol * bnorm && normF > 0.0 && res <= 1e-12 * normF * xnorm;
    if (res <= ksp_rtol * bnorm || *backward) return 0;
    return (!refine && std::isfinite(res)) ? 1 : -1;
}
inline int direct_solve_verdict(const lsa_op_parts& P, bool refine, double res, double bnorm, double xnorm, bool* backward) {
    return direct_solve_verdict(P.ksp_rtol, P.normF, refine, res, bnorm, xnorm, backward);
}

// ---- the basis of the self-adjoint outer iterations (lanczos.hip): real or complex scalars, orthonormal in a real symmetric inner
// product, with an operator behind its step; the loop is lsa_lanczos_solve (dense.hip) -------------------------------------------
// A basis of scalar type dtype (LSA_F64, LSA_C128) for an owner that has checked the operator itself; who: the owner's name in the
// messages ("lsa_growth", "lsa_resolvent").  A basis with complex scalars has no operator until lanczos_set_operator gives it one.
int lanczos_create_basis(lsa_ctx* ctx, lsa_op* op, int32_t ncv, int dtype, const char* who, lsa_lanczos** out);
// The same for an owner without a shift-invert operator (stochastic.hip keeps factor sets of its own): P names what the basis reads of
// one -- n, Kmul (the inner product) and st, which outlives the basis -- and op is null: such a basis has no default operator.
int lanczos_create_basis_on(lsa_ctx* ctx, lsa_op* op, const lsa_op_parts& P, int32_t ncv, int dtype, const char* who, lsa_lanczos** out);
int lanczos_shape(const lsa_lanczos* l, int64_t* n, int32_t* ncv);
// the inner product x^H Q y (Q real symmetric positive semidefinite; the operator's M on a new basis).  No right-hand side is left
// over: a start vector must follow, the basis in hand being orthonormal in the old inner product.
void lanczos_set_inner_product(lsa_lanczos* l, const lsa_mat* Q);
// v_j = host vector orthonormalised against v_0..v_{j-1} (continues after a breakdown; j = 0: lsa_lanczos_set_start)
int lanczos_inject(lsa_ctx* ctx, lsa_lanczos* l, int32_t j, const void* host_v);
// thick restart: V[:, 0:knew] = V[:, 0:m] Y (Y real, m x knew column-major on the host: the eigenvectors of the real projected
// matrix), V[:, knew] = V[:, m]
int lanczos_restart(lsa_ctx* ctx, lsa_lanczos* l, int32_t m, int32_t knew, const double* Y, int32_t ldy);
// X = V[:, 0:m] Y to the host in the caller's row numbering, each column's entry of largest magnitude (real) positive
int lanczos_ritz_vectors(lsa_ctx* ctx, lsa_lanczos* l, int32_t m, int32_t nvec, const double* Y, int32_t ldy, void* X);
// the columns lanczos_ritz_vectors left on the device (n x nvec, the basis' own row numbering; an owner may overwrite them), and
// nvec of them to the host in the caller's row numbering
void* lanczos_ritz_device(const lsa_lanczos* l);
int lanczos_ritz_to_host(lsa_ctx* ctx, lsa_lanczos* l, int32_t nvec, void* X);
// the device copy of the row permutation (basis row i is the caller's row perm[i]), or null where none is set
const int32_t* lanczos_row_permutation(const lsa_lanczos* l);
// The operator behind a step: it queues w = OP v_j and names the inner solves the step's first reduction checks.  The default of a
// real basis is the single solve w = C^-1 rhs on the op's shared refinement flag; growth.hip puts a march of solves there,
// resolvent.hip an adjoint solve, a weight and a forward solve.
struct lanczos_check {  // one checked solve: right-hand side b, z = C (or C^H) times its solution, both of the basis' scalar type
    const void *b, *z;
    bool refined;        // the solve carried the refinement step and left |its solution|^2 at xnorm2_dev
    double* xnorm2_dev;  // (given by the basis: it travels with the step's slot)
};
struct lanczos_sums {  // what the step's read-back holds of one check: |b - z|, |b|, and |solution| of a refined solve (else 0)
    double res, bnorm, xnorm;
};
struct lanczos_operator {
    void* self;
    int nchecks;  // the checks of a step: the real step kernels take one, the complex ones two
    // queue w = OP v_j from rhs = Q v_j (rhs stays intact: a step may be done again) and fill chk[0..nchecks).  z, r: work vectors.
    int (*enqueue)(lsa_ctx* ctx, void* self, int32_t j, const void* rhs, void* w, void* z, void* r, lanczos_check* chk);
    // queue the read-back of what the operator logged on the device (null: nothing); the step's one synchronisation follows
    int (*read_back)(lsa_ctx* ctx, void* self);
    // after the synchronisation: the sums of the step's checks.  0: accepted (and booked), 1: do the step again, -1: failed (the error is set)
    int (*judge)(lsa_ctx* ctx, void* self, int32_t j, const lanczos_sums* sums);
};
// hook outlives the basis' steps; null: the default.  LSA_ERR_ARG where nchecks is not what the basis' kernels take.
int lanczos_set_operator(lsa_ctx* ctx, lsa_lanczos* l, const lanczos_operator* hook);

// ---- the lockstep expansion of a group of complex bases (lanczos.hip), driven by lsa_resolvent_solve_batch (dense.hip) -------------
// The operator of a group: it says which members it can queue together and queues w = OP v_j for R of them in batched launches.
struct lanczos_group_operator {
    void* self;
    // whether member z may advance in lockstep in this expansion, beside member `lead` (-1: z would lead)
    bool (*eligible)(void* self, int32_t z, int32_t lead);
    // queue w[r] = OP v from rhs[r] for the members idx[0..R) (rhs stays intact; z[r]: a work vector) and fill chk[r][0..2); every
    // member's own judge follows the read-back.  Adds its kernel launches to *launches.
    int (*enqueue)(lsa_ctx* ctx, void* self, int32_t R, const int32_t* idx, const void* const* rhs, void* const* w, void* const* z,
                   lanczos_check* const* chk, int32_t* launches);
};
struct LanczosGroupBuf {  // the members' slots side by side: one copy reads a round back
    int32_t J;
    size_t slot_doubles;
    double* slots;
};
int lanczos_group_alloc(lsa_ctx* ctx, int32_t J, lsa_lanczos* const* ls, LanczosGroupBuf* gb);
void lanczos_group_free(LanczosGroupBuf* gb);
// lsa_lanczos_extend(ls[z], j0[z], j1, T[z], ldt) for every active member z, in lockstep where the basis and the group operator allow;
// status[z] and breakdown[z] per member (an error stops that member alone; its text, naming the problem, goes to errs[z]); info:
// counters, or null.  Every member is left with the bits of its own lsa_lanczos_extend.
int lanczos_extend_batch(lsa_ctx* ctx, LanczosGroupBuf* gb, lsa_lanczos* const* ls, const lanczos_group_operator* gop, const uint8_t* active,
                         const int32_t* j0, int32_t j1, double* const* T, int32_t ldt, int32_t* breakdown, int32_t* status, std::string* errs,
                         lsa_ks_batch_info* info);
// whether B has A's pattern: the index arrays or the pattern object shared, or equal host copies (spmv.hip)
bool k_spmv_same_pattern(const lsa_mat* A, const lsa_mat* B);

// ---- the resolvent iteration (resolvent.hip): the basis with complex scalars and the step W = C^-1 Q_f C^-H Q_q behind it; the loop
// is the one of lsa_lanczos_solve (dense.hip), which reaches the handle through these pieces --------------------------------------
int resolvent_shape(const lsa_resolvent* r, int64_t* n, int32_t* ncv);
int resolvent_inject(lsa_ctx* ctx, lsa_resolvent* r, int32_t j, const cplx* host_v);
int resolvent_restart(lsa_ctx* ctx, lsa_resolvent* r, int32_t m, int32_t knew, const double* Y, int32_t ldy);
// Q = V[:, 0:m] Y to the host in the caller's row numbering, each column's entry of largest magnitude real positive; the columns stay
// on the device for resolvent_forcings
int resolvent_ritz_vectors(lsa_ctx* ctx, lsa_resolvent* r, int32_t m, int32_t nvec, const double* Y, int32_t ldy, cplx* Q);
// F[:, c] = -C^-H M q_c / gain[c] for the columns resolvent_ritz_vectors left: one checked adjoint solve each (with
// lsa_resolvent_set_block_forcings: one block solve for all of them, each column checked, the same results)
int resolvent_forcings(lsa_ctx* ctx, lsa_resolvent* r, int32_t nvec, const double* gain, cplx* F);
// accepted adjoint solves, accepted forward solves, and how many of each carried the refinement step
void resolvent_counts(const lsa_resolvent* r, int64_t counts[4]);
// A lockstep group (lsa_resolvent_extend_batch, lsa_resolvent_solve_batch): the argument errors of a group -- J outside [1, 16], a null
// or foreign handle, a handle or an operator given twice, other shapes, weights on more than one pattern --, its buffers, the
// expansion of every active member (lanczos_extend_batch behind the group's operator), and the context's text from the members' errors
int resolvent_group_check(lsa_ctx* ctx, const char* who, int32_t J, lsa_resolvent* const* rs);
int resolvent_group_alloc(lsa_ctx* ctx, int32_t J, lsa_resolvent* const* rs, LanczosGroupBuf* gb);
int resolvent_extend_batch(lsa_ctx* ctx, LanczosGroupBuf* gb, int32_t J, lsa_resolvent* const* rs, const uint8_t* active, const int32_t* j0, int32_t j1,
                           double* const* T, int32_t ldt, int32_t* breakdown, int32_t* status, std::string* errs, lsa_ks_batch_info* info);
int resolvent_group_status(lsa_ctx* ctx, int32_t J, const int32_t* status, const std::string* errs);

// ---- transient growth (growth.hip): the real basis of an lsa_lanczos with a march of 2N solves behind every step; the loop is the
// one of lsa_lanczos_solve (dense.hip), which reaches the handle through these pieces ------------------------------------------------
int growth_shape(const lsa_growth* g, int64_t* n, int32_t* ncv, int32_t* nsteps);
// v_j = keep (.) host vector, M-orthonormalised against v_0..v_{j-1}
int growth_inject(lsa_ctx* ctx, lsa_growth* g, int32_t j, const double* host_v);
int growth_restart(lsa_ctx* ctx, lsa_growth* g, int32_t m, int32_t knew, const double* Y, int32_t ldy);
// Q0 = V[:, 0:m] Y to the host in the caller's row numbering, each column's entry of largest magnitude positive; the columns stay on
// the device for growth_responses
int growth_ritz_vectors(lsa_ctx* ctx, lsa_growth* g, int32_t m, int32_t nvec, const double* Y, int32_t ldy, double* Q0);
// QT[:, c] = Phi q0_c and energy[c (N + 1) + s] = ||Phi_s q0_c||_M^2, s = 0..N, for the columns growth_ritz_vectors left: one forward
// march of N checked solves each, 2N under LSA_GROWTH_SDIRK2 with the energies at each time step's second stage (either destination may
// be null)
int growth_responses(lsa_ctx* ctx, lsa_growth* g, int32_t nvec, double* QT, double* energy);
// accepted forward solves, accepted transposed solves, and how many of each carried the refinement step
void growth_counts(const lsa_growth* g, int64_t counts[4]);

// ---- stochastic forcing (stochastic.hip): the real basis of an lsa_lanczos with 2N solves on N kept factor sets behind every step;
// the loop is the one of lsa_lanczos_solve (dense.hip), which reaches the handle through these pieces ------------------------------
int stochastic_shape(const lsa_stochastic* h, int64_t* n, int32_t* ncv);
int stochastic_inject(lsa_ctx* ctx, lsa_stochastic* h, int32_t j, const double* host_v);
int stochastic_extend(lsa_ctx* ctx, lsa_stochastic* h, int32_t j0, int32_t j1, double* T, int32_t ldt, int32_t* breakdown);
int stochastic_restart(lsa_ctx* ctx, lsa_stochastic* h, int32_t m, int32_t knew, const double* Y, int32_t ldy);
// X = V[:, 0:m] Y to the host in the caller's row numbering, orthonormal in the kind's weight, each column's entry of largest magnitude positive
int stochastic_ritz_vectors(lsa_ctx* ctx, lsa_stochastic* h, int32_t m, int32_t nvec, const double* Y, int32_t ldy, double* X);
// accepted adjoint solves, accepted forward solves, and how many of each carried the refinement step
void stochastic_counts(const lsa_stochastic* h, int64_t counts[4]);
void stochastic_book_dense(lsa_stochastic* h, double seconds);

// ---- ILU (ilu.hip) -------------------------------------------------------------------------------------
struct lsa_ilu {
    lsa_ctx* ctx;
    int32_t n;
    int64_t nnz;
    int dtype;  // scalar type of the factors
    int32_t *rp, *ci, *diag;   // device pattern of the factors + position of the diagonal
    void* val;                 // device factor values (L strictly lower, unit diagonal implied; U upper)
    void* dinv;                // device 1/u_ii
    int32_t *order_l, *order_u;  // device row lists sorted by dependency level
    std::vector<int32_t> lvl_ptr_l, lvl_ptr_u;  // host level pointers into the row lists
    std::vector<int32_t> h_rp, h_ci, h_diag;
    int32_t nshift;
    int32_t* flag;   // device int[4]: abort / error / shift count / spare
    int sptrsv_blocks_l, sptrsv_blocks_u;  // workgroups used by the sync-free solves
    int algo;                               // 0 = level-by-level launches, 1 = sync-free, 2 = blocked (inverted diagonal blocks)
    void* tmp;                              // device vector (intermediate of L then U), sized on demand
    int tmp_dtype;
    // blocked form (sptrsv_block.hip)
    int32_t blk_B = 0, blk_nb = 0;
    int32_t *lsplit = nullptr, *usplit = nullptr;  // device: first in-block L entry / first out-of-block U entry per row
    void *linv = nullptr, *uinv = nullptr;         // device: n x B row-major dense inverses of the diagonal blocks
    void *blk_t[2] = {nullptr, nullptr}, *blk_y[2] = {nullptr, nullptr};      // per vector dtype: work vectors
    void *blk_in[2] = {nullptr, nullptr}, *blk_out[2] = {nullptr, nullptr};  // fixed graph input / output
    void* blk_graph[2] = {nullptr, nullptr};                                 // hipGraphExec_t of the full apply
};

int ilu_solve_dev(lsa_ctx* ctx, lsa_ilu* pc, int which, int vdtype, const void* b, void* x);
int blk_setup(lsa_ctx* ctx, lsa_ilu* pc, int32_t B);
int blk_solve(lsa_ctx* ctx, lsa_ilu* pc, int which, int vdtype, const void* b, void* x);
void blk_release(lsa_ilu* pc);

// ---- nested-dissection multifrontal LU: the solves on its factors are declared in ndlu_internal.h (ndlu_solve_dev, NdSolve)
struct lsa_ndlu;
