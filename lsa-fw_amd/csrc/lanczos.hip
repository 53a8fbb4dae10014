// Thick-restart Lanczos (the symmetric variant of Krylov-Schur) for symmetric-definite pencils K x = lambda M x: what SLEPc runs
// behind EPS_GHEP / EPS_HEP (reference: Solver/utils.py:244-270 with iEpsProblemType.GHEP; Elasticity/utils.py:141-155).
//
// OP = (K - sigma M)^-1 M with a real sigma is self-adjoint in the M-inner product, so the basis V (n x (ncv + 1) doubles) is kept
// M-orthonormal, V^T M V = I, the projected matrix is real symmetric, and no complex number is stored or moved: half of the bytes of
// the general path's basis, sweeps and products.  This file holds the basis handle, the step and its kernels; the outer loop and
// the dense symmetric eigen-solve are lsa_lanczos_solve and lsa_dense_syev (dense.hip).
//
// One step j (rhs = M v_j is left by the previous step's tail):
//     w = C^-1 rhs                          the real sweeps of the exact LU (ndlu_solve_dev, float64 vectors)
//     z = C w                               for the inner-solve check |rhs - z| <= ksp_rtol |rhs| (one refinement step if it fails)
//     twice:  t = M w;  h = V^T t;  w -= V h    lz_dot_kernel + lz_update_kernel: full reorthogonalisation against v_0..v_j
//     t = M w;  beta^2 = w^T t              lz_dot_kernel on the one extra column
//     v_{j+1} = w / beta;  rhs' = t / beta  lz_tail_kernel, which also leaves beta^2 and the check's two sums in the step's slot
// Three products with M per step, one host synchronisation (the read-back of the slot).  For a standard problem (M = NULL) t is w.
// The first line is the default; lanczos_set_operator puts another operator behind a step (growth.hip: a march of solves), which
// leaves w, z and the right-hand side of its last solve where the single solve does and judges its solves itself.
//
// Every reduction runs in a fixed order (per-thread strided sums, a shuffle tree inside the wavefront, the four wave sums in wave
// order, the chunks' partial sums strided over 64 lanes and the same tree) and there are no floating-point atomics: two runs give
// the same bits, and the order is that of k_multi_dot / k_multi_axpy, so the unfused form of a step gives them too.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "lsa_internal.h"

namespace {

constexpr int kLzThreads = 256;     // four wavefronts of 64
constexpr int kLzColTile = 8;       // basis columns per workgroup of lz_dot_kernel
constexpr int kLzMaxChunks = 2048;  // row chunks of lz_dot_kernel = partial sums per coefficient (k_multi_dot's rule)
constexpr int kLzUnroll = 16;       // basis entries of a row requested at a time by lz_update_kernel

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The sums of these kernels are taken in the order of the library's unfused kernels (k_multi_dot: rows strided over the 256
// threads of a chunk, xor tree over the wavefront, the four waves in wave order, the chunks strided over 64 lanes and the same
// tree; k_multi_axpy: the columns of a row one after the other), so that the fused and the unfused form of a step (LSA_LANCZOS_FUSED)
// give the same bits: a Krylov basis amplifies a difference of one rounding to 1e-8 within 40 steps, and nothing short of the same
// order keeps the two forms comparable.

// sum over the 64 lanes by the xor tree of blas.hip's wave_sum; every lane ends with the same value
__device__ __forceinline__ double lz_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the partial sums part[0..nchunks) of one coefficient: lane k adds the chunks k, k + 64, ... in that order (eight requested at a
// time), then the tree; called by a whole wavefront
__device__ __forceinline__ double lz_finish_sum(const double* __restrict__ part, int nchunks, int lane) {
    double a = 0.0;
    for (int k0 = lane; k0 < nchunks; k0 += 8 * 64) {
        double pv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) pv[u] = (k0 + 64 * u < nchunks) ? part[k0 + 64 * u] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (k0 + 64 * u < nchunks) a += pv[u];
    }
    return lz_wave_sum(a);
}

// Partial sums of V^T t for the columns 0..ncols-1 and of w^T t (stored as column `ncols`), one pass over V: workgroup
// (chunk, tile) sums kLzColTile columns over the rows of its chunk into part[c * ldp + chunk].  The workgroups of tile 0 also sum
// the inner-solve check over their rows when chk_part is given: chk_part[2 chunk] = |chk_b - chk_z|^2, [2 chunk + 1] = |chk_b|^2.
// Two rows per thread and trip, so that 2 x kLzColTile loads of V are in flight per lane before the first addition (the additions
// into a column's sum keep the order of a one-row loop).
__global__ __launch_bounds__(kLzThreads) void lz_dot_kernel(int64_t n, int ncols, int64_t rows_per_block, const double* __restrict__ V, int64_t ldv,
                                                            const double* t, const double* w, double* __restrict__ part, int ldp,
                                                            const double* __restrict__ chk_b, const double* __restrict__ chk_z,
                                                            double* __restrict__ chk_part) {
    __shared__ double wsum[4][kLzColTile];
    __shared__ double csum[4][2];
    const int chunk = blockIdx.x;
    const int c0 = blockIdx.y * kLzColTile;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r0 = (int64_t)chunk * rows_per_block;
    const int64_t r1 = (r0 + rows_per_block < n) ? r0 + rows_per_block : n;
    // column c of the tile: a basis column, or w for the one behind the basis
    const double* col[kLzColTile];
#pragma unroll
    for (int c = 0; c < kLzColTile; ++c) col[c] = (c0 + c < ncols) ? V + (int64_t)(c0 + c) * ldv : w;
    const int nc = (ncols + 1 - c0 < kLzColTile) ? (ncols + 1 - c0) : kLzColTile;
    double acc[kLzColTile];
#pragma unroll
    for (int c = 0; c < kLzColTile; ++c) acc[c] = 0.0;
    int64_t i = r0 + threadIdx.x;
    if (nc == kLzColTile) {
        for (; i + kLzThreads < r1; i += 2 * kLzThreads) {
            const double ta = t[i], tb = t[i + kLzThreads];
            double va[kLzColTile], vb[kLzColTile];
#pragma unroll
            for (int c = 0; c < kLzColTile; ++c) {
                va[c] = col[c][i];
                vb[c] = col[c][i + kLzThreads];
            }
#pragma unroll
            for (int c = 0; c < kLzColTile; ++c) {
                acc[c] = fma(va[c], ta, acc[c]);
                acc[c] = fma(vb[c], tb, acc[c]);
            }
        }
    }
    for (; i < r1; i += kLzThreads) {
        const double tv = t[i];
#pragma unroll
        for (int c = 0; c < kLzColTile; ++c)
            if (c < nc) acc[c] = fma(col[c][i], tv, acc[c]);
    }
#pragma unroll
    for (int c = 0; c < kLzColTile; ++c) {
        const double s = lz_wave_sum(acc[c]);
        if (lane == 0) wsum[wave][c] = s;
    }
    const bool chk = chk_part != nullptr && blockIdx.y == 0;
    if (chk) {
        double rw = 0.0, rb = 0.0;
        for (int64_t r = r0 + threadIdx.x; r < r1; r += kLzThreads) {
            const double b = chk_b[r], d = b - chk_z[r];
            rw = fma(d, d, rw);
            rb = fma(b, b, rb);
        }
        rw = lz_wave_sum(rw);
        rb = lz_wave_sum(rb);
        if (lane == 0) {
            csum[wave][0] = rw;
            csum[wave][1] = rb;
        }
    }
    __syncthreads();
    if (threadIdx.x < nc) {
        const int c = threadIdx.x;
        part[(int64_t)(c0 + c) * ldp + chunk] = ((wsum[0][c] + wsum[1][c]) + wsum[2][c]) + wsum[3][c];
    }
    if (chk && threadIdx.x >= 64 && threadIdx.x < 66) {
        const int q = threadIdx.x - 64;
        chk_part[2 * chunk + q] = ((csum[0][q] + csum[1][q]) + csum[2][q]) + csum[3][q];
    }
}

// w -= V h for the columns 0..ncols-1.  The prologue finishes h from the partial sums (lz_finish_sum: every workgroup gets the
// same bits; wave q takes the columns q, q + 4, ...); workgroup 0 writes h to h_out for the host.  Then a thread per row, the rows
// of a workgroup strided over the grid: sixteen entries of the row are requested at a time -- the first sixteen ahead of the
// prologue, which does not depend on them -- and added column after column.
__global__ __launch_bounds__(kLzThreads) void lz_update_kernel(int64_t n, int ncols, const double* __restrict__ V, int64_t ldv,
                                                               const double* __restrict__ part, int nchunks, int ldp, double* w,
                                                               double* __restrict__ h_out) {
    extern __shared__ double hs[];  // ncols coefficients
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * kLzThreads;
    int64_t i = (int64_t)blockIdx.x * kLzThreads + threadIdx.x;
    double v[kLzUnroll];
#pragma unroll
    for (int u = 0; u < kLzUnroll; ++u) v[u] = (i < n && u < ncols) ? V[i + (int64_t)u * ldv] : 0.0;
    for (int c = q; c < ncols; c += 4) {
        const double a = lz_finish_sum(part + (int64_t)c * ldp, nchunks, lane);
        if (lane == 0) {
            hs[c] = a;
            if (blockIdx.x == 0) h_out[c] = a;
        }
    }
    __syncthreads();
    bool first = true;
    for (; i < n; i += stride) {
        double acc = 0.0;
        for (int c0 = 0; c0 < ncols; c0 += kLzUnroll) {
            if (!(first && c0 == 0)) {
#pragma unroll
                for (int u = 0; u < kLzUnroll; ++u) v[u] = (c0 + u < ncols) ? V[i + (int64_t)(c0 + u) * ldv] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kLzUnroll; ++u)
                if (c0 + u < ncols) acc = fma(hs[c0 + u], v[u], acc);
        }
        first = false;
        w[i] -= acc;
    }
}

// From the partial sums of w^T t (part[0..nchunks), lz_finish_sum): beta^2, then v_next = w / beta and rhs_next = t / beta.
// Workgroup 0 leaves beta^2 and the two sums of the inner-solve check (chk_part, nchk pairs) in out[0..2].  A beta^2 that is not
// positive and finite scales by zero: the host reads it from the slot and stops.
__global__ __launch_bounds__(kLzThreads) void lz_tail_kernel(int64_t n, const double* w, const double* t, const double* __restrict__ part, int nchunks,
                                                             double* vnext, double* rhs_next, const double* __restrict__ chk_part, int nchk,
                                                             double* __restrict__ out) {
    __shared__ double b2s;
    if (threadIdx.x < 64) {
        const double a = lz_finish_sum(part, nchunks, threadIdx.x);
        if (threadIdx.x == 0) b2s = a;
        if (blockIdx.x == 0) {
            double c0 = 0.0, c1 = 0.0;
            if (chk_part)
                for (int k = threadIdx.x; k < nchk; k += 64) {
                    c0 += chk_part[2 * k];
                    c1 += chk_part[2 * k + 1];
                }
            c0 = lz_wave_sum(c0);
            c1 = lz_wave_sum(c1);
            if (threadIdx.x == 0) {
                out[0] = a;
                out[1] = c0;
                out[2] = c1;
            }
        }
    }
    __syncthreads();
    const double b2 = b2s;
    const double inv = (b2 > 0.0 && b2 < 1.7e308) ? 1.0 / sqrt(b2) : 0.0;
    const int64_t stride = (int64_t)gridDim.x * kLzThreads;
    for (int64_t i = (int64_t)blockIdx.x * kLzThreads + threadIdx.x; i < n; i += stride) {
        const double wi = w[i], ti = t[i];
        vnext[i] = wi * inv;
        rhs_next[i] = ti * inv;
    }
}

// Each column's entry of largest magnitude (the first of equals) made positive: one workgroup per column.
__global__ __launch_bounds__(kLzThreads) void lz_sign_kernel(int64_t n, double* X, int64_t ldx) {
    __shared__ double bm[kLzThreads];
    __shared__ long long bi[kLzThreads];
    double* x = X + (int64_t)blockIdx.x * ldx;
    double best = -1.0;
    long long at = 0;
    for (int64_t i = threadIdx.x; i < n; i += kLzThreads) {
        const double a = fabs(x[i]);
        if (a > best) best = a, at = i;
    }
    bm[threadIdx.x] = best;
    bi[threadIdx.x] = at;
    __syncthreads();
    for (int s = kLzThreads / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const double o = bm[threadIdx.x + s];
            const long long oi = bi[threadIdx.x + s];
            if (o > bm[threadIdx.x] || (o == bm[threadIdx.x] && oi < bi[threadIdx.x])) bm[threadIdx.x] = o, bi[threadIdx.x] = oi;
        }
        __syncthreads();
    }
    if (n == 0) return;
    const bool flip = x[bi[0]] < 0.0;
    __syncthreads();
    if (flip)
        for (int64_t i = threadIdx.x; i < n; i += kLzThreads) x[i] = -x[i];
}

int lz_check_launch(lsa_ctx* ctx, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lsa_set_error(ctx, LSA_ERR_HIP, "%s: kernel launch failed: %s", what, hipGetErrorString(e));
    return LSA_OK;
}

// the fused kernels unless LSA_LANCZOS_FUSED=0 (read once per process, like LSA_KRYLOV_FUSED): then k_multi_dot + k_multi_axpy
bool lz_fused() {
    static const bool fused = env_flag("LSA_LANCZOS_FUSED", true);
    return fused;
}

}  // namespace

struct lsa_lanczos {
    lsa_ctx* ctx = nullptr;
    lsa_op* op = nullptr;
    lsa_op_parts P{};
    int64_t n = 0;
    int32_t ncv = 0;
    // the n x (ncv + 1) arrays: the basis, the restart's second basis and (with a row permutation, on first use) the Ritz vectors in
    // the caller's numbering
    double *V = nullptr, *V2 = nullptr, *xtmp = nullptr;
    int32_t* row_perm = nullptr;
    double *w = nullptr, *t = nullptr, *z = nullptr, *r = nullptr;  // work vectors: OP v_j, M w, C w, the refinement's residual
    double* rhs[2] = {nullptr, nullptr};  // M v_j of the current step / of the next one (a step that is redone finds its own intact)
    int cur = 0;
    int32_t rhs_for = -1;   // rhs[cur] holds M v_j for this j, -1: nothing
    double* part = nullptr;      // (ncv + 2) x kLzMaxChunks partial sums, a coefficient's chunks side by side
    double* chk_part = nullptr;  // kLzMaxChunks pairs
    double* slot = nullptr;      // h of pass 1 (ncv + 1), h of pass 2 (ncv + 1), beta^2, |rhs - C w|^2, |rhs|^2, the unfused form's w^T t,
                                 // |w|^2 of a refined solve
    double* qdev = nullptr;      // (ncv + 1)^2: the restart's and the Ritz vectors' coefficients
    int ldp = 0;
    std::vector<double> hslot;
    // another operator behind a step than the single solve (lanczos_set_operator), and the right-hand side of its last solve: the
    // check pair of the step's first reduction is (chk_b, z) then
    const lanczos_operator* hook = nullptr;
    const double* chk_b = nullptr;
};

namespace {

size_t lz_slot_doubles(int32_t ncv) { return (size_t)2 * (ncv + 1) + 5; }

void lz_free(lsa_lanczos* l) {
    for (void* p : {(void*)l->V, (void*)l->V2, (void*)l->xtmp, (void*)l->row_perm, (void*)l->w, (void*)l->t, (void*)l->z, (void*)l->r, (void*)l->rhs[0],
                    (void*)l->rhs[1], (void*)l->part, (void*)l->chk_part, (void*)l->slot, (void*)l->qdev})
        if (p) (void)hipFree(p);
    delete l;
}

double* lz_col(const lsa_lanczos* l, int32_t j) { return l->V + (size_t)j * (size_t)l->n; }

// t = M w (or t aliases w for a standard problem)
int lz_mass(lsa_ctx* ctx, lsa_lanczos* l, const double* x, double* y) {
    if (!l->P.Kmul) return LSA_OK;
    ++l->P.st->spmv_calls;
    return k_spmv(ctx, l->P.Kmul, LSA_F64, x, y);
}

// M-orthogonalise l->w against the columns 0..ncols-1 (two passes), then v = w / beta into column `target` and M v into the
// other right-hand side buffer; the slot's beta^2 and check sums are read back by the caller.  chk: this step's check pairs ride
// in the first reduction.
int lz_orth_tail(lsa_ctx* ctx, lsa_lanczos* l, int32_t ncols, int32_t target, bool chk) {
    const int64_t n = l->n;
    const bool has_m = l->P.Kmul != nullptr;
    const double* t = has_m ? l->t : l->w;
    double* vnext = lz_col(l, target);
    double* rhs_next = l->rhs[l->cur ^ 1];
    double* out = l->slot + 2 * (size_t)(l->ncv + 1);
    const double* chk_b = l->chk_b ? l->chk_b : l->rhs[l->cur];
    if (lz_fused()) {
        // k_multi_dot's chunks: at most 2048 of them, whole multiples of 256 rows, at least 512 rows
        int64_t rows_per_block = ((n + kLzMaxChunks - 1) / kLzMaxChunks + kLzThreads - 1) / kLzThreads * kLzThreads;
        rows_per_block = std::max<int64_t>(rows_per_block, 2 * kLzThreads);
        const int nchunks = (int)std::max<int64_t>((n + rows_per_block - 1) / rows_per_block, 1);
        // every workgroup of the update finishes h for itself: a few hundred of them, their rows strided over the grid
        const int ublocks = (int)std::max<int64_t>(std::min<int64_t>((n + kLzThreads - 1) / kLzThreads, (int64_t)ctx->num_cu * 2), 1);
        for (int pass = 0; pass < 2 && ncols > 0; ++pass) {
            LSA_CHECK(lz_mass(ctx, l, l->w, l->t));
            const int tiles = (ncols + 1 + kLzColTile - 1) / kLzColTile;
            const bool c = chk && pass == 0;
            hipLaunchKernelGGL(lz_dot_kernel, dim3(nchunks, tiles), dim3(kLzThreads), 0, ctx->stream, n, ncols, rows_per_block, l->V, n, t, l->w, l->part,
                               nchunks, c ? chk_b : nullptr, c ? l->z : nullptr, c ? l->chk_part : nullptr);
            hipLaunchKernelGGL(lz_update_kernel, dim3(ublocks), dim3(kLzThreads), (size_t)ncols * sizeof(double), ctx->stream, n, ncols, l->V,
                               n, l->part, nchunks, nchunks, l->w, l->slot + (size_t)pass * (l->ncv + 1));
        }
        LSA_CHECK(lz_mass(ctx, l, l->w, l->t));
        const bool c = chk && ncols == 0;
        hipLaunchKernelGGL(lz_dot_kernel, dim3(nchunks, 1), dim3(kLzThreads), 0, ctx->stream, n, 0, rows_per_block, l->V, n, t, l->w, l->part, nchunks,
                           c ? chk_b : nullptr, c ? l->z : nullptr, c ? l->chk_part : nullptr);
        const int tblocks = (int)std::max<int64_t>(std::min<int64_t>((n + kLzThreads - 1) / kLzThreads, (int64_t)ctx->num_cu * 8), 1);
        hipLaunchKernelGGL(lz_tail_kernel, dim3(tblocks), dim3(kLzThreads), 0, ctx->stream, n, l->w, t, l->part, nchunks, vnext, rhs_next,
                           chk ? l->chk_part : nullptr, nchunks, out);
        return lz_check_launch(ctx, "lanczos step");
    }
    // the unfused form: the library's multi-dot and multi-axpy, the same tail with single partial sums
    if (chk) LSA_CHECK(k_residual_norms(ctx, LSA_F64, n, chk_b, l->z, l->r, l->chk_part));
    for (int pass = 0; pass < 2 && ncols > 0; ++pass) {
        LSA_CHECK(lz_mass(ctx, l, l->w, l->t));
        double* h = l->slot + (size_t)pass * (l->ncv + 1);
        LSA_CHECK(k_multi_dot(ctx, LSA_F64, n, ncols, l->V, n, t, h));
        LSA_CHECK(k_multi_axpy(ctx, LSA_F64, n, ncols, l->V, n, h, l->w, nullptr));
    }
    LSA_CHECK(lz_mass(ctx, l, l->w, l->t));
    LSA_CHECK(k_multi_dot(ctx, LSA_F64, n, 1, l->w, n, t, out + 3));
    const int tblocks = (int)std::max<int64_t>(std::min<int64_t>((n + kLzThreads - 1) / kLzThreads, (int64_t)ctx->num_cu * 8), 1);
    hipLaunchKernelGGL(lz_tail_kernel, dim3(tblocks), dim3(kLzThreads), 0, ctx->stream, n, l->w, t, out + 3, 1, vnext, rhs_next,
                       chk ? l->chk_part : nullptr, 1, out);
    return lz_check_launch(ctx, "lanczos step (unfused)");
}

// the slot to the host: one synchronisation
int lz_read_slot(lsa_ctx* ctx, lsa_lanczos* l) {
    const size_t bytes = lz_slot_doubles(l->ncv) * sizeof(double);
    LSA_CHECK(lsa_ensure_scratch(ctx, 0, bytes));
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(ctx->pinned, l->slot, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (l->hook) LSA_CHECK(l->hook->read_back(ctx, l->hook->self));  // (its log travels behind the same synchronisation)
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(l->hslot.data(), ctx->pinned, bytes);
    return LSA_OK;
}

}  // namespace

int lanczos_shape(const lsa_lanczos* l, int64_t* n, int32_t* ncv) {
    if (!l) return LSA_ERR_ARG;
    if (n) *n = l->n;
    if (ncv) *ncv = l->ncv;
    return LSA_OK;
}

void lanczos_set_operator(lsa_lanczos* l, const lanczos_operator* hook) { l->hook = hook; }

const double* lanczos_ritz_device(const lsa_lanczos* l) { return l->V2; }

int lanczos_inject(lsa_ctx* ctx, lsa_lanczos* l, int32_t j, const double* host_v) {
    if (!ctx || !l || !host_v) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos: null argument");
    if (j < 0 || j > l->ncv) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos: column %d out of range", j);
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(l->w, host_v, (size_t)l->n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    LSA_CHECK(lz_orth_tail(ctx, l, j, j, false));
    LSA_CHECK(lz_read_slot(ctx, l));
    const double b2 = l->hslot[2 * (size_t)(l->ncv + 1)];
    if (!(b2 > 0.0) || !std::isfinite(b2))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos: v^T M v = %.3e for the injected vector: M is not positive definite on the Krylov space (or the "
                                               "vector is zero or not finite)", b2);
    l->cur ^= 1;
    l->rhs_for = j;
    return LSA_OK;
}

int lanczos_restart(lsa_ctx* ctx, lsa_lanczos* l, int32_t m, int32_t knew, const double* Y, int32_t ldy) {
    if (!ctx || !l || !Y) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos restart: null argument");
    if (m < 1 || m > l->ncv || knew < 1 || knew > m || ldy < m) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos restart: bad sizes m=%d knew=%d", m, knew);
    LSA_CHECK(basis_times_host_matrix(ctx, LSA_F64, l->n, m, knew, l->V, Y, ldy, l->qdev, l->V2, 0));
    LSA_CHECK(k_copy(ctx, LSA_F64, l->n, lz_col(l, m), l->V2 + (size_t)knew * (size_t)l->n));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    std::swap(l->V, l->V2);
    if (l->rhs_for == m) l->rhs_for = knew;  // (the same vector under its new index)
    else l->rhs_for = -1;
    return LSA_OK;
}

int lanczos_ritz_vectors(lsa_ctx* ctx, lsa_lanczos* l, int32_t m, int32_t nvec, const double* Y, int32_t ldy, double* X) {
    if (!ctx || !l || !Y || !X) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos vectors: null argument");
    if (m < 1 || m > l->ncv || nvec < 0 || nvec > l->ncv || ldy < m) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos vectors: bad sizes");
    if (nvec == 0) return LSA_OK;
    const size_t vb = (size_t)l->n * sizeof(double);
    LSA_CHECK(basis_times_host_matrix(ctx, LSA_F64, l->n, m, nvec, l->V, Y, ldy, l->qdev, l->V2, 0));
    hipLaunchKernelGGL(lz_sign_kernel, dim3(nvec), dim3(kLzThreads), 0, ctx->stream, l->n, l->V2, l->n);
    const double* src = l->V2;
    if (l->row_perm) {
        if (!l->xtmp) LSA_HIP_ALLOC(ctx, hipMalloc((void**)&l->xtmp, std::max<size_t>(vb, 8) * (size_t)(l->ncv + 1)));
        LSA_CHECK(k_scatter_rows(ctx, LSA_F64, l->n, nvec, l->row_perm, l->V2, l->xtmp));
        src = l->xtmp;
    }
    LSA_CHECK(lz_check_launch(ctx, "lanczos vectors"));
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(X, src, vb * (size_t)nvec, hipMemcpyDeviceToHost, ctx->stream));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return LSA_OK;
}

extern "C" {

int lsa_lanczos_create(lsa_ctx* ctx, lsa_op* op, int32_t ncv, lsa_lanczos** out) {
    if (!ctx || !op || !out || ncv < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_create: bad argument");
    lsa_op_parts P{};
    LSA_CHECK(lsa_op_get_parts(op, &P));
    if (!P.plain || ctx->nranks != 1)
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_create: needs a shift-invert operator (mode 0), forward and unprojected, on one rank");
    if (!P.nd || !P.Kfac || P.Kfac->dtype != LSA_F64 || (P.Kmul && P.Kmul->dtype != LSA_F64))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_create: needs real matrices, a real shift and the exact LU (pc_type 2) of K - sigma M");
    if ((int64_t)ncv > P.n) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_create: ncv = %d exceeds the problem size %lld", ncv, (long long)P.n);
    lsa_lanczos* l = new lsa_lanczos();
    l->ctx = ctx;
    l->op = op;
    l->P = P;
    l->n = P.n;
    l->ncv = ncv;
    l->ldp = ncv + 2;
    l->hslot.assign(lz_slot_doubles(ncv), 0.0);
    const size_t vb = (size_t)std::max<int64_t>(l->n, 1) * sizeof(double);
    bool ok = hipMalloc((void**)&l->V, vb * (size_t)(ncv + 1)) == hipSuccess && hipMalloc((void**)&l->V2, vb * (size_t)(ncv + 1)) == hipSuccess;
    for (double** p : {&l->w, &l->t, &l->z, &l->r, &l->rhs[0], &l->rhs[1]}) ok = ok && hipMalloc((void**)p, vb) == hipSuccess;
    ok = ok && hipMalloc((void**)&l->part, (size_t)kLzMaxChunks * l->ldp * sizeof(double)) == hipSuccess &&
         hipMalloc((void**)&l->chk_part, (size_t)kLzMaxChunks * 2 * sizeof(double)) == hipSuccess &&
         hipMalloc((void**)&l->slot, lz_slot_doubles(ncv) * sizeof(double)) == hipSuccess &&
         hipMalloc((void**)&l->qdev, (size_t)(ncv + 1) * (size_t)(ncv + 1) * sizeof(double)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        lz_free(l);
        return lsa_set_error(ctx, LSA_ERR_OOM, "lsa_lanczos_create: out of device memory (n=%lld, ncv=%d)", (long long)P.n, ncv);
    }
    (void)hipMemsetAsync(l->slot, 0, lz_slot_doubles(ncv) * sizeof(double), ctx->stream);
    *out = l;
    return LSA_OK;
}

void lsa_lanczos_destroy(lsa_lanczos* l) {
    if (!l) return;
    if (l->ctx && l->ctx->stream) (void)hipStreamSynchronize(l->ctx->stream);
    lz_free(l);
}

int lsa_lanczos_set_row_permutation(lsa_ctx* ctx, lsa_lanczos* l, const int32_t* perm) {
    if (!ctx || !l) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_set_row_permutation: null argument");
    return basis_upload_row_permutation(ctx, "lsa_lanczos_set_row_permutation", l->n, perm, &l->row_perm);
}

int lsa_lanczos_set_start(lsa_ctx* ctx, lsa_lanczos* l, const double* host_v) { return lanczos_inject(ctx, l, 0, host_v); }

int lsa_lanczos_extend(lsa_ctx* ctx, lsa_lanczos* l, int32_t j0, int32_t j1, double* T, int32_t ldt, int32_t* breakdown) {
    if (!ctx || !l || !T) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_extend: null argument");
    if (j0 < 0 || j1 < j0 || j1 > l->ncv || ldt < j1 + 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_extend: bad step range [%d, %d) for ncv %d", j0, j1, l->ncv);
    if (breakdown) *breakdown = -1;
    const double t0 = now_s();
    const int64_t n = l->n;
    lsa_stats* st = l->P.st;
    const double rtol = l->P.ksp_rtol;
    const size_t b2_at = 2 * (size_t)(l->ncv + 1);
    int rc = LSA_OK;
    for (int32_t j = j0; j < j1 && rc == LSA_OK; ++j) {
        if (l->rhs_for != j) {  // (after lsa_lanczos_basis users, a restart that moved another column here, or the standard problem's first step)
            if (l->P.Kmul) rc = lz_mass(ctx, l, lz_col(l, j), l->rhs[l->cur]);
            else rc = k_copy(ctx, LSA_F64, n, lz_col(l, j), l->rhs[l->cur]);
            if (rc != LSA_OK) break;
            l->rhs_for = j;
        }
        while (l->hook) {
            // the hook's operator: it queues w = OP v_j from rhs = M v_j and names the right-hand side of its last solve (z = C w of
            // that solve is in l->z); the step's reductions, tail and single read-back are those of the default; the hook judges
            bool refined = false;
            rc = l->hook->enqueue(ctx, l->hook->self, j, l->rhs[l->cur], l->w, l->z, l->r, l->slot + b2_at + 4, &l->chk_b, &refined);
            if (rc == LSA_OK) rc = lz_orth_tail(ctx, l, j + 1, j + 1, true);
            if (rc == LSA_OK) rc = lz_read_slot(ctx, l);
            if (rc != LSA_OK) break;
            const int verdict = l->hook->judge(ctx, l->hook->self, j, std::sqrt(l->hslot[b2_at + 1]), std::sqrt(l->hslot[b2_at + 2]),
                                               refined ? std::sqrt(l->hslot[b2_at + 4]) : 0.0);
            if (verdict == 0) break;
            if (verdict < 0) {  // (the hook has set the error)
                rc = LSA_ERR_DIVERGED;
                break;
            }
        }
        while (!l->hook) {
            const bool refine = *l->P.refine;
            // (w += C^-1 (rhs - C w) with refine: takes what large factors leave behind to rounding level)
            rc = direct_solve_enqueue(ctx, l->op, LSA_F64, l->rhs[l->cur], l->w, l->z, l->r, refine, l->chk_part);
            if (rc == LSA_OK && refine) rc = k_nrm2(ctx, LSA_F64, n, l->w, l->slot + b2_at + 4);  // for the backward-error judgement below
            if (rc == LSA_OK) rc = lz_orth_tail(ctx, l, j + 1, j + 1, true);
            if (rc == LSA_OK) rc = lz_read_slot(ctx, l);
            if (rc != LSA_OK) break;
            const double res = std::sqrt(l->hslot[b2_at + 1]), bnorm = std::sqrt(l->hslot[b2_at + 2]);
            // The library's judgement of a direct solve (gmres_run): within ksp_rtol, or, after the refinement step, a backward
            // error within 1e-12 ||C||_F -- ||rhs - C w|| cannot go below eps ||C|| ||w||, whatever the solver.
            const bool backward = refine && res > rtol * bnorm && l->P.normF > 0.0 && res <= 1e-12 * l->P.normF * std::sqrt(l->hslot[b2_at + 4]);
            if (backward) ++st->backward_accepted;
            if (res <= rtol * bnorm || backward) {
                stats_book_direct_solve(st, 1, refine, res, bnorm);
                break;
            }
            if (!refine && std::isfinite(res)) {  // from here on every step carries the refinement step; this one is done again
                *l->P.refine = true;
                continue;
            }
            rc = lsa_set_error(ctx, LSA_ERR_DIVERGED, "lsa_lanczos_extend: the inner solve of step %d left a relative residual of %.3e after its refinement "
                                                      "step (ksp_rtol %.1e) and a backward error above 1e-12 ||C||_F", j, bnorm > 0.0 ? res / bnorm : res, rtol);
            break;
        }
        if (rc != LSA_OK) break;
        const double alpha = l->hslot[j] + l->hslot[(size_t)(l->ncv + 1) + j];
        const double b2 = l->hslot[b2_at];
        if (!std::isfinite(alpha) || !std::isfinite(b2)) {
            rc = lsa_set_error(ctx, LSA_ERR_NONFINITE, "Lanczos: non-finite recurrence coefficient at step %d", j);
            break;
        }
        // what is left of w after both passes, against the size of what was taken out of it (the rule of the general loop's columns)
        double colmax = std::fabs(alpha);
        for (int32_t i = 0; i < j; ++i) colmax = std::max(colmax, std::fabs(l->hslot[i] + l->hslot[(size_t)(l->ncv + 1) + i]));
        const double thr = 1e-14 * std::max(colmax, 1e-300);
        if (b2 < -thr * thr) {
            rc = lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_extend: w^T M w = %.3e at step %d: M is not positive definite on the Krylov space", b2, j);
            break;
        }
        const double beta = b2 > 0.0 ? std::sqrt(b2) : 0.0;
        const bool broke = beta <= thr;
        T[(size_t)j * ldt + j] = alpha;
        T[(size_t)j * ldt + j + 1] = broke ? 0.0 : beta;
        if (j + 1 < l->ncv && j + 1 < ldt) T[(size_t)(j + 1) * ldt + j] = broke ? 0.0 : beta;
        l->cur ^= 1;
        l->rhs_for = j + 1;
        if (broke) {
            l->rhs_for = -1;
            if (breakdown) *breakdown = j;
            break;
        }
    }
    st->seconds_solve += now_s() - t0;
    return rc;
}

int lsa_lanczos_basis(lsa_ctx* ctx, const lsa_lanczos* l, int32_t ncols, double* host_V) {
    if (!ctx || !l || !host_V) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_basis: null argument");
    if (ncols < 0 || ncols > l->ncv + 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_basis: %d columns of %d", ncols, l->ncv + 1);
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(host_V, l->V, (size_t)l->n * (size_t)ncols * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return LSA_OK;
}

}  // extern "C"
