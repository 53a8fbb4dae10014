// Region eigensolver: all eigenvalues of A x = lambda M x inside an ellipse, with a statement of completeness, by a contour-integral
// (FEAST-type) subspace iteration on an n x L complex128 block Y (column-major):
//     B = M Y                                                  ci_spmm_kernel
//     for every node z_k of the contour: X = C_k^-1 B on the nested-dissection LU of C_k = A - z_k M (ndlu_solve_run; under
//         lsa_contour_set_batch_nodes all nodes' X_k first, in lockstep: the same request on a batch of sets), each
//         column checked (R = C_k X by ci_spmm_kernel, the three sums by ci_residual_kernel), then Q (+)= -w_k X
//                                                              ci_accumulate_kernel
//     U = orth(Q) through the Gram matrix, twice               ci_gram_kernel + host Hermitian eigen-decomposition + k_basis_gemm
//     A_h = U^H (A U), M_h = U^H (M U), Ritz pairs of M_h^-1 A_h on the host (complex LU, lsa_dense_schur)
//     residuals of all Ritz pairs from A U, M U and S          k_basis_gemm + ci_residual_kernel
// Q = -sum_k w_k C_k^-1 M Y is the quadrature of the spectral projector (1 / 2 pi i) oint (z M - A)^-1 M dz applied to Y.  The two
// building blocks are also entry points of their own (lsa_spmm, lsa_block_gram), and so is the transposed block product a left
// (adjoint) phase needs (lsa_spmm_transpose: ci_spmm_kernel on the pattern's transposed index); blocks have leading dimensions >= n
// there and n inside the iteration.
//
// Every sum runs in a fixed order and there are no floating-point atomics: two calls give the same bits.
//   ci_spmm_kernel   the entries of a row strided over the 8 lanes of its row group, each lane adding its entries in order; then the
//                    xor tree over the 8 lanes.  A pass of up to 8 columns reads the matrix's indices and values once.
//   ci_gram_kernel   the rows of a chunk strided over the 256 threads, each adding its rows in order; the xor tree of the wavefront;
//                    the four waves in wave order; ci_gram_finish_kernel then adds the chunks in chunk order.
#include <algorithm>
#include <cmath>
#include <complex>
#include <numeric>

#include "shifted_sets.h"

namespace {

constexpr int kCiThreads = 256;       // four wavefronts of 64
constexpr int kCiRowLanes = 8;        // lanes that share a row of ci_spmm_kernel
constexpr int kCiColTile = 8;         // columns of a pass of ci_spmm_kernel: 8 accumulators of 16 bytes per lane
constexpr int kCiGramTile = 4;        // ci_gram_kernel: a workgroup sums a 4 x 4 tile of G (16 accumulators per thread)
constexpr int kCiGramMaxChunks = 64;  // row chunks of ci_gram_kernel = partial sums per entry of G
constexpr int kCiMaxCols = 128;       // p, q of lsa_block_gram

// a complex entry is moved as one 16-byte access (cplx itself is only 8-byte aligned); every array of this file is 16-byte
// aligned: hipMalloc, offsets in whole complex numbers
typedef double ci_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ cplx ci_ld(const cplx* p) {
    const ci_d2 v = *reinterpret_cast<const ci_d2*>(p);
    return cplx{v.x, v.y};
}
__device__ __forceinline__ double ci_ld(const double* p) { return *p; }
__device__ __forceinline__ void ci_st(cplx* p, cplx v) {
    ci_d2 o;
    o.x = v.re;
    o.y = v.im;
    *reinterpret_cast<ci_d2*>(p) = o;
}

// Y[:, 0:nc] = A X[:, 0:nc], nc <= kCiColTile.  Row r belongs to the 8 lanes 8 (r % 32) .. of workgroup r / 32; lane s takes the
// entries rp[r] + s, rp[r] + s + 8, ...: one load of the column index and of the value per entry, then the nc entries of that row
// of X (all requested before the first multiply-add of a full pass).  Rows beyond n take an empty range, so that every lane of a
// wavefront reaches the shuffles.
// TRANS: Y = A^T X (conj != 0: A^H X) in pull form on the pattern's transposed index (TransposeIndex: rp, ci are its arrays, the
// value of entry p lies at val[src[p]]) -- an output's entries ordered by row, the same lanes and tree, no atomics.
template <typename MT, bool TRANS>
__global__ __launch_bounds__(kCiThreads) void ci_spmm_kernel(int32_t n, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                                             const int32_t* __restrict__ src, int conj, const MT* __restrict__ val, int nc,
                                                             const cplx* __restrict__ X, int64_t ldx, cplx* __restrict__ Y, int64_t ldy) {
    auto entry = [&](int32_t p) {
        if constexpr (TRANS) {
            const MT a = ci_ld(val + src[p]);
            return conj ? s_conj(a) : a;
        } else {
            return ci_ld(val + p);
        }
    };
    const int sub = threadIdx.x & (kCiRowLanes - 1);
    const int64_t row = (int64_t)blockIdx.x * (kCiThreads / kCiRowLanes) + (threadIdx.x / kCiRowLanes);
    int32_t p0 = 0, p1 = 0;
    if (row < n) {
        p0 = rp[row];
        p1 = rp[row + 1];
    }
    cplx acc[kCiColTile];
#pragma unroll
    for (int u = 0; u < kCiColTile; ++u) acc[u] = cplx{0.0, 0.0};
    if (nc == kCiColTile) {
        for (int32_t p = p0 + sub; p < p1; p += kCiRowLanes) {
            const cplx* x = X + ci[p];
            const MT a = entry(p);
            cplx xv[kCiColTile];
#pragma unroll
            for (int u = 0; u < kCiColTile; ++u) xv[u] = ci_ld(x + (int64_t)u * ldx);
#pragma unroll
            for (int u = 0; u < kCiColTile; ++u) fma_acc(acc[u], a, xv[u]);
        }
    } else {
        for (int32_t p = p0 + sub; p < p1; p += kCiRowLanes) {
            const cplx* x = X + ci[p];
            const MT a = entry(p);
#pragma unroll
            for (int u = 0; u < kCiColTile; ++u)
                if (u < nc) fma_acc(acc[u], a, ci_ld(x + (int64_t)u * ldx));
        }
    }
#pragma unroll
    for (int u = 0; u < kCiColTile; ++u) {
#pragma unroll
        for (int off = kCiRowLanes / 2; off >= 1; off >>= 1) {
            acc[u].re += __shfl_xor(acc[u].re, off, 64);
            acc[u].im += __shfl_xor(acc[u].im, off, 64);
        }
    }
    if (sub == 0 && row < n) {
#pragma unroll
        for (int u = 0; u < kCiColTile; ++u)
            if (u < nc) ci_st(Y + row + (int64_t)u * ldy, acc[u]);
    }
}

__device__ __forceinline__ cplx ci_wave_sum(cplx v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        v.re += __shfl_xor(v.re, off, 64);
        v.im += __shfl_xor(v.im, off, 64);
    }
    return v;
}

// Partial sums of the tile G[i0 .. i0 + 4, j0 .. j0 + 4) of G = U^H W over the rows of one chunk: workgroup (chunk, i0 / 4, j0 / 4)
// writes part[(chunk q + j) p + i].  A full tile has its eight 16-byte loads of a row in flight before the first addition.
__global__ __launch_bounds__(kCiThreads) void ci_gram_kernel(int64_t n, int64_t rows_per_block, int p, int q, const cplx* __restrict__ U, int64_t ldu,
                                                             const cplx* __restrict__ W, int64_t ldw, cplx* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) cplx wsum[4][kCiGramTile * kCiGramTile];
    const int chunk = blockIdx.x;
    const int i0 = blockIdx.y * kCiGramTile, j0 = blockIdx.z * kCiGramTile;
    const int np = (p - i0 < kCiGramTile) ? p - i0 : kCiGramTile;
    const int nq = (q - j0 < kCiGramTile) ? q - j0 : kCiGramTile;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r0 = (int64_t)chunk * rows_per_block;
    const int64_t r1 = (r0 + rows_per_block < n) ? r0 + rows_per_block : n;
    const cplx* ucol = U + (int64_t)i0 * ldu;
    const cplx* wcol = W + (int64_t)j0 * ldw;
    cplx acc[kCiGramTile][kCiGramTile];
#pragma unroll
    for (int a = 0; a < kCiGramTile; ++a)
#pragma unroll
        for (int b = 0; b < kCiGramTile; ++b) acc[a][b] = cplx{0.0, 0.0};
    if (np == kCiGramTile && nq == kCiGramTile) {
        for (int64_t i = r0 + threadIdx.x; i < r1; i += kCiThreads) {
            cplx u[kCiGramTile], w[kCiGramTile];
#pragma unroll
            for (int a = 0; a < kCiGramTile; ++a) u[a] = ci_ld(ucol + i + (int64_t)a * ldu);
#pragma unroll
            for (int b = 0; b < kCiGramTile; ++b) w[b] = ci_ld(wcol + i + (int64_t)b * ldw);
#pragma unroll
            for (int a = 0; a < kCiGramTile; ++a)
#pragma unroll
                for (int b = 0; b < kCiGramTile; ++b) fma_conj_acc(acc[a][b], u[a], w[b]);
        }
    } else {
        for (int64_t i = r0 + threadIdx.x; i < r1; i += kCiThreads) {
            cplx u[kCiGramTile], w[kCiGramTile];
#pragma unroll
            for (int a = 0; a < kCiGramTile; ++a) u[a] = (a < np) ? ci_ld(ucol + i + (int64_t)a * ldu) : cplx{0.0, 0.0};
#pragma unroll
            for (int b = 0; b < kCiGramTile; ++b) w[b] = (b < nq) ? ci_ld(wcol + i + (int64_t)b * ldw) : cplx{0.0, 0.0};
#pragma unroll
            for (int a = 0; a < kCiGramTile; ++a)
#pragma unroll
                for (int b = 0; b < kCiGramTile; ++b)
                    if (a < np && b < nq) fma_conj_acc(acc[a][b], u[a], w[b]);
        }
    }
#pragma unroll
    for (int a = 0; a < kCiGramTile; ++a)
#pragma unroll
        for (int b = 0; b < kCiGramTile; ++b) {
            const cplx s = ci_wave_sum(acc[a][b]);
            if (lane == 0) ci_st(&wsum[wave][a * kCiGramTile + b], s);
        }
    __syncthreads();
    if (threadIdx.x < kCiGramTile * kCiGramTile) {
        const int a = threadIdx.x / kCiGramTile, b = threadIdx.x % kCiGramTile;
        if (a < np && b < nq) {
            const int e = threadIdx.x;
            const cplx s = s_add(s_add(s_add(wsum[0][e], wsum[1][e]), wsum[2][e]), wsum[3][e]);
            ci_st(part + ((int64_t)chunk * q + (j0 + b)) * p + (i0 + a), s);
        }
    }
}

// G[e] = the chunks' partial sums of entry e, added in chunk order (a thread per entry: neighbouring threads read neighbouring
// entries of a chunk).  self: G = U^H U, whose diagonal is real -- the imaginary part the two roundings of conj(u) u leave is dropped.
__global__ __launch_bounds__(kCiThreads) void ci_gram_finish_kernel(int p, int q, int nchunks, const cplx* __restrict__ part, int self, cplx* __restrict__ G) {
    const int e = blockIdx.x * kCiThreads + threadIdx.x;
    if (e >= p * q) return;
    cplx s = ci_ld(part + e);
    for (int c = 1; c < nchunks; ++c) s = s_add(s, ci_ld(part + (int64_t)c * p * q + e));
    if (self && e % p == e / p) s.im = 0.0;
    ci_st(G + e, s);
}

// Q = alpha X + beta Q on a block (beta = 0: Q is not read), one pass: the quadrature accumulation Q (+)= -w_k X_k, and the two
// updates of a refinement step (R = B - R, X += D).  Column blockIdx.y, rows strided over the grid.
__global__ __launch_bounds__(kCiThreads) void ci_accumulate_kernel(int64_t n, cplx alpha, const cplx* __restrict__ X, int64_t ldx, double beta, cplx* Q,
                                                                   int64_t ldq) {
    const cplx* x = X + (int64_t)blockIdx.y * ldx;
    cplx* q = Q + (int64_t)blockIdx.y * ldq;
    const int64_t stride = (int64_t)gridDim.x * kCiThreads;
    for (int64_t i = (int64_t)blockIdx.x * kCiThreads + threadIdx.x; i < n; i += stride) {
        cplx v = s_mul(alpha, ci_ld(x + i));
        if (beta != 0.0) {
            const cplx o = ci_ld(q + i);
            v.re = fma(beta, o.re, v.re);
            v.im = fma(beta, o.im, v.im);
        }
        ci_st(q + i, v);
    }
}

__device__ __forceinline__ double ci_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Three sums per column j over the rows of one chunk: |P_j - lam_j Q_j|^2, |P_j|^2, |T_j|^2 (lam == null: 1) into
// part[(chunk cols + j) 3 + 0..2].  The residuals of all Ritz pairs (P = A U S, Q = T = M U S, lam the Ritz values) and the check of
// a block solve (P = B, Q = C_k X, T = X) are this kernel.
__global__ __launch_bounds__(kCiThreads) void ci_residual_kernel(int64_t n, int64_t rows_per_block, const cplx* __restrict__ P, int64_t ldp,
                                                                 const cplx* __restrict__ Qb, int64_t ldq, const cplx* __restrict__ T, int64_t ldt,
                                                                 const cplx* __restrict__ lam, double* __restrict__ part) {
    __shared__ double ws[4][3];
    const int chunk = blockIdx.x, j = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r0 = (int64_t)chunk * rows_per_block;
    const int64_t r1 = (r0 + rows_per_block < n) ? r0 + rows_per_block : n;
    const cplx l = lam ? ci_ld(lam + j) : cplx{1.0, 0.0};
    const cplx ml = cplx{-l.re, -l.im};
    const cplx *p = P + (int64_t)j * ldp, *q = Qb + (int64_t)j * ldq, *t = T + (int64_t)j * ldt;
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = r0 + threadIdx.x; i < r1; i += kCiThreads) {
        const cplx pv = ci_ld(p + i), qv = ci_ld(q + i), tv = ci_ld(t + i);
        cplx d = pv;
        fma_acc(d, ml, qv);
        s[0] = fma(d.im, d.im, fma(d.re, d.re, s[0]));
        s[1] = fma(pv.im, pv.im, fma(pv.re, pv.re, s[1]));
        s[2] = fma(tv.im, tv.im, fma(tv.re, tv.re, s[2]));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double v = ci_wave_sum(s[k]);
        if (lane == 0) ws[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) part[((int64_t)chunk * gridDim.y + j) * 3 + threadIdx.x] = ((ws[0][threadIdx.x] + ws[1][threadIdx.x]) + ws[2][threadIdx.x]) + ws[3][threadIdx.x];
}

// out[e] = the chunks' partial sums of entry e < entries, added in chunk order
__global__ __launch_bounds__(kCiThreads) void ci_residual_finish_kernel(int entries, int nchunks, const double* __restrict__ part, double* __restrict__ out) {
    const int e = blockIdx.x * kCiThreads + threadIdx.x;
    if (e >= entries) return;
    double s = part[e];
    for (int c = 1; c < nchunks; ++c) s += part[(int64_t)c * entries + e];
    out[e] = s;
}

// row chunks of the two-stage sums: whole multiples of 256 rows, at least 1024 rows, at most kCiGramMaxChunks of them
int64_t ci_chunk_rows(int64_t n) {
    const int64_t rows = ((n + kCiGramMaxChunks - 1) / kCiGramMaxChunks + kCiThreads - 1) / kCiThreads * kCiThreads;
    return std::max<int64_t>(rows, 4 * kCiThreads);
}

int ci_check_launch(lsa_ctx* ctx, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lsa_set_error(ctx, LSA_ERR_HIP, "%s: kernel launch failed: %s", what, hipGetErrorString(e));
    return LSA_OK;
}

// what a column-major block of `cols` columns of `rows` rows needs of its vector
bool ci_block_fits(const lsa_vec* v, int64_t rows, int32_t cols, int64_t ld) { return ld >= rows && v->n >= ld * (int64_t)(cols - 1) + rows; }

}  // namespace

int k_spmm(lsa_ctx* ctx, const lsa_mat* A, int32_t ncols, const void* X, int64_t ldx, void* Y, int64_t ldy) {
    if (A->n < 1 || ncols < 1) return LSA_OK;
    const int per_block = kCiThreads / kCiRowLanes;
    const int blocks = (A->n + per_block - 1) / per_block;
    for (int32_t c0 = 0; c0 < ncols; c0 += kCiColTile) {
        const int nc = std::min<int32_t>(kCiColTile, ncols - c0);
        const cplx* x = (const cplx*)X + (int64_t)c0 * ldx;
        cplx* y = (cplx*)Y + (int64_t)c0 * ldy;
        if (A->dtype == LSA_C128)
            hipLaunchKernelGGL((ci_spmm_kernel<cplx, false>), dim3(blocks), dim3(kCiThreads), 0, ctx->stream, A->n, A->rp, A->ci, nullptr, 0,
                               (const cplx*)A->val, nc, x, ldx, y, ldy);
        else
            hipLaunchKernelGGL((ci_spmm_kernel<double, false>), dim3(blocks), dim3(kCiThreads), 0, ctx->stream, A->n, A->rp, A->ci, nullptr, 0,
                               (const double*)A->val, nc, x, ldx, y, ldy);
    }
    return ci_check_launch(ctx, "k_spmm");
}

// Y[:, c] = A^T X[:, c] (conj != 0: A^H X[:, c]) for a whole square matrix: the passes of k_spmm on the transposed index of A's pattern
// (built by the first transposed product of any matrix of the pattern, shared by all of them)
int k_spmm_transpose(lsa_ctx* ctx, const lsa_mat* A, int conj, int32_t ncols, const void* X, int64_t ldx, void* Y, int64_t ldy) {
    if (A->n < 1 || ncols < 1) return LSA_OK;
    const TransposeIndex* T = nullptr;
    LSA_CHECK(k_transpose_index(ctx, A, &T));
    const int per_block = kCiThreads / kCiRowLanes;
    const int blocks = (A->ncols + per_block - 1) / per_block;
    for (int32_t c0 = 0; c0 < ncols; c0 += kCiColTile) {
        const int nc = std::min<int32_t>(kCiColTile, ncols - c0);
        const cplx* x = (const cplx*)X + (int64_t)c0 * ldx;
        cplx* y = (cplx*)Y + (int64_t)c0 * ldy;
        if (A->dtype == LSA_C128)
            hipLaunchKernelGGL((ci_spmm_kernel<cplx, true>), dim3(blocks), dim3(kCiThreads), 0, ctx->stream, A->ncols, T->rp, T->ci, T->src, conj,
                               (const cplx*)A->val, nc, x, ldx, y, ldy);
        else
            hipLaunchKernelGGL((ci_spmm_kernel<double, true>), dim3(blocks), dim3(kCiThreads), 0, ctx->stream, A->ncols, T->rp, T->ci, T->src, conj,
                               (const double*)A->val, nc, x, ldx, y, ldy);
    }
    return ci_check_launch(ctx, "k_spmm_transpose");
}

int k_block_gram(lsa_ctx* ctx, int64_t n, int32_t p, const void* U, int64_t ldu, int32_t q, const void* W, int64_t ldw, void* G_host) {
    const int64_t rows_per_block = ci_chunk_rows(n);
    const int nchunks = (int)((n + rows_per_block - 1) / rows_per_block);
    const size_t entries = (size_t)p * (size_t)q;
    LSA_CHECK(lsa_ensure_scratch(ctx, ((size_t)nchunks + 1) * entries * sizeof(cplx), entries * sizeof(cplx)));
    cplx* part = (cplx*)ctx->dscratch;
    cplx* G = part + (size_t)nchunks * entries;
    const int self = U == W && ldu == ldw && p == q;
    hipLaunchKernelGGL(ci_gram_kernel, dim3(nchunks, (p + kCiGramTile - 1) / kCiGramTile, (q + kCiGramTile - 1) / kCiGramTile), dim3(kCiThreads), 0,
                       ctx->stream, n, rows_per_block, p, q, (const cplx*)U, ldu, (const cplx*)W, ldw, part);
    hipLaunchKernelGGL(ci_gram_finish_kernel, dim3((int)((entries + kCiThreads - 1) / kCiThreads)), dim3(kCiThreads), 0, ctx->stream, p, q, nchunks, part,
                       self, G);
    LSA_CHECK(ci_check_launch(ctx, "k_block_gram"));
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(ctx->pinned, G, entries * sizeof(cplx), hipMemcpyDeviceToHost, ctx->stream));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(G_host, ctx->pinned, entries * sizeof(cplx));
    return LSA_OK;
}

extern "C" {

int lsa_spmm(lsa_ctx* ctx, const lsa_mat* A, int32_t ncols, const lsa_vec* X, int64_t ldx, lsa_vec* Y, int64_t ldy) {
    if (!ctx || !A || !X || !Y) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_spmm: null argument");
    if (A->n != A->ncols || A->row0 != 0) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_spmm: the matrix is a row shard (%d x %d): whole square matrices only", A->n, A->ncols);
    if (ncols < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_spmm: %d columns", ncols);
    if (X->dtype != LSA_C128 || Y->dtype != LSA_C128) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_spmm: the blocks must be complex128");
    if (X->d == Y->d) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_spmm: X and Y must not alias");
    if (!ci_block_fits(X, A->ncols, ncols, ldx) || !ci_block_fits(Y, A->n, ncols, ldy))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_spmm: a block of %d columns of %d rows with ldx = %lld, ldy = %lld does not fit vectors of %lld and %lld entries "
                                               "(ld >= n, length >= ld (ncols - 1) + n)", ncols, A->n, (long long)ldx, (long long)ldy, (long long)X->n, (long long)Y->n);
    return k_spmm(ctx, A, ncols, X->d, ldx, Y->d, ldy);
}

int lsa_spmm_transpose(lsa_ctx* ctx, const lsa_mat* A, int conj, int32_t ncols, const lsa_vec* X, int64_t ldx, lsa_vec* Y, int64_t ldy) {
    if (!ctx || !A || !X || !Y) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_spmm_transpose: null argument");
    if (A->n != A->ncols || A->row0 != 0)
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_spmm_transpose: the matrix is a row shard (%d x %d): whole square matrices only", A->n, A->ncols);
    if (ncols < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_spmm_transpose: %d columns", ncols);
    if (X->dtype != LSA_C128 || Y->dtype != LSA_C128) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_spmm_transpose: the blocks must be complex128");
    if (X->d == Y->d) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_spmm_transpose: X and Y must not alias");
    if (!ci_block_fits(X, A->n, ncols, ldx) || !ci_block_fits(Y, A->ncols, ncols, ldy))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_spmm_transpose: a block of %d columns of %d rows with ldx = %lld, ldy = %lld does not fit vectors of %lld and %lld "
                                               "entries (ld >= n, length >= ld (ncols - 1) + n)", ncols, A->n, (long long)ldx, (long long)ldy, (long long)X->n,
                             (long long)Y->n);
    return k_spmm_transpose(ctx, A, conj, ncols, X->d, ldx, Y->d, ldy);
}

int lsa_block_gram(lsa_ctx* ctx, int64_t n, int32_t p, const lsa_vec* U, int64_t ldu, int32_t q, const lsa_vec* W, int64_t ldw, void* G) {
    if (!ctx || !U || !W || !G) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_block_gram: null argument");
    if (n < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_block_gram: %lld rows", (long long)n);
    if (p < 1 || p > kCiMaxCols || q < 1 || q > kCiMaxCols) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_block_gram: %d x %d: between 1 and %d columns each", p, q, kCiMaxCols);
    if (U->dtype != LSA_C128 || W->dtype != LSA_C128) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_block_gram: the blocks must be complex128");
    if (!ci_block_fits(U, n, p, ldu) || !ci_block_fits(W, n, q, ldw))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_block_gram: blocks of %d and %d columns of %lld rows with ldu = %lld, ldw = %lld do not fit vectors of %lld and %lld "
                                               "entries (ld >= n, length >= ld (cols - 1) + n)", p, q, (long long)n, (long long)ldu, (long long)ldw, (long long)U->n,
                             (long long)W->n);
    return k_block_gram(ctx, n, p, U->d, ldu, q, W->d, ldw, G);
}

}  // extern "C"

// ---- the contour iteration ------------------------------------------------------------------------------------------------------

typedef std::complex<double> ci_z;

struct lsa_contour {
    lsa_ctx* ctx = nullptr;
    int64_t n = 0;
    int32_t N = 0, L = 0;  // nodes, columns of the subspace
    bool keep = false;     // N factor sets alive, or one that is refactorised node by node
    double ksp_rtol = 0.0;
    double centre[2] = {0.0, 0.0}, radii[2] = {0.0, 0.0};
    std::vector<ci_z> w;            // the nodes' weights
    // the pencils C_k = A - z_k M at the nodes with their factor sets; refine[0][k]: node k's block solves carry the refinement step
    shifted_sets* S = nullptr;
    // n x L blocks: the basis, M Y, a node's solutions, the quadrature sum, and two work blocks (C_k X; A U and M U)
    cplx *Y = nullptr, *B = nullptr, *X = nullptr, *Q = nullptr, *W1 = nullptr, *W2 = nullptr;
    cplx *qdev = nullptr, *lamdev = nullptr;  // L x L coefficients of k_basis_gemm, L Ritz values
    double *sums = nullptr, *imag2 = nullptr;  // 3 L column sums; what k_columns_canonical reports (not read)
    int32_t* row_perm = nullptr;
    // lsa_contour_set_batch_nodes: one n x L solution block per node (node k at XN + k n L), and what the lockstep solves did
    bool batch_nodes = false;
    cplx* XN = nullptr;
    int64_t batch_groups = 0, batch_columns = 0, serial_columns = 0;
    lsa_stats st{};
    int64_t bytes = 0;
    double sec_solve = 0.0, sec_product = 0.0, sec_gram = 0.0, sec_dense = 0.0;
    lsa_contour_left_stats left{};  // what the left phases did and took: booked apart from everything above (lsa_contour_left_info)
};

namespace {

void ct_free(lsa_contour* h) {
    shifted_sets_free(h->S);
    for (void* p : {(void*)h->Y, (void*)h->B, (void*)h->X, (void*)h->Q, (void*)h->W1, (void*)h->W2, (void*)h->qdev, (void*)h->lamdev, (void*)h->sums,
                    (void*)h->imag2, (void*)h->row_perm, (void*)h->XN})
        if (p) (void)hipFree(p);
    delete h;
}

int ct_sync(lsa_ctx* ctx) {
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return LSA_OK;
}

int ct_accumulate(lsa_ctx* ctx, int64_t n, int32_t cols, ci_z alpha, const cplx* X, double beta, cplx* Q) {
    const int blocks = (int)std::max<int64_t>(std::min<int64_t>((n + kCiThreads - 1) / kCiThreads, (int64_t)ctx->num_cu * 2), 1);
    hipLaunchKernelGGL(ci_accumulate_kernel, dim3(blocks, cols), dim3(kCiThreads), 0, ctx->stream, n, cplx{alpha.real(), alpha.imag()}, X, n, beta, Q, n);
    return ci_check_launch(ctx, "ci_accumulate_kernel");
}

// out[3 j + 0..2] = |P_j - lam_j Q_j|^2, |P_j|^2, |T_j|^2 for j < cols, on the host (one synchronisation)
int ct_column_sums(lsa_ctx* ctx, lsa_contour* h, int32_t cols, const cplx* P, const cplx* Qb, const cplx* T, const cplx* lam, double* out) {
    const int64_t n = h->n, rows_per_block = ci_chunk_rows(n);
    const int nchunks = (int)((n + rows_per_block - 1) / rows_per_block);
    const int entries = 3 * cols;
    LSA_CHECK(lsa_ensure_scratch(ctx, (size_t)nchunks * entries * sizeof(double), (size_t)entries * sizeof(double)));
    double* part = (double*)ctx->dscratch;
    hipLaunchKernelGGL(ci_residual_kernel, dim3(nchunks, cols), dim3(kCiThreads), 0, ctx->stream, n, rows_per_block, P, n, Qb, n, T, n, lam, part);
    hipLaunchKernelGGL(ci_residual_finish_kernel, dim3((entries + kCiThreads - 1) / kCiThreads), dim3(kCiThreads), 0, ctx->stream, entries, nchunks, part,
                       h->sums);
    LSA_CHECK(ci_check_launch(ctx, "ci_residual_kernel"));
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(ctx->pinned, h->sums, (size_t)entries * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    LSA_CHECK(ct_sync(ctx));
    memcpy(out, ctx->pinned, (size_t)entries * sizeof(double));
    return LSA_OK;
}

// Out[:, 0:k] = V[:, 0:m] T for a host matrix T (m x k, dense); the stream is drained first: the pinned staging area is the context's
int ct_times_host(lsa_ctx* ctx, lsa_contour* h, int m, int k, const cplx* V, const ci_z* T, cplx* Out) {
    LSA_CHECK(ct_sync(ctx));
    return basis_times_host_matrix(ctx, LSA_C128, h->n, m, k, V, T, m, h->qdev, Out, 0);
}

// The two phases share every step; `adj` picks the operators.  Right phase: A, M, C_k.  Left phase: their conjugate transposes -- the
// pencil (A^H, M^H), whose node matrices on the conjugate contour are C_k^H = A^H - conj(z_k) M^H: the same factor sets, the
// transposed sweeps and the transposed block product.
int ct_mul(lsa_ctx* ctx, bool adj, const lsa_mat* A, int32_t cols, const cplx* X, int64_t n, cplx* Y) {
    return adj ? k_spmm_transpose(ctx, A, 1, cols, X, n, Y, n) : k_spmm(ctx, A, cols, X, n, Y, n);
}
int ct_solve_dev(lsa_ctx* ctx, bool adj, lsa_ndlu* f, int32_t cols, const cplx* B, int64_t n, cplx* X) {
    const void* b = B;
    void* x = X;
    const NdSolve rq = {1, &f, false, adj ? 2 : 0, LSA_C128, cols, &b, n, &x, n, adj ? "lsa_contour_solve_left" : "lsa_contour_solve"};
    return ndlu_solve_run(ctx, rq);
}

// the accepted columns of a node's block solve into the counters (s: the three sums per column of ct_column_sums)
void ct_book_columns(lsa_contour* h, int32_t cols, const double* s, bool refined, double* worst) {
    for (int32_t j = 0; j < cols; ++j) {
        const double res = std::sqrt(s[3 * (size_t)j]), bnorm = std::sqrt(s[3 * (size_t)j + 1]);
        if (res > h->ksp_rtol * bnorm) ++h->st.backward_accepted;
        stats_book_direct_solve(&h->st, 1, refined, res, bnorm);
        if (bnorm > 0.0) *worst = std::max(*worst, res / bnorm);
    }
}

// X = C_k^-1 B for cols columns, every column judged by the rule of lsa_lanczos_extend: within ksp_rtol, else one refinement step (and
// every later block solve of this node carries it), else a backward error within 1e-12 ||C_k||_F ||x||, else LSA_ERR_DIVERGED
int ct_block_solve(lsa_ctx* ctx, lsa_contour* h, bool adj, int32_t k, int32_t cols, double* worst) {
    const int64_t n = h->n;
    lsa_ndlu* f = nullptr;
    LSA_CHECK(shifted_sets_factors(ctx, h->S, "lsa_contour", k, &f));
    const lsa_mat* C = h->S->C[(size_t)k];
    char& refine = h->S->refine[adj ? 1 : 0][(size_t)k];
    const char* who = adj ? "lsa_contour_solve_left: the adjoint solve" : "lsa_contour_solve: the solve";
    const double t0 = now_s();
    std::vector<double> s((size_t)3 * cols);
    bool refined = false;
    int rc = ct_solve_dev(ctx, adj, f, cols, h->B, n, h->X);
    while (rc == LSA_OK) {
        if (refine && !refined) {
            // R = B - C X;  D = C^-1 R;  X += D
            rc = ct_mul(ctx, adj, C, cols, h->X, n, h->W1);
            if (rc == LSA_OK) rc = ct_accumulate(ctx, n, cols, ci_z(1.0, 0.0), h->B, -1.0, h->W1);
            if (rc == LSA_OK) rc = ct_solve_dev(ctx, adj, f, cols, h->W1, n, h->W1);
            if (rc == LSA_OK) rc = ct_accumulate(ctx, n, cols, ci_z(1.0, 0.0), h->W1, 1.0, h->X);
            if (rc != LSA_OK) break;
            refined = true;
        }
        rc = ct_mul(ctx, adj, C, cols, h->X, n, h->W1);
        if (rc == LSA_OK) rc = ct_column_sums(ctx, h, cols, h->B, h->W1, h->X, nullptr, s.data());
        if (rc != LSA_OK) break;
        bool again = false;
        for (int32_t j = 0; j < cols && rc == LSA_OK; ++j) {
            const double res = std::sqrt(s[3 * (size_t)j]), bnorm = std::sqrt(s[3 * (size_t)j + 1]), xnorm = std::sqrt(s[3 * (size_t)j + 2]);
            bool backward = false;
            const int verdict = shifted_sets_verdict(h->S, k, h->ksp_rtol, refined, res, bnorm, xnorm, &backward);
            if (verdict > 0) {
                again = true;
                break;
            }
            if (verdict < 0)
                rc = refined ? lsa_set_error(ctx, LSA_ERR_DIVERGED, "%s of column %d at node %d left a relative residual of %.3e "
                                                                    "after its refinement step (ksp_rtol %.1e) and a backward error above 1e-12 ||C||_F", who, j, k,
                                             bnorm > 0.0 ? res / bnorm : res, h->ksp_rtol)
                             : lsa_set_error(ctx, LSA_ERR_DIVERGED, "%s of column %d at node %d left a residual that is not finite "
                                                                    "(%.3e, ||b|| = %.3e); no refinement step was taken", who, j, k, res, bnorm);
        }
        if (rc != LSA_OK) break;
        if (again) {
            refine = 1;
            continue;
        }
        ct_book_columns(h, cols, s.data(), refined, worst);
        break;
    }
    h->sec_solve += now_s() - t0;
    if (h->batch_nodes) h->serial_columns += cols;
    return rc;
}

// lsa_contour_set_batch_nodes: X_k = C_k^-1 B for every node that does not carry the refinement step, into the nodes' own blocks
// -- run by run (shifted_sets_next_run), each run one block solve on all its sets from the shared B.  solved[k] = 1: X_k is there,
// with the bits ct_block_solve's first solve gives.
int ct_batch_solve(lsa_ctx* ctx, lsa_contour* h, bool adj, int32_t cols, std::vector<char>& solved) {
    const int64_t n = h->n;
    const double t0 = now_s();
    int rc = LSA_OK;
    shifted_run run;
    for (int32_t k = 0; k < h->N && rc == LSA_OK;) {
        k = shifted_sets_next_run(h->S, k, h->S->refine[adj ? 1 : 0], &run);
        if (run.J == 0) break;
        const void* bs[kNdBatchMax];
        void* xs[kNdBatchMax];
        for (int32_t z = 0; z < run.J; ++z) {
            bs[z] = h->B;
            xs[z] = h->XN + (size_t)run.node[z] * (size_t)n * (size_t)h->L;
            solved[(size_t)run.node[z]] = 1;
        }
        const NdSolve rq = {run.J, run.f, true, adj ? 2 : 0, LSA_C128, cols, bs, n, xs, n, adj ? "lsa_contour_solve_left" : "lsa_contour_solve"};
        NdSolveInfo ran;
        rc = ndlu_solve_run(ctx, rq, &ran);
        h->batch_groups += ran.passes;
        h->batch_columns += (int64_t)run.J * cols;
    }
    h->sec_solve += now_s() - t0;
    return rc;
}

// the check of a node's batched block: the product and the column sums of ct_block_solve on X_k.  *ok = 0: a column misses ksp_rtol
// (or is not finite) -- nothing is booked, and ct_block_solve takes the node; else the columns are booked as its unrefined solves are.
int ct_batch_check(lsa_ctx* ctx, lsa_contour* h, bool adj, int32_t k, int32_t cols, const cplx* Xk, double* worst, bool* ok) {
    const int64_t n = h->n;
    const double t0 = now_s();
    std::vector<double> s((size_t)3 * cols);
    int rc = ct_mul(ctx, adj, h->S->C[(size_t)k], cols, Xk, n, h->W1);
    if (rc == LSA_OK) rc = ct_column_sums(ctx, h, cols, h->B, h->W1, Xk, nullptr, s.data());
    *ok = rc == LSA_OK;
    for (int32_t j = 0; j < cols && *ok; ++j)
        if (!(std::sqrt(s[3 * (size_t)j]) <= h->ksp_rtol * std::sqrt(s[3 * (size_t)j + 1]))) *ok = false;
    if (*ok) ct_book_columns(h, cols, s.data(), false, worst);
    h->sec_solve += now_s() - t0;
    return rc;
}

// Hermitian eigen-decomposition of the m x m host matrix G through the complex Schur form (diagonal for a Hermitian matrix):
// eigenvalues descending in val, their eigenvectors in the columns of vec
int ct_herm_eig(lsa_ctx* ctx, int32_t m, std::vector<ci_z>& G, std::vector<double>& val, std::vector<ci_z>& vec) {
    for (const ci_z& g : G)
        if (!std::isfinite(g.real()) || !std::isfinite(g.imag())) return lsa_set_error(ctx, LSA_ERR_NONFINITE, "lsa_contour_solve: a Gram matrix is not finite");
    for (int32_t j = 0; j < m; ++j)  // exactly Hermitian: the mean of the two triangles
        for (int32_t i = 0; i <= j; ++i) {
            const ci_z a = 0.5 * (G[(size_t)j * m + i] + std::conj(G[(size_t)i * m + j]));
            G[(size_t)j * m + i] = i == j ? ci_z(a.real(), 0.0) : a;
            G[(size_t)i * m + j] = i == j ? ci_z(a.real(), 0.0) : std::conj(a);
        }
    std::vector<ci_z> Qs((size_t)m * m);
    if (lsa_dense_schur(m, G.data(), m, Qs.data(), m) != LSA_OK) return lsa_set_error(ctx, LSA_ERR_DIVERGED, "lsa_contour_solve: the QR algorithm stalled on a Gram matrix");
    std::vector<int32_t> order((size_t)m);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return G[(size_t)a * m + a].real() > G[(size_t)b * m + b].real(); });
    val.resize((size_t)m);
    vec.resize((size_t)m * m);
    for (int32_t c = 0; c < m; ++c) {
        val[(size_t)c] = G[(size_t)order[(size_t)c] * m + order[(size_t)c]].real();
        std::copy(Qs.begin() + (size_t)order[(size_t)c] * m, Qs.begin() + (size_t)(order[(size_t)c] + 1) * m, vec.begin() + (size_t)c * m);
    }
    return LSA_OK;
}

// out = in W Lambda^-1/2 over the eigenpairs of in^H in with eigenvalue >= 1e-14 max (the Gram matrix squares the singular values:
// nothing below a relative 1e-7 is trusted); *rank: the columns kept
int ct_orth_pass(lsa_ctx* ctx, lsa_contour* h, const cplx* in, int32_t cols, cplx* out, int32_t* rank) {
    std::vector<ci_z> G((size_t)cols * cols), vec;
    std::vector<double> val;
    double t0 = now_s();
    LSA_CHECK(k_block_gram(ctx, h->n, cols, in, h->n, cols, in, h->n, G.data()));
    h->sec_gram += now_s() - t0;
    t0 = now_s();
    LSA_CHECK(ct_herm_eig(ctx, cols, G, val, vec));
    if (!(val[0] > 0.0)) return lsa_set_error(ctx, LSA_ERR_NONFINITE, "lsa_contour_solve: the block has no direction left (largest Gram eigenvalue %.3e)", val[0]);
    int32_t r = 0;
    while (r < cols && val[(size_t)r] >= 1e-14 * val[0]) ++r;
    std::vector<ci_z> T((size_t)cols * r);
    for (int32_t c = 0; c < r; ++c) {
        const double sc = 1.0 / std::sqrt(val[(size_t)c]);
        for (int32_t i = 0; i < cols; ++i) T[(size_t)c * cols + i] = sc * vec[(size_t)c * cols + i];
    }
    h->sec_dense += now_s() - t0;
    t0 = now_s();
    LSA_CHECK(ct_times_host(ctx, h, cols, r, in, T.data(), out));
    h->sec_gram += now_s() - t0;
    *rank = r;
    return LSA_OK;
}

// the normalised radius of lambda: < 1 inside the ellipse
double ct_radius2(const lsa_contour* h, ci_z lam) {
    const double a = (lam.real() - h->centre[0]) / h->radii[0], b = (lam.imag() - h->centre[1]) / h->radii[1];
    return a * a + b * b;
}

}  // namespace

extern "C" {

int lsa_contour_create(lsa_ctx* ctx, const lsa_mat* A, const lsa_mat* M, int32_t nodes, const double centre[2], const double radii[2], int32_t subspace,
                       int keep_factors, double ksp_rtol, lsa_contour** out) {
    if (!ctx || !A || !out || !centre || !radii) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_create: null argument");
    *out = nullptr;
    if (ctx->nranks != 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_create: the context is one of %d ranks: one rank only", ctx->nranks);
    if (A->n != A->ncols || A->row0 != 0) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_create: A is a row shard: whole square matrices only");
    if (!M) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_create: M is missing: the contour integral is that of the pencil (A, M)");
    if (M->dtype != LSA_F64) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_create: M is complex: a real M only");
    if (M->n != A->n || M->ncols != A->ncols || M->nnz != A->nnz) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_create: A and M do not share one pattern");
    if (nodes < 4 || nodes % 2 != 0) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_create: nodes = %d: an even number of at least 4", nodes);
    if (subspace < 2 || subspace > kCiMaxCols || (int64_t)subspace > A->n)
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_create: subspace = %d: between 2 and min(%d, n = %d)", subspace, kCiMaxCols, A->n);
    if (!(radii[0] > 0.0) || !(radii[1] > 0.0) || !std::isfinite(radii[0]) || !std::isfinite(radii[1]) || !std::isfinite(centre[0]) || !std::isfinite(centre[1]))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_create: radii (%.3e, %.3e): finite and positive, with a finite centre", radii[0], radii[1]);
    if (!(ksp_rtol > 0.0)) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_create: ksp_rtol = %.3e must be positive", ksp_rtol);
    lsa_contour* h = new lsa_contour();
    h->ctx = ctx;
    h->n = A->n;
    h->N = nodes;
    h->L = subspace;
    h->keep = keep_factors != 0;
    h->ksp_rtol = ksp_rtol;
    for (int q = 0; q < 2; ++q) {
        h->centre[q] = centre[q];
        h->radii[q] = radii[q];
    }
    std::vector<ci_z> z;
    const double pi = 3.14159265358979323846;
    for (int32_t k = 0; k < nodes; ++k) {
        const double th = 2.0 * pi * (k + 0.5) / nodes;
        z.push_back(ci_z(centre[0] + radii[0] * std::cos(th), centre[1] + radii[1] * std::sin(th)));
        h->w.push_back(ci_z(radii[1] * std::cos(th) / nodes, radii[0] * std::sin(th) / nodes));
    }
    const size_t blk = (size_t)h->n * sizeof(cplx) * (size_t)subspace, LL = (size_t)subspace * subspace * sizeof(cplx);
    bool ok = true;
    for (cplx** p : {&h->Y, &h->B, &h->X, &h->Q, &h->W1, &h->W2}) ok = ok && hipMalloc((void**)p, blk) == hipSuccess;
    ok = ok && hipMalloc((void**)&h->qdev, LL) == hipSuccess && hipMalloc((void**)&h->lamdev, (size_t)subspace * sizeof(cplx)) == hipSuccess &&
         hipMalloc((void**)&h->sums, (size_t)3 * subspace * sizeof(double)) == hipSuccess && hipMalloc((void**)&h->imag2, (size_t)subspace * sizeof(double)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        ct_free(h);
        return lsa_set_error(ctx, LSA_ERR_OOM, "lsa_contour_create: out of device memory (n=%d, subspace=%d)", A->n, subspace);
    }
    h->bytes = (int64_t)(6 * blk + LL) + (int64_t)nodes * A->nnz * (int64_t)sizeof(cplx);
    const int rc = shifted_sets_create(ctx, "lsa_contour_create", A, M, z, h->keep ? (size_t)nodes : 1, 0.0, &h->S);
    if (rc != LSA_OK) {
        ct_free(h);
        return rc;
    }
    h->st.analysis_reused = h->S->analysis_reused;
    h->st.seconds_factor = h->S->seconds_factor;
    *out = h;
    return LSA_OK;
}

void lsa_contour_destroy(lsa_contour* h) {
    if (!h) return;
    if (h->ctx && h->ctx->stream) (void)hipStreamSynchronize(h->ctx->stream);
    ct_free(h);
}

int lsa_contour_set_row_permutation(lsa_ctx* ctx, lsa_contour* h, const int32_t* perm) {
    if (!ctx || !h) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_set_row_permutation: null argument");
    return basis_upload_row_permutation(ctx, "lsa_contour_set_row_permutation", h->n, perm, &h->row_perm);
}

int lsa_contour_info(const lsa_contour* h, lsa_contour_stats* out) {
    if (!h || !out) return LSA_ERR_ARG;
    out->kept = h->keep ? 1 : 0;
    out->nodes = h->N;
    out->bytes = h->bytes;
    out->seconds_factor = h->S->seconds_factor;
    out->seconds_solve = h->sec_solve;
    out->seconds_product = h->sec_product;
    out->seconds_gram = h->sec_gram;
    out->seconds_dense = h->sec_dense;
    out->solver = h->st;
    return LSA_OK;
}

int lsa_contour_set_batch_nodes(lsa_ctx* ctx, lsa_contour* h, int on) {
    if (!ctx || !h) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_set_batch_nodes: null argument");
    if (on && !h->keep) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_set_batch_nodes: the handle was made with keep_factors = 0: solving the nodes in lockstep needs all their factor sets alive");
    const size_t need = (size_t)h->N * (size_t)h->n * (size_t)h->L * sizeof(cplx);
    if (on && !h->XN) {
        if (hipMalloc((void**)&h->XN, need) != hipSuccess) {
            (void)hipGetLastError();
            h->XN = nullptr;
            size_t free_b = 0, total_b = 0;
            (void)hipMemGetInfo(&free_b, &total_b);
            return lsa_set_error(ctx, LSA_ERR_OOM, "lsa_contour_set_batch_nodes: %d solution blocks of %lld x %d need %.0f bytes, %.0f bytes of device memory are free", h->N,
                                 (long long)h->n, h->L, (double)need, (double)free_b);
        }
        h->bytes += (int64_t)need;
    } else if (!on && h->XN) {
        LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        (void)hipFree(h->XN);
        h->XN = nullptr;
        h->bytes -= (int64_t)need;
    }
    h->batch_nodes = on != 0;
    return LSA_OK;
}

int lsa_contour_batch_info(const lsa_contour* h, lsa_contour_batch_stats* out) {
    if (!h || !out) return LSA_ERR_ARG;
    out->enabled = h->batch_nodes ? 1 : 0;
    out->pad0 = 0;
    out->groups = h->batch_groups;
    out->batched_columns = h->batch_columns;
    out->serial_columns = h->serial_columns;
    return LSA_OK;
}

}  // extern "C"

// The iteration of either phase from the start block Y0 (the steps of this file's header).  adj: the left phase -- the same steps on the
// adjoint pencil (A^H, M^H), whose eigenvalues mu are the conjugates of the pencil's and whose region is the conjugate ellipse: Ritz
// pairs (mu, s) of (U^H A^H U, U^H M^H U), residual ||A^H w - mu M^H w|| / (||A^H w|| + |mu| ||M^H w||), inside when conj(mu) lies in
// the caller's ellipse, and lam_out holds conj(mu).
static int ct_iterate(lsa_ctx* ctx, lsa_contour* h, bool adj, const char* who, double tol, int32_t max_it, const void* Y0_host, int32_t max_out, void* lam_out,
                      void* X_out, double* res_out, lsa_contour_result* result) {
    const int64_t n = h->n;
    const int32_t L = h->L;
    // the value in the caller's region: the Ritz value itself, or for the left phase the conjugate of the adjoint pencil's mu
    auto region_value = [adj](ci_z v) { return adj ? std::conj(v) : v; };
    *result = lsa_contour_result{};
    const int64_t solves0 = h->st.op_applies, refined0 = h->st.refined_solves, backward0 = h->st.backward_accepted;
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(h->Y, Y0_host, (size_t)n * L * sizeof(cplx), hipMemcpyHostToDevice, ctx->stream));
    LSA_CHECK(ct_sync(ctx));
    int32_t cols = L, r = 0, inside = 0, conv = 0;
    bool stopped = false;
    double worst = 0.0;
    std::vector<ci_z> lam, S;
    std::vector<double> res;
    std::vector<int32_t> in_idx;
    int32_t it = 0;
    for (; it < max_it; ++it) {
        // B = M Y, then the quadrature over the nodes: Q = -sum_k w_k C_k^-1 B (left phase: B = M^H Y, Q = -sum_k conj(w_k) C_k^-H B: the
        // adjoint pencil's nodes conj(z_k) run through the conjugate contour at the angles -theta_k, where its weights are conj(w_k))
        double t0 = now_s();
        LSA_CHECK(ct_mul(ctx, adj, h->S->M, cols, h->Y, n, h->B));
        h->st.spmv_calls += cols;
        h->sec_product += now_s() - t0;
        std::vector<char> solved((size_t)h->N, 0);
        if (h->batch_nodes) LSA_CHECK(ct_batch_solve(ctx, h, adj, cols, solved));
        for (int32_t k = 0; k < h->N; ++k) {
            const cplx* Xk = h->X;
            bool ok = false;
            if (solved[(size_t)k]) {
                Xk = h->XN + (size_t)k * (size_t)n * (size_t)L;
                LSA_CHECK(ct_batch_check(ctx, h, adj, k, cols, Xk, &worst, &ok));
            }
            if (!ok) {  // the default path; after a batched solve that missed: the same solve again, then its refinement step
                LSA_CHECK(ct_block_solve(ctx, h, adj, k, cols, &worst));
                Xk = h->X;
            }
            LSA_CHECK(ct_accumulate(ctx, n, cols, adj ? -std::conj(h->w[(size_t)k]) : -h->w[(size_t)k], Xk, k == 0 ? 0.0 : 1.0, h->Q));
        }
        if (it == 0) {  // the stochastic estimate of the count inside: Re sum_j y_j^H q_j / L
            std::vector<ci_z> G((size_t)cols * cols);
            t0 = now_s();
            LSA_CHECK(k_block_gram(ctx, n, cols, h->Y, n, cols, h->Q, n, G.data()));
            h->sec_gram += now_s() - t0;
            double tr = 0.0;
            for (int32_t j = 0; j < cols; ++j) tr += G[(size_t)j * cols + j].real();
            result->estimate = tr / cols;
        }
        // U = orth(Q), twice through the Gram matrix: Q -> X -> Y
        int32_t r1 = 0;
        LSA_CHECK(ct_orth_pass(ctx, h, h->Q, cols, h->X, &r1));
        LSA_CHECK(ct_orth_pass(ctx, h, h->X, r1, h->Y, &r));
        // A U, M U and the projected pencil
        t0 = now_s();
        LSA_CHECK(ct_mul(ctx, adj, h->S->A, r, h->Y, n, h->W1));
        LSA_CHECK(ct_mul(ctx, adj, h->S->M, r, h->Y, n, h->W2));
        h->st.spmv_calls += 2 * r;
        LSA_CHECK(ct_sync(ctx));
        h->sec_product += now_s() - t0;
        std::vector<ci_z> Ah((size_t)r * r), Mh((size_t)r * r);
        t0 = now_s();
        LSA_CHECK(k_block_gram(ctx, n, r, h->Y, n, r, h->W1, n, Ah.data()));
        LSA_CHECK(k_block_gram(ctx, n, r, h->Y, n, r, h->W2, n, Mh.data()));
        h->sec_gram += now_s() - t0;
        t0 = now_s();
        if (!dense_lu_solve(r, Mh.data(), Ah.data())) return lsa_set_error(ctx, LSA_ERR_ZERO_PIVOT, "%s: U^H M U is singular at iteration %d (rank %d)", who, it, r);
        std::vector<ci_z> Qs((size_t)r * r), St((size_t)r * r);
        if (lsa_dense_schur(r, Ah.data(), r, Qs.data(), r) != LSA_OK) return lsa_set_error(ctx, LSA_ERR_DIVERGED, "%s: the QR algorithm stalled on the projected problem", who);
        LSA_CHECK(lsa_dense_tri_eigenvectors(r, Ah.data(), r, St.data(), r));
        lam.assign((size_t)r, ci_z());
        S.assign((size_t)r * r, ci_z());
        for (int32_t j = 0; j < r; ++j) {
            lam[(size_t)j] = Ah[(size_t)j * r + j];
            for (int32_t k = 0; k <= j; ++k)  // (the eigenvectors of a triangular matrix are triangular)
                for (int32_t i = 0; i < r; ++i) S[(size_t)j * r + i] += Qs[(size_t)k * r + i] * St[(size_t)j * r + k];
        }
        for (const ci_z& l : lam)
            if (!std::isfinite(l.real()) || !std::isfinite(l.imag())) return lsa_set_error(ctx, LSA_ERR_NONFINITE, "%s: a Ritz value is not finite at iteration %d", who, it);
        h->sec_dense += now_s() - t0;
        // residuals ||A x - lam M x|| / (||A x|| + |lam| ||M x||) of all Ritz pairs from A U S and M U S
        t0 = now_s();
        LSA_CHECK(ct_times_host(ctx, h, r, r, h->W1, S.data(), h->X));
        LSA_CHECK(ct_times_host(ctx, h, r, r, h->W2, S.data(), h->B));
        LSA_HIP_CHECK(ctx, hipMemcpyAsync(h->lamdev, lam.data(), (size_t)r * sizeof(cplx), hipMemcpyHostToDevice, ctx->stream));
        LSA_CHECK(ct_sync(ctx));
        std::vector<double> s((size_t)3 * r);
        LSA_CHECK(ct_column_sums(ctx, h, r, h->X, h->B, h->B, h->lamdev, s.data()));
        h->sec_product += now_s() - t0;
        res.assign((size_t)r, 0.0);
        in_idx.clear();
        conv = 0;
        for (int32_t j = 0; j < r; ++j) {
            res[(size_t)j] = std::sqrt(s[3 * (size_t)j]) / (std::sqrt(s[3 * (size_t)j + 1]) + std::abs(lam[(size_t)j]) * std::sqrt(s[3 * (size_t)j + 2]) + 1e-16);
            if (ct_radius2(h, region_value(lam[(size_t)j])) < 1.0) {
                in_idx.push_back(j);
                if (res[(size_t)j] <= tol) ++conv;
            }
        }
        inside = (int32_t)in_idx.size();
        cols = r;
        // (an iteration that shows NO Ritz value inside proves little on its own: a large cluster just outside the contour can fill
        //  the block in the first quadrature; an empty region is declared only when a second iteration shows none either)
        if (conv == inside && (inside > 0 || it > 0)) {
            stopped = true;
            ++it;
            break;
        }
    }
    result->iterations = it;
    result->rank = r;
    result->inside = inside;
    result->converged_inside = conv;
    result->complete = stopped && inside < r ? 1 : 0;
    result->block_solves = h->st.op_applies - solves0;
    result->refined_solves = h->st.refined_solves - refined0;
    result->backward_accepted = h->st.backward_accepted - backward0;
    result->worst_rel_res = worst;
    // the inside pairs, nearest the centre (in the ellipse's own metric) first
    std::stable_sort(in_idx.begin(), in_idx.end(), [&](int32_t a, int32_t b) { return ct_radius2(h, region_value(lam[(size_t)a])) < ct_radius2(h, region_value(lam[(size_t)b])); });
    const int32_t nout = std::min<int32_t>(inside, max_out);
    result->nout = nout;
    for (int32_t c = 0; c < nout; ++c) {
        ((ci_z*)lam_out)[c] = region_value(lam[(size_t)in_idx[(size_t)c]]);
        res_out[c] = res[(size_t)in_idx[(size_t)c]];
    }
    if (nout > 0 && X_out) {
        std::vector<ci_z> Sel((size_t)r * nout);
        for (int32_t c = 0; c < nout; ++c) std::copy(S.begin() + (size_t)in_idx[(size_t)c] * r, S.begin() + (size_t)(in_idx[(size_t)c] + 1) * r, Sel.begin() + (size_t)c * r);
        LSA_CHECK(ct_times_host(ctx, h, r, nout, h->Y, Sel.data(), h->Q));
        LSA_CHECK(k_columns_canonical(ctx, n, nout, h->Q, n, 1, h->imag2));
        const cplx* src = h->Q;
        if (h->row_perm) {
            LSA_CHECK(k_scatter_rows(ctx, LSA_C128, n, nout, h->row_perm, h->Q, h->W1));
            src = h->W1;
        }
        LSA_HIP_CHECK(ctx, hipMemcpyAsync(X_out, src, (size_t)n * nout * sizeof(cplx), hipMemcpyDeviceToHost, ctx->stream));
        LSA_CHECK(ct_sync(ctx));
    }
    h->st.seconds_solve = h->sec_solve;
    return LSA_OK;
}

extern "C" {

int lsa_contour_solve(lsa_ctx* ctx, lsa_contour* h, double tol, int32_t max_it, const void* Y0_host, int32_t max_out, void* lam_out, void* X_out,
                      double* res_out, lsa_contour_result* result) {
    if (!ctx || !h || !Y0_host || !result) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_solve: null argument");
    if (!(tol > 0.0) || max_it < 1 || max_out < 0 || (max_out > 0 && (!lam_out || !res_out)))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_solve: bad argument (tol %.3e, max_it %d, max_out %d)", tol, max_it, max_out);
    return ct_iterate(ctx, h, false, "lsa_contour_solve", tol, max_it, Y0_host, max_out, lam_out, X_out, res_out, result);
}

// The left phase on the same handle and factor sets.  Its counters and times are booked apart: the handle's own books (lsa_contour_info,
// lsa_contour_batch_info) are put back as they were, the differences go to lsa_contour_left_info.
int lsa_contour_solve_left(lsa_ctx* ctx, lsa_contour* h, double tol, int32_t max_it, const void* Y0_host, int32_t max_out, void* lam_out, void* W_out,
                           double* res_out, lsa_contour_result* result) {
    if (!ctx || !h || !Y0_host || !result) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_solve_left: null argument");
    if (!(tol > 0.0) || max_it < 1 || max_out < 0 || (max_out > 0 && (!lam_out || !res_out)))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_contour_solve_left: bad argument (tol %.3e, max_it %d, max_out %d)", tol, max_it, max_out);
    const lsa_stats st0 = h->st;
    const double sec0[5] = {h->sec_solve, h->sec_product, h->sec_gram, h->sec_dense, h->S->seconds_factor};
    const int64_t b0[3] = {h->batch_groups, h->batch_columns, h->serial_columns};
    const int rc = ct_iterate(ctx, h, true, "lsa_contour_solve_left", tol, max_it, Y0_host, max_out, lam_out, W_out, res_out, result);
    lsa_contour_left_stats& l = h->left;
    l.solves += 1;
    l.iterations += result->iterations;
    l.block_solves += h->st.op_applies - st0.op_applies;
    l.refined_solves += h->st.refined_solves - st0.refined_solves;
    l.backward_accepted += h->st.backward_accepted - st0.backward_accepted;
    l.groups += h->batch_groups - b0[0];
    l.batched_columns += h->batch_columns - b0[1];
    l.serial_columns += h->serial_columns - b0[2];
    l.seconds_solve += h->sec_solve - sec0[0];
    l.seconds_product += h->sec_product - sec0[1];
    l.seconds_gram += h->sec_gram - sec0[2];
    l.seconds_dense += h->sec_dense - sec0[3];
    l.seconds_factor += h->S->seconds_factor - sec0[4];
    h->st = st0;
    h->sec_solve = sec0[0], h->sec_product = sec0[1], h->sec_gram = sec0[2], h->sec_dense = sec0[3];
    h->batch_groups = b0[0], h->batch_columns = b0[1], h->serial_columns = b0[2];
    return rc;
}

int lsa_contour_left_info(const lsa_contour* h, lsa_contour_left_stats* out) {
    if (!h || !out) return LSA_ERR_ARG;
    *out = h->left;
    return LSA_OK;
}

}  // extern "C"
