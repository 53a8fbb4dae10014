// The trace of the quadrature operator of stochastic forcing (stochastic.hip) by block probes, on the handle's kept factor family:
// tr S is the sum of ALL variances, the total the leading ones are a share of.  For a real probe z with E[z z^T] = I, z^T S z is
// unbiased for tr S, and with two solves of one direction
//     z^T S  z = (1 / pi) sum_k w_k Re[(C_k^-H z)^H Q_f (C_k^-H Q_q z)]        kind 0: adjoint solves only
//     z^T S' z = (1 / pi) sum_k w_k Re[(C_k^-1 z)^H Q_q (C_k^-1 Q_f z)]        kind 1: forward solves only
// (z^T C^-1 Q_f C^-H Q_q z = (C^-H z)^H Q_f (C^-H Q_q z)): a probe is two independent columns, z and Q z with Q the kind's inner
// weight, shared by all nodes, through one direction's block sweeps.  With modes U of the kind, Q-orthonormal, S U = U Theta, the
// second column is Q p, p = z - U (U^T Q z), and E[z^T S p] = tr(S (I - U U^T Q)) = tr S - sum_j theta_j.
//
// One batch of R probes (B is n x 2R, X, ZC, T are n x 2R per node, node after node):
//     B[:, 0:R] = Z                             st_probe_kernel (generated) or st_gather_kernel (the caller's, through the row permutation)
//     W = Q Z;  G = U^T W;  P = Z - U G         k_spmm, st_gram_kernel + st_finish_kernel, st_deflate_kernel     (ndeflate > 0)
//     B[:, R:2R] = Q P                          k_spmm (no deflation: Q Z)
//     X_k = C_k^-H B (kind 1: C_k^-1 B)         ndlu_solve_run: one request of 2R columns per run of <= 16 compatible sets, all sets
//                                               reading the one B; a node that carries the refinement step alone, with
//                                               X_k += C_k^-H (B - C_k^H X_k) behind it
//     ZC[:, c] = C_c^H X[:, c] for all 2RN c    k_shifted_spmm_transpose (kind 1: k_shifted_spmm), ONE launch, a shift per column
//     T = Q_mid X                               one k_spmm over the whole block
//     log[7 (k R + r) + 0..6]                   st_forms_kernel + st_finish_kernel: Re(y^H t), then |b - Cx|^2, |b|^2, |x|^2 of
//                                               the column of z (y = X_k[:, r]) and of the column of Q p (x = X_k[:, R + r], t = T_k[:, R + r])
// and one read-back behind one synchronisation.  Every solve is judged by shifted_sets_verdict as sf_judge judges a step's.
//
// The probes: with mix(x) the output function of splitmix64,
//     x += 0x9E3779B97F4A7C15;  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;  x = (x ^ (x >> 27)) * 0x94D049BB133111EB;  return x ^ (x >> 31)
// (64-bit unsigned, wrapping), Z[i, p] = +1 where the top bit of mix(mix(mix(seed) + p) + i) is 0, else -1, with i the CALLER's row:
// the handle's row permutation maps the device row to it, so neither the permutation, nor the batch width, nor the probes that share a
// launch change an entry.
//
// Every sum runs in a fixed order and there are no floating-point atomics: two runs give the same bits, and so does every batch width
// (each column of a block solve holds its solo sweep's bits; the products and the sums treat every column alone).
//   st_gram_kernel, st_forms_kernel   the rows of a chunk (dot_chunks) strided over the 256 threads, the xor tree of the wavefront, the
//                                     four waves in wave order; the finish kernels add the chunks strided over 64 lanes and the same
//                                     tree (sf_sums_kernel / sf_sums_finish_kernel's order)
//   st_deflate_kernel                 a thread per entry, the modes ascending
#include <algorithm>
#include <cmath>
#include <string>

#include "stochastic_internal.h"

namespace {

constexpr int kStThreads = 256;    // four wavefronts of 64
constexpr int kStSums = 7;         // doubles of the log per (node, probe)
constexpr int kStMaxDeflate = 128;
constexpr int kStMaxBatch = 64;
constexpr int kStEvents = 5;

__device__ __forceinline__ double st_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__host__ __device__ inline uint64_t st_mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// Probes p0 .. p0 + R - 1 (column blockIdx.y), rows strided over the grid: device row i is the caller's row perm[i] (null: i).
// Z (null: none): the complex block in the device's numbering, imaginary part 0; out (null: none): the real block in the caller's.
__global__ __launch_bounds__(kStThreads) void st_probe_kernel(int64_t n, int32_t p0, uint64_t seed, const int32_t* __restrict__ perm, cplx* __restrict__ Z,
                                                              double* __restrict__ out) {
    const int c = blockIdx.y;
    const uint64_t key = st_mix(st_mix(seed) + (uint64_t)(p0 + c));
    const int64_t stride = (int64_t)gridDim.x * kStThreads;
    for (int64_t i = (int64_t)blockIdx.x * kStThreads + threadIdx.x; i < n; i += stride) {
        const int64_t row = perm ? perm[i] : i;
        const double s = (st_mix(key + (uint64_t)row) >> 63) ? -1.0 : 1.0;
        if (Z) rz_st(Z + (int64_t)c * n + i, cplx{s, 0.0});
        if (out) out[(int64_t)c * n + row] = s;
    }
}

// Column blockIdx.y of a real block in the caller's numbering into the device's: Zc (complex, imaginary part 0) or Zr (real)
__global__ __launch_bounds__(kStThreads) void st_gather_kernel(int64_t n, const int32_t* __restrict__ perm, const double* __restrict__ src, cplx* __restrict__ Zc,
                                                               double* __restrict__ Zr) {
    const int64_t col = (int64_t)blockIdx.y * n;
    const int64_t stride = (int64_t)gridDim.x * kStThreads;
    for (int64_t i = (int64_t)blockIdx.x * kStThreads + threadIdx.x; i < n; i += stride) {
        const double v = src[col + (perm ? perm[i] : i)];
        if (Zc) rz_st(Zc + col + i, cplx{v, 0.0});
        if (Zr) Zr[col + i] = v;
    }
}

// Uc = U + 0 i on a block of n x d entries
__global__ __launch_bounds__(kStThreads) void st_widen_kernel(int64_t count, const double* __restrict__ U, cplx* __restrict__ Uc) {
    const int64_t stride = (int64_t)gridDim.x * kStThreads;
    for (int64_t i = (int64_t)blockIdx.x * kStThreads + threadIdx.x; i < count; i += stride) rz_st(Uc + i, cplx{U[i], 0.0});
}

// out = alpha a + beta b on count complex entries (out may be a or b): the two updates of a block refinement step
__global__ __launch_bounds__(kStThreads) void st_axpby_kernel(int64_t count, double alpha, const cplx* a, double beta, const cplx* b, cplx* out) {
    const int64_t stride = (int64_t)gridDim.x * kStThreads;
    for (int64_t i = (int64_t)blockIdx.x * kStThreads + threadIdx.x; i < count; i += stride) {
        const cplx av = rz_ld(a + i), bv = rz_ld(b + i);
        rz_st(out + i, cplx{fma(alpha, av.re, beta * bv.re), fma(alpha, av.im, beta * bv.im)});
    }
}

// part[(c d + j) nchunks + chunk] = sum over the rows of the chunk of U[i, j] Re W[i, c]: workgroup (chunk, c d + j)
__global__ __launch_bounds__(kStThreads) void st_gram_kernel(int64_t n, int d, int64_t rows_per_chunk, int nchunks, const double* __restrict__ U,
                                                             const cplx* __restrict__ W, double* __restrict__ part) {
    __shared__ double ws[4];
    const int chunk = blockIdx.x, e = blockIdx.y;
    const double* u = U + (int64_t)(e % d) * n;
    const cplx* w = W + (int64_t)(e / d) * n;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r0 = (int64_t)chunk * rows_per_chunk;
    const int64_t r1 = (r0 + rows_per_chunk < n) ? r0 + rows_per_chunk : n;
    double s = 0.0;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += kStThreads) s = fma(u[i], rz_ld(w + i).re, s);
    s = st_wave_sum(s);
    if (lane == 0) ws[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(int64_t)e * nchunks + chunk] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

// Wave q of workgroup g finishes entry e = 4 g + q < entries into out[e]: lane k adds the chunks k, k + 64, ... in that order, then the
// tree.  Serves the Gram matrices (entries = d x columns) and the forms (entries = 7 per pair).
__global__ __launch_bounds__(kStThreads) void st_finish_kernel(int entries, int nchunks, const double* __restrict__ part, double* __restrict__ out) {
    const int e = 4 * blockIdx.x + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e >= entries) return;  // (a whole wavefront leaves: the shuffles below stay among the lanes of one entry)
    const double* p = part + (int64_t)e * nchunks;
    double a = 0.0;
    for (int k = lane; k < nchunks; k += 64) a += p[k];
    a = st_wave_sum(a);
    if (lane == 0) out[e] = a;
}

// P[:, c] = Z[:, c] - U G[:, c] (G d x R column-major, real; Z, P complex with imaginary part 0), the modes ascending; column blockIdx.y
__global__ __launch_bounds__(kStThreads) void st_deflate_kernel(int64_t n, int d, const double* __restrict__ U, const double* __restrict__ G,
                                                                const cplx* __restrict__ Z, cplx* __restrict__ P) {
    const int c = blockIdx.y;
    const double* g = G + (int64_t)c * d;
    const int64_t stride = (int64_t)gridDim.x * kStThreads;
    for (int64_t i = (int64_t)blockIdx.x * kStThreads + threadIdx.x; i < n; i += stride) {
        double acc = rz_ld(Z + (int64_t)c * n + i).re;
        for (int j = 0; j < d; ++j) acc = fma(-U[(int64_t)j * n + i], g[j], acc);
        rz_st(P + (int64_t)c * n + i, cplx{acc, 0.0});
    }
}

// The sums of pair s = k R + r (node k, probe r of the batch) over the rows of one chunk: workgroup (chunk, s) writes
// part[(7 s + q) nchunks + chunk], q = 0: Re(y^H t); 1..3: |b - c|^2, |b|^2, |x|^2 of the column of z (b = B[:, r], solution y =
// X_k[:, r], check product ZC_k[:, r]); 4..6: the same of the column of Q p (B[:, R + r], x = X_k[:, R + r], ZC_k[:, R + r]), and
// t = T_k[:, R + r].  Every entry is one 16-byte load.
__global__ __launch_bounds__(kStThreads) void st_forms_kernel(int64_t n, int R, int64_t rows_per_chunk, int nchunks, const cplx* __restrict__ B,
                                                              const cplx* __restrict__ X, const cplx* __restrict__ ZC, const cplx* __restrict__ T,
                                                              double* __restrict__ part) {
    __shared__ double ws[4][kStSums];
    const int chunk = blockIdx.x, s = blockIdx.y;
    const int k = s / R, r = s - k * R;
    const int64_t cy = ((int64_t)k * 2 * R + r) * n, cx = cy + (int64_t)R * n;
    const cplx *by = B + (int64_t)r * n, *bx = B + (int64_t)(R + r) * n;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r0 = (int64_t)chunk * rows_per_chunk;
    const int64_t r1 = (r0 + rows_per_chunk < n) ? r0 + rows_per_chunk : n;
    double a[kStSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = r0 + threadIdx.x; i < r1; i += kStThreads) {
        const cplx yv = rz_ld(X + cy + i), xv = rz_ld(X + cx + i), tv = rz_ld(T + cx + i);
        const cplx b1 = rz_ld(by + i), b2 = rz_ld(bx + i);
        const cplx d1 = s_sub(b1, rz_ld(ZC + cy + i)), d2 = s_sub(b2, rz_ld(ZC + cx + i));
        a[0] = fma(yv.im, tv.im, fma(yv.re, tv.re, a[0]));
        a[1] = fma(d1.im, d1.im, fma(d1.re, d1.re, a[1]));
        a[2] = fma(b1.im, b1.im, fma(b1.re, b1.re, a[2]));
        a[3] = fma(yv.im, yv.im, fma(yv.re, yv.re, a[3]));
        a[4] = fma(d2.im, d2.im, fma(d2.re, d2.re, a[4]));
        a[5] = fma(b2.im, b2.im, fma(b2.re, b2.re, a[5]));
        a[6] = fma(xv.im, xv.im, fma(xv.re, xv.re, a[6]));
    }
#pragma unroll
    for (int q = 0; q < kStSums; ++q) {
        const double v = st_wave_sum(a[q]);
        if (lane == 0) ws[wave][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < kStSums) {
        const int q = threadIdx.x;
        part[((int64_t)kStSums * s + q) * nchunks + chunk] = ((ws[0][q] + ws[1][q]) + ws[2][q]) + ws[3][q];
    }
}

int st_grid(lsa_ctx* ctx, int64_t n, int per_cu) {
    return (int)std::max<int64_t>(std::min<int64_t>((n + kStThreads - 1) / kStThreads, (int64_t)ctx->num_cu * per_cu), 1);
}

// what a call holds on the device and the host beside the handle; released when the call returns, however it does
struct StWork {
    cplx *B = nullptr, *X = nullptr, *ZC = nullptr, *T = nullptr, *W = nullptr, *P = nullptr, *zcol = nullptr;
    double *U = nullptr, *stage = nullptr, *G = nullptr, *part = nullptr, *log = nullptr, *hlog = nullptr;
    hipEvent_t ev[kStEvents] = {};
    int32_t zcol_R = 0;  // the batch width zcol is laid out for
    ~StWork() {
        for (void* p : {(void*)B, (void*)X, (void*)ZC, (void*)T, (void*)W, (void*)P, (void*)zcol, (void*)U, (void*)stage, (void*)G, (void*)part, (void*)log})
            if (p) (void)hipFree(p);
        if (hlog) (void)hipHostFree(hlog);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// G (d x cols, column-major, on the device) = U^T Re W in the fixed order of the two kernels
int st_gram(lsa_ctx* ctx, int64_t n, int d, int cols, const double* U, const cplx* W, double* part, double* G) {
    int64_t rows_per_chunk;
    const int nchunks = dot_chunks(n, &rows_per_chunk);
    const int entries = d * cols;
    hipLaunchKernelGGL(st_gram_kernel, dim3(nchunks, entries), dim3(kStThreads), 0, ctx->stream, n, d, rows_per_chunk, nchunks, U, W, part);
    hipLaunchKernelGGL(st_finish_kernel, dim3((entries + 3) / 4), dim3(kStThreads), 0, ctx->stream, entries, nchunks, part, G);
    return lsa_check_launch(ctx, "st_gram_kernel");
}

// X_k = op(C_k)^-1 B for all nodes and the 2R columns of B: run by run through the batched sweeps, a node that carries the refinement
// step alone with X_k += op(C_k)^-1 (B - op(C_k) X_k) behind its solve (ZC_k and T_k are its product and its residual: both are
// written anew afterwards)
int st_solve_all(lsa_ctx* ctx, lsa_stochastic* h, StWork& w, bool adjoint, int32_t R, const std::vector<char>& ref, lsa_stochastic_trace_stats* st) {
    const int64_t n = h->n;
    const int32_t cols = 2 * R;
    const size_t blk = (size_t)n * (size_t)cols;
    const int trans = adjoint ? 2 : 0;
    shifted_run run;
    for (int32_t k = 0; k < h->N;) {
        k = shifted_sets_next_run(h->S, k, ref, &run);
        if (run.J == 0) break;
        const void* bs[kNdBatchMax];
        void* xs[kNdBatchMax];
        for (int32_t z = 0; z < run.J; ++z) {
            bs[z] = w.B;
            xs[z] = w.X + (size_t)run.node[z] * blk;
        }
        const NdSolve rq = {run.J, run.f, true, trans, LSA_C128, cols, bs, n, xs, n, "lsa_stochastic_trace"};
        NdSolveInfo ran;
        LSA_CHECK(ndlu_solve_run(ctx, rq, &ran));
        if (run.J > 1) ++st->grouped_sweeps;
        st->widest_pass = std::max(st->widest_pass, ran.width);
    }
    const int grid = st_grid(ctx, (int64_t)blk, 8);
    for (int32_t k = 0; k < h->N; ++k) {
        if (!ref[(size_t)k]) continue;
        lsa_ndlu* f = h->S->F[(size_t)k];
        const lsa_mat* C = h->S->C[(size_t)k];
        cplx *x = w.X + (size_t)k * blk, *prod = w.ZC + (size_t)k * blk, *res = w.T + (size_t)k * blk;
        const void* bs = w.B;
        void* xs = x;
        const NdSolve first = {1, &f, false, trans, LSA_C128, cols, &bs, n, &xs, n, "lsa_stochastic_trace"};
        NdSolveInfo ran;
        LSA_CHECK(ndlu_solve_run(ctx, first, &ran));
        st->widest_pass = std::max(st->widest_pass, ran.width);
        LSA_CHECK(adjoint ? k_spmm_transpose(ctx, C, 1, cols, x, n, prod, n) : k_spmm(ctx, C, cols, x, n, prod, n));
        hipLaunchKernelGGL(st_axpby_kernel, dim3(grid), dim3(kStThreads), 0, ctx->stream, (int64_t)blk, 1.0, w.B, -1.0, prod, res);
        LSA_CHECK(lsa_check_launch(ctx, "st_axpby_kernel"));
        const void* rs = res;
        void* ds = res;
        const NdSolve second = {1, &f, false, trans, LSA_C128, cols, &rs, n, &ds, n, "lsa_stochastic_trace"};
        LSA_CHECK(ndlu_solve_run(ctx, second));
        hipLaunchKernelGGL(st_axpby_kernel, dim3(grid), dim3(kStThreads), 0, ctx->stream, (int64_t)blk, 1.0, x, 1.0, res, x);
        LSA_CHECK(lsa_check_launch(ctx, "st_axpby_kernel"));
    }
    return LSA_OK;
}

// the shift of every column of the node-after-node blocks of width 2R, on the device (made anew when the width changes)
int st_column_shifts(lsa_ctx* ctx, lsa_stochastic* h, StWork& w, int32_t R) {
    if (w.zcol_R == R) return LSA_OK;
    std::vector<sf_z> zc((size_t)2 * R * h->N);
    for (int32_t k = 0; k < h->N; ++k) std::fill(zc.begin() + (size_t)k * 2 * R, zc.begin() + (size_t)(k + 1) * 2 * R, h->S->z[(size_t)k]);
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (nothing queued reads the old layout any more)
    LSA_HIP_CHECK(ctx, hipMemcpy(w.zcol, zc.data(), zc.size() * sizeof(cplx), hipMemcpyHostToDevice));
    w.zcol_R = R;
    return LSA_OK;
}

int st_checked_args(lsa_ctx* ctx, const lsa_stochastic* h, int32_t nprobes, int32_t ndeflate, const double* U, int32_t batch) {
    if (nprobes < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_trace: nprobes = %d: at least one probe", nprobes);
    if (ndeflate < 0) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_trace: ndeflate = %d is negative", ndeflate);
    if (ndeflate > kStMaxDeflate || ndeflate > h->n)
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_trace: ndeflate = %d: at most %d modes (and no more than the problem size %lld)", ndeflate, kStMaxDeflate,
                             (long long)h->n);
    if (ndeflate > 0 && !U) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_trace: ndeflate = %d but U is NULL", ndeflate);
    if (batch < 0) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_trace: batch = %d is negative (0: chosen)", batch);
    return LSA_OK;
}

}  // namespace

extern "C" {

int lsa_stochastic_probes(lsa_ctx* ctx, lsa_stochastic* h, int32_t nprobes, uint64_t seed, double* Z_host) {
    if (!ctx || !h || !Z_host) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_probes: null argument");
    if (nprobes < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_probes: nprobes = %d: at least one probe", nprobes);
    const int64_t n = h->n;
    const size_t bytes = (size_t)n * sizeof(double);
    const int32_t width = std::min<int32_t>(nprobes, kStMaxBatch);
    StWork w;
    LSA_HIP_ALLOC(ctx, hipMalloc((void**)&w.stage, bytes * (size_t)width));
    for (int32_t p0 = 0; p0 < nprobes; p0 += width) {
        const int32_t R = std::min<int32_t>(width, nprobes - p0);
        hipLaunchKernelGGL(st_probe_kernel, dim3(st_grid(ctx, n, 8), R), dim3(kStThreads), 0, ctx->stream, n, p0, seed, lanczos_row_permutation(h->lz), (cplx*)nullptr,
                           w.stage);
        LSA_CHECK(lsa_check_launch(ctx, "st_probe_kernel"));
        LSA_HIP_CHECK(ctx, hipMemcpyAsync(Z_host + (size_t)p0 * (size_t)n, w.stage, bytes * (size_t)R, hipMemcpyDeviceToHost, ctx->stream));
        LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return LSA_OK;
}

int lsa_stochastic_trace(lsa_ctx* ctx, lsa_stochastic* h, int32_t nprobes, uint64_t seed, const double* probes, int32_t ndeflate, const double* U, int32_t batch,
                         double* forms, double* node_terms, lsa_stochastic_trace_stats* stats) {
    if (!ctx || !h || !forms) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_trace: null argument");
    LSA_CHECK(st_checked_args(ctx, h, nprobes, ndeflate, U, batch));
    lsa_stochastic_trace_stats st{};
    const int64_t n = h->n;
    const int32_t N = h->N, d = ndeflate;
    const bool adjoint = h->kind == 0;
    const int dir = adjoint ? 1 : 0;
    const lsa_mat *Q = sf_inner(h), *Qmid = sf_middle(h);
    const int32_t* perm = lanczos_row_permutation(h->lz);
    const size_t vb = (size_t)std::max<int64_t>(n, 1) * sizeof(cplx);
    int64_t rows_per_chunk;
    const int nchunks = dot_chunks(n, &rows_per_chunk);

    // the batch width: as given, or 8 and halved until the blocks fit 0.8 of the free memory
    int32_t Rb = std::min<int32_t>(std::min<int32_t>(batch > 0 ? batch : 8, nprobes), kStMaxBatch);
    auto need = [&](int32_t R) {
        const double cols = 2.0 * R;
        return (double)vb * (cols + 3.0 * cols * N + (d > 0 ? 2.0 * R + 2.0 * d : 0.0)) + (double)(vb / 2) * ((probes ? R : 0) + 2.0 * d);
    };
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        while (batch == 0 && Rb > 1 && need(Rb) > 0.8 * (double)free_b) Rb = (Rb + 1) / 2;
        if (need(Rb) > 0.8 * (double)free_b)
            return lsa_set_error(ctx, LSA_ERR_OOM, "lsa_stochastic_trace: a batch of %d probe%s on %d nodes needs %.0f bytes, 0.8 of the %.0f bytes of free device "
                                                   "memory hold %.0f", Rb, Rb == 1 ? "" : "s", N, need(Rb), (double)free_b, 0.8 * (double)free_b);
    } else {
        (void)hipGetLastError();
    }
    st.batch = Rb;
    st.bytes = (int64_t)need(Rb);

    StWork w;
    const size_t blk = vb * (size_t)2 * (size_t)Rb;
    const size_t gram_entries = (size_t)std::max(d, 1) * (size_t)std::max<int32_t>(Rb, d);
    const size_t part_entries = std::max<size_t>((size_t)kStSums * (size_t)N * (size_t)Rb, gram_entries) * (size_t)nchunks;
    bool ok = hipMalloc((void**)&w.B, blk) == hipSuccess;
    for (cplx** p : {&w.X, &w.ZC, &w.T}) ok = ok && hipMalloc((void**)p, blk * (size_t)N) == hipSuccess;
    ok = ok && hipMalloc((void**)&w.zcol, (size_t)2 * Rb * N * sizeof(cplx)) == hipSuccess && hipMalloc((void**)&w.part, part_entries * sizeof(double)) == hipSuccess &&
         hipMalloc((void**)&w.log, (size_t)kStSums * N * Rb * sizeof(double)) == hipSuccess &&
         hipHostMalloc((void**)&w.hlog, std::max((size_t)kStSums * N * Rb, gram_entries) * sizeof(double)) == hipSuccess;
    if (probes) ok = ok && hipMalloc((void**)&w.stage, (vb / 2) * (size_t)std::max<int32_t>(Rb, d)) == hipSuccess;
    if (d > 0) {
        // W and P serve the check of U first (n x d each), then the deflation of a batch (n x Rb each)
        const size_t wide = vb * (size_t)std::max<int32_t>(Rb, d);
        ok = ok && hipMalloc((void**)&w.W, wide) == hipSuccess && hipMalloc((void**)&w.P, wide) == hipSuccess && hipMalloc((void**)&w.U, (vb / 2) * (size_t)d) == hipSuccess &&
             hipMalloc((void**)&w.G, gram_entries * sizeof(double)) == hipSuccess;
        if (!w.stage) ok = ok && hipMalloc((void**)&w.stage, (vb / 2) * (size_t)d) == hipSuccess;
    }
    for (hipEvent_t& e : w.ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        return lsa_set_error(ctx, LSA_ERR_OOM, "lsa_stochastic_trace: out of device memory (n=%lld, nodes=%d, batch=%d)", (long long)n, N, Rb);
    }

    if (d > 0) {
        // U once per call, into the device's numbering; its Gram matrix in the kind's weight before any solve
        LSA_HIP_CHECK(ctx, hipMemcpyAsync(w.stage, U, (vb / 2) * (size_t)d, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(st_gather_kernel, dim3(st_grid(ctx, n, 8), d), dim3(kStThreads), 0, ctx->stream, n, perm, w.stage, (cplx*)nullptr, w.U);
        hipLaunchKernelGGL(st_widen_kernel, dim3(st_grid(ctx, n * d, 8)), dim3(kStThreads), 0, ctx->stream, n * d, w.U, w.P);
        LSA_CHECK(lsa_check_launch(ctx, "st_gather_kernel"));
        LSA_CHECK(k_spmm(ctx, Q, d, w.P, n, w.W, n));
        LSA_CHECK(st_gram(ctx, n, d, d, w.U, w.W, w.part, w.G));
        LSA_HIP_CHECK(ctx, hipMemcpyAsync(w.hlog, w.G, (size_t)d * d * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        for (int32_t c = 0; c < d; ++c)
            for (int32_t j = 0; j < d; ++j) {
                const double g = w.hlog[(size_t)c * d + j], off = std::fabs(g - (j == c ? 1.0 : 0.0));
                if (!(off <= 1e-6))
                    return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_trace: U is not orthonormal in the kind's weight: (U^T Q U)[%d, %d] = %.9g, further from "
                                                           "the identity than 1e-6", j, c, g);
            }
    }

    for (int32_t p0 = 0; p0 < nprobes; p0 += Rb) {
        const int32_t R = std::min<int32_t>(Rb, nprobes - p0);
        const int32_t cols = 2 * R;
        LSA_CHECK(st_column_shifts(ctx, h, w, R));
        while (true) {
            std::vector<char> used = h->S->refine[dir];
            if (h->force_refine) used.assign((size_t)N, 1);
            ++st.batches;
            LSA_HIP_CHECK(ctx, hipEventRecord(w.ev[0], ctx->stream));
            if (probes) {
                LSA_HIP_CHECK(ctx, hipMemcpyAsync(w.stage, probes + (size_t)p0 * (size_t)n, (vb / 2) * (size_t)R, hipMemcpyHostToDevice, ctx->stream));
                hipLaunchKernelGGL(st_gather_kernel, dim3(st_grid(ctx, n, 8), R), dim3(kStThreads), 0, ctx->stream, n, perm, w.stage, w.B, (double*)nullptr);
            } else {
                hipLaunchKernelGGL(st_probe_kernel, dim3(st_grid(ctx, n, 8), R), dim3(kStThreads), 0, ctx->stream, n, p0, seed, perm, w.B, (double*)nullptr);
            }
            LSA_CHECK(lsa_check_launch(ctx, "the probes of lsa_stochastic_trace"));
            cplx* second = w.B + (size_t)R * (size_t)n;
            if (d > 0) {
                LSA_CHECK(k_spmm(ctx, Q, R, w.B, n, w.W, n));
                LSA_CHECK(st_gram(ctx, n, d, R, w.U, w.W, w.part, w.G));
                hipLaunchKernelGGL(st_deflate_kernel, dim3(st_grid(ctx, n, 8), R), dim3(kStThreads), 0, ctx->stream, n, d, w.U, w.G, w.B, w.P);
                LSA_CHECK(lsa_check_launch(ctx, "st_deflate_kernel"));
                LSA_CHECK(k_spmm(ctx, Q, R, w.P, n, second, n));
            } else {
                LSA_CHECK(k_spmm(ctx, Q, R, w.B, n, second, n));
            }
            LSA_HIP_CHECK(ctx, hipEventRecord(w.ev[1], ctx->stream));
            LSA_CHECK(st_solve_all(ctx, h, w, adjoint, R, used, &st));
            LSA_HIP_CHECK(ctx, hipEventRecord(w.ev[2], ctx->stream));
            LSA_CHECK(adjoint ? k_shifted_spmm_transpose(ctx, h->S->A, h->S->M, cols * N, w.zcol, w.X, w.ZC) : k_shifted_spmm(ctx, h->S->A, h->S->M, cols * N, w.zcol, w.X, w.ZC));
            LSA_CHECK(k_spmm(ctx, Qmid, cols * N, w.X, n, w.T, n));
            LSA_HIP_CHECK(ctx, hipEventRecord(w.ev[3], ctx->stream));
            hipLaunchKernelGGL(st_forms_kernel, dim3(nchunks, N * R), dim3(kStThreads), 0, ctx->stream, n, R, rows_per_chunk, nchunks, w.B, w.X, w.ZC, w.T, w.part);
            hipLaunchKernelGGL(st_finish_kernel, dim3((kStSums * N * R + 3) / 4), dim3(kStThreads), 0, ctx->stream, kStSums * N * R, nchunks, w.part, w.log);
            LSA_CHECK(lsa_check_launch(ctx, "st_forms_kernel"));
            LSA_HIP_CHECK(ctx, hipEventRecord(w.ev[4], ctx->stream));
            LSA_HIP_CHECK(ctx, hipMemcpyAsync(w.hlog, w.log, (size_t)kStSums * N * R * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            float ms[kStEvents - 1] = {};
            for (int e = 0; e + 1 < kStEvents; ++e)
                if (hipEventElapsedTime(&ms[e], w.ev[e], w.ev[e + 1]) != hipSuccess) ms[e] = 0.0f;
            (void)hipGetLastError();
            st.seconds_product += 1e-3 * (ms[0] + ms[2]);
            st.seconds_solve += 1e-3 * ms[1];
            st.seconds_forms += 1e-3 * ms[3];

            // the verdict on the 2 N R solves, as sf_judge's on a step's
            bool again = false;
            for (int32_t k = 0; k < N; ++k)
                for (int32_t r = 0; r < R; ++r)
                    for (int col = 0; col < 2; ++col) {
                        const double* e = w.hlog + (size_t)kStSums * ((size_t)k * R + r) + 1 + 3 * col;
                        const bool refine = used[(size_t)k] != 0;
                        const double res = std::sqrt(e[0]), bnorm = std::sqrt(e[1]);
                        bool backward = false;
                        const int v = shifted_sets_verdict(h->S, k, h->ksp_rtol, refine, res, bnorm, std::sqrt(e[2]), &backward);
                        if (v < 0)
                            return lsa_set_error(ctx, LSA_ERR_DIVERGED, "lsa_stochastic_trace: the %s solve of node %d (z = %.6g%+.6gi) for the %s column of probe %d left a "
                                                                        "relative residual of %.3e%s (ksp_rtol %.1e)%s", adjoint ? "adjoint" : "forward", k,
                                                 h->S->z[(size_t)k].real(), h->S->z[(size_t)k].imag(), col == 0 ? "first" : "second", p0 + r, bnorm > 0.0 ? res / bnorm : res,
                                                 refine ? " after its refinement step" : ", which is not finite", h->ksp_rtol,
                                                 refine ? " and a backward error above 1e-12 ||C||_F" : "");
                        if (v > 0) {
                            h->S->refine[dir][(size_t)k] = 1;
                            again = true;
                        }
                    }
            if (again) continue;
            for (int32_t k = 0; k < N; ++k) {
                (adjoint ? st.solves_adjoint : st.solves_forward) += cols;
                if (used[(size_t)k]) st.refined_solves += cols;
            }
            for (int32_t r = 0; r < R; ++r) {
                double sum = 0.0;
                for (int32_t k = 0; k < N; ++k) {
                    const double term = h->c[(size_t)k] * w.hlog[(size_t)kStSums * ((size_t)k * R + r)];
                    if (node_terms) node_terms[(size_t)k * (size_t)nprobes + (size_t)(p0 + r)] = term;
                    sum += term;
                }
                forms[p0 + r] = sum;
            }
            break;
        }
    }
    if (stats) *stats = st;
    return LSA_OK;
}

}  // extern "C"
