// Response to stochastic forcing of M q' = A q + f: under forcing that is white in time with spatial weight Q_f the response covariance
// of a stable pair is P = (1 / 2 pi) int R Q_f R^H d omega, R(z) = (z M - A)^-1, and the structures that carry the variance (EOFs,
// measured in Q_q) are the eigenvectors of P Q_q = (1 / 2 pi) int W(i omega) d omega with W(z) = C^-1 Q_f C^-H Q_q, C = A - z M: the
// operator a resolvent step applies (resolvent.hip).  For real A, M, W(conj z) = conj W(z), so the integral over the whole axis is
//     S = (1 / pi) sum_k w_k Re W(z_k)          over a quadrature z_k = beta + i omega_k, omega_k >= 0, w_k > 0,
// a REAL operator, self-adjoint and non-negative in the Q_q-semi-inner product.  So the real thick-restart Lanczos iteration of
// lanczos.hip serves as it is -- basis, reorthogonalisation, tail, restart and Ritz vectors are an lsa_lanczos this handle owns --
// with S as the operator behind a step (lanczos_operator), on N factor sets of C_k kept alive on one ordering and one analysis
// (shifted_sets.hip: the family lsa_contour_create keeps too).  The stochastic optimals (kind 1) are the eigenvectors of
// S' = (1 / pi) sum_k w_k Re(C_k^-H Q_q C_k^-1 Q_f) in the Q_f-inner product: the same step with the two solves and the two weights
// swapped.  The results are those of the quadrature operator; whether N nodes resolve the integral is the caller's to check.
//
// One step j of kind 0 (rhs = Q_q v_j is left by the previous step's tail):
//     b = rhs + 0 i                             sf_widen_kernel: one complex right-hand side for all nodes
//     for every node k:  z_k = C_k^-H b         the transposed, conjugated sweeps (ndlu_solve_run), node by node, or the
//                                               batched ones in groups of <= 16 sets (set_batch_adjoint)
//                        ca_k = C_k^H z_k       k_spmv_transpose, for the check (set_batch_adjoint: k_spmv_transpose_batch, 16 per launch)
//     TM = Q_f [z_0 .. z_{N-1}]                 one k_spmm on the block
//     for every node k:  w_k = C_k^-1 tm_k      the forward sweeps, or the batched ones in groups of <= 16 sets (set_batch_forward)
//     CF[:, k] = C_k w_k for all k              sf_shifted_spmm_kernel: ONE launch, A's and M's values read once for <= 16 columns
//     log[4 s + 0..3], s < 2N                   sf_sums_kernel + sf_sums_finish_kernel: |b - z|^2, |b|^2, |x|^2 of all 2N solves and
//                                               Re(rhs^H w_k) of the second ones, one launch pair
//     w = (1 / pi) sum_k w_k Re w_k             sf_accumulate_kernel, k ascending
// The log travels to the host behind the step's one synchronisation (the hook's read_back); every solve is judged by
// direct_solve_verdict with its node's ||C_k||_F: within ksp_rtol, else that node and direction carry a refinement step from then on
// and the step is done again, else the backward-error bound, else LSA_ERR_DIVERGED naming node and direction.  The kernels of
// lanczos.hip stay as they are: the real basis' one check slot gets the pair (rhs, rhs), which cannot fail.
//
// Every sum runs in a fixed order and there are no floating-point atomics: two runs give the same bits, and so do the batched and
// the node-by-node solves of either direction (each column of lsa_ndlu_solve_batch holds lsa_ndlu_solve's bits, each of
// lsa_ndlu_solve_batch_adjoint lsa_ndlu_solve_adjoint's, each of k_spmv_transpose_batch k_spmv_transpose's).
//   sf_shifted_spmm_kernel   shifted_sets.hip
//   sf_sums_kernel          the rows of a chunk (dot_chunks) strided over the 256 threads, the xor tree of the wavefront, the four
//                            waves in wave order; sf_sums_finish_kernel adds the chunks strided over 64 lanes and the same tree
//                            (tg_march_kernel / tg_log_kernel's order)
#include <algorithm>
#include <cmath>
#include <complex>

#include "stochastic_internal.h"

namespace {

constexpr int kSfThreads = 256;   // four wavefronts of 64

__device__ __forceinline__ double sf_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The sums of all 2N solves of a step over the rows of one chunk: workgroup (chunk, s) writes part[(4 s + q) nchunks + chunk],
// q = 0..3: |b - z|^2, |b|^2, |x|^2 and, for a second solve (s >= N), Re(rhs^H x).  Solve s < N is node s's first one: right-hand
// side rhs (shared by all nodes), solution X1[:, s], check product Z1[:, s]; solve N + k is node k's second one: TM[:, k], X2[:, k],
// Z2[:, k].  Every entry is one 16-byte load.
__global__ __launch_bounds__(kSfThreads) void sf_sums_kernel(int64_t n, int N, int64_t rows_per_chunk, int nchunks, const cplx* __restrict__ rhs,
                                                             const cplx* __restrict__ X1, const cplx* __restrict__ Z1, const cplx* __restrict__ TM,
                                                             const cplx* __restrict__ X2, const cplx* __restrict__ Z2, double* __restrict__ part) {
    __shared__ double ws[4][4];
    const int chunk = blockIdx.x, s = blockIdx.y;
    const bool second = s >= N;
    const int64_t col = (int64_t)(second ? s - N : s) * n;
    const cplx *b = second ? TM + col : rhs, *x = (second ? X2 : X1) + col, *z = (second ? Z2 : Z1) + col;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r0 = (int64_t)chunk * rows_per_chunk;
    const int64_t r1 = (r0 + rows_per_chunk < n) ? r0 + rows_per_chunk : n;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += kSfThreads) {
        const cplx bv = rz_ld(b + i), zv = rz_ld(z + i), xv = rz_ld(x + i);
        const cplx d = s_sub(bv, zv);
        s0 = fma(d.im, d.im, fma(d.re, d.re, s0));
        s1 = fma(bv.im, bv.im, fma(bv.re, bv.re, s1));
        s2 = fma(xv.im, xv.im, fma(xv.re, xv.re, s2));
        if (second) {
            const cplx rv = rz_ld(rhs + i);
            s3 = fma(rv.im, xv.im, fma(rv.re, xv.re, s3));
        }
    }
    s0 = sf_wave_sum(s0);
    s1 = sf_wave_sum(s1);
    s2 = sf_wave_sum(s2);
    s3 = sf_wave_sum(s3);
    if (lane == 0) {
        ws[wave][0] = s0;
        ws[wave][1] = s1;
        ws[wave][2] = s2;
        ws[wave][3] = s3;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int q = threadIdx.x;
        part[((int64_t)4 * s + q) * nchunks + chunk] = ((ws[0][q] + ws[1][q]) + ws[2][q]) + ws[3][q];
    }
}

// Workgroup s: wave q finishes sum q of solve s into log[4 s + q] (lane k adds the chunks k, k + 64, ... in that order, then the tree)
__global__ __launch_bounds__(kSfThreads) void sf_sums_finish_kernel(int nchunks, const double* __restrict__ part, double* __restrict__ log) {
    const int s = blockIdx.x, q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double* p = part + ((int64_t)4 * s + q) * nchunks;
    double a = 0.0;
    for (int k = lane; k < nchunks; k += 64) a += p[k];
    a = sf_wave_sum(a);
    if (lane == 0) log[4 * s + q] = a;
}

// y[i] = sum_k c[k] Re W[i, k], k ascending (c[k] = w_k / pi): N complex columns in, one real vector out; a thread per row, the rows
// of a workgroup strided over the grid, up to eight columns of the row requested at a time
__global__ __launch_bounds__(kSfThreads) void sf_accumulate_kernel(int64_t n, int N, const double* __restrict__ c, const cplx* __restrict__ W,
                                                                   double* __restrict__ y) {
    const int64_t stride = (int64_t)gridDim.x * kSfThreads;
    for (int64_t i = (int64_t)blockIdx.x * kSfThreads + threadIdx.x; i < n; i += stride) {
        double acc = 0.0;
        for (int k0 = 0; k0 < N; k0 += 8) {
            cplx v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = (k0 + u < N) ? rz_ld(W + i + (int64_t)(k0 + u) * n) : cplx{0.0, 0.0};
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (k0 + u < N) acc = fma(c[k0 + u], v[u].re, acc);
        }
        y[i] = acc;
    }
}

// b = x + 0 i: the complex right-hand side all nodes share, from the real Q v
__global__ __launch_bounds__(kSfThreads) void sf_widen_kernel(int64_t n, const double* __restrict__ x, cplx* __restrict__ b) {
    const int64_t stride = (int64_t)gridDim.x * kSfThreads;
    for (int64_t i = (int64_t)blockIdx.x * kSfThreads + threadIdx.x; i < n; i += stride) rz_st(b + i, cplx{x[i], 0.0});
}

int sf_grid(lsa_ctx* ctx, int64_t n, int per_cu) {
    return (int)std::max<int64_t>(std::min<int64_t>((n + kSfThreads - 1) / kSfThreads, (int64_t)ctx->num_cu * per_cu), 1);
}

}  // namespace

namespace {

void sf_free(lsa_stochastic* h) {
    if (h->lz) lsa_lanczos_destroy(h->lz);
    shifted_sets_free(h->S);
    for (void* p : {(void*)h->cdev, (void*)h->b, (void*)h->X1, (void*)h->Z1, (void*)h->TM, (void*)h->X2, (void*)h->Z2, (void*)h->r, (void*)h->d,
                    (void*)h->part, (void*)h->log, (void*)h->rnorms, (void*)h->vdev, (void*)h->rhsdev, (void*)h->ydev})
        if (p) (void)hipFree(p);
    if (h->hlog) (void)hipHostFree(h->hlog);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    delete h;
}

// x_z = C_z^-1 b_z (adjoint: C_z^-H b_z) on J factor sets: one set is the solo instance of the sweeps, a longer run the batch
int sf_request(lsa_ctx* ctx, int32_t J, lsa_ndlu* const* f, bool adjoint, const void* const* b, void* const* x) {
    const NdSolve rq = {J, f, J > 1, adjoint ? 2 : 0, LSA_C128, 1, b, 0, x, 0, "lsa_stochastic"};
    return ndlu_solve_run(ctx, rq);
}

int sf_sweeps(lsa_ctx* ctx, lsa_stochastic* h, int32_t k, bool adjoint, const cplx* b, cplx* x) {
    const void* bs = b;
    void* xs = x;
    return sf_request(ctx, 1, &h->S->F[(size_t)k], adjoint, &bs, &xs);
}

int sf_times_c(lsa_ctx* ctx, lsa_stochastic* h, int32_t k, bool adjoint, const cplx* x, cplx* y) {
    return adjoint ? k_spmv_transpose(ctx, h->S->C[(size_t)k], 1, LSA_C128, x, y) : k_spmv(ctx, h->S->C[(size_t)k], LSA_C128, x, y);
}

// X[:, k] = C_k^-1 B_k (adjoint: C_k^-H) for all nodes, B_k = B + k ldb (ldb = 0: one right-hand side for all).  Under the
// direction's switch (set_batch_forward, set_batch_adjoint) the solves go through the batched sweeps of that direction in groups
// of at most kNdBatchMax compatible sets; a node whose solves carry the refinement step runs alone and takes
// x += C^-1 (b - C x) behind its solve.
int sf_solve_all(lsa_ctx* ctx, lsa_stochastic* h, bool adjoint, const cplx* B, int64_t ldb, cplx* X) {
    const int64_t n = h->n;
    const std::vector<char>& ref = h->used[adjoint ? 1 : 0];
    std::vector<char> done((size_t)h->N, 0);
    if (adjoint ? h->batch_adjoint : h->batch_forward) {
        shifted_run run;
        for (int32_t k = 0; k < h->N;) {
            k = shifted_sets_next_run(h->S, k, ref, &run);
            if (run.J == 0) break;
            const void* bs[kNdBatchMax];
            void* xs[kNdBatchMax];
            for (int32_t z = 0; z < run.J; ++z) {
                bs[z] = B + (size_t)run.node[z] * (size_t)ldb;
                xs[z] = X + (size_t)run.node[z] * (size_t)n;
                done[(size_t)run.node[z]] = 1;
            }
            LSA_CHECK(sf_request(ctx, run.J, run.f, adjoint, bs, xs));
            if (run.J > 1) ++(adjoint ? h->adjoint_batches : h->forward_batches);
        }
    }
    const double one[2] = {1.0, 0.0};
    for (int32_t k = 0; k < h->N; ++k) {
        const cplx* b = B + (size_t)k * (size_t)ldb;
        cplx* x = X + (size_t)k * (size_t)n;
        if (!done[(size_t)k]) LSA_CHECK(sf_sweeps(ctx, h, k, adjoint, b, x));
        if (!ref[(size_t)k]) continue;
        LSA_CHECK(sf_times_c(ctx, h, k, adjoint, x, h->d));
        LSA_CHECK(k_residual_norms(ctx, LSA_C128, n, b, h->d, h->r, h->rnorms));
        LSA_CHECK(sf_sweeps(ctx, h, k, adjoint, h->r, h->d));
        LSA_CHECK(k_axpy(ctx, LSA_C128, n, one, h->d, x));
    }
    return LSA_OK;
}

// Z[:, k] = C_k X[:, k] for all nodes in one launch, or C_k^H X[:, k] node by node -- under set_batch_adjoint in groups of
// kNdBatchMax nodes per launch (the C_k are built on A's index arrays: one transposed index serves them all)
int sf_check_products(lsa_ctx* ctx, lsa_stochastic* h, bool adjoint, const cplx* X, cplx* Z) {
    if (!adjoint) return k_shifted_spmm(ctx, h->S->A, h->S->M, h->N, h->S->zdev, X, Z);
    const size_t n = (size_t)h->n;
    if (!h->batch_adjoint) {
        for (int32_t k = 0; k < h->N; ++k) LSA_CHECK(sf_times_c(ctx, h, k, true, X + (size_t)k * n, Z + (size_t)k * n));
        return LSA_OK;
    }
    for (int32_t k0 = 0; k0 < h->N; k0 += kNdBatchMax) {
        const int32_t J = std::min<int32_t>(kNdBatchMax, h->N - k0);
        const void* xs[kNdBatchMax];
        void* zs[kNdBatchMax];
        for (int32_t z = 0; z < J; ++z) {
            xs[z] = X + (size_t)(k0 + z) * n;
            zs[z] = Z + (size_t)(k0 + z) * n;
        }
        LSA_CHECK(k_spmv_transpose_batch(ctx, J, h->S->C.data() + k0, 1, LSA_C128, xs, zs));
    }
    return LSA_OK;
}

// Queues w = S v from rhs = Q v (both real, on the device) and the log of its 2N solves; nothing is read back.
int sf_enqueue(lsa_ctx* ctx, lsa_stochastic* h, const double* rhs, double* w) {
    const int64_t n = h->n;
    const int32_t N = h->N;
    for (int dir = 0; dir < 2; ++dir) {
        h->used[dir] = h->S->refine[dir];
        if (h->force_refine) h->used[dir].assign((size_t)N, 1);
    }
    const bool first_adj = sf_adjoint(h, 0), second_adj = sf_adjoint(h, 1);
    int e = 0;
    auto mark = [&]() { return hipEventRecord(h->ev[e++], ctx->stream); };
    hipLaunchKernelGGL(sf_widen_kernel, dim3(sf_grid(ctx, n, 8)), dim3(kSfThreads), 0, ctx->stream, n, rhs, h->b);
    LSA_CHECK(lsa_check_launch(ctx, "sf_widen_kernel"));
    LSA_HIP_CHECK(ctx, mark());
    LSA_CHECK(sf_solve_all(ctx, h, first_adj, h->b, 0, h->X1));
    LSA_HIP_CHECK(ctx, mark());
    LSA_CHECK(sf_check_products(ctx, h, first_adj, h->X1, h->Z1));
    LSA_HIP_CHECK(ctx, mark());
    LSA_CHECK(k_spmm(ctx, sf_middle(h), N, h->X1, n, h->TM, n));
    h->st.spmv_calls += N;
    LSA_HIP_CHECK(ctx, mark());
    LSA_CHECK(sf_solve_all(ctx, h, second_adj, h->TM, n, h->X2));
    LSA_HIP_CHECK(ctx, mark());
    LSA_CHECK(sf_check_products(ctx, h, second_adj, h->X2, h->Z2));
    LSA_HIP_CHECK(ctx, mark());
    int64_t rows_per_chunk;
    const int nchunks = dot_chunks(n, &rows_per_chunk);
    hipLaunchKernelGGL(sf_sums_kernel, dim3(nchunks, 2 * N), dim3(kSfThreads), 0, ctx->stream, n, N, rows_per_chunk, nchunks, h->b, h->X1, h->Z1, h->TM, h->X2,
                       h->Z2, h->part);
    hipLaunchKernelGGL(sf_sums_finish_kernel, dim3(2 * N), dim3(kSfThreads), 0, ctx->stream, nchunks, h->part, h->log);
    hipLaunchKernelGGL(sf_accumulate_kernel, dim3(sf_grid(ctx, n, 4)), dim3(kSfThreads), 0, ctx->stream, n, N, h->cdev, h->X2, w);
    LSA_CHECK(lsa_check_launch(ctx, "stochastic step"));
    LSA_HIP_CHECK(ctx, mark());
    h->timed = true;
    return LSA_OK;
}

int sf_read_back(lsa_ctx* ctx, lsa_stochastic* h) {
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(h->hlog, h->log, (size_t)8 * (size_t)h->N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    return LSA_OK;
}

// After the synchronisation: the phase times of the step from its events, then the verdict on its 2N solves.  0: all accepted and
// booked; 1: a node's direction switched its refinement step on, the step is done again; -1: LSA_ERR_DIVERGED is set.
int sf_judge(lsa_ctx* ctx, lsa_stochastic* h, const char* who, const char* what, int32_t where) {
    if (h->timed) {
        float ms[kSfEvents - 1] = {};
        for (int e = 0; e + 1 < kSfEvents; ++e)
            if (hipEventElapsedTime(&ms[e], h->ev[e], h->ev[e + 1]) != hipSuccess) ms[e] = 0.0f;
        (void)hipGetLastError();
        h->sec_solve += 1e-3 * (ms[0] + ms[3]);
        h->sec_product += 1e-3 * (ms[1] + ms[2] + ms[4] + ms[5]);
        const int a = sf_adjoint(h, 0) ? 0 : 3;  // the adjoint solves are the first or the second ones; their check products follow them
        h->sec_solve_adj += 1e-3 * ms[a];
        h->sec_product_adj += 1e-3 * ms[a + 1];
        h->timed = false;
    }
    const int32_t N = h->N;
    struct One {
        bool refine, backward;
        double res, bnorm;
    };
    std::vector<One> sv((size_t)2 * N);
    int worst = 0;
    for (int32_t s = 0; s < 2 * N; ++s) {
        const int pos = s >= N ? 1 : 0;
        const int32_t k = s - pos * N;
        const bool adj = sf_adjoint(h, pos);
        const double* e = h->hlog + (size_t)4 * (size_t)s;
        One& o = sv[(size_t)s];
        o = One{h->used[adj ? 1 : 0][(size_t)k] != 0, false, std::sqrt(e[0]), std::sqrt(e[1])};
        const int v = shifted_sets_verdict(h->S, k, h->ksp_rtol, o.refine, o.res, o.bnorm, std::sqrt(e[2]), &o.backward);
        if (v < 0) {
            lsa_set_error(ctx, LSA_ERR_DIVERGED, "%s: the %s solve of node %d (z = %.6g%+.6gi) of %s %d left a relative residual of %.3e%s (ksp_rtol %.1e)%s", who,
                          adj ? "adjoint" : "forward", k, h->S->z[(size_t)k].real(), h->S->z[(size_t)k].imag(), what, where, o.bnorm > 0.0 ? o.res / o.bnorm : o.res,
                          o.refine ? " after its refinement step" : ", which is not finite", h->ksp_rtol, o.refine ? " and a backward error above 1e-12 ||C||_F" : "");
            return -1;
        }
        if (v > 0) {
            h->S->refine[adj ? 1 : 0][(size_t)k] = 1;
            worst = 1;
        }
    }
    if (worst) return worst;
    for (int32_t s = 0; s < 2 * N; ++s) {
        const One& o = sv[(size_t)s];
        const bool adj = sf_adjoint(h, s >= N ? 1 : 0);
        if (o.backward) ++h->st.backward_accepted;
        stats_book_direct_solve(&h->st, 1, o.refine, o.res, o.bnorm);
        ++(adj ? h->solves_adj : h->solves_fwd);
        if (o.refine) ++(adj ? h->refined_adj : h->refined_fwd);
    }
    return 0;
}

// ---- the operator behind a Lanczos step -------------------------------------------------------------------------------------------
int sf_hook_enqueue(lsa_ctx* ctx, void* self, int32_t, const void* rhs, void* w, void*, void*, lanczos_check* chk) {
    lsa_stochastic* h = (lsa_stochastic*)self;
    LSA_CHECK(sf_enqueue(ctx, h, (const double*)rhs, (double*)w));
    // The real step kernels sum one check pair in their first reduction, and this step has 2N complex ones, which its own log
    // carries.  The slot gets a pair that cannot fail, b = z = rhs (|b - z| = 0 <= ksp_rtol |b|): lanczos.hip stays as it is.
    chk[0].b = rhs;
    chk[0].z = rhs;
    chk[0].refined = false;
    return LSA_OK;
}

int sf_hook_read_back(lsa_ctx* ctx, void* self) { return sf_read_back(ctx, (lsa_stochastic*)self); }

int sf_hook_judge(lsa_ctx* ctx, void* self, int32_t j, const lanczos_sums*) { return sf_judge(ctx, (lsa_stochastic*)self, "lsa_stochastic_solve", "step", j); }

}  // namespace

int stochastic_shape(const lsa_stochastic* h, int64_t* n, int32_t* ncv) {
    if (!h) return LSA_ERR_ARG;
    if (n) *n = h->n;
    if (ncv) *ncv = h->ncv;
    return LSA_OK;
}

void stochastic_counts(const lsa_stochastic* h, int64_t counts[4]) {
    counts[0] = h->solves_adj;
    counts[1] = h->solves_fwd;
    counts[2] = h->refined_adj;
    counts[3] = h->refined_fwd;
}

void stochastic_book_dense(lsa_stochastic* h, double seconds) { h->sec_dense += seconds; }

int stochastic_inject(lsa_ctx* ctx, lsa_stochastic* h, int32_t j, const double* host_v) {
    if (!h) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic: null argument");
    return lanczos_inject(ctx, h->lz, j, host_v);
}

int stochastic_extend(lsa_ctx* ctx, lsa_stochastic* h, int32_t j0, int32_t j1, double* T, int32_t ldt, int32_t* breakdown) {
    if (!h || !T) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic extend: null argument");
    return lsa_lanczos_extend(ctx, h->lz, j0, j1, T, ldt, breakdown);
}

int stochastic_restart(lsa_ctx* ctx, lsa_stochastic* h, int32_t m, int32_t knew, const double* Y, int32_t ldy) {
    if (!h) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic restart: null argument");
    return lanczos_restart(ctx, h->lz, m, knew, Y, ldy);
}

int stochastic_ritz_vectors(lsa_ctx* ctx, lsa_stochastic* h, int32_t m, int32_t nvec, const double* Y, int32_t ldy, double* X) {
    if (!h) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic vectors: null argument");
    return lanczos_ritz_vectors(ctx, h->lz, m, nvec, Y, ldy, X);
}

extern "C" {

int lsa_stochastic_create(lsa_ctx* ctx, const lsa_mat* A, const lsa_mat* M, int32_t nodes, const double* shifts, const double* weights, int32_t ncv,
                          double ksp_rtol, lsa_stochastic** out) {
    if (!ctx || !A || !out || !shifts || !weights) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_create: null argument");
    *out = nullptr;
    if (ctx->nranks != 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_create: the context is one of %d ranks: one rank only", ctx->nranks);
    if (A->n != A->ncols || A->row0 != 0) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_create: A is a row shard: whole square matrices only");
    if (!M) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_create: M is missing: the variance is measured in the M-inner product");
    if (A->dtype != LSA_F64) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_create: A is complex: the quadrature over omega >= 0 stands for the whole axis only for a real pencil");
    if (M->dtype != LSA_F64) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_create: M is complex: a real symmetric M only");
    if (!sf_same_pattern(A, M)) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_create: A and M do not share one pattern");
    if (nodes < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_create: nodes = %d: a quadrature has at least one node", nodes);
    if (ncv < 1 || (int64_t)ncv > A->n) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_create: ncv = %d: between 1 and the problem size %d", ncv, A->n);
    if (!(ksp_rtol > 0.0)) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_create: ksp_rtol = %.3e must be positive", ksp_rtol);
    for (int32_t k = 0; k < nodes; ++k) {
        if (!(weights[k] > 0.0) || !std::isfinite(weights[k]))
            return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_create: weight %d is %.3e: a quadrature weight is positive and finite", k, weights[k]);
        if (!std::isfinite(shifts[2 * k]) || !std::isfinite(shifts[2 * k + 1]))
            return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_create: node %d is not finite", k);
    }
    lsa_stochastic* h = new lsa_stochastic();
    h->ctx = ctx;
    h->n = A->n;
    h->N = nodes;
    h->ncv = ncv;
    h->ksp_rtol = ksp_rtol;
    h->Qf = h->Qq = M;
    std::vector<sf_z> z;
    const double pi = 3.14159265358979323846;
    for (int32_t k = 0; k < nodes; ++k) {
        z.push_back(sf_z(shifts[2 * k], shifts[2 * k + 1]));
        h->c.push_back(weights[k] / pi);
    }
    for (int dir = 0; dir < 2; ++dir) h->used[dir].assign((size_t)nodes, 0);
    h->P.n = h->n;
    h->P.Kmul = M;
    h->P.ksp_rtol = ksp_rtol;
    h->P.one_rank = true;
    h->P.st = &h->st;
    const size_t vb = (size_t)std::max<int64_t>(h->n, 1) * sizeof(cplx), blk = vb * (size_t)nodes;
    int64_t rows_per_chunk;
    const int nchunks = dot_chunks(h->n, &rows_per_chunk);
    bool ok = true;
    for (cplx** p : {&h->b, &h->r, &h->d}) ok = ok && hipMalloc((void**)p, vb) == hipSuccess;
    for (cplx** p : {&h->X1, &h->Z1, &h->TM, &h->X2, &h->Z2}) ok = ok && hipMalloc((void**)p, blk) == hipSuccess;
    for (double** p : {&h->vdev, &h->rhsdev, &h->ydev}) ok = ok && hipMalloc((void**)p, vb / 2) == hipSuccess;
    ok = ok && hipMalloc((void**)&h->cdev, (size_t)nodes * sizeof(double)) == hipSuccess &&
         hipMalloc((void**)&h->part, (size_t)8 * (size_t)nodes * (size_t)nchunks * sizeof(double)) == hipSuccess &&
         hipMalloc((void**)&h->log, (size_t)8 * (size_t)nodes * sizeof(double)) == hipSuccess && hipMalloc((void**)&h->rnorms, 2 * sizeof(double)) == hipSuccess &&
         hipHostMalloc((void**)&h->hlog, (size_t)8 * (size_t)nodes * sizeof(double)) == hipSuccess;
    for (hipEvent_t& e : h->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    ok = ok && hipMemcpy(h->cdev, h->c.data(), (size_t)nodes * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemset(h->log, 0, (size_t)8 * (size_t)nodes * sizeof(double)) == hipSuccess;  // (a start vector's read-back copies it before any step)
    if (!ok) {
        (void)hipGetLastError();
        sf_free(h);
        return lsa_set_error(ctx, LSA_ERR_OOM, "lsa_stochastic_create: out of device memory (n=%d, nodes=%d)", A->n, nodes);
    }
    h->bytes = (int64_t)(3 * vb + 5 * blk + 3 * (vb / 2)) + (int64_t)nodes * A->nnz * (int64_t)sizeof(cplx) + (int64_t)2 * 8 * h->n * (ncv + 1);
    int rc = shifted_sets_create(ctx, "lsa_stochastic_create", A, M, z, (size_t)nodes, 0.8, &h->S);
    const double t0 = now_s();
    if (rc == LSA_OK) rc = lanczos_create_basis_on(ctx, nullptr, h->P, ncv, LSA_F64, "lsa_stochastic", &h->lz);
    if (rc == LSA_OK) {
        h->hook = lanczos_operator{h, 1, sf_hook_enqueue, sf_hook_read_back, sf_hook_judge};
        rc = lanczos_set_operator(ctx, h->lz, &h->hook);
    }
    if (rc != LSA_OK) {
        const std::string msg = ctx->err;
        sf_free(h);
        return lsa_set_error(ctx, rc, "%s", msg.c_str());
    }
    h->bytes += (int64_t)nodes * std::max<int64_t>(shifted_sets_bytes_per_set(h->S->F[0]->S), 0);
    h->st.analysis_reused = h->S->analysis_reused;
    h->S->seconds_factor += now_s() - t0;  // (this handle's figure counts its basis in)
    h->st.seconds_factor = h->S->seconds_factor;
    *out = h;
    return LSA_OK;
}

void lsa_stochastic_destroy(lsa_stochastic* h) {
    if (!h) return;
    if (h->ctx && h->ctx->stream) (void)hipStreamSynchronize(h->ctx->stream);
    sf_free(h);
}

int lsa_stochastic_set_row_permutation(lsa_ctx* ctx, lsa_stochastic* h, const int32_t* perm) {
    if (!ctx || !h) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_set_row_permutation: null argument");
    return lsa_lanczos_set_row_permutation(ctx, h->lz, perm);
}

int lsa_stochastic_set_weights(lsa_ctx* ctx, lsa_stochastic* h, const lsa_mat* Qf, const lsa_mat* Qq) {
    if (!ctx || !h) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_set_weights: null argument");
    const lsa_mat* both[2] = {Qf, Qq};
    for (int k = 0; k < 2; ++k) {
        const lsa_mat* Q = both[k];
        const char* which = k == 0 ? "forcing" : "response";
        if (!Q) continue;
        if (Q->dtype != LSA_F64)
            return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_set_weights: the %s weight is complex: a weight is real symmetric positive semidefinite", which);
        if (Q->row0 != 0 || (int64_t)Q->n != h->n || (int64_t)Q->ncols != h->n)
            return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_set_weights: the %s weight is %d x %d (from row %d), the problem has size %lld", which, Q->n,
                                 Q->ncols, Q->row0, (long long)h->n);
    }
    h->Qf = Qf ? Qf : h->S->M;
    h->Qq = Qq ? Qq : h->S->M;
    // other inner products begin as a new handle does: no right-hand side is left over (the basis forgets it), the refinement steps
    // are off again, and a start vector must follow (the basis in hand is orthonormal in the old weight)
    lanczos_set_inner_product(h->lz, sf_inner(h));
    for (int dir = 0; dir < 2; ++dir) h->S->refine[dir].assign((size_t)h->N, 0);
    return LSA_OK;
}

int lsa_stochastic_set_kind(lsa_ctx* ctx, lsa_stochastic* h, int32_t kind) {
    if (!ctx || !h) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_set_kind: null argument");
    if (kind != 0 && kind != 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_set_kind: kind = %d is neither 0 (EOFs) nor 1 (stochastic optimals)", kind);
    h->kind = kind;
    lanczos_set_inner_product(h->lz, sf_inner(h));
    for (int dir = 0; dir < 2; ++dir) h->S->refine[dir].assign((size_t)h->N, 0);
    return LSA_OK;
}

int lsa_stochastic_set_batch_forward(lsa_ctx* ctx, lsa_stochastic* h, int on) {
    if (!ctx || !h) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_set_batch_forward: null argument");
    h->batch_forward = on != 0;
    return LSA_OK;
}

int lsa_stochastic_set_batch_adjoint(lsa_ctx* ctx, lsa_stochastic* h, int on) {
    if (!ctx || !h) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_set_batch_adjoint: null argument");
    h->batch_adjoint = on != 0;
    return LSA_OK;
}

int lsa_stochastic_set_refinement(lsa_ctx* ctx, lsa_stochastic* h, int on) {
    if (!ctx || !h) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_set_refinement: null argument");
    h->force_refine = on != 0;
    return LSA_OK;
}

int lsa_stochastic_apply(lsa_ctx* ctx, lsa_stochastic* h, const double* host_v, double* host_y, double* node_terms) {
    if (!ctx || !h || !host_v || !host_y) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_apply: null argument");
    const size_t bytes = (size_t)h->n * sizeof(double);
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(h->vdev, host_v, bytes, hipMemcpyHostToDevice, ctx->stream));
    ++h->st.spmv_calls;
    LSA_CHECK(k_spmv(ctx, sf_inner(h), LSA_F64, h->vdev, h->rhsdev));
    while (true) {
        LSA_CHECK(sf_enqueue(ctx, h, h->rhsdev, h->ydev));
        LSA_CHECK(sf_read_back(ctx, h));
        LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        const int verdict = sf_judge(ctx, h, "lsa_stochastic_apply", "apply", 0);
        if (verdict == 0) break;
        if (verdict < 0) return LSA_ERR_DIVERGED;
    }
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(host_y, h->ydev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (node_terms)
        for (int32_t k = 0; k < h->N; ++k) node_terms[k] = h->c[(size_t)k] * h->hlog[(size_t)4 * (size_t)(h->N + k) + 3];
    return LSA_OK;
}

int lsa_stochastic_info(const lsa_stochastic* h, lsa_stochastic_stats* out) {
    if (!h || !out) return LSA_ERR_ARG;
    out->nodes = h->N;
    out->kind = h->kind;
    out->bytes = h->bytes;
    out->seconds_factor = h->S->seconds_factor;
    out->seconds_solve = h->sec_solve;
    out->seconds_product = h->sec_product;
    out->seconds_dense = h->sec_dense;
    out->solver = h->st;
    out->batch_adjoint = h->batch_adjoint ? 1 : 0;
    out->adjoint_batches = h->adjoint_batches;
    out->forward_batches = h->forward_batches;
    out->seconds_solve_adjoint = h->sec_solve_adj;
    out->seconds_product_adjoint = h->sec_product_adj;
    return LSA_OK;
}

}  // extern "C"
