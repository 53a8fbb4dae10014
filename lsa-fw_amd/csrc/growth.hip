// Transient growth of M q' = A q: the optimal energy gains G_1 >= G_2 >= ... over a horizon T = N dt are the maxima of
// ||q(T)||_M^2 / ||q(0)||_M^2.  One implicit-Euler step (M - dt A) q+ = M q is q+ = -sigma C^-1 M q with C = A - sigma M and the real
// sigma = 1 / dt: the shift-invert operator the library factorises.  The propagator over N steps is Phi = (-sigma C^-1 M)^N, its
// adjoint in the M-inner product (M symmetric) is Phi+ = (-sigma C^-T M)^N on the same factors, and the gains are the largest
// eigenvalues of W = Phi+ Phi, which is M-self-adjoint, non-negative and real.  So the real thick-restart Lanczos iteration of
// lanczos.hip serves as it is -- basis, reorthogonalisation, tail, restart and Ritz vectors are an lsa_lanczos this handle owns --
// with another operator behind a step (lanczos_operator): a march of 2N solves on ONE factorisation of C instead of one solve.
//
// One step j (rhs = M v_j is left by the previous step's tail; keep: the 0/1 mask of the free dofs):
//     for k = 0 .. 2N-1:   x = C^-1 b_k (k < N) or C^-T b_k (k >= N),  z = C x (or C^T x);   b_0 = rhs
//         k < 2N-1:   mx = M x;  b_{k+1} = -sigma keep (.) mx;  log[k] = |b_k - z|^2, |b_k|^2, x^T mx, |x|^2     tg_march_kernel + tg_log_kernel
//     w = -sigma keep (.) x_{2N-1}          tg_scale_kernel: the one factor -sigma the march does not cover (b_0 carries none)
//     the pair (b_{2N-1}, z) of the last solve rides in the step's first lz_dot_kernel reduction, where the default's single solve does
// The march log travels to the host behind the step's one synchronisation; every solve is judged by direct_solve_verdict.
// Each direction carries its own refinement step once one of its solves missed ksp_rtol.
//
// lsa_growth_set_scheme(LSA_GROWTH_SDIRK2) marches by the L-stable, stiffly accurate two-stage SDIRK method with gamma = 1 - 1/sqrt 2
// instead: second order in dt.  Both stages solve with M - gamma dt A, so sigma = 1 / (gamma dt) and C is the same one matrix; with
// S = -sigma C^-1 M one time step is Phi_1 = S (a S + b I), a = 1 + sqrt 2, b = -sqrt 2 (the stability function
// (1 + (1 - 2 gamma) z) / (1 - gamma z)^2 written in s = 1 / (1 - gamma z)), its M-adjoint S+ (a S+ + b I) with S+ = -sigma C^-T M.  The
// march of a step is 4N solves (k < 2N forward, k >= 2N transposed) and only the transition after an even solve differs:
//         k odd:    b_{k+1} = -sigma keep (.) mx                        the next solve is a first stage: the statement above
//         k even:   b_{k+1} = (-a sigma) keep (.) mx + b b_k            the next solve is the second stage: b_k already is -sigma keep (.) M q
// b_k is the vector the kernel reads for the residual sum anyway: the combining form costs no load, no buffer and no launch more.
//
// lsa_growth_set_response_weight measures the response in a weight Q instead of M: G = max ||q(T)||_Q^2 / ||q(0)||_M^2, the eigenvalues of
// W = M^-1 Phi^T Q Phi = (C^-T M)^(N-1) C^-T Q Phi up to the -sigma factors, still M-self-adjoint.  The one change is the turn of the
// march: after the last forward solve (k = N - 1, N = stages * nsteps) mx = Q x instead of M x, for the next right-hand side and for
// the x^T mx sum (log entry N - 1: the windowed energy at T).  Under SDIRK2 that index is odd, so the transition is the plain one, and
// the combining transition after the first transposed solve reads that same right-hand side as its b_k.  An initial-condition weight
// would need Q^-1 and is not built.
//
// The sums of tg_march_kernel are taken in the order of k_multi_dot (rows strided over the 256 threads of a chunk of at least 512
// rows, xor tree over the wavefront, the four waves in wave order; tg_log_kernel: the chunks strided over 64 lanes and the same tree)
// and there are no floating-point atomics: two runs give the same bits, and LSA_GROWTH_FUSED=0 -- the same step through
// k_residual_norms, k_multi_dot and the scale -- gives them too.  A lane's rows are 256 apart in that order, so the loads are 8 bytes
// each, two rows in flight per lane as in lz_dot_kernel: a 16-byte load would take a row of the neighbouring lane's sum.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "lsa_internal.h"

namespace {

constexpr int kTgThreads = 256;  // four wavefronts of 64

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

__device__ __forceinline__ double tg_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// After an inner solve x of right-hand side b with z = C x and mx = M x, one pass over the rows: next = alpha keep (.) mx (alpha =
// -sigma; next == null: the last solve of a final march, nothing follows) and the chunk sums part[q nchunks + chunk], q = 0..3, of
// |b - z|^2, |b|^2, x^T mx and |x|^2.  The chunks are strided over the grid (sized from the CU count); next may not alias b.
// kCombine (a second-stage right-hand side of SDIRK2; next is not null): next = cb b + alpha keep (.) mx, alpha then being -a sigma.
template <bool kCombine>
__global__ __launch_bounds__(kTgThreads) void tg_march_kernel(int64_t n, int64_t rows_per_chunk, int nchunks, double alpha, const double* __restrict__ b,
                                                              const double* __restrict__ z, const double* __restrict__ x,
                                                              const double* __restrict__ mx, const double* __restrict__ keep, double* __restrict__ next,
                                                              double* __restrict__ part, double cb) {
    __shared__ double wsum[4][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const int64_t r0 = (int64_t)chunk * rows_per_chunk;
        const int64_t r1 = (r0 + rows_per_chunk < n) ? r0 + rows_per_chunk : n;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int64_t i = r0 + threadIdx.x;
        for (; i + kTgThreads < r1; i += 2 * kTgThreads) {
            const int64_t i2 = i + kTgThreads;
            const double ba = b[i], bb = b[i2], za = z[i], zb = z[i2], xa = x[i], xb = x[i2], ma = mx[i], mb = mx[i2], ka = keep[i], kb = keep[i2];
            const double da = ba - za, db = bb - zb;
            s0 = fma(da, da, s0);
            s0 = fma(db, db, s0);
            s1 = fma(ba, ba, s1);
            s1 = fma(bb, bb, s1);
            s2 = fma(xa, ma, s2);
            s2 = fma(xb, mb, s2);
            s3 = fma(xa, xa, s3);
            s3 = fma(xb, xb, s3);
            if constexpr (kCombine) {
                next[i] = fma(cb, ba, alpha * (ka * ma));
                next[i2] = fma(cb, bb, alpha * (kb * mb));
            } else if (next) {
                next[i] = alpha * (ka * ma);
                next[i2] = alpha * (kb * mb);
            }
        }
        for (; i < r1; i += kTgThreads) {
            const double bi = b[i], xi = x[i], mi = mx[i];
            const double d = bi - z[i];
            s0 = fma(d, d, s0);
            s1 = fma(bi, bi, s1);
            s2 = fma(xi, mi, s2);
            s3 = fma(xi, xi, s3);
            if constexpr (kCombine)
                next[i] = fma(cb, bi, alpha * (keep[i] * mi));
            else if (next)
                next[i] = alpha * (keep[i] * mi);
        }
        s0 = tg_wave_sum(s0);
        s1 = tg_wave_sum(s1);
        s2 = tg_wave_sum(s2);
        s3 = tg_wave_sum(s3);
        __syncthreads();  // (the previous chunk's sums have been read)
        if (lane == 0) {
            wsum[wave][0] = s0;
            wsum[wave][1] = s1;
            wsum[wave][2] = s2;
            wsum[wave][3] = s3;
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            const int q = threadIdx.x;
            part[(int64_t)q * nchunks + chunk] = ((wsum[0][q] + wsum[1][q]) + wsum[2][q]) + wsum[3][q];
        }
    }
}

// One workgroup: wave q finishes sum q of the march kernel's partial sums into out[q] (lane k adds the chunks k, k + 64, ... in that
// order, then the tree: multi_dot_finish_kernel's order)
__global__ __launch_bounds__(kTgThreads) void tg_log_kernel(int nchunks, const double* __restrict__ part, double* __restrict__ out) {
    const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double a = 0.0;
    for (int k = lane; k < nchunks; k += 64) a += part[(int64_t)q * nchunks + k];
    a = tg_wave_sum(a);
    if (lane == 0) out[q] = a;
}

// y = alpha keep (.) x   (y may be x)
__global__ __launch_bounds__(kTgThreads) void tg_scale_kernel(int64_t n, double alpha, const double* __restrict__ keep, const double* x, double* y) {
    const int64_t stride = (int64_t)gridDim.x * kTgThreads;
    for (int64_t i = (int64_t)blockIdx.x * kTgThreads + threadIdx.x; i < n; i += stride) y[i] = alpha * (keep[i] * x[i]);
}

// y = cb b + ca keep (.) x: the combining transition of the unfused form, tg_march_kernel<true>'s expression (y may alias neither)
__global__ __launch_bounds__(kTgThreads) void tg_combine_kernel(int64_t n, double ca, double cb, const double* __restrict__ keep, const double* __restrict__ x,
                                                                const double* __restrict__ b, double* __restrict__ y) {
    const int64_t stride = (int64_t)gridDim.x * kTgThreads;
    for (int64_t i = (int64_t)blockIdx.x * kTgThreads + threadIdx.x; i < n; i += stride) y[i] = fma(cb, b[i], ca * (keep[i] * x[i]));
}

// tg_march_kernel + tg_log_kernel unless LSA_GROWTH_FUSED=0 (read once per process): then k_residual_norms, k_multi_dot and the scale
// (a combined right-hand side: tg_combine_kernel)
bool tg_fused() {
    static const bool fused = env_flag("LSA_GROWTH_FUSED", true);
    return fused;
}

}  // namespace

struct lsa_growth {
    lsa_ctx* ctx = nullptr;
    lsa_op* op = nullptr;
    lsa_op_parts P{};
    lsa_lanczos* lz = nullptr;  // the basis and everything of a step but its operator
    lanczos_operator hook{};
    int64_t n = 0;
    int32_t ncv = 0, nsteps = 0, log_cap = 0;
    int32_t scheme = LSA_GROWTH_EULER;  // LSA_GROWTH_SDIRK2: two solves per time step, the second on a combined right-hand side
    double sigma = 0.0;
    const lsa_mat* Q = nullptr;  // the response weight at the turn of a step's march (lsa_growth_set_response_weight; borrowed), null: M
    std::vector<double> renergy;  // x(T)^T Q x(T) of the modes the last final marches ran (lsa_growth_response_energy)
    double* keep = nullptr;  // device 0/1 mask, the basis' row numbering
    std::vector<double> hkeep;
    // the march's own vectors: the two right-hand sides it alternates between (the step's rhs stays intact), a solution, C x, M x and
    // the residual of a refinement step (of the unfused form too)
    double *pp[2] = {nullptr, nullptr}, *x = nullptr, *cz = nullptr, *mx = nullptr, *r = nullptr;
    double* part = nullptr;    // 4 x kDotMaxChunks partial sums
    double* log = nullptr;     // 4 sums per marched solve, and one more quadruple (a final march's q0^T M q0; scratch of the unfused form)
    double* rnorms = nullptr;  // the two sums a refinement step's residual pass leaves (not read)
    double* hlog = nullptr;    // pinned host copy of the log
    int32_t logged = 0;        // quadruples the last read-back carries
    double* resp = nullptr;
    void* xtmp = nullptr;  // the responses of lsa_growth_solve (n x ncv) and, with a row permutation, their scattered form
    int32_t* row_perm = nullptr;
    bool refine_fwd = false, refine_adj = false, used_fwd = false, used_adj = false;  // used_*: what the march being judged was queued with
    int64_t solves_fwd = 0, solves_adj = 0, refined_fwd = 0, refined_adj = 0;
};

namespace {

void tg_free(lsa_growth* g) {
    if (g->lz) lsa_lanczos_destroy(g->lz);
    for (void* p : {(void*)g->keep, (void*)g->pp[0], (void*)g->pp[1], (void*)g->x, (void*)g->cz, (void*)g->mx, (void*)g->r, (void*)g->part, (void*)g->log,
                    (void*)g->rnorms, (void*)g->resp, g->xtmp, (void*)g->row_perm})
        if (p) (void)hipFree(p);
    if (g->hlog) (void)hipHostFree(g->hlog);
    delete g;
}

// SDIRK2's coefficients: Phi_1 = S (a S + b I)
const double kTgA = 1.0 + std::sqrt(2.0), kTgB = -std::sqrt(2.0);

int32_t tg_stages(int32_t scheme) { return scheme == LSA_GROWTH_SDIRK2 ? 2 : 1; }

// whether the right-hand side after solve k of a march is the combined one: under SDIRK2 the solves alternate first stage, second stage
bool tg_combines(const lsa_growth* g, int32_t k) { return g->scheme == LSA_GROWTH_SDIRK2 && (k & 1) == 0; }

int tg_grid(lsa_ctx* ctx, int64_t work, int per_cu) { return (int)std::max<int64_t>(std::min<int64_t>(work, (int64_t)ctx->num_cu * per_cu), 1); }

// the device log and its pinned copy for `entries` marched solves (and the spare quadruple behind them)
int tg_reserve_log(lsa_ctx* ctx, lsa_growth* g, int32_t entries) {
    if (entries <= g->log_cap) return LSA_OK;
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (g->log) (void)hipFree(g->log);
    if (g->hlog) (void)hipHostFree(g->hlog);
    g->log = g->hlog = nullptr;
    g->log_cap = 0;
    const size_t bytes = (size_t)4 * (size_t)(entries + 1) * sizeof(double);
    LSA_HIP_ALLOC(ctx, hipMalloc((void**)&g->log, bytes));
    LSA_HIP_ALLOC(ctx, hipHostMalloc((void**)&g->hlog, bytes));
    LSA_HIP_CHECK(ctx, hipMemsetAsync(g->log, 0, bytes, ctx->stream));
    g->log_cap = entries;
    return LSA_OK;
}

// y = W x for the weight W: M, or the response weight at the turn
int tg_mass(lsa_ctx* ctx, lsa_growth* g, const lsa_mat* W, const double* x, double* y) {
    ++g->P.st->spmv_calls;
    return k_spmv(ctx, W, LSA_F64, x, y);
}

int tg_scale(lsa_ctx* ctx, lsa_growth* g, double alpha, const double* x, double* y) {
    hipLaunchKernelGGL(tg_scale_kernel, dim3(tg_grid(ctx, (g->n + kTgThreads - 1) / kTgThreads, 8)), dim3(kTgThreads), 0, ctx->stream, g->n, alpha, g->keep, x, y);
    return lsa_check_launch(ctx, "growth scale");
}

int tg_combine(lsa_ctx* ctx, lsa_growth* g, double ca, double cb, const double* x, const double* b, double* y) {
    hipLaunchKernelGGL(tg_combine_kernel, dim3(tg_grid(ctx, (g->n + kTgThreads - 1) / kTgThreads, 8)), dim3(kTgThreads), 0, ctx->stream, g->n, ca, cb, g->keep, x, b,
                       y);
    return lsa_check_launch(ctx, "growth combine");
}

// What follows the inner solve x of b (z = C x): mx = W x (W: M, or the response weight after the last forward solve of a step's
// march), the next right-hand side -sigma keep (.) mx (next == null: none; combine, with a next: (-a sigma) keep (.) mx + b b, SDIRK2's
// second stage) and the four sums of log entry k.
int tg_after_solve(lsa_ctx* ctx, lsa_growth* g, const lsa_mat* W, int32_t k, const double* b, const double* z, const double* x, double* next, bool combine) {
    const int64_t n = g->n;
    combine = combine && next;
    const double ca = kTgA * -g->sigma, cb = kTgB;
    double* out = g->log + (size_t)4 * (size_t)k;
    LSA_CHECK(tg_mass(ctx, g, W, x, g->mx));
    if (tg_fused()) {
        int64_t rows_per_chunk;
        const int nchunks = dot_chunks(n, &rows_per_chunk);
        if (combine)
            hipLaunchKernelGGL(tg_march_kernel<true>, dim3(tg_grid(ctx, nchunks, 4)), dim3(kTgThreads), 0, ctx->stream, n, rows_per_chunk, nchunks, ca, b, z, x,
                               g->mx, g->keep, next, g->part, cb);
        else
            hipLaunchKernelGGL(tg_march_kernel<false>, dim3(tg_grid(ctx, nchunks, 4)), dim3(kTgThreads), 0, ctx->stream, n, rows_per_chunk, nchunks, -g->sigma, b, z,
                               x, g->mx, g->keep, next, g->part, 0.0);
        hipLaunchKernelGGL(tg_log_kernel, dim3(1), dim3(kTgThreads), 0, ctx->stream, nchunks, g->part, out);
        return lsa_check_launch(ctx, "growth march");
    }
    // the unfused form: r = b - z (its own two sums go to the spare quadruple and are not read), then the four sums as single dots
    LSA_CHECK(k_residual_norms(ctx, LSA_F64, n, b, z, g->r, g->log + (size_t)4 * (size_t)g->log_cap));
    LSA_CHECK(k_multi_dot(ctx, LSA_F64, n, 1, g->r, n, g->r, out));
    LSA_CHECK(k_multi_dot(ctx, LSA_F64, n, 1, b, n, b, out + 1));
    LSA_CHECK(k_multi_dot(ctx, LSA_F64, n, 1, x, n, g->mx, out + 2));
    LSA_CHECK(k_multi_dot(ctx, LSA_F64, n, 1, x, n, x, out + 3));
    if (combine) return tg_combine(ctx, g, ca, cb, g->mx, b, next);
    return next ? tg_scale(ctx, g, -g->sigma, g->mx, next) : LSA_OK;
}

struct TgSolve {  // one solve of a march as the host sees it
    bool adjoint, refine, backward;
    double res, bnorm, xnorm;
};

// Judges the solves of one march: all accepted -> books them and returns 0; a miss without refinement switches the direction's flag
// on and returns 1 (the march is done again); a miss after it sets LSA_ERR_DIVERGED naming direction, march index and `where`.
int tg_judge_march(lsa_ctx* ctx, lsa_growth* g, std::vector<TgSolve>& sv, const char* who, const char* what, int32_t where) {
    int worst = 0;
    for (size_t k = 0; k < sv.size(); ++k) {
        TgSolve& s = sv[k];
        const int v = direct_solve_verdict(g->P, s.refine, s.res, s.bnorm, s.xnorm, &s.backward);
        if (v < 0) {
            lsa_set_error(ctx, LSA_ERR_DIVERGED, "%s: the %s solve %d of the march of %s %d left a relative residual of %.3e after its refinement step "
                                                 "(ksp_rtol %.1e) and a backward error above 1e-12 ||C||_F", who, s.adjoint ? "transposed" : "forward", (int)k, what,
                          where, s.bnorm > 0.0 ? s.res / s.bnorm : s.res, g->P.ksp_rtol);
            return -1;
        }
        if (v > 0) {
            (s.adjoint ? g->refine_adj : g->refine_fwd) = true;
            worst = 1;
        }
    }
    if (worst) return worst;
    for (const TgSolve& s : sv) {
        if (s.backward) ++g->P.st->backward_accepted;
        stats_book_direct_solve(g->P.st, 1, s.refine, s.res, s.bnorm);
        ++(s.adjoint ? g->solves_adj : g->solves_fwd);
        if (s.refine) ++(s.adjoint ? g->refined_adj : g->refined_fwd);
    }
    return 0;
}

// ---- the operator behind a Lanczos step -------------------------------------------------------------------------------------------
int tg_hook_enqueue(lsa_ctx* ctx, void* self, int32_t, const void* rhs, void* w, void* z, void* r, lanczos_check* chk) {
    lsa_growth* g = (lsa_growth*)self;
    const int32_t N = tg_stages(g->scheme) * g->nsteps, last = 2 * N - 1;  // N solves each way
    g->used_fwd = g->refine_fwd;
    g->used_adj = g->refine_adj;
    const double* b = (const double*)rhs;
    for (int32_t k = 0; k < last; ++k) {
        const bool adj = k >= N;
        LSA_CHECK(direct_solve_enqueue(ctx, g->op, LSA_F64, b, g->x, g->cz, g->r, adj ? g->used_adj : g->used_fwd, g->rnorms, adj ? 1 : 0));
        double* next = g->pp[k & 1];
        // the turn: the response is measured in Q, so Phi+ begins from -sigma keep (.) Q x(T) (log entry N - 1: the windowed energy at T)
        const lsa_mat* W = (k == N - 1 && g->Q) ? g->Q : g->P.Kmul;
        LSA_CHECK(tg_after_solve(ctx, g, W, k, b, g->cz, g->x, next, tg_combines(g, k)));
        b = next;
    }
    // the last solve lands where the default's single solve does; the step's first reduction checks it
    LSA_CHECK(direct_solve_enqueue(ctx, g->op, LSA_F64, b, w, z, r, g->used_adj, g->rnorms, 1));
    if (g->used_adj) LSA_CHECK(k_nrm2(ctx, LSA_F64, g->n, w, chk[0].xnorm2_dev));
    LSA_CHECK(tg_scale(ctx, g, -g->sigma, (const double*)w, (double*)w));
    chk[0].b = b;
    chk[0].z = z;
    chk[0].refined = g->used_adj;
    g->logged = last;
    return LSA_OK;
}

int tg_hook_read_back(lsa_ctx* ctx, void* self) {
    lsa_growth* g = (lsa_growth*)self;
    if (g->logged <= 0) return LSA_OK;
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(g->hlog, g->log, (size_t)4 * (size_t)g->logged * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    return LSA_OK;
}

int tg_hook_judge(lsa_ctx* ctx, void* self, int32_t j, const lanczos_sums* s) {
    lsa_growth* g = (lsa_growth*)self;
    const int32_t N = tg_stages(g->scheme) * g->nsteps, last = 2 * N - 1;
    std::vector<TgSolve> sv((size_t)last + 1);
    for (int32_t k = 0; k < last; ++k) {
        const double* e = g->hlog + (size_t)4 * (size_t)k;
        const bool adj = k >= N;
        sv[(size_t)k] = TgSolve{adj, adj ? g->used_adj : g->used_fwd, false, std::sqrt(e[0]), std::sqrt(e[1]), std::sqrt(e[3])};
    }
    sv[(size_t)last] = TgSolve{true, g->used_adj, false, s[0].res, s[0].bnorm, s[0].xnorm};
    g->logged = 0;
    return tg_judge_march(ctx, g, sv, "lsa_growth_extend", "step", j);
}

}  // namespace

int growth_shape(const lsa_growth* g, int64_t* n, int32_t* ncv, int32_t* nsteps) {
    if (!g) return LSA_ERR_ARG;
    if (n) *n = g->n;
    if (ncv) *ncv = g->ncv;
    if (nsteps) *nsteps = g->nsteps;
    return LSA_OK;
}

void growth_counts(const lsa_growth* g, int64_t counts[4]) {
    counts[0] = g->solves_fwd;
    counts[1] = g->solves_adj;
    counts[2] = g->refined_fwd;
    counts[3] = g->refined_adj;
}

int growth_inject(lsa_ctx* ctx, lsa_growth* g, int32_t j, const double* host_v) {
    if (!ctx || !g || !host_v) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth: null argument");
    std::vector<double> v((size_t)g->n);
    for (int64_t i = 0; i < g->n; ++i) v[(size_t)i] = g->hkeep[(size_t)i] * host_v[i];
    g->logged = 0;
    return lanczos_inject(ctx, g->lz, j, v.data());
}

int growth_restart(lsa_ctx* ctx, lsa_growth* g, int32_t m, int32_t knew, const double* Y, int32_t ldy) {
    if (!g) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth restart: null argument");
    return lanczos_restart(ctx, g->lz, m, knew, Y, ldy);
}

int growth_ritz_vectors(lsa_ctx* ctx, lsa_growth* g, int32_t m, int32_t nvec, const double* Y, int32_t ldy, double* Q0) {
    if (!g) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth vectors: null argument");
    return lanczos_ritz_vectors(ctx, g->lz, m, nvec, Y, ldy, Q0);
}

int growth_responses(lsa_ctx* ctx, lsa_growth* g, int32_t nvec, double* QT, double* energy) {
    if (!ctx || !g) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth responses: null argument");
    if (nvec < 0 || nvec > g->ncv) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth responses: bad sizes");
    if (nvec == 0) return LSA_OK;
    const int64_t n = g->n;
    const int32_t stages = tg_stages(g->scheme), steps = g->nsteps, N = stages * steps;  // N solves; a time step's energy: its last stage's
    const size_t vb = (size_t)std::max<int64_t>(n, 1) * sizeof(double);
    if (!g->resp) LSA_HIP_ALLOC(ctx, hipMalloc((void**)&g->resp, vb * (size_t)g->ncv));
    const double* Q0 = (const double*)lanczos_ritz_device(g->lz);
    const double t0 = now_s();
    std::vector<TgSolve> sv((size_t)N);
    g->renergy.assign((size_t)nvec, 0.0);
    for (int32_t c = 0; c < nvec; ++c) {
        const double* q0 = Q0 + (size_t)c * (size_t)n;
        double* e0 = g->log + (size_t)4 * (size_t)N;  // (entry N: q0^T M q0 alone)
        while (true) {
            const bool refine = g->refine_fwd;
            LSA_CHECK(tg_mass(ctx, g, g->P.Kmul, q0, g->mx));
            LSA_CHECK(k_multi_dot(ctx, LSA_F64, n, 1, q0, n, g->mx, e0));
            LSA_CHECK(tg_scale(ctx, g, -g->sigma, g->mx, g->pp[1]));
            const double* b = g->pp[1];
            for (int32_t s = 0; s < N; ++s) {
                LSA_CHECK(direct_solve_enqueue(ctx, g->op, LSA_F64, b, g->x, g->cz, g->r, refine, g->rnorms, 0));
                double* next = s + 1 < N ? g->pp[s & 1] : nullptr;
                LSA_CHECK(tg_after_solve(ctx, g, g->P.Kmul, s, b, g->cz, g->x, next, tg_combines(g, s)));
                b = next;
            }
            if (g->Q) {  // the windowed energy at T behind q0^T M q0: one more product and dot
                LSA_CHECK(tg_mass(ctx, g, g->Q, g->x, g->mx));
                LSA_CHECK(k_multi_dot(ctx, LSA_F64, n, 1, g->x, n, g->mx, e0 + 1));
            }
            LSA_CHECK(k_copy(ctx, LSA_F64, n, g->x, g->resp + (size_t)c * (size_t)n));
            LSA_HIP_CHECK(ctx, hipMemcpyAsync(g->hlog, g->log, ((size_t)4 * (size_t)N + 2) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            for (int32_t s = 0; s < N; ++s) {
                const double* e = g->hlog + (size_t)4 * (size_t)s;
                sv[(size_t)s] = TgSolve{false, refine, false, std::sqrt(e[0]), std::sqrt(e[1]), std::sqrt(e[3])};
            }
            const int verdict = tg_judge_march(ctx, g, sv, "lsa_growth_solve", "response", c);
            if (verdict == 0) break;
            if (verdict < 0) return LSA_ERR_DIVERGED;
        }
        g->renergy[(size_t)c] = g->Q ? g->hlog[(size_t)4 * (size_t)N + 1] : g->hlog[(size_t)4 * (size_t)(N - 1) + 2];
        if (energy) {
            energy[(size_t)c * (size_t)(steps + 1)] = g->hlog[(size_t)4 * (size_t)N];
            for (int32_t s = 0; s < steps; ++s)
                energy[(size_t)c * (size_t)(steps + 1) + (size_t)s + 1] = g->hlog[(size_t)4 * (size_t)(stages * (s + 1) - 1) + 2];
        }
    }
    g->P.st->seconds_solve += now_s() - t0;
    return QT ? basis_columns_to_host(ctx, LSA_F64, n, nvec, g->row_perm, g->resp, &g->xtmp, g->ncv, QT) : LSA_OK;
}

extern "C" {

int lsa_growth_create(lsa_ctx* ctx, lsa_op* op, int32_t ncv, int32_t nsteps, const double* keep, lsa_growth** out) {
    if (!ctx || !op || !out || ncv < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_create: bad argument");
    if (nsteps < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_create: nsteps = %d: a horizon has at least one step", nsteps);
    lsa_op_parts P{};
    LSA_CHECK(lsa_op_get_parts(op, &P));
    if (!P.shift_invert) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_create: the operator is not shift-invert (mode 0): C = A - M / dt is what gets factorised");
    if (P.adjoint) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_create: the operator is in adjoint mode (lsa_op_set_adjoint): the march picks each solve's direction itself");
    if (P.projected) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_create: the operator is projected (lsa_op_set_projection): the keep mask of this handle is the restriction");
    if (!P.one_rank || ctx->nranks != 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_create: the operator is spread over several ranks: one rank only");
    if (!P.Kmul) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_create: the operator has no M: the energy is measured in the M-inner product");
    if (P.Kmul->dtype != LSA_F64) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_create: M is complex: the M-inner product needs a real symmetric M");
    if (!P.nd || !P.Kfac) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_create: the operator has no exact LU (pc_type 2): every solve of the march runs on its factors");
    if (P.sigma[1] != 0.0 || P.Kfac->dtype != LSA_F64)
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_create: the shift is complex or the factors are: sigma = 1 / dt is real and so are A and M");
    if (!(P.sigma[0] > 0.0) || !std::isfinite(P.sigma[0]))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_create: the shift sigma = %.3e is not positive: sigma = 1 / dt with a time step dt > 0", P.sigma[0]);
    if ((int64_t)ncv > P.n) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_create: ncv = %d exceeds the problem size %lld", ncv, (long long)P.n);
    if (keep)
        for (int64_t i = 0; i < P.n; ++i)
            if (keep[i] != 0.0 && keep[i] != 1.0) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_create: keep[%lld] = %.3e is neither 0 nor 1", (long long)i, keep[i]);
    lsa_growth* g = new lsa_growth();
    g->ctx = ctx;
    g->op = op;
    g->P = P;
    g->n = P.n;
    g->ncv = ncv;
    g->nsteps = nsteps;
    g->sigma = P.sigma[0];
    g->hkeep.assign((size_t)P.n, 1.0);
    if (keep) std::copy(keep, keep + P.n, g->hkeep.begin());
    int rc = lanczos_create_basis(ctx, op, ncv, LSA_F64, "lsa_growth", &g->lz);
    if (rc != LSA_OK) {
        g->lz = nullptr;
        tg_free(g);
        return rc;
    }
    const size_t vb = (size_t)std::max<int64_t>(g->n, 1) * sizeof(double);
    bool ok = true;
    for (double** p : {&g->keep, &g->pp[0], &g->pp[1], &g->x, &g->cz, &g->mx, &g->r}) ok = ok && hipMalloc((void**)p, vb) == hipSuccess;
    ok = ok && hipMalloc((void**)&g->part, (size_t)kDotMaxChunks * 4 * sizeof(double)) == hipSuccess && hipMalloc((void**)&g->rnorms, 2 * sizeof(double)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        tg_free(g);
        return lsa_set_error(ctx, LSA_ERR_OOM, "lsa_growth_create: out of device memory (n=%lld, ncv=%d)", (long long)P.n, ncv);
    }
    rc = tg_reserve_log(ctx, g, 2 * nsteps);
    if (rc == LSA_OK && hipMemcpy(g->keep, g->hkeep.data(), (size_t)g->n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        rc = lsa_set_error(ctx, LSA_ERR_HIP, "lsa_growth_create: the upload of the keep mask failed");
    if (rc != LSA_OK) {
        tg_free(g);
        return rc;
    }
    g->hook = lanczos_operator{g, 1, tg_hook_enqueue, tg_hook_read_back, tg_hook_judge};
    rc = lanczos_set_operator(ctx, g->lz, &g->hook);
    if (rc != LSA_OK) {
        tg_free(g);
        return rc;
    }
    *out = g;
    return LSA_OK;
}

void lsa_growth_destroy(lsa_growth* g) {
    if (!g) return;
    if (g->ctx && g->ctx->stream) (void)hipStreamSynchronize(g->ctx->stream);
    tg_free(g);
}

int lsa_growth_set_row_permutation(lsa_ctx* ctx, lsa_growth* g, const int32_t* perm) {
    if (!ctx || !g) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_set_row_permutation: null argument");
    LSA_CHECK(basis_upload_row_permutation(ctx, "lsa_growth_set_row_permutation", g->n, perm, &g->row_perm));
    return lsa_lanczos_set_row_permutation(ctx, g->lz, perm);
}

int lsa_growth_set_steps(lsa_ctx* ctx, lsa_growth* g, int32_t nsteps) {
    if (!ctx || !g) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_set_steps: null argument");
    if (nsteps < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_set_steps: nsteps = %d: a horizon has at least one step", nsteps);
    LSA_CHECK(tg_reserve_log(ctx, g, 2 * tg_stages(g->scheme) * nsteps));
    g->nsteps = nsteps;
    // a new horizon begins as a new handle does: the bytes of a horizon do not depend on what ran before it on these factors
    g->refine_fwd = g->refine_adj = false;
    g->logged = 0;
    return LSA_OK;
}

int lsa_growth_set_scheme(lsa_ctx* ctx, lsa_growth* g, int32_t scheme) {
    if (!ctx || !g) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_set_scheme: null argument");
    if (scheme != LSA_GROWTH_EULER && scheme != LSA_GROWTH_SDIRK2)
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_set_scheme: scheme = %d is neither LSA_GROWTH_EULER (0) nor LSA_GROWTH_SDIRK2 (1)", scheme);
    LSA_CHECK(tg_reserve_log(ctx, g, 2 * tg_stages(scheme) * g->nsteps));
    g->scheme = scheme;
    // as a new horizon: the bytes of a scheme do not depend on what ran before it on these factors
    g->refine_fwd = g->refine_adj = false;
    g->logged = 0;
    return LSA_OK;
}

int lsa_growth_set_response_weight(lsa_ctx* ctx, lsa_growth* g, const lsa_mat* Q) {
    if (!ctx || !g) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_set_response_weight: null argument");
    if (Q && Q->dtype != LSA_F64)
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_set_response_weight: the weight is complex: a weight is real symmetric positive semidefinite");
    if (Q && (Q->row0 != 0 || (int64_t)Q->n != g->n || (int64_t)Q->ncols != g->n))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_set_response_weight: the weight is %d x %d (from row %d), the problem has size %lld", Q->n, Q->ncols,
                             Q->row0, (long long)g->n);
    g->Q = Q;
    // as a new scheme: the bytes of a weight do not depend on what ran before it on these factors
    g->refine_fwd = g->refine_adj = false;
    g->logged = 0;
    g->renergy.clear();
    return LSA_OK;
}

int lsa_growth_response_energy(lsa_ctx* ctx, const lsa_growth* g, int32_t nvec, double* out) {
    if (!ctx || !g || !out) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_response_energy: null argument");
    if (nvec < 0 || (size_t)nvec > g->renergy.size())
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_response_energy: %d values asked for, the last lsa_growth_solve marched %d responses", nvec,
                             (int)g->renergy.size());
    std::copy(g->renergy.begin(), g->renergy.begin() + nvec, out);
    return LSA_OK;
}

int lsa_growth_set_start(lsa_ctx* ctx, lsa_growth* g, const double* host_v) { return growth_inject(ctx, g, 0, host_v); }

int lsa_growth_extend(lsa_ctx* ctx, lsa_growth* g, int32_t j0, int32_t j1, double* T, int32_t ldt, int32_t* breakdown) {
    if (!ctx || !g || !T) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_extend: null argument");
    return lsa_lanczos_extend(ctx, g->lz, j0, j1, T, ldt, breakdown);
}

int lsa_growth_basis(lsa_ctx* ctx, const lsa_growth* g, int32_t ncols, double* host_V) {
    if (!ctx || !g || !host_V) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_basis: null argument");
    return lsa_lanczos_basis(ctx, g->lz, ncols, host_V);
}

}  // extern "C"
