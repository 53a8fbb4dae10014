// Resolvent (input-output) analysis of M q' = A q + M f at a real frequency omega: the optimal gains sigma_1 >= sigma_2 >= ... are the
// maxima of ||q||_M / ||f||_M over q = R M f, R = (i omega M - A)^-1, and sigma_j^2 are the largest eigenvalues of
//     W = R M R^H M = C^-1 M C^-H M,   C = A - i omega M  (the sign cancels),
// which is self-adjoint and non-negative in the M-(semi-)inner product.  So the thick-restart Lanczos iteration of lanczos.hip serves
// as it is -- basis, reorthogonalisation, tail, restart and Ritz vectors are an lsa_lanczos with complex scalars (n x (ncv + 1)
// complex128, V^H M V = I, the same real symmetric projected matrix) that this handle owns -- with W as the operator behind a step
// (lanczos_operator).  This file holds what is the resolvent's own: that operator, the weights and the forcings; the outer loop is
// the one of lsa_lanczos_solve (dense.hip).
//
// The operator of step j (rhs = M v_j is left by the previous step's tail), on ONE factorisation of C (shift-invert mode 0 at
// sigma = i omega):
//     z = C^-H rhs                          the transposed, conjugated sweeps (ndlu_solve_adjoint_dev)
//     ca = C^H z                            for the check |rhs - ca| <= ksp_rtol |rhs|
//     tm = M z
//     w = C^-1 tm                           the forward sweeps
//     cf = C w                              for the check |tm - cf| <= ksp_rtol |tm|
// Both checks ride in the step's first reduction (rz_dot_kernel takes two pairs) and come back with the step's one read-back.
// lsa_resolvent_set_weights puts a forcing weight Q_f and a response weight Q_q (real symmetric positive semidefinite, e.g. the windowed
// D M D of lsa_csr_window) where M stands: q = R Q_f f, sigma = max ||q||_Qq / ||f||_Qf, W = C^-1 Q_f C^-H Q_q, self-adjoint in the
// Q_q-semi-inner product.  No inverse of a weight appears and the step keeps its launches: Q_q is the basis' inner product
// (lanczos_set_inner_product: rhs = Q_q v_j, t = Q_q w) and tm = Q_f z (rz_forcing); both are M on a new handle, whose bits are those
// of a handle without weights.  Nothing in the step needs Re sigma = 0: a shift beta + i omega gives the discounted resolvent.
// Each direction decides about its own refinement step (direct_solve_enqueue with an explicit direction: the operator's own direction,
// and the state lsa_op_set_adjoint clears, stay).
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "ndlu_internal.h"

namespace {

constexpr int kRzThreads = 256;  // four wavefronts of 64

// x <- alpha x (the forcing's -1 / gain)
__global__ __launch_bounds__(kRzThreads) void rz_scale_kernel(int64_t n, double alpha, const cplx* x, cplx* y) {
    const int64_t stride = (int64_t)gridDim.x * kRzThreads;
    for (int64_t i = (int64_t)blockIdx.x * kRzThreads + threadIdx.x; i < n; i += stride) rz_st(y + i, s_mul(alpha, rz_ld(x + i)));
}

}  // namespace

struct lsa_resolvent {
    lsa_ctx* ctx = nullptr;
    lsa_op* op = nullptr;
    lsa_op_parts P{};
    lsa_lanczos* lz = nullptr;  // the basis with complex scalars and everything of a step but its operator
    lanczos_operator hook{};
    int64_t n = 0;
    int32_t ncv = 0;
    // the forcing and the response weight (lsa_resolvent_set_weights; borrowed): both are the operator's M on a new handle
    const lsa_mat *Qf = nullptr, *Qq = nullptr;
    // the operator's own vectors: C^-H rhs and C^H of it, Q_f z and the refinement's residual (of the forcings' solves too)
    cplx *za = nullptr, *ca = nullptr, *tm = nullptr, *r = nullptr;
    double* norms = nullptr;  // the two sums a refinement step's residual pass leaves (not read), then a forcing's |tm - C^H z|^2, |tm|^2, |z|^2
    // each direction carries its own refinement step once one of its solves missed ksp_rtol; used_*: what the step being judged was queued with
    bool refine_adj = false, refine_fwd = false, used_adj = false, used_fwd = false;
    int64_t solves_adj = 0, solves_fwd = 0, refined_adj = 0, refined_fwd = 0;
    // lsa_resolvent_set_block_forcings: the forcings' adjoint solves as one block solve.  Its work vectors (M q_c and C^-H M q_c,
    // blk_cols columns each) and the three sums per column of the check are made by the first block call.
    bool block_forcings = false;
    cplx *blk_tm = nullptr, *blk_za = nullptr;
    double* blk_norms = nullptr;
    int32_t blk_cols = 0;
};

namespace {

void rz_free(lsa_resolvent* l) {
    if (l->lz) lsa_lanczos_destroy(l->lz);
    for (void* p : {(void*)l->za, (void*)l->ca, (void*)l->tm, (void*)l->r, (void*)l->norms, (void*)l->blk_tm, (void*)l->blk_za, (void*)l->blk_norms})
        if (p) (void)hipFree(p);
    delete l;
}

// y = Q_q x, the response product (Q_q real, complex vectors; M unless lsa_resolvent_set_weights gave another)
int rz_response(lsa_ctx* ctx, lsa_resolvent* l, const cplx* x, cplx* y) {
    ++l->P.st->spmv_calls;
    return k_spmv(ctx, l->Qq, LSA_C128, x, y);
}

// y = Q_f x, the forcing product
int rz_forcing(lsa_ctx* ctx, lsa_resolvent* l, const cplx* x, cplx* y) {
    ++l->P.st->spmv_calls;
    return k_spmv(ctx, l->Qf, LSA_C128, x, y);
}

int rz_grid(lsa_ctx* ctx, int64_t n, int per_cu) {
    return (int)std::max<int64_t>(std::min<int64_t>((n + kRzThreads - 1) / kRzThreads, (int64_t)ctx->num_cu * per_cu), 1);
}

void rz_book(lsa_resolvent* l, bool adjoint, bool refine, bool backward, double res, double bnorm) {
    if (backward) ++l->P.st->backward_accepted;
    stats_book_direct_solve(l->P.st, 1, refine, res, bnorm);
    ++(adjoint ? l->solves_adj : l->solves_fwd);
    if (refine) ++(adjoint ? l->refined_adj : l->refined_fwd);
}

// ---- the operator behind a Lanczos step: W = C^-1 Q_f C^-H on rhs = Q_q v_j ---------------------------------------------------------
int rz_hook_enqueue(lsa_ctx* ctx, void* self, int32_t, const void* rhs, void* w, void* cf, void*, lanczos_check* chk) {
    lsa_resolvent* l = (lsa_resolvent*)self;
    const bool ra = l->used_adj = l->refine_adj, rf = l->used_fwd = l->refine_fwd;
    // z = C^-H rhs, ca = C^H z;  tm = Q_f z;  w = C^-1 tm, cf = C w  (each with its direction's refinement step once switched on)
    LSA_CHECK(direct_solve_enqueue(ctx, l->op, LSA_C128, rhs, l->za, l->ca, l->r, ra, l->norms, 1));
    if (ra) LSA_CHECK(k_nrm2(ctx, LSA_C128, l->n, l->za, chk[0].xnorm2_dev));  // for the backward-error judgement
    LSA_CHECK(rz_forcing(ctx, l, l->za, l->tm));
    LSA_CHECK(direct_solve_enqueue(ctx, l->op, LSA_C128, l->tm, w, cf, l->r, rf, l->norms, 0));
    if (rf) LSA_CHECK(k_nrm2(ctx, LSA_C128, l->n, w, chk[1].xnorm2_dev));
    chk[0].b = rhs, chk[0].z = l->ca, chk[0].refined = ra;
    chk[1].b = l->tm, chk[1].z = cf, chk[1].refined = rf;
    return LSA_OK;
}

int rz_hook_judge(lsa_ctx* ctx, void* self, int32_t j, const lanczos_sums* s) {
    lsa_resolvent* l = (lsa_resolvent*)self;
    const bool ra = l->used_adj, rf = l->used_fwd;
    bool back_a = false, back_f = false;
    const int va = direct_solve_verdict(l->P, ra, s[0].res, s[0].bnorm, s[0].xnorm, &back_a);
    const int vf = direct_solve_verdict(l->P, rf, s[1].res, s[1].bnorm, s[1].xnorm, &back_f);
    if (va == 0 && vf == 0) {
        rz_book(l, true, ra, back_a, s[0].res, s[0].bnorm);
        rz_book(l, false, rf, back_f, s[1].res, s[1].bnorm);
        return 0;
    }
    if (va < 0 || vf < 0) {
        const lanczos_sums& f = s[va < 0 ? 0 : 1];
        lsa_set_error(ctx, LSA_ERR_DIVERGED, "lsa_resolvent_extend: the %s solve of step %d left a relative residual of %.3e after its refinement "
                                             "step (ksp_rtol %.1e) and a backward error above 1e-12 ||C||_F", va < 0 ? "adjoint" : "forward", j,
                      f.bnorm > 0.0 ? f.res / f.bnorm : f.res, l->P.ksp_rtol);
        return -1;
    }
    // from here on every solve of a direction that missed carries the refinement step; this step is done again
    if (va > 0) l->refine_adj = true;
    if (vf > 0) l->refine_fwd = true;
    return 1;
}

// The forcings' first attempts as ONE adjoint block solve (lsa_resolvent_set_block_forcings, no refinement step switched on yet):
// tm_c = M q_c for all columns, z_c = C^-H tm_c in the wide passes of the transposed sweeps, then per column what
// direct_solve_enqueue and the loop of resolvent_forcings queue behind the sweeps -- the check product C^H z_c, its residual sums
// and |z_c|^2 -- and one read-back for all of them.  The columns are judged in order: an accepted one is booked and scaled as the
// loop does it; the first that misses ksp_rtol switches the refinement step on and ends the block.  *done: the columns finished;
// the loop takes the rest (every column is the loop's, bit for bit and count for count).  An allocation that fails leaves all
// columns to the loop.
int rz_forcings_block(lsa_ctx* ctx, lsa_resolvent* l, cplx* Q, int32_t nvec, const double* gain, int32_t* done) {
    *done = 0;
    const int64_t n = l->n;
    if (l->blk_cols < nvec) {
        for (void* p : {(void*)l->blk_tm, (void*)l->blk_za, (void*)l->blk_norms})
            if (p) (void)hipFree(p);
        l->blk_tm = l->blk_za = nullptr;
        l->blk_norms = nullptr;
        l->blk_cols = 0;
        const size_t bytes = (size_t)std::max<int64_t>(n, 1) * sizeof(cplx) * (size_t)nvec;
        if (hipMalloc((void**)&l->blk_tm, bytes) != hipSuccess || hipMalloc((void**)&l->blk_za, bytes) != hipSuccess ||
            hipMalloc((void**)&l->blk_norms, (size_t)3 * (size_t)nvec * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            for (void* p : {(void*)l->blk_tm, (void*)l->blk_za, (void*)l->blk_norms})
                if (p) (void)hipFree(p);
            l->blk_tm = l->blk_za = nullptr;
            l->blk_norms = nullptr;
            return LSA_OK;
        }
        l->blk_cols = nvec;
    }
    for (int32_t c = 0; c < nvec; ++c)
        if (!(gain[c] > 0.0) || !std::isfinite(gain[c]))
            return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent forcings: gain %d is %.3e: no forcing belongs to it", c, gain[c]);
    // (a product is counted where its column is accepted: a column the loop takes over forms, and counts, its own)
    for (int32_t c = 0; c < nvec; ++c) LSA_CHECK(k_spmv(ctx, l->Qq, LSA_C128, Q + (size_t)c * (size_t)n, l->blk_tm + (size_t)c * (size_t)n));
    const void* tms = l->blk_tm;
    void* zas = l->blk_za;
    const NdSolve rq = {1, &l->P.nd, false, 2, LSA_C128, nvec, &tms, n, &zas, n, "lsa_resolvent forcings"};
    LSA_CHECK(ndlu_solve_run(ctx, rq));
    for (int32_t c = 0; c < nvec; ++c) {
        const cplx* tm = l->blk_tm + (size_t)c * (size_t)n;
        const cplx* za = l->blk_za + (size_t)c * (size_t)n;
        LSA_CHECK(k_spmv_transpose(ctx, l->P.Kfac, 1, LSA_C128, za, l->ca));
        LSA_CHECK(k_residual_norms(ctx, LSA_C128, n, tm, l->ca, l->r, l->blk_norms + 3 * (size_t)c));
        LSA_CHECK(k_nrm2(ctx, LSA_C128, n, za, l->blk_norms + 3 * (size_t)c + 2));
    }
    const size_t bytes = (size_t)3 * (size_t)nvec * sizeof(double);
    LSA_CHECK(lsa_ensure_scratch(ctx, 0, bytes));
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(ctx->pinned, l->blk_norms, bytes, hipMemcpyDeviceToHost, ctx->stream));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<double> sums((const double*)ctx->pinned, (const double*)ctx->pinned + 3 * (size_t)nvec);
    for (int32_t c = 0; c < nvec; ++c) {
        const double res = std::sqrt(sums[3 * (size_t)c]), bnorm = std::sqrt(sums[3 * (size_t)c + 1]), xnorm = std::sqrt(sums[3 * (size_t)c + 2]);
        bool backward = false;
        const int verdict = direct_solve_verdict(l->P, false, res, bnorm, xnorm, &backward);
        if (verdict > 0) {
            l->refine_adj = true;
            break;
        }
        if (verdict < 0)
            return lsa_set_error(ctx, LSA_ERR_DIVERGED, "lsa_resolvent forcings: the adjoint solve of forcing %d left a relative residual of %.3e after its "
                                                        "refinement step (ksp_rtol %.1e) and a backward error above 1e-12 ||C||_F", c,
                                 bnorm > 0.0 ? res / bnorm : res, l->P.ksp_rtol);
        ++l->P.st->spmv_calls;
        rz_book(l, true, false, backward, res, bnorm);
        hipLaunchKernelGGL(rz_scale_kernel, dim3(rz_grid(ctx, n, 8)), dim3(kRzThreads), 0, ctx->stream, n, -1.0 / gain[c], l->blk_za + (size_t)c * (size_t)n,
                           Q + (size_t)c * (size_t)n);
        LSA_CHECK(lsa_check_launch(ctx, "resolvent forcings"));
        *done = c + 1;
    }
    return LSA_OK;
}

}  // namespace

int resolvent_shape(const lsa_resolvent* l, int64_t* n, int32_t* ncv) {
    if (!l) return LSA_ERR_ARG;
    if (n) *n = l->n;
    if (ncv) *ncv = l->ncv;
    return LSA_OK;
}

void resolvent_counts(const lsa_resolvent* l, int64_t counts[4]) {
    counts[0] = l->solves_adj;
    counts[1] = l->solves_fwd;
    counts[2] = l->refined_adj;
    counts[3] = l->refined_fwd;
}

int resolvent_inject(lsa_ctx* ctx, lsa_resolvent* l, int32_t j, const cplx* host_v) {
    if (!l) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent: null argument");
    return lanczos_inject(ctx, l->lz, j, host_v);
}

int resolvent_restart(lsa_ctx* ctx, lsa_resolvent* l, int32_t m, int32_t knew, const double* Y, int32_t ldy) {
    if (!l) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent restart: null argument");
    return lanczos_restart(ctx, l->lz, m, knew, Y, ldy);
}

int resolvent_ritz_vectors(lsa_ctx* ctx, lsa_resolvent* l, int32_t m, int32_t nvec, const double* Y, int32_t ldy, cplx* Q) {
    if (!l) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent vectors: null argument");
    return lanczos_ritz_vectors(ctx, l->lz, m, nvec, Y, ldy, Q);
}

int resolvent_forcings(lsa_ctx* ctx, lsa_resolvent* l, int32_t nvec, const double* gain, cplx* F) {
    if (!ctx || !l || !gain || !F) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent forcings: null argument");
    if (nvec < 0 || nvec > l->ncv) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent forcings: bad sizes");
    const int64_t n = l->n;
    cplx* Q = (cplx*)lanczos_ritz_device(l->lz);  // the responses; each becomes its forcing
    double* norms = l->norms + 2;                 // |tm - C^H z|^2, |tm|^2, and |z|^2 behind them
    int32_t first = 0;
    if (l->block_forcings && !l->refine_adj && nvec > 1) LSA_CHECK(rz_forcings_block(ctx, l, Q, nvec, gain, &first));
    for (int32_t c = first; c < nvec; ++c) {
        if (!(gain[c] > 0.0) || !std::isfinite(gain[c]))
            return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent forcings: gain %d is %.3e: no forcing belongs to it", c, gain[c]);
        cplx* q = Q + (size_t)c * (size_t)n;
        LSA_CHECK(rz_response(ctx, l, q, l->tm));
        while (true) {
            const bool refine = l->refine_adj;
            LSA_CHECK(direct_solve_enqueue(ctx, l->op, LSA_C128, l->tm, l->za, l->ca, l->r, refine, l->norms, 1));
            LSA_CHECK(k_residual_norms(ctx, LSA_C128, n, l->tm, l->ca, l->r, norms));
            LSA_CHECK(k_nrm2(ctx, LSA_C128, n, l->za, norms + 2));
            double sums[3];
            LSA_CHECK(lsa_ensure_scratch(ctx, 0, sizeof(sums)));
            LSA_HIP_CHECK(ctx, hipMemcpyAsync(ctx->pinned, norms, sizeof(sums), hipMemcpyDeviceToHost, ctx->stream));
            LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            memcpy(sums, ctx->pinned, sizeof(sums));
            const double res = std::sqrt(sums[0]), bnorm = std::sqrt(sums[1]), xnorm = std::sqrt(sums[2]);
            bool backward = false;
            const int verdict = direct_solve_verdict(l->P, refine, res, bnorm, xnorm, &backward);
            if (verdict == 0) {
                rz_book(l, true, refine, backward, res, bnorm);
                break;
            }
            if (verdict > 0) {
                l->refine_adj = true;
                continue;
            }
            return lsa_set_error(ctx, LSA_ERR_DIVERGED, "lsa_resolvent forcings: the adjoint solve of forcing %d left a relative residual of %.3e after its "
                                                        "refinement step (ksp_rtol %.1e) and a backward error above 1e-12 ||C||_F", c,
                                 bnorm > 0.0 ? res / bnorm : res, l->P.ksp_rtol);
        }
        // f = R^H M q / gain with R = -C^-1
        hipLaunchKernelGGL(rz_scale_kernel, dim3(rz_grid(ctx, n, 8)), dim3(kRzThreads), 0, ctx->stream, n, -1.0 / gain[c], l->za, q);
        LSA_CHECK(lsa_check_launch(ctx, "resolvent forcings"));
    }
    if (nvec == 0) return LSA_OK;
    return lanczos_ritz_to_host(ctx, l->lz, nvec, F);
}

// ---- the operator of a lockstep group: W_z = C_z^-1 Q_f C_z^-H for several frequencies of one sweep in batched launches ---------------
// A member is in while its factors are complex and of the lead's analysis (nd_batch_compatible) and neither direction carries its
// refinement step; the round is rz_hook_enqueue's sequence with one launch where it has one: the adjoint sweeps of all members' factor
// sets (ndlu_solve_run on a batch of sets, trans = 2), C_z^H z_z (k_spmv_transpose_batch), Q_f z_z (k_spmv_batch), the forward sweeps,
// C_z w_z (k_spmv_batch).  Every piece leaves its solo bits per member, and each member's own rz_hook_judge follows the read-back.
namespace {

bool rz_group_eligible(void* self, int32_t z, int32_t lead) {
    lsa_resolvent* const* rs = (lsa_resolvent* const*)self;
    const lsa_resolvent* l = rs[z];
    if (l->P.Kfac->dtype != LSA_C128 || l->refine_adj || l->refine_fwd) return false;
    return lead < 0 || nd_batch_compatible(rs[lead]->P.nd, l->P.nd);
}

int rz_group_enqueue(lsa_ctx* ctx, void* self, int32_t R, const int32_t* idx, const void* const* rhs, void* const* w, void* const* cf,
                     lanczos_check* const* chk, int32_t* launches) {
    lsa_resolvent* const* rs = (lsa_resolvent* const*)self;
    lsa_ndlu* nd[kKrylovGroupMax];
    const lsa_mat *C[kKrylovGroupMax], *Qf[kKrylovGroupMax];
    const void *za_c[kKrylovGroupMax], *tm_c[kKrylovGroupMax], *w_c[kKrylovGroupMax];
    void *za[kKrylovGroupMax], *ca[kKrylovGroupMax], *tm[kKrylovGroupMax];
    for (int32_t r = 0; r < R; ++r) {
        lsa_resolvent* l = rs[idx[r]];
        l->used_adj = l->used_fwd = false;
        nd[r] = l->P.nd;
        C[r] = l->P.Kfac;
        Qf[r] = l->Qf;
        za[r] = l->za, za_c[r] = l->za;
        ca[r] = l->ca;
        tm[r] = l->tm, tm_c[r] = l->tm;
        w_c[r] = w[r];
        ++l->P.st->spmv_calls;
    }
    const NdSolve adj = {R, nd, true, 2, LSA_C128, 1, rhs, 0, za, 0, "lsa_resolvent_extend_batch"};
    LSA_CHECK(ndlu_solve_run(ctx, adj));
    LSA_CHECK(k_spmv_transpose_batch(ctx, R, C, 1, LSA_C128, za_c, ca));
    LSA_CHECK(k_spmv_batch(ctx, R, Qf, LSA_C128, za_c, tm));
    const NdSolve fwd = {R, nd, true, 0, LSA_C128, 1, tm_c, 0, w, 0, "lsa_resolvent_extend_batch"};
    LSA_CHECK(ndlu_solve_run(ctx, fwd));
    LSA_CHECK(k_spmv_batch(ctx, R, C, LSA_C128, w_c, cf));
    for (int32_t r = 0; r < R; ++r) {
        const lsa_resolvent* l = rs[idx[r]];
        chk[r][0].b = rhs[r], chk[r][0].z = l->ca, chk[r][0].refined = false;
        chk[r][1].b = l->tm, chk[r][1].z = cf[r], chk[r][1].refined = false;
    }
    int32_t sweep_launches = 0;
    (void)lsa_ndlu_info(nd[0], nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &sweep_launches, nullptr, nullptr, nullptr);
    *launches += 2 * sweep_launches + 3;
    return LSA_OK;
}

}  // namespace

int resolvent_group_check(lsa_ctx* ctx, const char* who, int32_t J, lsa_resolvent* const* rs) {
    if (J < 1 || J > kKrylovGroupMax) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: J = %d outside [1, %d]", who, J, kKrylovGroupMax);
    if (!rs) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: null argument", who);
    for (int32_t z = 0; z < J; ++z) {
        if (!rs[z]) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: null handle (problem %d)", who, z);
        if (rs[z]->ctx != ctx) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: the handle of problem %d lives in another context", who, z);
        for (int32_t y = 0; y < z; ++y)
            if (rs[y] == rs[z] || rs[y]->op == rs[z]->op) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: problems %d and %d share a handle or an operator", who, y, z);
        if (rs[z]->n != rs[0]->n || rs[z]->ncv != rs[0]->ncv)
            return lsa_set_error(ctx, LSA_ERR_ARG, "%s: problem %d has another shape (n = %lld, ncv = %d) than problem 0 (n = %lld, ncv = %d)", who, z,
                                 (long long)rs[z]->n, rs[z]->ncv, (long long)rs[0]->n, rs[0]->ncv);
        // the batched products take each member's own weights on the index arrays of ONE pattern
        if ((rs[z]->Qf != rs[0]->Qf && !k_spmv_same_pattern(rs[0]->Qf, rs[z]->Qf)) || (rs[z]->Qq != rs[0]->Qq && !k_spmv_same_pattern(rs[0]->Qq, rs[z]->Qq)))
            return lsa_set_error(ctx, LSA_ERR_ARG, "%s: the weights of problem %d have another pattern than those of problem 0: the members of a group may hold "
                                                   "different weights only on one pattern (lsa_csr_window of one M)", who, z);
    }
    return LSA_OK;
}

int resolvent_extend_batch(lsa_ctx* ctx, LanczosGroupBuf* gb, int32_t J, lsa_resolvent* const* rs, const uint8_t* active, const int32_t* j0, int32_t j1,
                           double* const* T, int32_t ldt, int32_t* breakdown, int32_t* status, std::string* errs, lsa_ks_batch_info* info) {
    lsa_lanczos* ls[kKrylovGroupMax];
    for (int32_t z = 0; z < J; ++z) ls[z] = rs[z]->lz;
    const lanczos_group_operator gop{(void*)rs, rz_group_eligible, rz_group_enqueue};
    return lanczos_extend_batch(ctx, gb, ls, &gop, active, j0, j1, T, ldt, breakdown, status, errs, info);
}

// the context's error text: those of all failed problems in problem order, each naming its problem; returns the first non-zero status
int resolvent_group_status(lsa_ctx* ctx, int32_t J, const int32_t* status, const std::string* errs) {
    int first_rc = LSA_OK;
    std::string all;
    for (int32_t z = 0; z < J; ++z)
        if (status[z] != LSA_OK) {
            if (first_rc == LSA_OK) first_rc = status[z];
            else all += "; ";
            all += errs[z];
        }
    if (first_rc != LSA_OK) ctx->err = all;
    return first_rc;
}

int resolvent_group_alloc(lsa_ctx* ctx, int32_t J, lsa_resolvent* const* rs, LanczosGroupBuf* gb) {
    lsa_lanczos* ls[kKrylovGroupMax];
    for (int32_t z = 0; z < J; ++z) ls[z] = rs[z]->lz;
    return lanczos_group_alloc(ctx, J, ls, gb);
}

extern "C" {

int lsa_resolvent_create(lsa_ctx* ctx, lsa_op* op, int32_t ncv, lsa_resolvent** out) {
    if (!ctx || !op || !out || ncv < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_create: bad argument");
    lsa_op_parts P{};
    LSA_CHECK(lsa_op_get_parts(op, &P));
    if (!P.shift_invert) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_create: the operator is not shift-invert (mode 0): C = A - i omega M is what gets factorised");
    if (P.adjoint) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_create: the operator is in adjoint mode (lsa_op_set_adjoint): the iteration picks each solve's direction itself");
    if (P.projected) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_create: the operator is projected (lsa_op_set_projection): a projected operator is not built; "
                                                            "restrict forcing and response with windows instead (lsa_csr_window, lsa_resolvent_set_weights)");
    if (!P.one_rank || ctx->nranks != 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_create: the operator is spread over several ranks: one rank only");
    if (!P.Kmul) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_create: the operator has no M: the gains are measured in the M-inner product");
    if (P.Kmul->dtype != LSA_F64) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_create: M is complex: the M-inner product needs a real symmetric M");
    if (!P.nd || !P.Kfac) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_create: the operator has no exact LU (pc_type 2): both inner solves run on its factors");
    if ((int64_t)ncv > P.n) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_create: ncv = %d exceeds the problem size %lld", ncv, (long long)P.n);
    lsa_resolvent* l = new lsa_resolvent();
    l->ctx = ctx;
    l->op = op;
    l->P = P;
    l->n = P.n;
    l->ncv = ncv;
    l->Qf = l->Qq = P.Kmul;
    l->hook = lanczos_operator{l, 2, rz_hook_enqueue, nullptr, rz_hook_judge};
    int rc = lanczos_create_basis(ctx, op, ncv, LSA_C128, "lsa_resolvent", &l->lz);
    if (rc == LSA_OK) rc = lanczos_set_operator(ctx, l->lz, &l->hook);
    if (rc != LSA_OK) {
        rz_free(l);
        return rc;
    }
    const size_t vb = (size_t)std::max<int64_t>(l->n, 1) * sizeof(cplx);
    bool ok = hipMalloc((void**)&l->norms, 5 * sizeof(double)) == hipSuccess;
    for (cplx** p : {&l->za, &l->ca, &l->tm, &l->r}) ok = ok && hipMalloc((void**)p, vb) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        rz_free(l);
        return lsa_set_error(ctx, LSA_ERR_OOM, "lsa_resolvent_create: out of device memory (n=%lld, ncv=%d)", (long long)P.n, ncv);
    }
    *out = l;
    return LSA_OK;
}

void lsa_resolvent_destroy(lsa_resolvent* l) {
    if (!l) return;
    if (l->ctx && l->ctx->stream) (void)hipStreamSynchronize(l->ctx->stream);
    rz_free(l);
}

int lsa_resolvent_set_row_permutation(lsa_ctx* ctx, lsa_resolvent* l, const int32_t* perm) {
    if (!ctx || !l) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_set_row_permutation: null argument");
    return lsa_lanczos_set_row_permutation(ctx, l->lz, perm);
}

int lsa_resolvent_set_block_forcings(lsa_ctx* ctx, lsa_resolvent* l, int on) {
    if (!ctx || !l) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_set_block_forcings: null argument");
    l->block_forcings = on != 0;
    return LSA_OK;
}

int lsa_resolvent_set_weights(lsa_ctx* ctx, lsa_resolvent* l, const lsa_mat* Qf, const lsa_mat* Qq) {
    if (!ctx || !l) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_set_weights: null argument");
    const lsa_mat* both[2] = {Qf, Qq};
    for (int k = 0; k < 2; ++k) {
        const lsa_mat* Q = both[k];
        const char* which = k == 0 ? "forcing" : "response";
        if (!Q) continue;
        if (Q->dtype != LSA_F64)
            return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_set_weights: the %s weight is complex: a weight is real symmetric positive semidefinite", which);
        if (Q->row0 != 0 || (int64_t)Q->n != l->n || (int64_t)Q->ncols != l->n)
            return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_set_weights: the %s weight is %d x %d (from row %d), the problem has size %lld", which, Q->n,
                                 Q->ncols, Q->row0, (long long)l->n);
    }
    l->Qf = Qf ? Qf : l->P.Kmul;
    l->Qq = Qq ? Qq : l->P.Kmul;
    // other inner products begin as a new handle does: no right-hand side is left over (the basis forgets it), the refinement steps
    // are off again, and a start vector must follow (the basis in hand is orthonormal in the old response weight)
    lanczos_set_inner_product(l->lz, l->Qq);
    l->refine_adj = l->refine_fwd = false;
    return LSA_OK;
}

int lsa_resolvent_set_start(lsa_ctx* ctx, lsa_resolvent* l, const void* host_v) { return resolvent_inject(ctx, l, 0, (const cplx*)host_v); }

int lsa_resolvent_extend(lsa_ctx* ctx, lsa_resolvent* l, int32_t j0, int32_t j1, double* T, int32_t ldt, int32_t* breakdown) {
    if (!ctx || !l || !T) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_extend: null argument");
    return lsa_lanczos_extend(ctx, l->lz, j0, j1, T, ldt, breakdown);
}

int lsa_resolvent_extend_batch(lsa_ctx* ctx, int32_t J, lsa_resolvent* const* rs, const uint8_t* active, const int32_t* j0, int32_t j1, double* const* T,
                               int32_t ldt, int32_t* breakdown, int32_t* status) {
    if (!ctx || !rs || !j0 || !T || !breakdown || !status) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_extend_batch: null argument");
    LSA_CHECK(resolvent_group_check(ctx, "lsa_resolvent_extend_batch", J, rs));
    uint8_t all[kKrylovGroupMax];
    for (int32_t z = 0; z < J; ++z) {
        all[z] = active ? active[z] : 1;
        if (all[z] && !T[z]) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_extend_batch: null T (problem %d)", z);
        status[z] = LSA_OK;
        breakdown[z] = -1;
    }
    LanczosGroupBuf gb;
    std::string errs[kKrylovGroupMax];
    int rc = resolvent_group_alloc(ctx, J, rs, &gb);
    if (rc == LSA_OK) rc = resolvent_extend_batch(ctx, &gb, J, rs, all, j0, j1, T, ldt, breakdown, status, errs, nullptr);
    lanczos_group_free(&gb);
    if (rc != LSA_OK) return rc;
    return resolvent_group_status(ctx, J, status, errs);
}

int lsa_resolvent_basis(lsa_ctx* ctx, const lsa_resolvent* l, int32_t ncols, void* host_V) {
    if (!ctx || !l || !host_V) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_basis: null argument");
    return lsa_lanczos_basis(ctx, l->lz, ncols, (double*)host_V);
}

}  // extern "C"
