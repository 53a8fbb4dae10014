// Device-resident Krylov loops: restarted GMRES (the ST's inner KSP), the shift-invert operator, and the
// Arnoldi recurrences + basis updates that Krylov-Schur needs (EPS.solve of the reference, Solver/utils.py:270).
// Only O(m) scalars per step cross PCIe (one Hessenberg column); vectors never leave HBM.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>

#include "ndlu_internal.h"  // (the solves on the exact LU's factors; esize, now_s, k_allgather_inplace)

int ilu_check_abort(lsa_ctx* ctx, lsa_ilu* pc);

namespace {

using zc = std::complex<double>;

// The switches of the Krylov steps ("Environment knobs"), read once per process.
struct KrylovSwitches {
    bool fused;        // LSA_KRYLOV_FUSED (default on): CGS2 in five launches where the shape allows; off: a kernel per stage
    bool four_passes;  // LSA_KRYLOV_PASSES=4: the per-stage CGS2 takes four passes over the basis instead of three
    bool tail;         // LSA_KRYLOV_TAIL (default on): the tail form of a pipelined step
    bool delayed;      // LSA_KRYLOV_DELAYED (default on): DCGS2 in the pipelined steps
    bool timing;       // LSA_KRYLOV_TIMING set: print queueing and waiting time per batch
    bool preapply;     // LSA_KRYLOV_PREAPPLY (default on): queueing ahead -- the next batch (or the flush) before a batch is read back, the next
                       // cycle's first inner solve under the host's Schur form, and a restart between them that does not wait for the stream
};
const KrylovSwitches& krylov_switches() {
    static const KrylovSwitches sw = [] {
        const char* passes = getenv("LSA_KRYLOV_PASSES");
        return KrylovSwitches{env_flag("LSA_KRYLOV_FUSED", true), passes && atoi(passes) == 4, env_flag("LSA_KRYLOV_TAIL", true),
                              env_flag("LSA_KRYLOV_DELAYED", true), getenv("LSA_KRYLOV_TIMING") != nullptr, env_flag("LSA_KRYLOV_PREAPPLY", true)};
    }();
    return sw;
}

// small device arrays used by the orthogonalisation (sized for `cap` basis vectors)
struct OrthWork {
    void *h1 = nullptr, *h2 = nullptr, *hcol = nullptr;
    double* nrm2 = nullptr;
    void* fused = nullptr;  // workspace of the five-launch CGS2 (k_cgs2_fused), allocated on first use
    int cap = 0;
    int ensure_fused(lsa_ctx* ctx, int64_t n) {
        if (fused) return LSA_OK;
        LSA_HIP_ALLOC(ctx, hipMalloc(&fused, k_cgs2_fused_work_bytes(ctx, n, cap)));
        return LSA_OK;
    }
    int alloc(lsa_ctx* ctx, int cap_, int dtype) {
        cap = cap_;
        const size_t b = (size_t)(cap + 2) * esize(dtype);
        LSA_HIP_CHECK(ctx, hipMalloc(&h1, b));
        LSA_HIP_CHECK(ctx, hipMalloc(&h2, b));
        LSA_HIP_CHECK(ctx, hipMalloc(&hcol, b));
        LSA_HIP_CHECK(ctx, hipMalloc((void**)&nrm2, 4 * sizeof(double)));
        return LSA_OK;
    }
    void release() {
        for (void* p : {h1, h2, hcol, (void*)nrm2, fused})
            if (p) (void)hipFree(p);
        h1 = h2 = hcol = fused = nullptr;
        nrm2 = nullptr;
    }
};

// the check of an inner solve that rides along with an orthogonalisation: out[0..2] = |b - z|^2, |b|^2 (r takes b - z where the
// check is a kernel of its own)
struct SolveCheck {
    const void *b, *z;
    void* r;
    double* out;
};

// the device part of CGS2: orthogonalise w against V[:, 0:j] and normalise into vnext; the j+1 Hessenberg entries go to
// `hcol_dev`, nothing is read back.  Five launches where the switches and the shape allow it, else a kernel per stage with
// three passes over the basis where k_multi_axpy_dot takes the shape, else four: the two fallbacks are selected by size.
int orthonormalize_enqueue(lsa_ctx* ctx, int dtype, int64_t n, const void* V, int64_t ldv, int j, void* w, void* vnext, OrthWork& ow,
                           void* hcol_dev, const SolveCheck* chk = nullptr) {
    const KrylovSwitches& sw = krylov_switches();
    if (sw.fused) {  // (the check rides in the first reduction)
        LSA_CHECK(ow.ensure_fused(ctx, n));
        const int frc = k_cgs2_fused(ctx, dtype, n, j, V, ldv, w, vnext, hcol_dev, ow.fused, chk ? chk->b : nullptr, chk ? chk->z : nullptr,
                                     chk ? chk->out : nullptr);
        if (frc <= 0) return frc;
    }
    if (chk) LSA_CHECK(k_residual_norms(ctx, dtype, n, chk->b, chk->z, chk->r, chk->out));
    LSA_CHECK(k_multi_dot(ctx, dtype, n, j, V, ldv, w, ow.h1));
    // long vectors: the first projection and the second dot product share one pass over the basis (three passes instead of four)
    const int arc = sw.four_passes ? 1 : k_multi_axpy_dot(ctx, dtype, n, j, V, ldv, ow.h1, w, ow.h2);
    if (arc < 0) return arc;
    if (arc > 0) {
        LSA_CHECK(k_multi_axpy(ctx, dtype, n, j, V, ldv, ow.h1, w, nullptr));
        LSA_CHECK(k_multi_dot(ctx, dtype, n, j, V, ldv, w, ow.h2));
    }
    LSA_CHECK(k_multi_axpy(ctx, dtype, n, j, V, ldv, ow.h2, w, ow.nrm2));
    LSA_CHECK(k_hess_column(ctx, dtype, j, ow.h1, ow.h2, ow.nrm2, hcol_dev));
    LSA_CHECK(k_scale_by_inv_norm(ctx, dtype, n, w, ow.nrm2, vnext));
    return LSA_OK;
}

// CGS2 with the Hessenberg entries brought to the host as complex numbers (real dtype is widened).  One stream
// synchronisation.
int orthonormalize(lsa_ctx* ctx, int dtype, int64_t n, const void* V, int64_t ldv, int j, void* w, void* vnext,
                   OrthWork& ow, zc* h_host) {
    LSA_CHECK(orthonormalize_enqueue(ctx, dtype, n, V, ldv, j, w, vnext, ow, ow.hcol));
    const size_t bytes = (size_t)(j + 1) * esize(dtype);
    LSA_CHECK(lsa_ensure_scratch(ctx, 0, bytes));
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(ctx->pinned, ow.hcol, bytes, hipMemcpyDeviceToHost, ctx->stream));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (dtype == LSA_C128) {
        const cplx* p = (const cplx*)ctx->pinned;
        for (int c = 0; c <= j; ++c) h_host[c] = zc(p[c].re, p[c].im);
    } else {
        const double* p = (const double*)ctx->pinned;
        for (int c = 0; c <= j; ++c) h_host[c] = zc(p[c], 0.0);
    }
    return LSA_OK;
}

int device_norm(lsa_ctx* ctx, int dtype, int64_t n, const void* x, double* nrm2_dev, double* out) {
    LSA_CHECK(k_nrm2(ctx, dtype, n, x, nrm2_dev));
    LSA_CHECK(lsa_ensure_scratch(ctx, 0, sizeof(double)));
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(ctx->pinned, nrm2_dev, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *out = std::sqrt(*(const double*)ctx->pinned);
    return LSA_OK;
}

// upload a small host array of complex numbers as `dtype`
int upload_small(lsa_ctx* ctx, int dtype, const zc* src, size_t count, void* dst) {
    LSA_CHECK(lsa_ensure_scratch(ctx, 0, count * 16));
    if (dtype == LSA_C128) {
        cplx* p = (cplx*)ctx->pinned;
        for (size_t i = 0; i < count; ++i) p[i] = cplx{src[i].real(), src[i].imag()};
    } else {
        double* p = (double*)ctx->pinned;
        for (size_t i = 0; i < count; ++i) p[i] = src[i].real();
    }
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(dst, ctx->pinned, count * esize(dtype), hipMemcpyHostToDevice, ctx->stream));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // pinned buffer is reused
    return LSA_OK;
}

// y = A x for a (possibly row-sharded) matrix; x and y are global-length vectors replicated on every rank: the
// shard writes its own rows, then the equal-sized padded blocks are exchanged with one in-place all-gather
int spmv_global(lsa_ctx* ctx, const lsa_mat* A, int dtype, const void* x, void* y, bool adjoint = false) {
    // y = A^H x with the whole matrix (lsa_op_set_adjoint sees to that on every rank); the pull-form product is reproducible bit for
    // bit, so the ranks' replicated vectors stay alike without an exchange
    if (adjoint) return k_spmv_transpose(ctx, A, 1, dtype, x, y);
    const size_t es = esize(dtype);
    LSA_CHECK(k_spmv(ctx, A, dtype, x, (char*)y + (size_t)A->row0 * es));
    // (a whole square matrix was multiplied on every rank: nothing to exchange)
    if (ctx->nranks > 1 && A->n != A->ncols) LSA_CHECK(k_allgather_inplace(ctx, y, (size_t)(A->ncols / ctx->nranks) * es));
    return LSA_OK;
}

// x = P^-1 b: block-Jacobi over ranks (each rank holds the ILU(k) of its diagonal block), then all-gather
struct PcRef {
    lsa_ilu* ilu = nullptr;  // ILU(k) + triangular solves
    lsa_ndlu* nd = nullptr;  // exact nested-dissection multifrontal LU
    bool nd_dist = false;    // the subtree-parallel form: reads and writes whole replicated vectors
    bool adjoint = false;    // solve with C^H on the same factors (nd only)
    double normF = 0.0;      // ||C||_F when known: lets a direct solve be judged by its backward error
    explicit operator bool() const { return ilu || nd; }
    bool exact() const { return nd != nullptr; }
};

int pc_global(lsa_ctx* ctx, PcRef pc, int32_t row0, int64_t nglobal, int dtype, const void* b, void* x) {
    const size_t es = esize(dtype);
    const char* bl = (const char*)b + (size_t)row0 * es;
    char* xl = (char*)x + (size_t)row0 * es;
    if (pc.nd && pc.adjoint) LSA_CHECK(ndlu_solve_adjoint_dev(ctx, pc.nd, 1, dtype, pc.nd_dist ? b : bl, pc.nd_dist ? x : xl));
    else if (pc.nd && pc.nd_dist) LSA_CHECK(ndlu_solve_dev(ctx, pc.nd, dtype, b, x));  // own subtrees + replicated top; x completed below
    else if (pc.nd) LSA_CHECK(ndlu_solve_dev(ctx, pc.nd, dtype, bl, xl));
    else LSA_CHECK(ilu_solve_dev(ctx, pc.ilu, 2, dtype, bl, xl));
    if (ctx->nranks > 1) LSA_CHECK(k_allgather_inplace(ctx, x, (size_t)(nglobal / ctx->nranks) * es));
    return LSA_OK;
}

struct GmresWork {
    int dtype = LSA_C128;
    int64_t n = 0;
    int restart = 0;
    void *V = nullptr, *w = nullptr, *z = nullptr, *ydev = nullptr;
    OrthWork ow;
    std::vector<zc> H, cs, sn, g, y, hcol;
    int alloc(lsa_ctx* ctx, int64_t n_, int restart_, int dtype_) {
        n = n_;
        restart = restart_;
        dtype = dtype_;
        const size_t vb = (size_t)std::max<int64_t>(n, 1) * esize(dtype);
        // (the basis itself is allocated when an iteration actually starts: behind an exact LU solve that is the exception,
        //  and 41 vectors are 330 MB at 500 k unknowns, per operator, i.e. per solve)
        LSA_HIP_CHECK(ctx, hipMalloc(&w, vb));
        LSA_HIP_CHECK(ctx, hipMalloc(&z, vb));
        // shards write only their own rows: the padding rows of the block layout must read as zero
        LSA_HIP_CHECK(ctx, hipMemsetAsync(w, 0, vb, ctx->stream));
        LSA_HIP_CHECK(ctx, hipMemsetAsync(z, 0, vb, ctx->stream));
        LSA_HIP_CHECK(ctx, hipMalloc(&ydev, (size_t)(restart + 2) * esize(dtype)));
        LSA_CHECK(ow.alloc(ctx, restart + 1, dtype));
        H.assign((size_t)(restart + 1) * restart, zc(0));
        cs.assign(restart + 1, zc(0));
        sn.assign(restart + 1, zc(0));
        g.assign(restart + 2, zc(0));
        y.assign(restart + 1, zc(0));
        hcol.assign(restart + 2, zc(0));
        return LSA_OK;
    }
    int ensure_basis(lsa_ctx* ctx) {
        if (V) return LSA_OK;
        const size_t vb = (size_t)std::max<int64_t>(n, 1) * esize(dtype);
        LSA_HIP_ALLOC(ctx, hipMalloc(&V, vb * (size_t)(restart + 1)));
        return LSA_OK;
    }
    void release() {
        for (void* p : {V, w, z, ydev})
            if (p) (void)hipFree(p);
        V = w = z = ydev = nullptr;
        ow.release();
    }
};

// right-preconditioned restarted GMRES on the device; x0 = x when use_x0, else 0
int gmres_run(lsa_ctx* ctx, const lsa_mat* C, PcRef pc, int dtype, const void* b, void* x, bool use_x0, double rtol,
              int maxit, GmresWork& W, int32_t* iters_out, double* relres_out, lsa_stats* st) {
    const int64_t n = W.n;
    const int m = W.restart;
    const size_t vb = (size_t)n * esize(dtype);
    auto col = [&](int j) { return (void*)((char*)W.V + (size_t)j * vb); };
    double bnorm = 0.0;
    double beta0 = -1.0;  // ||b - C x|| of the first cycle when it was computed together with ||b||
    int total = 0;
    double relres = 0.0;
    if (pc.exact() && !use_x0) {
        // exact (LU) preconditioner: x = P^-1 b is already the solution on one GPU; the loop below then only
        // checks b - C x and iterates on the residual when the factors are block-Jacobi over ranks.  The check and
        // ||b|| come from one fused pass and one stream synchronisation.
        LSA_CHECK(pc_global(ctx, pc, C->row0, n, dtype, b, x));
        if (st) st->sptrsv_calls += 2;
        LSA_CHECK(spmv_global(ctx, C, dtype, x, W.z, pc.adjoint));
        if (st) ++st->spmv_calls;
        LSA_CHECK(k_residual_norms(ctx, dtype, n, b, W.z, W.w, W.ow.nrm2));
        LSA_CHECK(lsa_ensure_scratch(ctx, 0, 2 * sizeof(double)));
        LSA_HIP_CHECK(ctx, hipMemcpyAsync(ctx->pinned, W.ow.nrm2, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        beta0 = std::sqrt(((const double*)ctx->pinned)[0]);
        bnorm = std::sqrt(((const double*)ctx->pinned)[1]);
        use_x0 = true;
        // Iterative refinement before any looser judgement: the residual b - C x is on the device already (W.w), one more
        // pair of sweeps and one product give x += C^-1 (b - C x).  Large 3D factorisations leave ||b - C x|| / ||b|| at 1e-11
        // (growth over tens of thousands of pivots per front); one step brings that to rounding level.  Repeated while it
        // helps (at most twice); what is left after that is the conditioning of C itself (a shift next to an eigenvalue).
        for (int pass = 0; pass < 2 && beta0 > rtol * bnorm && std::isfinite(beta0) && bnorm > 0.0; ++pass) {
            LSA_CHECK(pc_global(ctx, pc, C->row0, n, dtype, W.w, W.z));
            const double one[2] = {1.0, 0.0};
            LSA_CHECK(k_axpy(ctx, dtype, n, one, W.z, x));
            LSA_CHECK(spmv_global(ctx, C, dtype, x, W.z, pc.adjoint));
            LSA_CHECK(k_residual_norms(ctx, dtype, n, b, W.z, W.w, W.ow.nrm2));
            LSA_HIP_CHECK(ctx, hipMemcpyAsync(ctx->pinned, W.ow.nrm2, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            const double before = beta0;
            beta0 = std::sqrt(((const double*)ctx->pinned)[0]);
            if (st) {
                st->sptrsv_calls += 2;
                ++st->spmv_calls;
                if (pass == 0) ++st->refined_solves;
            }
            if (!(beta0 < 0.5 * before)) break;  // no longer helping: x is as good as these factors make it
        }
        if (beta0 > rtol * bnorm && pc.normF > 0.0 && std::isfinite(beta0)) {
            // A direct solve is judged by its backward error.  For a shift next to an eigenvalue ||x|| >> ||b|| / ||C|| and
            // ||b - C x|| / ||b|| cannot go below eps ||C|| ||x|| / ||b||, whatever the solver (the reference shifts the
            // adjoint problem exactly at a converged eigenvalue, Sensitivity/__init__.py:260-262).  x is accepted when it
            // solves a system within 1e-12 ||C||_F of C exactly; GMRES could not improve on that.
            double xnorm = 0.0;
            LSA_CHECK(device_norm(ctx, dtype, n, x, W.ow.nrm2, &xnorm));
            if (beta0 <= 1e-12 * pc.normF * xnorm) {
                if (st) {
                    ++st->backward_accepted;
                    st->last_rel_res = beta0 / bnorm;
                    st->max_rel_res = std::max(st->max_rel_res, beta0 / bnorm);  // (reported as it is: the Python layer warns above 10 rtol)
                }
                if (iters_out) *iters_out = 0;
                if (relres_out) *relres_out = beta0 / bnorm;
                return LSA_OK;
            }
        }
    } else {
        LSA_CHECK(device_norm(ctx, dtype, n, b, W.ow.nrm2, &bnorm));
    }
    if (!std::isfinite(bnorm)) return lsa_set_error(ctx, LSA_ERR_NONFINITE, "GMRES: right-hand side is not finite");
    if (!use_x0) LSA_CHECK(k_set_zero(ctx, dtype, n, x));
    if (bnorm == 0.0) {
        LSA_CHECK(k_set_zero(ctx, dtype, n, x));
        if (iters_out) *iters_out = 0;
        if (relres_out) *relres_out = 0.0;
        return LSA_OK;
    }
    bool converged = false;
    bool first_cycle = true;
    int verified_cycles = 0;  // cycles that ended on the recurrence estimate and were then checked against b - C x
    bool pending = false;     // a cycle claimed convergence; the claim still has to be checked
    double last_verified = 1e300;
    while (!converged && (total < maxit || pending)) {
        // r = b - C x  -> w
        if (beta0 >= 0.0) {
            // already in W.w
        } else if (first_cycle && !use_x0) {
            LSA_CHECK(k_copy(ctx, dtype, n, b, W.w));
        } else {
            LSA_CHECK(spmv_global(ctx, C, dtype, x, W.z, pc.adjoint));
            if (st) ++st->spmv_calls;
            LSA_CHECK(k_copy(ctx, dtype, n, b, W.w));
            const double minus1[2] = {-1.0, 0.0};
            LSA_CHECK(k_axpy(ctx, dtype, n, minus1, W.z, W.w));
        }
        first_cycle = false;
        double beta = beta0;
        if (beta0 < 0.0) LSA_CHECK(device_norm(ctx, dtype, n, W.w, W.ow.nrm2, &beta));
        beta0 = -1.0;
        if (!std::isfinite(beta)) return lsa_set_error(ctx, LSA_ERR_NONFINITE, "GMRES: residual is not finite");
        relres = beta / bnorm;
        pending = false;
        // The true residual decides.  After a cycle that claimed convergence, accept the rounding floor of b - C x:
        // for a shift close to an eigenvalue ||x|| >> ||b|| / ||C|| and the attainable ||r|| / ||b|| is
        // eps * ||C|| ||x|| / ||b||, above a tight rtol.  A residual that no longer halves from one verified cycle to
        // the next has reached that floor (a direct solver does no better); it is reported through the statistics.
        if (relres <= rtol || (verified_cycles > 0 && relres <= 10.0 * rtol)) {
            converged = true;
            break;
        }
        if (verified_cycles >= 2 && relres > 0.5 * last_verified) {
            // stagnation at the rounding floor of b - C x.  Accepted within 1000 rtol (reported through max_rel_res and
            // the stagnation counter, which the Python layer turns into a warning); anything looser is a failed solve.
            converged = relres <= 1e3 * rtol;
            if (converged && st) ++st->stagnated_solves;
            break;
        }
        if (verified_cycles > 0) last_verified = relres;
        LSA_CHECK(W.ensure_basis(ctx));
        LSA_CHECK(k_scale_by_inv_norm(ctx, dtype, n, W.w, W.ow.nrm2, col(0)));
        std::fill(W.g.begin(), W.g.end(), zc(0));
        W.g[0] = zc(beta, 0);
        int jj = 0;
        for (int j = 0; j < m && total < maxit; ++j) {
            const void* vj = col(j);
            const void* src = vj;
            if (pc) {
                LSA_CHECK(pc_global(ctx, pc, C->row0, n, dtype, vj, W.z));
                if (st) st->sptrsv_calls += 2;
                src = W.z;
            }
            LSA_CHECK(spmv_global(ctx, C, dtype, src, W.w, pc.adjoint));
            if (st) ++st->spmv_calls;
            LSA_CHECK(orthonormalize(ctx, dtype, n, W.V, n, j + 1, W.w, col(j + 1), W.ow, W.hcol.data()));
            ++total;
            zc* Hj = &W.H[(size_t)j * (m + 1)];
            for (int i = 0; i <= j + 1; ++i) Hj[i] = W.hcol[i];
            if (!std::isfinite(Hj[j + 1].real())) {
                if (pc.ilu) LSA_CHECK(ilu_check_abort(ctx, pc.ilu));
                return lsa_set_error(ctx, LSA_ERR_NONFINITE, "GMRES: non-finite Hessenberg entry at iteration %d", total);
            }
            for (int i = 0; i < j; ++i) {
                const zc t = std::conj(W.cs[i]) * Hj[i] + std::conj(W.sn[i]) * Hj[i + 1];
                Hj[i + 1] = -W.sn[i] * Hj[i] + W.cs[i] * Hj[i + 1];
                Hj[i] = t;
            }
            // rotation that zeroes Hj[j+1]
            const double a = std::abs(Hj[j]), bb = std::abs(Hj[j + 1]);
            const double rr = std::hypot(a, bb);
            if (rr == 0.0) {
                W.cs[j] = zc(1);
                W.sn[j] = zc(0);
            } else {
                W.cs[j] = Hj[j] / rr;
                W.sn[j] = Hj[j + 1] / rr;
            }
            Hj[j] = std::conj(W.cs[j]) * Hj[j] + std::conj(W.sn[j]) * Hj[j + 1];
            Hj[j + 1] = zc(0);
            W.g[j + 1] = -W.sn[j] * W.g[j];
            W.g[j] = std::conj(W.cs[j]) * W.g[j];
            jj = j + 1;
            relres = std::abs(W.g[j + 1]) / bnorm;
            if (relres <= rtol) {  // recurrence estimate: verified against b - C x at the top of the next cycle
                ++verified_cycles;
                pending = true;
                break;
            }
        }
        // y = R^-1 g ;  x += P^-1 (V y)
        for (int i = jj - 1; i >= 0; --i) {
            zc s = W.g[i];
            for (int k = i + 1; k < jj; ++k) s -= W.H[(size_t)k * (m + 1) + i] * W.y[k];
            W.y[i] = s / W.H[(size_t)i * (m + 1) + i];
        }
        if (jj > 0) {
            LSA_CHECK(upload_small(ctx, dtype, W.y.data(), (size_t)jj, W.ydev));
            LSA_CHECK(k_basis_gemm(ctx, dtype, n, jj, 1, W.V, n, W.ydev, jj, W.w, n));
            const double one[2] = {1.0, 0.0};
            if (pc) {
                LSA_CHECK(pc_global(ctx, pc, C->row0, n, dtype, W.w, W.z));
                if (st) st->sptrsv_calls += 2;
                LSA_CHECK(k_axpy(ctx, dtype, n, one, W.z, x));
            } else {
                LSA_CHECK(k_axpy(ctx, dtype, n, one, W.w, x));
            }
        }
    }
    if (pc.ilu) LSA_CHECK(ilu_check_abort(ctx, pc.ilu));
    if (iters_out) *iters_out = total;
    if (relres_out) *relres_out = relres;
    if (st) {
        st->gmres_iters += total;
        st->last_rel_res = relres;
        st->max_rel_res = std::max(st->max_rel_res, relres);
    }
    if (!converged)
        return lsa_set_error(ctx, LSA_ERR_DIVERGED, "GMRES did not reach rtol %.1e in %d iterations (relative residual %.3e)", rtol,
                             total, relres);
    return LSA_OK;
}

template <typename T>
__global__ void shift_diag_kernel(int32_t n, int32_t row0, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                  T* __restrict__ val, cplx shift, int32_t* __restrict__ missing) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int32_t target = (int32_t)i + row0;
        int32_t lo = rp[i], hi = rp[i + 1];
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (ci[mid] < target) lo = mid + 1;
            else hi = mid;
        }
        if (lo < rp[i + 1] && ci[lo] == target) {
            cplx v = to_cplx(val[lo]);
            s_from(val[lo], v.re - shift.re, v.im - shift.im);
        } else {
            atomicAdd(missing, 1);
        }
    }
}

}  // namespace

// ---- objects ------------------------------------------------------------------------------------------------------
static_assert(sizeof(lsa_op_options) == 56, "lsa_op_options layout is part of the C-ABI (tests/test_abi.py)");

// the caller's elimination forest for the subtree-parallel factorisation (lsa_op_create_dist)
struct TreeArg {
    int32_t nt;
    const int32_t *first, *size, *parent, *owner;
    int32_t row0, row1;  // this rank's rows of the padded layout
};

struct lsa_op {
    lsa_ctx* ctx;
    int64_t n;
    const lsa_mat* Kmul;  // y = Kfac^-1 (Kmul x); either may be null (identity)
    const lsa_mat* Kfac;
    lsa_mat* owned;       // the matrix built here (C = A - sigma M), destroyed with the operator
    lsa_mat* owned_mul = nullptr;  // Cayley: A + nu M
    lsa_mat* owned_diag;  // sharded layout: this rank's diagonal block of C (input of the block-Jacobi ILU)
    lsa_ilu* pc;
    lsa_ndlu* nd = nullptr;  // exact nested-dissection LU (opts.pc_type == 2)
    bool nd_dist = false;    // ... subtree-parallel over the ranks: works on whole replicated vectors
    bool adjoint = false;    // y = Kfac^-H Kmul^H x on the same factors (lsa_op_set_adjoint)
    double normF = 0.0;      // ||Kfac||_F
    double sigma[2] = {0.0, 0.0};  // the shift the operator was built at
    lsa_mat *view_fac = nullptr, *view_mul = nullptr;  // this rank's rows of the whole matrices (subtree-parallel layout)
    const lsa_mat* M_whole = nullptr;                  // the caller's M (modes 0 and 2)
    lsa_op_options opts;
    GmresWork gw;
    bool gw_ready;
    void* t;  // device temp vector (complex)
    double* keep = nullptr;  // device 0/1 mask of the projected operator (lsa_op_set_projection), or null
    bool refine = false;     // queued Arnoldi steps carry one step of iterative refinement (set the first time a direct solve misses rtol)
    lsa_stats st;
};

static PcRef pc_of(const lsa_op* op) {
    PcRef pc;
    pc.ilu = op->pc;
    pc.nd = op->nd;
    pc.nd_dist = op->nd_dist;
    pc.adjoint = op->adjoint;
    pc.normF = op->normF;
    return pc;
}

struct lsa_krylov {
    lsa_ctx* ctx;
    lsa_op* op;
    int64_t n;
    int32_t ncv;
    int32_t* row_perm = nullptr;  // device: row i of the basis is unknown row_perm[i] of the caller (lsa_krylov_set_row_permutation)
    void *V, *V2, *w, *qdev;
    OrthWork ow;
    std::vector<zc> hcol;
    // pipelined Arnoldi steps (exact inner solves): Hessenberg columns and the b - C x checks of a batch of steps stay on
    // the device until the batch is read back with one synchronisation
    double* imag2 = nullptr;         // device: sum Im^2 of the columns of the last canonical Ritz vectors
    void* xtmp = nullptr;            // device: the Ritz vectors in the caller's row order (ncv + 1 columns), allocated on first use
    std::vector<double> imag_norms;  // ... their square roots on the host (lsa_krylov_imag_norms)
    void* Hdev = nullptr;      // two sets of max(batch, 1) slots of 2 ncv + 4 complex: a Hessenberg column (CGS2) or a, b, nu, c, ||w|| (DCGS2)
    double* checks = nullptr;  // two sets of max(batch, 1) x 2: ||b - C x||^2, ||b||^2
    int32_t batch = 0;
    bool pipeline = false;  // the pipelined path may run (false after a solve needed the one-step path's judgement)
    // tail form of a pipelined step (k_cgs2_fused_tail): the step's last launch also multiplies t = M v_{j+1} for the next step
    // and leaves the pairs of this step's check of the inner solve; w2 takes the orthogonalised vector (w keeps the solve's result)
    void* w2 = nullptr;
    double* tail_parts = nullptr;  // two sets of batch x tail_nparts pairs
    int32_t tail_nparts = 0;
    int32_t t_for = -1;            // op->t holds M v_j for this j (valid inside one lsa_krylov_extend call), -1: nothing
    // The apply queued ahead of a restart (krylov_preapply): op->t = M v and w = C^-1 op->t of v = V[:, pre_col], which the restart
    // copies to column pre_for, the first step of the next lsa_krylov_extend.  Written by pre_op; dropped by whatever else writes
    // w or op->t, and at the latest by the next expansion, which takes it or not.
    bool pre_armed = false;  // the solve loop wants the apply queued behind the flush of a full expansion
    int32_t pre_col = -1, pre_for = -1;
    const lsa_op* pre_op = nullptr;
    void drop_preapply() { pre_col = pre_for = -1; }
    hipEvent_t ev_read[2] = {nullptr, nullptr};  // the end of the read-back of either set of slots (queueing ahead)
    int ensure_events(lsa_ctx* ctx_) {
        for (hipEvent_t& e : ev_read)
            if (!e) LSA_HIP_CHECK(ctx_, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return LSA_OK;
    }
};

// bytes of one step's slot in Hdev: a CGS2 Hessenberg column (ncv + 2 entries) or DCGS2's a, b, nu, c, ||w|| (2 ncv + 3)
static size_t krylov_slot_bytes(int32_t ncv) { return (size_t)(2 * ncv + 4) * 16; }

static void krylov_free(lsa_krylov* k) {
    for (void* p : {k->V, k->V2, k->w, k->qdev, k->Hdev, (void*)k->checks, (void*)k->imag2, k->xtmp, (void*)k->row_perm, k->w2, (void*)k->tail_parts})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : k->ev_read)
        if (e) (void)hipEventDestroy(e);
    k->ow.release();
    delete k;
}

extern "C" {

int lsa_gmres(lsa_ctx* ctx, const lsa_mat* C, lsa_ilu* pc, const lsa_vec* b, lsa_vec* x, int use_x0, double rtol, int restart,
              int maxit, int32_t* iters, double* rel_res) {
    if (!ctx || !C || !b || !x) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_gmres: null argument");
    if (C->n != C->ncols || b->n != C->n || x->n != C->n || b->dtype != x->dtype)
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_gmres: shape/dtype mismatch");
    if (C->dtype == LSA_C128 && b->dtype != LSA_C128) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_gmres: complex matrix needs complex vectors");
    if (restart < 1 || maxit < 1 || !(rtol > 0.0)) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_gmres: restart, maxit, rtol must be positive");
    restart = std::min(restart, maxit);
    if (restart > k_basis_gemm_max_cols(b->dtype))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_gmres: restart=%d, the basis product handles at most %d basis vectors", restart, k_basis_gemm_max_cols(b->dtype));
    GmresWork W;
    int rc = W.alloc(ctx, C->n, restart, b->dtype);
    PcRef pcr;
    pcr.ilu = pc;
    if (rc == LSA_OK) rc = gmres_run(ctx, C, pcr, b->dtype, b->d, x->d, use_x0 != 0, rtol, maxit, W, iters, rel_res, nullptr);
    (void)hipStreamSynchronize(ctx->stream);
    W.release();
    return rc;
}

// C = A - sigma M on the shared pattern (M null: A - sigma I through a diagonal shift); rows may be a shard
static int build_shifted(lsa_ctx* ctx, const lsa_mat* A, const lsa_mat* M, const double sigma[2], bool cdt, lsa_mat** out) {
    const bool zshift = sigma[0] == 0.0 && sigma[1] == 0.0;
    const double one[2] = {1.0, 0.0}, ms[2] = {-sigma[0], -sigma[1]}, zero[2] = {0.0, 0.0};
    lsa_mat* C = nullptr;
    int rc;
    if (M) rc = lsa_csr_axpby(ctx, A, M, one, ms, cdt ? LSA_C128 : LSA_F64, &C);
    else {
        rc = lsa_csr_axpby(ctx, A, A, one, zero, cdt ? LSA_C128 : LSA_F64, &C);
        if (rc == LSA_OK && !zshift) {
            int32_t* miss = (int32_t*)ctx->dscratch;
            (void)hipMemsetAsync(miss, 0, sizeof(int32_t), ctx->stream);
            const int blocks = std::max(1, std::min((int)((C->n + 255) / 256), ctx->num_cu * 8));
            if (cdt) hipLaunchKernelGGL((shift_diag_kernel<cplx>), dim3(blocks), dim3(256), 0, ctx->stream, C->n, C->row0, C->rp, C->ci, (cplx*)C->val, cplx{sigma[0], sigma[1]}, miss);
            else hipLaunchKernelGGL((shift_diag_kernel<double>), dim3(blocks), dim3(256), 0, ctx->stream, C->n, C->row0, C->rp, C->ci, (double*)C->val, cplx{sigma[0], sigma[1]}, miss);
            int32_t hm = 0;
            (void)hipMemcpyAsync(&hm, miss, sizeof hm, hipMemcpyDeviceToHost, ctx->stream);
            if (hipStreamSynchronize(ctx->stream) != hipSuccess) rc = lsa_set_error(ctx, LSA_ERR_HIP, "diagonal shift failed");
            else if (hm != 0) rc = lsa_set_error(ctx, LSA_ERR_ARG, "A - sigma*I needs a structurally present diagonal (%d rows have none)", hm);
        }
    }
    if (rc != LSA_OK) {
        if (C) lsa_mat_destroy(C);
        return rc;
    }
    *out = C;
    return LSA_OK;
}

// shared builder: (A, M) are the full matrices or this rank's row shards; (Ad, Md) are null or the rank's diagonal blocks
static int op_build(lsa_ctx* ctx, const lsa_mat* A, const lsa_mat* M, const lsa_mat* Ad, const lsa_mat* Md, const double sigma[2],
                    int mode, const lsa_op_options* opts, lsa_op** out, const TreeArg* tree = nullptr) {
    if (!ctx || !A || !sigma || !opts || !out) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_create: null argument");
    const bool sharded = Ad != nullptr;
    if (tree) {
        const int nr = std::max(1, ctx->nranks);
        if (sharded || A->n != A->ncols || A->row0 != 0 || (mode != 0 && mode != 2) || opts->pc_type != 2)
            return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_create_dist: needs the whole square matrices, a factorising mode (0 or 2) and pc_type 2");
        if (A->ncols % nr != 0 || tree->row0 != (int64_t)ctx->rank * (A->ncols / nr) || tree->row1 < tree->row0 || tree->row1 > tree->row0 + A->ncols / nr)
            return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_create_dist: this rank's rows do not sit on its block of the padded layout");
    }
    if (!sharded && A->n != A->ncols) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_create: A must be square (got %d x %d)", A->n, A->ncols);
    if (M && (M->n != A->n || M->ncols != A->ncols || M->row0 != A->row0)) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_create: M does not match A's shape");
    if (mode < 0 || mode > 2) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_create: mode must be 0 (sinvert), 1 (shift) or 2 (Cayley)");
    if (sharded) {
        if (Ad->n != Ad->ncols || Ad->n != A->n || (Md && (Md->n != Ad->n || Md->ncols != Ad->ncols)) || (M != nullptr) != (Md != nullptr))
            return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_create_sharded: diagonal blocks must be square with the shard's row count");
        if (A->ncols % std::max(1, ctx->nranks) != 0 || A->row0 != (int64_t)ctx->rank * (A->ncols / std::max(1, ctx->nranks)))
            return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_create_sharded: shard does not sit on this rank's block of the padded layout");
        if (A->n > A->ncols / std::max(1, ctx->nranks)) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_create_sharded: shard larger than its padded block");
    }
    const double t0 = now_s();
    lsa_op* op = new lsa_op();
    op->ctx = ctx;
    op->n = A->ncols;  // vectors are global-length (padded block layout when sharded)
    op->Kmul = op->Kfac = nullptr;
    op->owned = op->owned_diag = nullptr;
    op->pc = nullptr;
    op->opts = *opts;
    op->sigma[0] = sigma[0];
    op->sigma[1] = sigma[1];
    op->gw_ready = false;
    op->t = nullptr;
    memset(&op->st, 0, sizeof op->st);
    const bool zshift = sigma[0] == 0.0 && sigma[1] == 0.0;
    const bool cdt = sigma[1] != 0.0 || A->dtype == LSA_C128 || (M && M->dtype == LSA_C128);
    int rc = LSA_OK;
    lsa_mat* C = nullptr;
    if (!(mode == 1 && zshift)) {
        rc = build_shifted(ctx, A, M, sigma, cdt, &C);
        if (rc != LSA_OK) {
            delete op;
            return rc;
        }
        op->owned = C;
    }
    const lsa_mat* fac_src = nullptr;  // the square matrix the preconditioner is built from
    if (mode == 0 || mode == 2) {
        op->Kfac = C;
        op->Kmul = M;
        op->M_whole = M;
        // Subtree-parallel layout: every rank holds the whole matrices.  A product over this rank's rows only must be
        // completed by an all-gather of the result (16 B per unknown over xGMI); the whole product costs 20 B per stored
        // entry from HBM.  With the ~30 entries per row of the 2D pattern the replicated product is the cheaper one at any
        // size (and bit-identical on every rank); with the ~100 of the 3D pattern the sharded one is.
        bool shard_rows = false;
        if (tree) {
            const char* e = getenv("LSA_DIST_SPMV");  // "shard" / "replicate": override (measurement)
            shard_rows = (e && *e) ? (e[0] == 's') : (C->nnz > 60 * (int64_t)C->n);
        }
        if (tree && shard_rows) {  // SpMV on this rank's rows of the whole matrices
            op->view_fac = mat_row_view(C, tree->row0, tree->row1);
            op->Kfac = op->view_fac;
            if (M) {
                op->view_mul = mat_row_view(M, tree->row0, tree->row1);
                op->Kmul = op->view_mul;
            }
        }
        if (mode == 2) {  // Cayley: multiply by A + nu M = A - (-nu) M
            const double mnu[2] = {-opts->antishift[0], -opts->antishift[1]};
            const bool cmul = cdt || opts->antishift[1] != 0.0;
            rc = build_shifted(ctx, A, M, mnu, cmul, &op->owned_mul);
            if (rc != LSA_OK) {
                lsa_op_destroy(op);
                return rc;
            }
            if (tree && shard_rows) {
                if (op->view_mul) lsa_mat_destroy(op->view_mul);
                op->view_mul = mat_row_view(op->owned_mul, tree->row0, tree->row1);
                op->Kmul = op->view_mul;
            } else op->Kmul = op->owned_mul;
        }
        if (sharded) {
            rc = build_shifted(ctx, Ad, Md, sigma, cdt, &op->owned_diag);
            if (rc != LSA_OK) {
                lsa_op_destroy(op);
                return rc;
            }
            fac_src = op->owned_diag;
        } else fac_src = C;
    } else {
        op->Kmul = C ? C : A;
        op->Kfac = M;
        fac_src = sharded ? Md : M;
    }
    bool lu_fell_back = false;
    if (opts->pc_type == 3) {
        lsa_op_destroy(op);
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_create: pc_type 3 (the banded block LU of round 1) left the product library; it lives on as a "
                                               "cross-check library for the tests (tests/xcheck).  Use pc_type 2, the nested-dissection LU");
    }
    if (op->Kfac && fac_src && opts->pc_type == 2) {
        // exact LU.  Only running out of device memory is answered by the leaner ILU(k) + GMRES (and said so on stderr
        // and in the statistics); a singular pivot block or any other failure is an error, as with PETSc's PC LU.
        if (tree) {
            rc = lsa_ndlu_create_tree(ctx, fac_src, tree->nt, tree->first, tree->size, tree->parent, tree->owner, &op->nd);
            op->nd_dist = rc == LSA_OK;
            if (rc == LSA_ERR_OOM) {  // no leaner collective method to agree on: an error on every rank that hits it
                lsa_op_destroy(op);
                return rc;
            }
        } else
            rc = lsa_ndlu_create(ctx, fac_src, 0, &op->nd);
        if (rc == LSA_OK && op->nd) {
            double sa = 1.0;
            (void)lsa_ndlu_info(op->nd, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &sa, nullptr, nullptr);
            op->st.analysis_reused = sa == 0.0 ? 1 : 0;
        }
        if (rc == LSA_ERR_OOM) {
            fprintf(stderr, "[lsa_hip] exact LU does not fit the device memory (%s): falling back to ILU(%d) + GMRES\n", ctx->err.c_str(),
                    opts->ilu_levels);
            lu_fell_back = true;
            op->st.pc_fallback = 1;
        } else if (rc != LSA_OK) {
            lsa_op_destroy(op);
            return rc;
        }
    }
    if (op->Kfac && fac_src && (opts->pc_type == 1 || lu_fell_back)) {
        rc = lsa_ilu_create(ctx, fac_src, opts->ilu_levels, opts->ilu_shift, &op->pc);
        if (rc != LSA_OK) {
            lsa_op_destroy(op);
            return rc;
        }
    }
    const size_t tb = (size_t)std::max<int64_t>(op->n, 1) * 16;
    if (hipMalloc(&op->t, tb) != hipSuccess || hipMemsetAsync(op->t, 0, tb, ctx->stream) != hipSuccess) {
        lsa_op_destroy(op);
        return lsa_set_error(ctx, LSA_ERR_HIP, "lsa_op_create: out of device memory");
    }
    if (op->Kfac && op->nd && fac_src && fac_src->nnz > 0) {
        // ||C||_F (one reduction over the values): the scale of the backward-error test of the direct solves
        // (the result goes to the head of the operator's own temp vector, not to the context's scratch: k_nrm2 keeps its partial
        //  sums there and may reallocate it; the head is zeroed again afterwards -- padding rows must read zero)
        double* nr = (double*)op->t;
        double v2 = 0.0;
        if (k_nrm2(ctx, fac_src->dtype, fac_src->nnz, fac_src->val, nr) == LSA_OK &&
            hipMemcpyAsync(&v2, nr, sizeof v2, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess &&
            std::isfinite(v2))
            op->normF = std::sqrt(v2);
        (void)hipMemsetAsync(op->t, 0, sizeof(double), ctx->stream);
    }
    op->st.seconds_factor = now_s() - t0;
    *out = op;
    return LSA_OK;
}

int lsa_op_create(lsa_ctx* ctx, const lsa_mat* A, const lsa_mat* M, const double sigma[2], int mode, const lsa_op_options* opts,
                  lsa_op** out) {
    return op_build(ctx, A, M, nullptr, nullptr, sigma, mode, opts, out);
}

int lsa_op_create_sharded(lsa_ctx* ctx, const lsa_mat* A_rows, const lsa_mat* M_rows, const lsa_mat* A_diag, const lsa_mat* M_diag,
                          const double sigma[2], int mode, const lsa_op_options* opts, lsa_op** out) {
    if (!A_diag) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_create_sharded: the diagonal block of A is required");
    return op_build(ctx, A_rows, M_rows, A_diag, M_diag, sigma, mode, opts, out);
}

int lsa_op_create_dist(lsa_ctx* ctx, const lsa_mat* A, const lsa_mat* M, int32_t row0, int32_t row1, int32_t ntree, const int32_t* first,
                       const int32_t* size, const int32_t* parent, const int32_t* owner, const double sigma[2], int mode, const lsa_op_options* opts,
                       lsa_op** out) {
    if (!first || !size || !parent || !owner || ntree < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_create_dist: the forest is required");
    const TreeArg tree{ntree, first, size, parent, owner, row0, row1};
    return op_build(ctx, A, M, nullptr, nullptr, sigma, mode, opts, out, &tree);
}

void lsa_op_destroy(lsa_op* op) {
    if (!op) return;
    if (op->ctx && op->ctx->stream) (void)hipStreamSynchronize(op->ctx->stream);
    if (op->pc) lsa_ilu_destroy(op->pc);
    if (op->nd) lsa_ndlu_destroy(op->nd);
    if (op->view_fac) lsa_mat_destroy(op->view_fac);
    if (op->view_mul) lsa_mat_destroy(op->view_mul);
    if (op->owned) lsa_mat_destroy(op->owned);
    if (op->owned_mul) lsa_mat_destroy(op->owned_mul);
    if (op->owned_diag) lsa_mat_destroy(op->owned_diag);
    if (op->gw_ready) op->gw.release();
    if (op->t) (void)hipFree(op->t);
    if (op->keep) (void)hipFree(op->keep);
    delete op;
}

// y = Kfac^-1 Kmul x on device pointers (complex vectors)
static int op_apply_dev(lsa_ctx* ctx, lsa_op* op, const void* x, void* y) {
    const int dtype = LSA_C128;
    ++op->st.op_applies;
    const void* rhs = x;
    if (op->Kmul) {
        void* dst = op->Kfac ? op->t : y;
        LSA_CHECK(spmv_global(ctx, op->Kmul, dtype, x, dst, op->adjoint));
        ++op->st.spmv_calls;
        rhs = dst;
    }
    if (!op->Kfac) {
        if (!op->Kmul) LSA_CHECK(k_copy(ctx, dtype, op->n, x, y));
        if (op->keep) LSA_CHECK(k_mask(ctx, dtype, op->n, op->keep, y));
        return LSA_OK;
    }
    if (!op->gw_ready) {
        int restart = std::max(1, std::min(op->opts.ksp_restart, op->opts.ksp_maxit));
        // with an exact factorisation on one GPU GMRES only polishes (0-2 iterations): keep its basis small
        if (op->nd && (ctx->nranks == 1 || op->nd_dist)) restart = std::min(restart, 40);
        LSA_CHECK(op->gw.alloc(ctx, op->n, restart, dtype));
        op->gw_ready = true;
    }
    LSA_CHECK(gmres_run(ctx, op->Kfac, pc_of(op), dtype, rhs, y, false, op->opts.ksp_rtol, op->opts.ksp_maxit, op->gw, nullptr, nullptr, &op->st));
    if (op->keep) LSA_CHECK(k_mask(ctx, dtype, op->n, op->keep, y));
    return LSA_OK;
}

int lsa_op_set_adjoint(lsa_ctx* ctx, lsa_op* op, int on) {
    if (!ctx || !op) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_set_adjoint: null argument");
    if (on && (!op->nd || !op->Kfac || (ctx->nranks != 1 && !op->nd_dist)))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_set_adjoint: needs the nested-dissection LU (pc_type 2) of a factorising mode, on one rank or in the "
                                                "subtree-parallel layout");
    if (op->nd_dist) {
        // Subtree-parallel layout: the transposed sweeps walk the same forest with the same exchanges (own subtrees, all-gather of
        // the subtree roots' update vectors, replicated top, all-gather of the solution blocks).  The transposed sparse products
        // are taken with the WHOLE matrices every rank holds (a transposed product over a row block would need a reduction
        // over the ranks instead of an all-gather), whatever the forward products use.
        op->Kfac = (on || !op->view_fac) ? op->owned : op->view_fac;
        op->Kmul = (on || !op->view_mul) ? (op->owned_mul ? op->owned_mul : op->M_whole) : op->view_mul;
    }
    // (the other direction's solves decide about their refinement step for themselves, as those of a new operator do)
    if (op->adjoint != (on != 0)) op->refine = false;
    op->adjoint = on != 0;
    return LSA_OK;
}

int lsa_op_set_projection(lsa_ctx* ctx, lsa_op* op, const double* keep) {
    if (!ctx || !op) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_set_projection: null argument");
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (!keep) {
        if (op->keep) (void)hipFree(op->keep);
        op->keep = nullptr;
        return LSA_OK;
    }
    for (int64_t i = 0; i < op->n; ++i)
        if (keep[i] != 0.0 && keep[i] != 1.0) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_set_projection: keep[%lld] is neither 0 nor 1", (long long)i);
    const size_t bytes = sizeof(double) * (size_t)std::max<int64_t>(op->n, 1);
    if (!op->keep) LSA_HIP_CHECK(ctx, hipMalloc((void**)&op->keep, bytes));
    LSA_HIP_CHECK(ctx, hipMemcpy(op->keep, keep, sizeof(double) * (size_t)op->n, hipMemcpyHostToDevice));
    return LSA_OK;
}

int lsa_op_apply(lsa_ctx* ctx, lsa_op* op, const lsa_vec* x, lsa_vec* y) {
    if (!ctx || !op || !x || !y) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_apply: null argument");
    if (x->n != op->n || y->n != op->n || x->dtype != LSA_C128 || y->dtype != LSA_C128 || x->d == y->d)
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_op_apply: x and y must be distinct complex vectors of length n");
    const double t0 = now_s();
    int rc = op_apply_dev(ctx, op, x->d, y->d);
    if (rc == LSA_OK) LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    op->st.seconds_solve += now_s() - t0;
    return rc;
}

}  // extern "C"

int lsa_op_get_parts(lsa_op* op, lsa_op_parts* out) {
    if (!op || !out) return LSA_ERR_ARG;
    out->n = op->n;
    out->Kmul = op->Kmul;
    out->Kfac = op->Kfac;
    out->nd = op->nd;
    // shift-invert (mode 0: the factorised matrix is the C = A - sigma M built here, the multiplied one the caller's M), forward,
    // unprojected, whole on one rank
    out->plain = op->Kfac && op->Kfac == op->owned && op->Kmul == op->M_whole && !op->owned_mul && !op->adjoint && !op->keep && !op->nd_dist &&
                 op->ctx->nranks == 1;
    out->shift_invert = op->Kfac && op->Kfac == op->owned && op->Kmul == op->M_whole && !op->owned_mul;
    out->adjoint = op->adjoint;
    out->projected = op->keep != nullptr;
    out->one_rank = !op->nd_dist && op->ctx->nranks == 1;
    out->ksp_rtol = op->opts.ksp_rtol;
    out->normF = op->normF;
    out->sigma[0] = op->sigma[0];
    out->sigma[1] = op->sigma[1];
    out->refine = &op->refine;
    out->st = &op->st;
    return LSA_OK;
}

int direct_solve_enqueue(lsa_ctx* ctx, lsa_op* op, int dtype, const void* rhs, void* y, void* z, void* r, bool refine, double* norms, int direction) {
    PcRef pc = pc_of(op);
    // (an explicit direction leaves the operator's own, and with it the refinement state lsa_op_set_adjoint would clear, alone)
    const bool adjoint = direction < 0 ? op->adjoint : direction != 0;
    pc.adjoint = adjoint;
    const lsa_mat* C = op->Kfac;
    LSA_CHECK(pc_global(ctx, pc, C->row0, op->n, dtype, rhs, y));
    LSA_CHECK(spmv_global(ctx, C, dtype, y, z, adjoint));
    if (refine) {
        // y += C^-1 (rhs - C y): the factors of a large 3D problem leave 1e-11 of the right-hand side behind, this step takes it to
        // rounding level
        LSA_CHECK(k_residual_norms(ctx, dtype, op->n, rhs, z, r, norms));
        LSA_CHECK(pc_global(ctx, pc, C->row0, op->n, dtype, r, z));
        const double one[2] = {1.0, 0.0};
        LSA_CHECK(k_axpy(ctx, dtype, op->n, one, z, y));
        LSA_CHECK(spmv_global(ctx, C, dtype, y, z, adjoint));
    }
    return LSA_OK;
}

void stats_book_direct_solve(lsa_stats* st, int products, bool refine, double res, double bnorm) {
    ++st->op_applies;
    st->spmv_calls += products + (refine ? 1 : 0);
    st->sptrsv_calls += refine ? 4 : 2;
    if (refine) ++st->refined_solves;
    st->last_rel_res = bnorm > 0.0 ? res / bnorm : 0.0;
    st->max_rel_res = std::max(st->max_rel_res, st->last_rel_res);
}

int basis_upload_row_permutation(lsa_ctx* ctx, const char* who, int64_t n, const int32_t* perm, int32_t** row_perm) {
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (*row_perm) (void)hipFree(*row_perm);
    *row_perm = nullptr;
    if (!perm) return LSA_OK;
    std::vector<char> seen((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) {
        if (perm[i] < 0 || perm[i] >= n || seen[(size_t)perm[i]]) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: not a permutation of 0..n-1", who);
        seen[(size_t)perm[i]] = 1;
    }
    LSA_HIP_ALLOC(ctx, hipMalloc((void**)row_perm, sizeof(int32_t) * (size_t)std::max<int64_t>(n, 1)));
    LSA_HIP_CHECK(ctx, hipMemcpy(*row_perm, perm, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
    return LSA_OK;
}

int basis_times_host_matrix(lsa_ctx* ctx, int dtype, int64_t n, int m, int k, const void* V, const void* Q, int ldq, void* qdev, void* Out,
                            size_t pinned_extra) {
    const size_t es = esize(dtype), qbytes = (size_t)m * k * es;
    LSA_CHECK(lsa_ensure_scratch(ctx, 0, qbytes + pinned_extra));
    for (int c = 0; c < k; ++c) memcpy((char*)ctx->pinned + (size_t)c * m * es, (const char*)Q + (size_t)c * ldq * es, (size_t)m * es);
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(qdev, ctx->pinned, qbytes, hipMemcpyHostToDevice, ctx->stream));
    return k_basis_gemm(ctx, dtype, n, m, k, V, n, qdev, m, Out, n);
}

int basis_columns_to_host(lsa_ctx* ctx, int dtype, int64_t n, int ncols, const int32_t* row_perm, const void* dev, void** xtmp, int xtmp_cols, void* host) {
    const size_t vb = (size_t)n * esize(dtype);
    const void* src = dev;
    if (row_perm) {
        if (!*xtmp) LSA_HIP_ALLOC(ctx, hipMalloc(xtmp, std::max<size_t>(vb, esize(dtype)) * (size_t)xtmp_cols));
        LSA_CHECK(k_scatter_rows(ctx, dtype, n, ncols, row_perm, dev, *xtmp));
        src = *xtmp;
    }
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(host, src, vb * (size_t)ncols, hipMemcpyDeviceToHost, ctx->stream));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return LSA_OK;
}

extern "C" {

int lsa_op_stats(const lsa_op* op, lsa_stats* out) {
    if (!op || !out) return LSA_ERR_ARG;
    *out = op->st;
    return LSA_OK;
}

// ---- Krylov basis ------------------------------------------------------------------------------------------------
int lsa_krylov_create(lsa_ctx* ctx, lsa_op* op, int32_t ncv, lsa_krylov** out) {
    if (!ctx || !op || !out || ncv < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_create: bad argument");
    if (ncv > k_basis_gemm_max_cols(LSA_C128))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_create: ncv=%d, the basis product handles at most %d basis vectors", ncv, k_basis_gemm_max_cols(LSA_C128));
    const size_t vb = (size_t)std::max<int64_t>(op->n, 1) * 16;
    const char* be = getenv("LSA_KRYLOV_BATCH");
    const int32_t batch = be && *be ? std::max(0, std::min(atoi(be), 256)) : 16;
    if (lsa_krylov* c = ctx->krylov_cache) {
        // A shift sweep (and every repeated solve) builds one Krylov workspace per solve: two bases of ncv + 1 vectors
        // (80 MB at 30 k unknowns, 1.3 GB at 500 k).  The last one destroyed is kept and handed out again when the shape
        // matches, instead of being freed and allocated anew (LSA_KRYLOV_NO_CACHE switches this off).
        ctx->krylov_cache = nullptr;
        if (c->n == op->n && c->ncv == ncv && c->batch == batch) {
            c->op = op;
            c->pipeline = true;
            c->pre_armed = false;
            c->drop_preapply();
            c->imag_norms.clear();
            (void)hipMemsetAsync(c->w, 0, vb, ctx->stream);
            *out = c;
            return LSA_OK;
        }
        krylov_free(c);
    }
    lsa_krylov* k = new lsa_krylov();
    k->ctx = ctx;
    k->op = op;
    k->n = op->n;
    k->ncv = ncv;
    k->V = k->V2 = k->w = k->qdev = nullptr;
    bool ok = hipMalloc(&k->V, vb * (size_t)(ncv + 1)) == hipSuccess && hipMalloc(&k->V2, vb * (size_t)(ncv + 1)) == hipSuccess &&
              hipMalloc(&k->w, vb) == hipSuccess && hipMalloc(&k->qdev, (size_t)(ncv + 1) * (size_t)(ncv + 1) * 16) == hipSuccess;
    if (!ok || k->ow.alloc(ctx, ncv + 1, LSA_C128) != LSA_OK) {
        lsa_krylov_destroy(k);
        return lsa_set_error(ctx, LSA_ERR_HIP, "lsa_krylov_create: out of device memory (n=%lld, ncv=%d)", (long long)op->n, ncv);
    }
    (void)hipMemsetAsync(k->w, 0, vb, ctx->stream);
    k->hcol.assign((size_t)ncv + 2, zc(0));
    // Arnoldi steps are queued in batches when the inner solve is one exact LU solve and the exchange (if any) is
    // stream-ordered (RCCL): LSA_KRYLOV_BATCH steps per read-back (default 16; 0 or 1 = one step at a time, except in the
    // delayed form, whose basis must not depend on the batch size: there it means one step per read-back)
    k->batch = batch;
    const size_t slots = 2 * (size_t)std::max(batch, 1);  // (two sets: one is read back while the other is filled)
    if (hipMalloc(&k->Hdev, slots * krylov_slot_bytes(ncv)) != hipSuccess || hipMalloc((void**)&k->checks, slots * 2 * sizeof(double)) != hipSuccess) {
        lsa_krylov_destroy(k);
        return lsa_set_error(ctx, LSA_ERR_HIP, "lsa_krylov_create: out of device memory (pipeline buffers)");
    }
    k->pipeline = true;
    *out = k;
    return LSA_OK;
}

void lsa_krylov_destroy(lsa_krylov* k) {
    if (!k) return;
    lsa_ctx* ctx = k->ctx;
    if (ctx && ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (k->row_perm) (void)hipFree(k->row_perm);
    k->row_perm = nullptr;
    k->op = nullptr;
    if (ctx && k->V && k->V2 && k->w && k->qdev && k->ow.h1 && !getenv("LSA_KRYLOV_NO_CACHE")) {  // (a half-built workspace is not worth keeping)
        if (ctx->krylov_cache) krylov_free(ctx->krylov_cache);
        ctx->krylov_cache = k;
        return;
    }
    krylov_free(k);
}

void lsa_krylov_drop_cache(lsa_ctx* ctx) {
    if (ctx && ctx->krylov_cache) {
        krylov_free(ctx->krylov_cache);
        ctx->krylov_cache = nullptr;
    }
}

int lsa_krylov_shape(const lsa_krylov* k, int64_t* n, int32_t* ncv) {
    if (!k) return LSA_ERR_ARG;
    if (n) *n = k->n;
    if (ncv) *ncv = k->ncv;
    return LSA_OK;
}

int lsa_krylov_set_row_permutation(lsa_ctx* ctx, lsa_krylov* k, const int32_t* perm) {
    if (!ctx || !k) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_set_row_permutation: null argument");
    return basis_upload_row_permutation(ctx, "lsa_krylov_set_row_permutation", k->n, perm, &k->row_perm);
}

int lsa_krylov_set_start(lsa_ctx* ctx, lsa_krylov* k, const void* host_v) {
    if (!ctx || !k || !host_v) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_set_start: null argument");
    k->pre_armed = false;
    k->drop_preapply();
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(k->w, host_v, (size_t)k->n * 16, hipMemcpyHostToDevice, ctx->stream));
    double nrm = 0.0;
    LSA_CHECK(device_norm(ctx, LSA_C128, k->n, k->w, k->ow.nrm2, &nrm));
    if (!(nrm > 0.0) || !std::isfinite(nrm)) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_set_start: start vector is zero or not finite");
    LSA_CHECK(k_scale_by_inv_norm(ctx, LSA_C128, k->n, k->w, k->ow.nrm2, k->V));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    k->pipeline = true;  // a start vector begins a new run: what the last run on this workspace found out about its solves is not this one's
    return LSA_OK;
}

int lsa_krylov_inject(lsa_ctx* ctx, lsa_krylov* k, int32_t j, const void* host_v) {
    if (!ctx || !k || !host_v) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_inject: null argument");
    if (j < 0 || j > k->ncv) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_inject: index %d out of range", j);
    if (j == 0) return lsa_krylov_set_start(ctx, k, host_v);
    k->drop_preapply();
    const size_t vb = (size_t)k->n * 16;
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(k->w, host_v, vb, hipMemcpyHostToDevice, ctx->stream));
    LSA_CHECK(orthonormalize(ctx, LSA_C128, k->n, k->V, k->n, j, k->w, (char*)k->V + (size_t)j * vb, k->ow, k->hcol.data()));
    const double beta = k->hcol[j].real();
    if (!(beta > 0.0) || !std::isfinite(beta)) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_inject: vector lies in the span of the basis");
    return LSA_OK;
}

// ---- Arnoldi steps ------------------------------------------------------------------------------------------------
// Which form a batch of Arnoldi steps takes.  One step at a time through op_apply_dev (GMRES, or a direct solve with the
// judgement of gmres_run), or pipelined: the steps of a batch are queued without a host round trip -- operator apply by one exact
// LU solve, the check b - C x of that solve, the orthogonalisation -- and everything the host decides on (the check, the
// Hessenberg column, breakdown) is read back once per batch.
enum class Orth {
    cgs2_fused,   // CGS2 in five launches; a step whose shape k_cgs2_fused does not take runs the per-stage kernels
    cgs2_staged,  // CGS2 with a kernel per stage (LSA_KRYLOV_FUSED=0)
    dcgs2,        // delayed reorthogonalisation: one reduction and one update per step (k_dcgs2_step).  On entry to step j, V[:, j]
                  // holds the previous step's vector projected once and column j-1 of H is provisional; step j's reduction finishes both
};
struct StepPlan {
    bool pipelined = false;
    Orth orth = Orth::cgs2_fused;
    bool tail = false;  // the step's last launch also multiplies t = M v_{j+1} for the next step and leaves the pairs of this step's check
};

// Decided anew for every batch.  Inside one lsa_krylov_extend call only two inputs move: k->pipeline (false from the first solve
// that needed the one-step path's judgement until the cache hands the workspace out again) and op->refine (off to on: the tail form
// is lost, never gained); the orthogonalisation is therefore the same for every batch of a call.
static StepPlan step_plan(lsa_ctx* ctx, const lsa_krylov* k) {
    const KrylovSwitches& sw = krylov_switches();
    const lsa_op* op = k->op;
    StepPlan p;
    // DCGS2 where the five-launch CGS2 runs otherwise: one rank, forward operator, a basis of at most 128 vectors of at most 262 k rows
    if (!sw.fused) p.orth = Orth::cgs2_staged;
    else if (sw.delayed && ctx->nranks == 1 && !op->adjoint && op->n == k->n && k_dcgs2_fits(k->n, k->ncv)) p.orth = Orth::dcgs2;
    // an operator apply is one exact LU solve whose result only needs checking, with nothing on the way that synchronises with the
    // host by itself (the host-staged exchange does); batches of one step only in the delayed form, whose basis must not depend on
    // the batch size
    p.pipelined = k->pipeline && (k->batch > 1 || p.orth == Orth::dcgs2) && op->Kfac && op->nd && !op->pc &&
                  !(ctx->nranks > 1 && (!op->nd_dist || ctx->host_gather));
    // tail form: a generalised problem whose M and C share their index arrays, whole on this rank, plain forward products, nothing
    // between the solve and the orthogonalisation (no projection mask, no refinement step)
    p.tail = p.pipelined && sw.tail && sw.fused && op->Kmul && !op->adjoint && !op->keep && !op->refine && op->n == k->n &&
             k_cgs2_tail_fits(ctx, k->n, k->ncv, op->Kmul, op->Kfac);
    return p;
}

// Queues step j of a pipelined batch into `slot`.  Tail form: [M v_j unless the previous step's tail left it] + the sweeps + the
// orthogonalisation + the tail (CGS2: 18 launches, DCGS2: 16).  Otherwise M v_j + the direct solve with its C y (and refinement
// step) + the mask + the orthogonalisation with the check riding in its first reduction.  first: V[:, j] is final (DCGS2: the
// first step of a run).
static int krylov_enqueue_step(lsa_ctx* ctx, lsa_krylov* k, const StepPlan& plan, int32_t j, int32_t slot, bool first) {
    lsa_op* op = k->op;
    const int dtype = LSA_C128;
    const size_t vb = (size_t)k->n * 16;
    const void* vj = (char*)k->V + (size_t)j * vb;
    void* vn = (char*)k->V + (size_t)(j + 1) * vb;
    void* sl = (char*)k->Hdev + (size_t)slot * krylov_slot_bytes(k->ncv);
    double* chk = k->checks + 2 * (size_t)slot;
    const bool dcgs2 = plan.orth == Orth::dcgs2;
    if (plan.orth != Orth::cgs2_staged) LSA_CHECK(k->ow.ensure_fused(ctx, k->n));
    // (the apply queued ahead of the restart is this step's: op->t and w hold it)
    const bool ahead = plan.tail && dcgs2 && first && k->pre_for == j && k->pre_op == op;
    k->drop_preapply();
    if (plan.tail) {
        if (!ahead && k->t_for != j) LSA_CHECK(spmv_global(ctx, op->Kmul, dtype, vj, op->t, false));
        k->t_for = -1;
        if (!ahead) LSA_CHECK(pc_global(ctx, pc_of(op), op->Kfac->row0, op->n, dtype, op->t, k->w));
        double* parts = k->tail_parts + (size_t)slot * 2 * (size_t)k->tail_nparts;
        if (dcgs2) {
            LSA_CHECK(k_dcgs2_step(ctx, k->n, j, k->V, k->n, k->w, first ? 1 : 0, sl, k->ncv, k->ow.fused, nullptr, nullptr, nullptr));
            LSA_CHECK(k_dcgs2_tail(ctx, k->n, j, k->V, k->n, k->w, k->ow.fused, op->Kmul, op->Kfac, op->t, parts, sl, k->ncv));
        } else {
            LSA_CHECK(k_cgs2_fused_tail(ctx, k->n, j + 1, k->V, k->n, k->w, k->w2, vn, sl, k->ow.fused, op->Kmul, op->Kfac, op->t, parts));
        }
        k->t_for = j + 1;
        return LSA_OK;
    }
    k->t_for = -1;
    const void* rhs = vj;
    if (op->Kmul) {
        LSA_CHECK(spmv_global(ctx, op->Kmul, dtype, vj, op->t, op->adjoint));
        rhs = op->t;
    }
    // (the norms a refinement step leaves in the check slot are overwritten by the final check below)
    LSA_CHECK(direct_solve_enqueue(ctx, op, dtype, rhs, k->w, op->gw.z, op->gw.w, op->refine, chk));
    // the check ||b - C y||, ||b|| rides in the first reduction of the orthogonalisation (its vector b - C y is needed only by the
    // one-step path, which recomputes it); the per-stage form has it as a kernel of its own, in front of the mask
    const SolveCheck check{rhs, op->gw.z, op->gw.w, chk};
    const bool rides = plan.orth != Orth::cgs2_staged;
    if (!rides) LSA_CHECK(k_residual_norms(ctx, dtype, op->n, check.b, check.z, check.r, check.out));
    if (op->keep) LSA_CHECK(k_mask(ctx, dtype, op->n, op->keep, k->w));
    if (dcgs2) {
        LSA_CHECK(k_dcgs2_step(ctx, k->n, j, k->V, k->n, k->w, first ? 1 : 0, sl, k->ncv, k->ow.fused, check.b, check.z, check.out));
        return k_dcgs2_norm(ctx, k->n, k->ow.fused, sl, k->ncv);
    }
    return orthonormalize_enqueue(ctx, dtype, k->n, k->V, k->n, j + 1, k->w, vn, k->ow, sl, rides ? &check : nullptr);
}

// the caller's H of one lsa_krylov_extend call: the columns before j0 are the caller's (Arnoldi relation, zero below row j0), those
// from j0 on are Hessenberg
struct HessView {
    cplx* Hh;
    int32_t ldh, j0, ncv;
    cplx* col(int32_t j) const { return Hh + (size_t)j * ldh; }
};

// what a column's new norm says: 1 = breakdown (nothing left of the vector against the size of what was taken out of it), -1 = not
// finite, 0 = go on
static int judge_norm(double beta, const cplx* col, int32_t rows) {
    if (!std::isfinite(beta)) return -1;
    double colmax = 0.0;
    for (int32_t i = 0; i < rows; ++i) colmax = std::max(colmax, std::hypot(col[i].re, col[i].im));
    return beta <= 1e-14 * std::max(colmax, 1e-300) ? 1 : 0;
}

// fills column j of H from h (j + 2 entries, the norm last)
static int take_column(const HessView& H, int32_t j, const cplx* h) {
    cplx* Hj = H.col(j);
    for (int32_t i = 0; i < H.ldh; ++i) Hj[i] = i <= j + 1 ? h[i] : cplx{0.0, 0.0};
    return judge_norm(h[j + 1].re, h, j + 1);
}

// delayed form: a step's a and nu (its slot's first entries and entry 2 ncv) finish column jc - 1 of H
static int finish_column(const HessView& H, int32_t jc, const cplx* sl) {
    cplx* Hp = H.col(jc - 1);
    const double nu = sl[2 * H.ncv].re;
    for (int32_t i = 0; i < jc; ++i) Hp[i] = cplx{Hp[i].re + sl[i].re, Hp[i].im + sl[i].im};
    Hp[jc] = cplx{nu, 0.0};
    return judge_norm(nu, Hp, jc);
}

// delayed form: column jc of H from a step's slot, h = ([b; c] - H[0:jc+1, 0:jc] a) / nu with the provisional ||w|| below it
// (first: a = 0, nu = 1); h: jc + 2 entries of work space
static int provisional_column(const HessView& H, int32_t jc, const cplx* sl, bool first, cplx* h) {
    const int32_t ncv = H.ncv;
    const double inv = 1.0 / sl[2 * ncv].re;
    for (int32_t i = 0; i < jc; ++i) h[i] = sl[ncv + i];
    h[jc] = sl[2 * ncv + 1];
    if (!first) {
        for (int32_t c = 0; c < jc; ++c) {
            const cplx a = sl[c];
            const cplx* Hc = H.col(c);
            const int32_t rows = std::min(jc, std::max(H.j0, c + 1));
            for (int32_t i = 0; i <= rows; ++i) {
                h[i].re -= Hc[i].re * a.re - Hc[i].im * a.im;
                h[i].im -= Hc[i].re * a.im + Hc[i].im * a.re;
            }
        }
        for (int32_t i = 0; i <= jc; ++i) h[i] = cplx{h[i].re * inv, h[i].im * inv};
    }
    h[jc + 1] = cplx{sl[2 * ncv + 2].re, 0.0};
    return take_column(H, jc, h);
}

static int arnoldi_nonfinite(lsa_ctx* ctx, int32_t j) { return lsa_set_error(ctx, LSA_ERR_NONFINITE, "Arnoldi: non-finite norm at step %d", j); }

// where an expansion stands: the first step not done, and (delayed form) whether V[:, j] is projected once only, column j - 1 of H
// provisional.  extend_pipelined can be entered with any such state: the lockstep driver hands a problem over this way.
struct ExtendCursor {
    int32_t j;
    bool pending;
};

// what a pipelined batch needs before its first step is queued: the operator's solve vectors and, in the tail form, its pairs
static int pipelined_prepare(lsa_ctx* ctx, lsa_krylov* k, const StepPlan& plan) {
    lsa_op* op = k->op;
    if (!op->gw_ready) {
        LSA_CHECK(op->gw.alloc(ctx, op->n, std::max(1, std::min({op->opts.ksp_restart, op->opts.ksp_maxit, 40})), LSA_C128));
        op->gw_ready = true;
    }
    if (plan.tail && !k->tail_parts) {
        const int32_t slots = 2 * std::max(k->batch, 1);
        k->tail_nparts = k_cgs2_tail_parts(k->n);
        LSA_HIP_ALLOC(ctx, hipMalloc(&k->w2, (size_t)k->n * 16));
        LSA_HIP_ALLOC(ctx, hipMalloc((void**)&k->tail_parts, (size_t)slots * 2 * (size_t)k->tail_nparts * sizeof(double)));
    }
    return LSA_OK;
}

// Queues the operator apply of the final vector V[:, m] ahead of the restart that will make it column `knew` (LSA_KRYLOV_PREAPPLY):
// t = M v, the sweeps, w = C^-1 t, which is how the first step of the next expansion begins where the plan is the pipelined DCGS2
// tail form.  Nothing is booked here: the step that takes the apply books it when its check is accepted.
static int preapply_enqueue(lsa_ctx* ctx, lsa_krylov* k, int32_t m) {
    if (k->pre_col == m && k->pre_op == k->op) return LSA_OK;  // (queued behind the flush already)
    k->drop_preapply();
    if (!krylov_switches().preapply || m < 1 || m > k->ncv) return LSA_OK;
    const StepPlan plan = step_plan(ctx, k);
    if (!(plan.pipelined && plan.tail && plan.orth == Orth::dcgs2)) return LSA_OK;
    LSA_CHECK(pipelined_prepare(ctx, k, plan));
    lsa_op* op = k->op;
    k->t_for = -1;
    LSA_CHECK(spmv_global(ctx, op->Kmul, LSA_C128, (char*)k->V + (size_t)m * (size_t)k->n * 16, op->t, false));
    LSA_CHECK(pc_global(ctx, pc_of(op), op->Kfac->row0, op->n, LSA_C128, op->t, k->w));
    k->pre_col = m;
    k->pre_op = op;
    return LSA_OK;
}

// The accept loop over the nb steps of one read-back, from step c->j on: slot s at slots + s * slot_stride, its check pair at
// chk + s * chk_stride.  Advances the cursor by the steps accepted (*accepted); fewer than nb: a solve missed rtol and op->refine
// or k->pipeline has changed.  A breakdown sets *breakdown and leaves the cursor alone (the caller restarts from there).
static int accept_steps(lsa_ctx* ctx, lsa_krylov* k, const HessView& H, bool delayed, const char* slots, size_t slot_stride, const double* chk,
                        size_t chk_stride, int32_t nb, ExtendCursor* c, int32_t* breakdown, int32_t* accepted_out) {
    lsa_op* op = k->op;
    const double rtol = op->opts.ksp_rtol;
    cplx* hwork = (cplx*)k->hcol.data();  // (ncv + 2 complex numbers)
    const int32_t j = c->j;
    int32_t accepted = 0;
    *accepted_out = 0;
    for (int32_t s = 0; s < nb; ++s, ++accepted) {
        const cplx* hc = (const cplx*)(slots + (size_t)s * slot_stride);
        const bool first = s == 0 && !c->pending;
        if (delayed && !first) {
            // the step's a and nu depend on V alone, not on its solve: they finish column j + s - 1 and V[:, j + s] even
            // when this step is cut below (it is queued again with V[:, j + s] final)
            c->pending = false;
            const int what = finish_column(H, j + s, hc);
            if (what < 0) return arnoldi_nonfinite(ctx, j + s - 1);
            if (what > 0) {
                *breakdown = j + s - 1;
                return LSA_OK;
            }
        }
        const double beta0 = std::sqrt(chk[(size_t)s * chk_stride]), bnorm = std::sqrt(chk[(size_t)s * chk_stride + 1]);
        if (!(beta0 <= rtol * bnorm)) {
            // a direct solve missed rtol: from here on every queued step carries one refinement step (large 3D factors; the
            // steps of this batch from s on are queued again).  Refined and still short of rtol: this solve needs the judgement
            // of the one-step path (backward error next to an eigenvalue, GMRES), and so will its neighbours: the rest of this
            // basis runs one step at a time
            if (!op->refine && std::isfinite(beta0)) op->refine = true;
            else k->pipeline = false;
            break;
        }
        stats_book_direct_solve(&op->st, op->Kmul ? 2 : 1, op->refine, beta0, bnorm);
        const int what = delayed ? provisional_column(H, j + s, hc, first, hwork) : take_column(H, j + s, hc);
        c->pending = delayed;
        if (what < 0) return arnoldi_nonfinite(ctx, j + s);
        if (what > 0) {  // the steps queued behind a breakdown worked on noise: the caller restarts from here
            *breakdown = j + s;
            return LSA_OK;
        }
    }
    c->j = j + accepted;
    *accepted_out = accepted;
    if (accepted < nb) k->t_for = -1;  // the steps behind the one that stopped the batch ran on; t is theirs
    return LSA_OK;
}

// Steps [c->j, j1) in batches while the plan pipelines; c: where the expansion stands on entry and on return.  Ends early on a
// breakdown (*breakdown) or when a solve needs the one-step path (k->pipeline goes false; the caller runs the rest there).
// Queueing ahead (LSA_KRYLOV_PREAPPLY): what follows a batch if all of it is accepted -- the next batch, or the flush of the delayed
// form and behind it the apply the solve loop has asked for -- is queued into the other set of slots BEFORE the batch is waited for,
// so that the device works while the host reads the batch back and accepts it.  The kernels and their order are those of queueing
// after the read-back.  A batch that is cut short or breaks down leaves what was queued behind it as it leaves its own later steps:
// work on noise, waited for and queued again from the cursor.
static int extend_pipelined(lsa_ctx* ctx, lsa_krylov* k, const HessView& H, ExtendCursor* c, int32_t j1, int32_t* breakdown) {
    StepPlan plan = step_plan(ctx, k);
    LSA_CHECK(pipelined_prepare(ctx, k, plan));
    const int32_t slots = std::max(k->batch, 1);
    const size_t colb = krylov_slot_bytes(k->ncv);
    const size_t region = (size_t)slots * (colb + 2 * sizeof(double));  // of the pinned buffer, per set of slots
    LSA_CHECK(lsa_ensure_scratch(ctx, 0, 2 * region));
    const bool delayed = plan.orth == Orth::dcgs2;
    const bool ahead = krylov_switches().preapply;
    if (ahead) LSA_CHECK(k->ensure_events(ctx));
    k->t_for = -1;  // (op->t is anybody's between calls)
    struct Queued {
        int32_t j, nb, set;  // nb = 0: the flush in front of step j
    };
    auto host_of = [&](int32_t set) { return (char*)ctx->pinned + (size_t)set * region; };
    auto slot_of = [&](int32_t set) { return (char*)k->Hdev + (size_t)set * (size_t)slots * colb; };
    auto queued = [&](int32_t set) -> int {  // marks the end of a read-back
        if (ahead) LSA_HIP_CHECK(ctx, hipEventRecord(k->ev_read[set], ctx->stream));
        return LSA_OK;
    };
    auto wait_for = [&](const Queued& q) -> int {
        const double tw = now_s();
        if (ahead) LSA_HIP_CHECK(ctx, hipEventSynchronize(k->ev_read[q.set]));
        else LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (krylov_switches().timing) fprintf(stderr, "[lsa_krylov] %d steps from %d: waited %.3f ms\n", q.nb, q.j, 1e3 * (now_s() - tw));
        return LSA_OK;
    };
    auto queue_batch = [&](const StepPlan& p, int32_t j, bool first, int32_t set, Queued* q) -> int {
        const int32_t nb = std::min<int32_t>(slots, j1 - j);
        const double tq = now_s();
        for (int32_t s = 0; s < nb; ++s) {
            const int rc = krylov_enqueue_step(ctx, k, p, j + s, set * slots + s, s == 0 && first);
            if (rc != LSA_OK) {
                (void)hipStreamSynchronize(ctx->stream);
                return rc;
            }
        }
        double* chk = k->checks + 2 * (size_t)set * (size_t)slots;
        if (p.tail) LSA_CHECK(k_cgs2_tail_checks(ctx, nb, k->tail_nparts, k->tail_parts + (size_t)set * (size_t)slots * 2 * (size_t)k->tail_nparts, chk));
        LSA_HIP_CHECK(ctx, hipMemcpyAsync(host_of(set), slot_of(set), (size_t)nb * colb, hipMemcpyDeviceToHost, ctx->stream));
        LSA_HIP_CHECK(ctx, hipMemcpyAsync(host_of(set) + (size_t)slots * colb, chk, (size_t)nb * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        LSA_CHECK(queued(set));
        if (krylov_switches().timing) fprintf(stderr, "[lsa_krylov] %d steps from %d queued in %.3f ms\n", nb, j, 1e3 * (now_s() - tq));
        *q = Queued{j, nb, set};
        return LSA_OK;
    };
    // the flush: the reduction and the update without a solve make V[:, j] and column j - 1 final, so that the restart, the Ritz
    // vectors and the next call see what CGS2 leaves
    auto queue_flush = [&](int32_t j, int32_t set, Queued* q) -> int {
        LSA_CHECK(k_dcgs2_step(ctx, k->n, j, k->V, k->n, nullptr, 0, slot_of(set), k->ncv, k->ow.fused, nullptr, nullptr, nullptr));
        LSA_HIP_CHECK(ctx, hipMemcpyAsync(host_of(set), slot_of(set), colb, hipMemcpyDeviceToHost, ctx->stream));
        LSA_CHECK(queued(set));
        // (the solve loop's next act on a full basis is that vector's apply: behind the flush, the stream does not run empty)
        if (k->pre_armed && j == k->ncv) LSA_CHECK(preapply_enqueue(ctx, k, j));
        *q = Queued{j, 0, set};
        return LSA_OK;
    };
    auto drain = [&]() -> int {  // what was queued ahead ran on noise: op->t, w and the slots are nobody's
        k->t_for = -1;
        k->drop_preapply();
        LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        return LSA_OK;
    };
    Queued cur{0, 0, 0}, next{0, 0, 0};
    bool have = false, flushed = false;
    if (c->j < j1 && plan.pipelined) {
        LSA_CHECK(queue_batch(plan, c->j, !c->pending, 0, &cur));
        have = true;
    }
    while (have) {
        bool have_next = false;
        if (ahead) {  // all of `cur` accepted: its last step leaves the delayed form pending
            const int32_t jn = cur.j + cur.nb;
            if (jn < j1) LSA_CHECK(queue_batch(plan, jn, !delayed, cur.set ^ 1, &next));
            else if (delayed) LSA_CHECK(queue_flush(jn, cur.set ^ 1, &next));
            have_next = jn < j1 || delayed;
        }
        LSA_CHECK(wait_for(cur));
        int32_t accepted = 0;
        const char* host = host_of(cur.set);
        const int arc = accept_steps(ctx, k, H, delayed, host, colb, (const double*)(host + (size_t)slots * colb), 2, cur.nb, c, breakdown, &accepted);
        if (arc != LSA_OK || *breakdown >= 0) {
            if (have_next) (void)drain();
            return arc;
        }
        if (accepted == cur.nb && have_next) {
            cur = next;
            if (cur.nb == 0) {
                flushed = true;
                break;
            }
            continue;
        }
        if (have_next) LSA_CHECK(drain());
        plan = step_plan(ctx, k);
        have = c->j < j1 && plan.pipelined;
        if (have) LSA_CHECK(queue_batch(plan, c->j, !c->pending, 0, &cur));
    }
    if (c->pending) {
        const int32_t j = c->j;
        if (!flushed) LSA_CHECK(queue_flush(j, 0, &cur));
        LSA_CHECK(wait_for(cur));
        c->pending = false;
        const int what = finish_column(H, j, (const cplx*)host_of(cur.set));
        if (what != 0) k->drop_preapply();  // (the apply of a vector that is noise)
        if (what < 0) return arnoldi_nonfinite(ctx, j - 1);
        if (what > 0) *breakdown = j - 1;
    }
    return LSA_OK;
}

// steps [j, j1) one at a time: the operator apply with its own judgement of the inner solve, CGS2, one read-back per step
static int extend_one_step(lsa_ctx* ctx, lsa_krylov* k, const HessView& H, int32_t j, int32_t j1, int32_t* breakdown) {
    const size_t vb = (size_t)k->n * 16;
    k->t_for = -1;
    if (j < j1) k->drop_preapply();
    for (; j < j1; ++j) {
        const void* vj = (char*)k->V + (size_t)j * vb;
        void* vn = (char*)k->V + (size_t)(j + 1) * vb;
        LSA_CHECK(op_apply_dev(ctx, k->op, vj, k->w));
        LSA_CHECK(orthonormalize(ctx, LSA_C128, k->n, k->V, k->n, j + 1, k->w, vn, k->ow, k->hcol.data()));
        const int what = take_column(H, j, (const cplx*)k->hcol.data());  // (std::complex<double> has cplx's layout)
        if (what < 0) return arnoldi_nonfinite(ctx, j);
        if (what > 0) {
            *breakdown = j;
            break;
        }
    }
    return LSA_OK;
}

// the steps from the cursor to j1 through the solo code: pipelined batches while the plan allows, then one step at a time
static int extend_rest(lsa_ctx* ctx, lsa_krylov* k, const HessView& H, ExtendCursor* c, int32_t j1, int32_t* bd) {
    int rc = LSA_OK;
    if (step_plan(ctx, k).pipelined) rc = extend_pipelined(ctx, k, H, c, j1, bd);
    if (rc == LSA_OK && *bd < 0) rc = extend_one_step(ctx, k, H, c->j, j1, bd);
    return rc;
}

int lsa_krylov_extend(lsa_ctx* ctx, lsa_krylov* k, int32_t j0, int32_t j1, void* H, int32_t ldh, int32_t* breakdown) {
    if (!ctx || !k || !H) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_extend: null argument");
    if (j0 < 0 || j1 < j0 || j1 > k->ncv || ldh < j1 + 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_extend: bad step range [%d, %d) for ncv %d", j0, j1, k->ncv);
    const double t0 = now_s();
    const HessView Hv{(cplx*)H, ldh, j0, k->ncv};
    ExtendCursor c{j0, false};
    int32_t bd = -1;
    if (k->pre_for != j0 || j0 >= j1) k->drop_preapply();  // (an apply queued ahead is this call's first step's, or nobody's)
    const int rc = extend_rest(ctx, k, Hv, &c, j1, &bd);
    k->pre_for = -1;
    if (breakdown) *breakdown = bd;
    k->op->st.seconds_solve += now_s() - t0;
    return rc;
}

}  // extern "C"

// ---- what the solve loop (KsState, dense.hip) asks for besides the public calls ------------------------------------------------------
void krylov_arm_preapply(lsa_krylov* k, bool on) { k->pre_armed = on && krylov_switches().preapply; }

int krylov_preapply(lsa_ctx* ctx, lsa_krylov* k, int32_t m) { return k->pre_armed ? preapply_enqueue(ctx, k, m) : (int)LSA_OK; }

// The restart of lsa_krylov_restart; queued: everything behind it is stream-ordered, so nothing waits here (the next read-back
// reports a failure).  Not where the next expansion may go one step at a time: GMRES fills the pinned buffer from the host while
// the copy of Q out of it would still be in flight.
static int krylov_restart_impl(lsa_ctx* ctx, lsa_krylov* k, int32_t m, int32_t knew, const void* Q, int32_t ldq, bool queued) {
    const size_t vb = (size_t)k->n * 16;
    const int32_t ahead = k->pre_col == m && k->pre_op == k->op ? knew : -1;
    k->drop_preapply();
    if (knew > 0) LSA_CHECK(basis_times_host_matrix(ctx, LSA_C128, k->n, m, knew, k->V, Q, ldq, k->qdev, k->V2, 0));
    LSA_CHECK(k_copy(ctx, LSA_C128, k->n, (char*)k->V + (size_t)m * vb, (char*)k->V2 + (size_t)knew * vb));
    if (!queued) LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    std::swap(k->V, k->V2);
    k->pre_for = ahead;
    return LSA_OK;
}

int krylov_restart_queued(lsa_ctx* ctx, lsa_krylov* k, int32_t m, int32_t knew, const void* Q, int32_t ldq) {
    return krylov_restart_impl(ctx, k, m, knew, Q, ldq, krylov_switches().preapply && step_plan(ctx, k).pipelined);
}

// ---- lockstep expansion of a group (lsa_krylov_solve_batch, dense.hip) ---------------------------------------------------------
// Problems whose plan is the pipelined DCGS2 tail form on factors of one analysis advance together: a round queues one step of
// every such problem that still has one in this read-back period -- M v_j where the previous tail did not leave it, ONE batched
// sweep pair (ndlu_solve_run on the round's sets), ONE batched reduction, update and tail -- and one read-back covers up to k->batch rounds of
// all of them (their slots, pairs and checks lie round-major in the group's buffers: two copies, one synchronisation).  The
// accept loop is accept_steps per problem over its own slots.  A problem whose plan changes (a miss of ksp_rtol, k->pipeline
// going false), that breaks down or is not eligible finishes its expansion through extend_rest from its cursor, exactly as its
// solo solve continues from there; it is asked again at the next expansion.
int krylov_group_alloc(lsa_ctx* ctx, int32_t J, lsa_krylov* const* ks, KrylovGroupBuf* gb) {
    memset(gb, 0, sizeof *gb);
    gb->J = J;
    gb->slots = std::max(ks[0]->batch, 1);
    gb->nparts = k_cgs2_tail_parts(ks[0]->n);
    const size_t cells = (size_t)J * (size_t)gb->slots;
    LSA_HIP_ALLOC(ctx, hipMalloc(&gb->Hdev, cells * krylov_slot_bytes(ks[0]->ncv)));
    LSA_HIP_ALLOC(ctx, hipMalloc((void**)&gb->checks, cells * 2 * sizeof(double)));
    LSA_HIP_ALLOC(ctx, hipMalloc((void**)&gb->tail_parts, cells * 2 * (size_t)gb->nparts * sizeof(double)));
    // (cells of a round without a step of their problem are summed and copied with the others and never looked at: finite or not)
    LSA_HIP_CHECK(ctx, hipMemsetAsync(gb->tail_parts, 0, cells * 2 * (size_t)gb->nparts * sizeof(double), ctx->stream));
    return LSA_OK;
}

void krylov_group_free(KrylovGroupBuf* gb) {
    for (void* p : {gb->Hdev, (void*)gb->checks, (void*)gb->tail_parts})
        if (p) (void)hipFree(p);
    memset(gb, 0, sizeof *gb);
}

int krylov_group_check(lsa_ctx* ctx, int32_t J, lsa_krylov* const* ks) {
    for (int32_t z = 0; z < J; ++z) {
        if (!ks[z] || !ks[z]->op) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_solve_batch: null workspace (problem %d)", z);
        if (ks[z]->ctx != ctx) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_solve_batch: the workspace of problem %d lives in another context", z);
        if (ks[z]->n != ks[0]->n || ks[z]->ncv != ks[0]->ncv || ks[z]->batch != ks[0]->batch)
            return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_solve_batch: problem %d has another shape (n = %lld, ncv = %d) than problem 0 (n = %lld, ncv = %d)", z,
                                 (long long)ks[z]->n, ks[z]->ncv, (long long)ks[0]->n, ks[0]->ncv);
        for (int32_t y = 0; y < z; ++y)
            if (ks[y] == ks[z] || ks[y]->op == ks[z]->op)
                return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_solve_batch: problems %d and %d share a workspace or an operator", y, z);
    }
    return LSA_OK;
}

int krylov_extend_batch(lsa_ctx* ctx, KrylovGroupBuf* gb, lsa_krylov* const* ks, const uint8_t* active, const int32_t* j0, int32_t j1, void* const* Hs,
                        int32_t ldh, int32_t* breakdown, int32_t* status, std::string* errs, lsa_ks_batch_info* info) {
    const int32_t J = gb->J, slots = gb->slots;
    const double t0 = now_s();
    auto fail = [&](int32_t z, int rc) {  // problem z stops with its own status and its own text, which names it
        status[z] = rc;
        lsa_name_problem(ctx, z);
        errs[z] = ctx->err;
    };
    struct Member {
        ExtendCursor c;
        HessView H;
        bool lock;   // still asked for the lockstep set
        int32_t nb;  // its steps in the current period (0: not a member)
    } mem[kKrylovGroupMax];
    int32_t nactive = 0;
    int32_t ncv = 0;
    for (int32_t z = 0; z < J; ++z) {
        mem[z] = Member{ExtendCursor{0, false}, HessView{nullptr, 0, 0, 0}, false, 0};
        if (!active[z]) continue;
        ++nactive;
        ncv = ks[z]->ncv;
        breakdown[z] = -1;
        status[z] = LSA_OK;
        mem[z] = Member{ExtendCursor{j0[z], false}, HessView{(cplx*)Hs[z], ldh, j0[z], ks[z]->ncv}, true, 0};
        ks[z]->t_for = -1;  // (op->t is anybody's between calls)
        ks[z]->drop_preapply();
    }
    const size_t colb = krylov_slot_bytes(ncv);
    const size_t cells = (size_t)J * (size_t)slots;
    while (true) {
        // ---- who is in lockstep in this read-back period
        int32_t lead = -1, rounds = 0;
        for (int32_t z = 0; z < J; ++z) {
            Member& m = mem[z];
            m.nb = 0;
            if (!active[z] || !m.lock || status[z] != LSA_OK || breakdown[z] >= 0 || m.c.j >= j1) continue;
            lsa_krylov* k = ks[z];
            const StepPlan plan = step_plan(ctx, k);
            bool in = plan.pipelined && plan.orth == Orth::dcgs2 && plan.tail;
            if (in && lead >= 0)
                in = nd_batch_compatible(ks[lead]->op->nd, k->op->nd) && ks[lead]->op->Kmul->dtype == k->op->Kmul->dtype;
            if (!in) {
                m.lock = false;
                continue;
            }
            int rc = pipelined_prepare(ctx, k, plan);
            if (rc == LSA_OK) rc = k->ow.ensure_fused(ctx, k->n);
            if (rc != LSA_OK) {
                fail(z, rc);
                continue;
            }
            if (lead < 0) lead = z;
            m.nb = std::min<int32_t>(slots, j1 - m.c.j);
            rounds = std::max(rounds, m.nb);
        }
        if (lead < 0) break;
        int rc = lsa_ensure_scratch(ctx, 0, cells * (colb + 2 * sizeof(double)));
        int32_t sweep_launches = 0;
        (void)lsa_ndlu_info(ks[lead]->op->nd, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &sweep_launches, nullptr, nullptr, nullptr);
        // ---- the rounds
        for (int32_t s = 0; s < rounds && rc == LSA_OK; ++s) {
            int32_t R = 0, jr[kKrylovGroupMax], fr[kKrylovGroupMax];
            lsa_ndlu* nd[kKrylovGroupMax];
            const lsa_mat *Mr[kKrylovGroupMax], *Cr[kKrylovGroupMax];
            const void *rhs[kKrylovGroupMax], *yr[kKrylovGroupMax];
            void *xr[kKrylovGroupMax], *Vr[kKrylovGroupMax], *slot[kKrylovGroupMax], *work[kKrylovGroupMax], *tr[kKrylovGroupMax];
            double* parts[kKrylovGroupMax];
            int32_t products = 0;
            for (int32_t z = 0; z < J && rc == LSA_OK; ++z) {
                if (s >= mem[z].nb) continue;
                lsa_krylov* k = ks[z];
                lsa_op* op = k->op;
                const int32_t j = mem[z].c.j + s;
                const size_t cell = (size_t)s * (size_t)J + (size_t)z;
                if (k->t_for != j) {
                    rc = spmv_global(ctx, op->Kmul, LSA_C128, (char*)k->V + (size_t)j * (size_t)k->n * 16, op->t, false);
                    ++products;
                }
                k->t_for = -1;
                jr[R] = j;
                fr[R] = (s == 0 && !mem[z].c.pending) ? 1 : 0;
                nd[R] = op->nd;
                Mr[R] = op->Kmul;
                Cr[R] = op->Kfac;
                rhs[R] = op->t;
                xr[R] = k->w;
                yr[R] = k->w;
                Vr[R] = k->V;
                slot[R] = (char*)gb->Hdev + cell * colb;
                work[R] = k->ow.fused;
                tr[R] = op->t;
                parts[R] = gb->tail_parts + cell * 2 * (size_t)gb->nparts;
                ++R;
            }
            const NdSolve sweeps = {R, nd, true, 0, LSA_C128, 1, rhs, 0, xr, 0, "lsa_krylov_solve_batch"};
            if (rc == LSA_OK) rc = ndlu_solve_run(ctx, sweeps);
            if (rc == LSA_OK) rc = k_dcgs2_step_batch(ctx, R, ks[lead]->n, jr, Vr, ks[lead]->n, yr, fr, slot, ncv, work);
            if (rc == LSA_OK) rc = k_dcgs2_tail_batch(ctx, R, ks[lead]->n, jr, Vr, ks[lead]->n, yr, work, Mr, Cr, tr, parts, slot, ncv);
            for (int32_t z = 0; z < J; ++z)
                if (s < mem[z].nb) ks[z]->t_for = mem[z].c.j + s + 1;
            if (info) {
                ++info->rounds;
                info->launches += sweep_launches + 3 + products;
            }
        }
        // ---- one read-back for the period: the checks of all cells in one launch, two copies, one synchronisation
        if (rc == LSA_OK) rc = k_cgs2_tail_checks(ctx, rounds * J, gb->nparts, gb->tail_parts, gb->checks);
        char* host = (char*)ctx->pinned;
        if (rc == LSA_OK && (hipMemcpyAsync(host, gb->Hdev, (size_t)rounds * J * colb, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                             hipMemcpyAsync(host + cells * colb, gb->checks, (size_t)rounds * J * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess))
            rc = lsa_set_error(ctx, LSA_ERR_HIP, "lsa_krylov_solve_batch: read-back of a period failed");
        if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == LSA_OK) rc = lsa_set_error(ctx, LSA_ERR_HIP, "lsa_krylov_solve_batch: a lockstep period failed on the device");
        if (info) ++info->periods;
        if (rc != LSA_OK) {  // the device work of the whole set is lost: an error of every member of this period
            const std::string text = ctx->err;
            for (int32_t z = 0; z < J; ++z)
                if (mem[z].nb > 0) {
                    ctx->err = text;
                    fail(z, rc);
                }
            break;
        }
        const double* chk = (const double*)(host + cells * colb);
        for (int32_t z = 0; z < J; ++z) {
            Member& m = mem[z];
            if (m.nb == 0) continue;
            int32_t accepted = 0;
            const int arc = accept_steps(ctx, ks[z], m.H, true, host + (size_t)z * colb, (size_t)J * colb, chk + 2 * (size_t)z, 2 * (size_t)J, m.nb, &m.c,
                                         &breakdown[z], &accepted);
            if (breakdown[z] >= 0) accepted = breakdown[z] + 1 - m.c.j;
            if (arc != LSA_OK) fail(z, arc);
            else if (info) info->lockstep_steps[z] += accepted;
        }
    }
    // ---- whatever is left of each expansion, through the solo code (at least the flush of a problem that stayed to the end)
    for (int32_t z = 0; z < J; ++z) {
        if (!active[z] || status[z] != LSA_OK || breakdown[z] >= 0) continue;
        const int32_t jb = mem[z].c.j;
        const int xrc = extend_rest(ctx, ks[z], mem[z].H, &mem[z].c, j1, &breakdown[z]);
        if (xrc != LSA_OK) fail(z, xrc);
        else if (info) info->solo_steps[z] += (breakdown[z] >= 0 ? breakdown[z] + 1 : j1) - jb;
    }
    const double share = (now_s() - t0) / std::max(nactive, 1);
    for (int32_t z = 0; z < J; ++z)
        if (active[z]) ks[z]->op->st.seconds_solve += share;
    return LSA_OK;
}

extern "C" {

int lsa_krylov_restart(lsa_ctx* ctx, lsa_krylov* k, int32_t m, int32_t knew, const void* Q, int32_t ldq) {
    if (!ctx || !k || !Q) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_restart: null argument");
    if (m < 1 || m > k->ncv || knew < 0 || knew > m || ldq < m) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_restart: bad sizes m=%d knew=%d", m, knew);
    return krylov_restart_impl(ctx, k, m, knew, Q, ldq, false);
}

int lsa_krylov_ritz_vectors(lsa_ctx* ctx, lsa_krylov* k, int32_t m, int32_t nvec, const void* Y, int32_t ldy, int normalise,
                            void* X) {
    if (!ctx || !k || !Y || !X) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_ritz_vectors: null argument");
    if (m < 1 || m > k->ncv + 1 || nvec < 0 || nvec > k->ncv + 1 || ldy < m) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_ritz_vectors: bad sizes");
    if (nvec == 0) return LSA_OK;
    const size_t vb = (size_t)k->n * 16;
    k->drop_preapply();  // (an apply queued ahead of a restart that did not come: the stream still runs it, nothing here reads w)
    // (the pinned scratch keeps room behind the packed Y for the norms of the imaginary parts)
    LSA_CHECK(basis_times_host_matrix(ctx, LSA_C128, k->n, m, nvec, k->V, Y, ldy, k->qdev, k->V2, (size_t)nvec * sizeof(double)));
    k->imag_norms.clear();
    if (normalise & 2) {
        // unit norm and canonical phase of all columns in three launches; the norms of the imaginary parts come back with them
        if (!k->imag2) LSA_HIP_ALLOC(ctx, hipMalloc((void**)&k->imag2, (size_t)(k->ncv + 2) * sizeof(double)));
        LSA_CHECK(k_columns_canonical(ctx, k->n, nvec, k->V2, k->n, normalise & 1, k->imag2));
        k->imag_norms.assign((size_t)nvec, 0.0);
        // (into the pinned scratch, behind the packed Y: an asynchronous copy to pageable memory is staged by the runtime)
        LSA_HIP_CHECK(ctx, hipMemcpyAsync((char*)ctx->pinned + (size_t)m * nvec * 16, k->imag2, (size_t)nvec * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    } else if (normalise) {
        for (int32_t c = 0; c < nvec; ++c) {
            void* col = (char*)k->V2 + (size_t)c * vb;
            LSA_CHECK(k_nrm2(ctx, LSA_C128, k->n, col, k->ow.nrm2));
            LSA_CHECK(k_copy(ctx, LSA_C128, k->n, col, k->w));
            LSA_CHECK(k_scale_by_inv_norm(ctx, LSA_C128, k->n, k->w, k->ow.nrm2, col));
        }
    }
    const void* src = k->V2;
    void* tmp = nullptr;
    if (k->row_perm) {  // rows back into the caller's numbering on the device (a fancy-indexed scatter of n x nvec on the host costs more than the solve's Schur forms)
        if (!k->xtmp) LSA_HIP_ALLOC(ctx, hipMalloc(&k->xtmp, vb * (size_t)(k->ncv + 1)));
        tmp = k->xtmp;
        LSA_CHECK(k_scatter_rows(ctx, LSA_C128, k->n, nvec, k->row_perm, k->V2, tmp));
        src = tmp;
    }
    const bool timing = krylov_switches().timing;
    if (timing) LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (the download alone)
    const double td = now_s();
    hipError_t e = hipMemcpyAsync(X, src, vb * (size_t)nvec, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return lsa_set_error(ctx, LSA_ERR_HIP, "lsa_krylov_ritz_vectors: download failed: %s", hipGetErrorString(e));
    if (timing) fprintf(stderr, "[lsa_krylov] %d Ritz vectors of %lld rows downloaded in %.3f ms\n", nvec, (long long)k->n, 1e3 * (now_s() - td));
    for (size_t c = 0; c < k->imag_norms.size(); ++c) k->imag_norms[c] = std::sqrt(((const double*)((const char*)ctx->pinned + (size_t)m * nvec * 16))[c]);
    return LSA_OK;
}

int lsa_krylov_imag_norms(const lsa_krylov* k, int32_t nvec, double* out) {
    if (!k || !out || nvec < 0 || (size_t)nvec > k->imag_norms.size()) return LSA_ERR_ARG;
    for (int32_t c = 0; c < nvec; ++c) out[c] = k->imag_norms[(size_t)c];
    return LSA_OK;
}

int lsa_eig_residuals(lsa_ctx* ctx, const lsa_mat* A, const lsa_mat* M, int32_t nvec, const void* lam, const void* X, double* res) {
    if (!ctx || !A || !lam || !X || !res || nvec < 0) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_eig_residuals: bad argument");
    const int64_t n = A->n;
    const size_t vb = (size_t)std::max<int64_t>(n, 1) * 16;
    void *x = nullptr, *ax = nullptr, *mx = nullptr;
    double* nr = nullptr;
    int rc = LSA_OK;
    if (hipMalloc(&x, vb) != hipSuccess || hipMalloc(&ax, vb) != hipSuccess || hipMalloc(&mx, vb) != hipSuccess ||
        hipMalloc((void**)&nr, 4 * sizeof(double)) != hipSuccess)
        rc = lsa_set_error(ctx, LSA_ERR_HIP, "lsa_eig_residuals: out of device memory");
    const cplx* lamh = (const cplx*)lam;
    for (int32_t c = 0; c < nvec && rc == LSA_OK; ++c) {
        double nax = 0, nmx = 0, nrr = 0;
        if (hipMemcpyAsync(x, (const char*)X + (size_t)c * (size_t)n * 16, (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
            rc = lsa_set_error(ctx, LSA_ERR_HIP, "lsa_eig_residuals: upload failed");
            break;
        }
        rc = k_spmv(ctx, A, LSA_C128, x, ax);
        if (rc == LSA_OK) rc = M ? k_spmv(ctx, M, LSA_C128, x, mx) : k_copy(ctx, LSA_C128, n, x, mx);
        if (rc == LSA_OK) rc = device_norm(ctx, LSA_C128, n, ax, nr, &nax);
        if (rc == LSA_OK) rc = device_norm(ctx, LSA_C128, n, mx, nr, &nmx);
        const double ml[2] = {-lamh[c].re, -lamh[c].im};
        if (rc == LSA_OK) rc = k_axpy(ctx, LSA_C128, n, ml, mx, ax);
        if (rc == LSA_OK) rc = device_norm(ctx, LSA_C128, n, ax, nr, &nrr);
        const double lmag = std::hypot(lamh[c].re, lamh[c].im);
        res[c] = nrr / (nax + lmag * nmx + 1e-16);
    }
    (void)hipStreamSynchronize(ctx->stream);
    for (void* p : {x, ax, mx, (void*)nr})
        if (p) (void)hipFree(p);
    return rc;
}

int lsa_eig_biorth(lsa_ctx* ctx, const lsa_mat* M, int64_t n, int32_t nvec, const void* X, const void* Z, void* G, double* norm_z, double* norm_mx) {
    if (!ctx || !X || !Z || !G || !norm_z || !norm_mx || n < 1 || nvec < 0) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_eig_biorth: bad argument");
    if (M && (M->n != n || M->ncols != n || M->row0 != 0))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_eig_biorth: M is %d x %d (first row %d), the vectors have %lld entries", M->n, M->ncols, M->row0, (long long)n);
    if (nvec == 0) return LSA_OK;
    const size_t vb = (size_t)n * 16, gb = (size_t)nvec * nvec * 16;
    void *z = nullptr, *x = nullptr, *mx = nullptr, *g = nullptr;
    double* nr = nullptr;  // (||z_j||^2, ||M x_j||^2) per column
    int rc = LSA_OK;
    if (hipMalloc(&z, vb * (size_t)nvec) != hipSuccess || hipMalloc(&x, vb) != hipSuccess || hipMalloc(&mx, vb) != hipSuccess ||
        hipMalloc(&g, gb) != hipSuccess || hipMalloc((void**)&nr, (size_t)nvec * 2 * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        rc = lsa_set_error(ctx, LSA_ERR_OOM, "lsa_eig_biorth: out of device memory (n=%lld, nvec=%d)", (long long)n, nvec);
    }
    if (rc == LSA_OK && hipMemcpyAsync(z, Z, vb * (size_t)nvec, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        rc = lsa_set_error(ctx, LSA_ERR_HIP, "lsa_eig_biorth: upload failed");
    for (int32_t c = 0; c < nvec && rc == LSA_OK; ++c) {
        if (hipMemcpyAsync(x, (const char*)X + (size_t)c * vb, vb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
            rc = lsa_set_error(ctx, LSA_ERR_HIP, "lsa_eig_biorth: upload failed");
            break;
        }
        rc = M ? k_spmv(ctx, M, LSA_C128, x, mx) : k_copy(ctx, LSA_C128, n, x, mx);
        // column c of G is the V^H w of the CGS kernels with V = Z, w = M x_c
        if (rc == LSA_OK) rc = k_multi_dot(ctx, LSA_C128, n, nvec, z, n, mx, (char*)g + (size_t)c * nvec * 16);
        if (rc == LSA_OK) rc = k_pair_nrm2(ctx, LSA_C128, n, (const char*)z + (size_t)c * vb, mx, nr + 2 * (size_t)c);
    }
    std::vector<double> nrh((size_t)nvec * 2);
    if (rc == LSA_OK && (hipMemcpyAsync(G, g, gb, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                         hipMemcpyAsync(nrh.data(), nr, nrh.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess))
        rc = lsa_set_error(ctx, LSA_ERR_HIP, "lsa_eig_biorth: download failed");
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (rc == LSA_OK && e != hipSuccess) rc = lsa_set_error(ctx, LSA_ERR_HIP, "lsa_eig_biorth: %s", hipGetErrorString(e));
    for (int32_t c = 0; c < nvec && rc == LSA_OK; ++c) {
        norm_z[c] = std::sqrt(nrh[2 * (size_t)c]);
        norm_mx[c] = std::sqrt(nrh[2 * (size_t)c + 1]);
    }
    for (void* p : {z, x, mx, g, (void*)nr})
        if (p) (void)hipFree(p);
    return rc;
}

}  // extern "C"
