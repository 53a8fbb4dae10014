// The family of shifted pencils C_k = A - z_k M behind the region eigensolver (contour.hip) and stochastic forcing (stochastic.hip):
// its matrices, norms and factor sets on one ordering and one analysis, the runs of sets a batched sweep takes, the verdict on a
// node's solve, and the family's product Y[:, k] = C_k X[:, k] in one launch.
//
// Every sum runs in a fixed order and there are no floating-point atomics: two runs give the same bits.
//   sf_shifted_spmm_kernel   the entries of a row strided over the 8 lanes of its row group, each lane adding its entries in order;
//                            then the xor tree over the 8 lanes (ci_spmm_kernel's order)
//   sf_shifted_spmm_transpose_kernel   the same order over the entries of a row of the transposed index
#include "shifted_sets.h"

#include <cmath>
#include <string>

namespace {

constexpr int kSfThreads = 256;   // four wavefronts of 64
constexpr int kSfRowLanes = 8;    // lanes that share a row of sf_shifted_spmm_kernel
constexpr int kSfColTile = 16;    // columns whose accumulators a lane holds at once: 16 x 16 bytes

// Y[:, k] = (A - z_k M) X[:, k], k < N.  Row r belongs to the 8 lanes 8 (r % 32) .. of workgroup r / 32; lane s takes the entries
// rp[r] + s, rp[r] + s + 8, ...: one load of the column index and of the two real values per entry serves a pass of up to 16 columns
// (all 16 entries of that row of X requested before the first multiply-add of a full pass); N > 16 takes further passes inside the
// launch.  c = a - z m is formed per column in registers: Re c = fma(-Re z, m, a), Im c = -(Im z) m.  Rows beyond n take an empty
// range, so that every lane of a wavefront reaches the shuffles.
__global__ __launch_bounds__(kSfThreads) void sf_shifted_spmm_kernel(int32_t n, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                                                     const double* __restrict__ a, const double* __restrict__ m, int N,
                                                                     const cplx* __restrict__ z, const cplx* __restrict__ X, int64_t ldx,
                                                                     cplx* __restrict__ Y, int64_t ldy) {
    const int sub = threadIdx.x & (kSfRowLanes - 1);
    const int64_t row = (int64_t)blockIdx.x * (kSfThreads / kSfRowLanes) + (threadIdx.x / kSfRowLanes);
    int32_t p0 = 0, p1 = 0;
    if (row < n) {
        p0 = rp[row];
        p1 = rp[row + 1];
    }
    for (int k0 = 0; k0 < N; k0 += kSfColTile) {
        const int nc = (N - k0 < kSfColTile) ? N - k0 : kSfColTile;
        cplx zz[kSfColTile], acc[kSfColTile];
#pragma unroll
        for (int u = 0; u < kSfColTile; ++u) {
            zz[u] = (u < nc) ? rz_ld(z + k0 + u) : cplx{0.0, 0.0};
            acc[u] = cplx{0.0, 0.0};
        }
        const cplx* Xt = X + (int64_t)k0 * ldx;
        if (nc == kSfColTile) {
            for (int32_t p = p0 + sub; p < p1; p += kSfRowLanes) {
                const cplx* x = Xt + ci[p];
                const double av = a[p], mv = m[p];
                cplx xv[kSfColTile];
#pragma unroll
                for (int u = 0; u < kSfColTile; ++u) xv[u] = rz_ld(x + (int64_t)u * ldx);
#pragma unroll
                for (int u = 0; u < kSfColTile; ++u) fma_acc(acc[u], cplx{fma(-zz[u].re, mv, av), -(zz[u].im * mv)}, xv[u]);
            }
        } else {
            for (int32_t p = p0 + sub; p < p1; p += kSfRowLanes) {
                const cplx* x = Xt + ci[p];
                const double av = a[p], mv = m[p];
#pragma unroll
                for (int u = 0; u < kSfColTile; ++u)
                    if (u < nc) fma_acc(acc[u], cplx{fma(-zz[u].re, mv, av), -(zz[u].im * mv)}, rz_ld(x + (int64_t)u * ldx));
            }
        }
#pragma unroll
        for (int u = 0; u < kSfColTile; ++u) {
#pragma unroll
            for (int off = kSfRowLanes / 2; off >= 1; off >>= 1) {
                acc[u].re += __shfl_xor(acc[u].re, off, 64);
                acc[u].im += __shfl_xor(acc[u].im, off, 64);
            }
        }
        if (sub == 0 && row < n) {
#pragma unroll
            for (int u = 0; u < kSfColTile; ++u)
                if (u < nc) rz_st(Y + row + (int64_t)(k0 + u) * ldy, acc[u]);
        }
    }
}

// Y[:, c] = (A - z_c M)^H X[:, c], c < N, on the pattern's transposed index (rp, ci, src of k_transpose_index: output row r sums the
// entries q in [rp[r], rp[r + 1]), the values at position src[q] of the CSR arrays times X[ci[q], c]).  The shape of
// sf_shifted_spmm_kernel: 8 lanes per output row, lane s takes the entries rp[r] + s, rp[r] + s + 8, ..., one load of the row index,
// the source position and the two real values per entry serves a pass of up to 16 columns, the 16 loads of X of a full pass requested
// before the first multiply-add; then the xor tree over the 8 lanes.  conj(a - z m) is formed per column in registers:
// Re = fma(-Re z, m, a), Im = (Im z) m.
__global__ __launch_bounds__(kSfThreads) void sf_shifted_spmm_transpose_kernel(int32_t n, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                                                               const int32_t* __restrict__ src, const double* __restrict__ a,
                                                                               const double* __restrict__ m, int N, const cplx* __restrict__ z,
                                                                               const cplx* __restrict__ X, int64_t ldx, cplx* __restrict__ Y, int64_t ldy) {
    const int sub = threadIdx.x & (kSfRowLanes - 1);
    const int64_t row = (int64_t)blockIdx.x * (kSfThreads / kSfRowLanes) + (threadIdx.x / kSfRowLanes);
    int32_t p0 = 0, p1 = 0;
    if (row < n) {
        p0 = rp[row];
        p1 = rp[row + 1];
    }
    for (int k0 = 0; k0 < N; k0 += kSfColTile) {
        const int nc = (N - k0 < kSfColTile) ? N - k0 : kSfColTile;
        cplx zz[kSfColTile], acc[kSfColTile];
#pragma unroll
        for (int u = 0; u < kSfColTile; ++u) {
            zz[u] = (u < nc) ? rz_ld(z + k0 + u) : cplx{0.0, 0.0};
            acc[u] = cplx{0.0, 0.0};
        }
        const cplx* Xt = X + (int64_t)k0 * ldx;
        if (nc == kSfColTile) {
            for (int32_t p = p0 + sub; p < p1; p += kSfRowLanes) {
                const cplx* x = Xt + ci[p];
                const int32_t q = src[p];
                const double av = a[q], mv = m[q];
                cplx xv[kSfColTile];
#pragma unroll
                for (int u = 0; u < kSfColTile; ++u) xv[u] = rz_ld(x + (int64_t)u * ldx);
#pragma unroll
                for (int u = 0; u < kSfColTile; ++u) fma_acc(acc[u], cplx{fma(-zz[u].re, mv, av), zz[u].im * mv}, xv[u]);
            }
        } else {
            for (int32_t p = p0 + sub; p < p1; p += kSfRowLanes) {
                const cplx* x = Xt + ci[p];
                const int32_t q = src[p];
                const double av = a[q], mv = m[q];
#pragma unroll
                for (int u = 0; u < kSfColTile; ++u)
                    if (u < nc) fma_acc(acc[u], cplx{fma(-zz[u].re, mv, av), zz[u].im * mv}, rz_ld(x + (int64_t)u * ldx));
            }
        }
#pragma unroll
        for (int u = 0; u < kSfColTile; ++u) {
#pragma unroll
            for (int off = kSfRowLanes / 2; off >= 1; off >>= 1) {
                acc[u].re += __shfl_xor(acc[u].re, off, 64);
                acc[u].im += __shfl_xor(acc[u].im, off, 64);
            }
        }
        if (sub == 0 && row < n) {
#pragma unroll
            for (int u = 0; u < kSfColTile; ++u)
                if (u < nc) rz_st(Y + row + (int64_t)(k0 + u) * ldy, acc[u]);
        }
    }
}

// the matrices, the norms and the factor sets of a family whose vectors are sized: shifted_sets_create's work between its allocations
// and its synchronisation.  What was made before a failure stays in the family for shifted_sets_free.
int ss_factorise(lsa_ctx* ctx, const char* who, shifted_sets* s, double budget) {
    const lsa_mat *A = s->A, *M = s->M;
    const size_t nsets = s->F.size();
    auto fits = [&](const NdSymbolic& S) {
        const int64_t per_set = shifted_sets_bytes_per_set(S);
        size_t free_b = 0, total_b = 0;
        if (per_set < 0 || hipMemGetInfo(&free_b, &total_b) != hipSuccess) return (int)LSA_OK;
        const double need = (double)nsets * (double)per_set;
        if (need <= budget * (double)free_b) return (int)LSA_OK;
        return lsa_set_error(ctx, LSA_ERR_OOM, "%s: %d factor sets need %.0f bytes, %.1f of the %.0f bytes of free device memory hold %.0f; fewer nodes fit "
                                               "(refactorising sets node by node is not built)", who, (int)nsets, need, budget, (double)free_b, budget * (double)free_b);
    };
    bool judged = false;
    if (budget > 0.0 && ctx->nd_cache && ctx->nd_cache->dtype == LSA_C128 && ctx->nd_cache->S.n == A->n && ctx->nd_cache->S.nnz == A->nnz) {
        LSA_CHECK(fits(ctx->nd_cache->S));
        judged = true;
    }
    int rc = LSA_OK;
    for (int32_t k = 0; k < s->N && rc == LSA_OK; ++k) {
        const double one[2] = {1.0, 0.0}, mz[2] = {-s->z[(size_t)k].real(), -s->z[(size_t)k].imag()};
        rc = lsa_csr_axpby(ctx, A, M, one, mz, LSA_C128, &s->C[(size_t)k]);
        if (rc == LSA_OK) rc = k_nrm2(ctx, LSA_C128, A->nnz, s->C[(size_t)k]->val, s->sum_dev);
        double v2 = 0.0;
        if (rc == LSA_OK && (hipMemcpyAsync(&v2, s->sum_dev, sizeof v2, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess))
            rc = lsa_set_error(ctx, LSA_ERR_HIP, "%s: reading ||C||_F failed", who);
        if (rc == LSA_OK && std::isfinite(v2)) s->normF[(size_t)k] = std::sqrt(v2);
    }
    for (size_t k = 0; k < nsets && rc == LSA_OK; ++k) {
        if (k == 0) {
            rc = lsa_ndlu_create(ctx, s->C[0], 0, &s->F[0]);
        } else {
            const NdSymbolic& S = s->F[0]->S;
            if (budget > 0.0 && !judged) {
                LSA_CHECK(fits(S));
                judged = true;
            }
            if (S.tree_hash != 0) {
                std::vector<int32_t> first((size_t)S.nt), size((size_t)S.nt);
                for (int32_t t = 0; t < S.nt; ++t) {
                    first[(size_t)t] = S.perm[(size_t)S.node_start[(size_t)t]];
                    size[(size_t)t] = S.node_start[(size_t)t + 1] - S.node_start[(size_t)t];
                }
                lsa_ndlu_drop_cache(ctx);
                rc = lsa_ndlu_create_tree(ctx, s->C[k], S.nt, first.data(), size.data(), S.parent.data(), nullptr, &s->F[k]);
            } else {
                lsa_ndlu_drop_cache(ctx);
                rc = lsa_ndlu_create(ctx, s->C[k], S.leaf_size, &s->F[k]);
            }
        }
        if (rc != LSA_OK) rc = lsa_set_error(ctx, rc, "%s: node %d (z = %.6g%+.6gi): %s", who, (int)k, s->z[k].real(), s->z[k].imag(), std::string(ctx->err).c_str());
    }
    return rc;
}

}  // namespace

int64_t shifted_sets_bytes_per_set(const NdSymbolic& S) {
    int64_t out[8] = {};
    if (nd_memory_report(S, (int32_t)sizeof(cplx), 0, out, nullptr, nullptr, nullptr) != LSA_OK) return -1;
    return out[0] + out[1] + out[2] + out[4] + out[7];
}

int shifted_sets_create(lsa_ctx* ctx, const char* who, const lsa_mat* A, const lsa_mat* M, const std::vector<std::complex<double>>& z, size_t nsets,
                        double budget, shifted_sets** out) {
    *out = nullptr;
    const double t0 = now_s();
    shifted_sets* s = new shifted_sets();
    s->A = A;
    s->M = M;
    s->n = A->n;
    s->N = (int32_t)z.size();
    s->z = z;
    s->C.assign(z.size(), nullptr);
    s->normF.assign(z.size(), 0.0);
    s->F.assign(nsets, nullptr);
    for (int dir = 0; dir < 2; ++dir) s->refine[dir].assign(z.size(), 0);
    int rc = LSA_OK;
    if (hipMalloc((void**)&s->zdev, z.size() * sizeof(cplx)) != hipSuccess || hipMalloc((void**)&s->sum_dev, sizeof(double)) != hipSuccess ||
        hipMemcpy(s->zdev, z.data(), z.size() * sizeof(cplx), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        rc = lsa_set_error(ctx, LSA_ERR_OOM, "%s: out of device memory (n=%d, nodes=%d)", who, A->n, s->N);
    }
    if (rc == LSA_OK) rc = ss_factorise(ctx, who, s, budget);
    if (rc == LSA_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = lsa_set_error(ctx, LSA_ERR_HIP, "%s: the factorisations failed", who);
    if (rc != LSA_OK) {
        const std::string msg = ctx->err;
        shifted_sets_free(s);
        return lsa_set_error(ctx, rc, "%s", msg.c_str());
    }
    s->cur = 0;
    s->analysis_reused = s->F[0]->seconds_analyse == 0.0 ? 1 : 0;
    s->seconds_factor = now_s() - t0;
    *out = s;
    return LSA_OK;
}

void shifted_sets_free(shifted_sets* s) {
    if (!s) return;
    for (lsa_ndlu* f : s->F)
        if (f) lsa_ndlu_destroy(f);
    for (lsa_mat* c : s->C)
        if (c) lsa_mat_destroy(c);
    if (s->zdev) (void)hipFree(s->zdev);
    if (s->sum_dev) (void)hipFree(s->sum_dev);
    delete s;
}

int shifted_sets_factors(lsa_ctx* ctx, shifted_sets* s, const char* who, int32_t k, lsa_ndlu** f) {
    if (s->F.size() == (size_t)s->N) {
        *f = s->F[(size_t)k];
        return LSA_OK;
    }
    if (s->cur != k) {
        const double t0 = now_s();
        s->cur = -1;
        int rc = lsa_ndlu_refactor(ctx, s->F[0], s->C[(size_t)k]);
        if (rc == LSA_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = lsa_set_error(ctx, LSA_ERR_HIP, "the refactorisation failed");
        s->seconds_factor += now_s() - t0;
        if (rc != LSA_OK) return lsa_set_error(ctx, rc, "%s: node %d (z = %.6g%+.6gi): %s", who, k, s->z[(size_t)k].real(), s->z[(size_t)k].imag(), std::string(ctx->err).c_str());
        s->cur = k;
    }
    *f = s->F[0];
    return LSA_OK;
}

int32_t shifted_sets_next_run(const shifted_sets* s, int32_t start, const std::vector<char>& skip, shifted_run* run) {
    run->J = 0;
    int32_t q = start;
    for (; q < s->N && run->J < kNdBatchMax; ++q) {
        if (skip[(size_t)q]) continue;
        if (run->J > 0 && !nd_batch_compatible(run->f[0], s->F[(size_t)q])) break;
        run->node[run->J] = q;
        run->f[run->J] = s->F[(size_t)q];
        ++run->J;
    }
    return q;
}

int k_shifted_spmm(lsa_ctx* ctx, const lsa_mat* A, const lsa_mat* M, int32_t N, const void* z_dev, const void* X, void* Y) {
    if (A->n < 1 || N < 1) return LSA_OK;
    const int per_block = kSfThreads / kSfRowLanes;
    hipLaunchKernelGGL(sf_shifted_spmm_kernel, dim3((A->n + per_block - 1) / per_block), dim3(kSfThreads), 0, ctx->stream, A->n, A->rp, A->ci,
                       (const double*)A->val, (const double*)M->val, N, (const cplx*)z_dev, (const cplx*)X, (int64_t)A->n, (cplx*)Y, (int64_t)A->n);
    return lsa_check_launch(ctx, "sf_shifted_spmm_kernel");
}

int k_shifted_spmm_transpose(lsa_ctx* ctx, const lsa_mat* A, const lsa_mat* M, int32_t N, const void* z_dev, const void* X, void* Y) {
    if (A->n < 1 || N < 1) return LSA_OK;
    const TransposeIndex* T = nullptr;
    LSA_CHECK(k_transpose_index(ctx, A, &T));
    const int per_block = kSfThreads / kSfRowLanes;
    hipLaunchKernelGGL(sf_shifted_spmm_transpose_kernel, dim3((A->ncols + per_block - 1) / per_block), dim3(kSfThreads), 0, ctx->stream, A->ncols, T->rp, T->ci,
                       T->src, (const double*)A->val, (const double*)M->val, N, (const cplx*)z_dev, (const cplx*)X, (int64_t)A->n, (cplx*)Y, (int64_t)A->n);
    return lsa_check_launch(ctx, "sf_shifted_spmm_transpose_kernel");
}

bool sf_same_pattern(const lsa_mat* A, const lsa_mat* M) {
    if (M->n != A->n || M->ncols != A->ncols || M->nnz != A->nnz) return false;
    if (A->rp == M->rp && A->ci == M->ci) return true;
    if (A->h_rp.size() > 0 && M->h_rp.size() > 0 && A->h_ci.size() > 0 && M->h_ci.size() > 0) return A->h_rp == M->h_rp && A->h_ci == M->h_ci;
    return true;
}

// lsa_shifted_spmm and lsa_shifted_spmm_transpose: the checks, the upload of the shifts, the one launch, the synchronisation
static int ss_shifted_spmm_entry(lsa_ctx* ctx, const char* who, bool transpose, const lsa_mat* A, const lsa_mat* M, int32_t nodes, const double* shifts,
                                 const lsa_vec* X, lsa_vec* Y) {
    if (!ctx || !A || !M || !shifts || !X || !Y) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: null argument", who);
    if (A->n != A->ncols || A->row0 != 0) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: A is a row shard (%d x %d): whole square matrices only", who, A->n, A->ncols);
    if (A->dtype != LSA_F64 || M->dtype != LSA_F64) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: A or M is complex: real matrices only", who);
    if (!sf_same_pattern(A, M)) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: A and M do not share one pattern", who);
    if (nodes < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: %d columns", who, nodes);
    if (X->dtype != LSA_C128 || Y->dtype != LSA_C128) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: the blocks must be complex128", who);
    if (X->d == Y->d) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: X and Y must not alias", who);
    const int64_t need = (int64_t)A->n * nodes;
    if (X->n < need || Y->n < need)
        return lsa_set_error(ctx, LSA_ERR_ARG, "%s: blocks of %d columns of %d rows do not fit vectors of %lld and %lld entries", who, nodes, A->n,
                             (long long)X->n, (long long)Y->n);
    cplx* zdev = nullptr;
    LSA_HIP_ALLOC(ctx, hipMalloc((void**)&zdev, (size_t)nodes * sizeof(cplx)));
    int rc = LSA_OK;
    if (hipMemcpy(zdev, shifts, (size_t)nodes * sizeof(cplx), hipMemcpyHostToDevice) != hipSuccess) rc = lsa_set_error(ctx, LSA_ERR_HIP, "%s: the upload of the shifts failed", who);
    if (rc == LSA_OK) rc = transpose ? k_shifted_spmm_transpose(ctx, A, M, nodes, zdev, X->d, Y->d) : k_shifted_spmm(ctx, A, M, nodes, zdev, X->d, Y->d);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == LSA_OK) rc = lsa_set_error(ctx, LSA_ERR_HIP, "%s: the kernel failed", who);
    (void)hipFree(zdev);
    return rc;
}

extern "C" {

int lsa_shifted_spmm(lsa_ctx* ctx, const lsa_mat* A, const lsa_mat* M, int32_t nodes, const double* shifts, const lsa_vec* X, lsa_vec* Y) {
    return ss_shifted_spmm_entry(ctx, "lsa_shifted_spmm", false, A, M, nodes, shifts, X, Y);
}

int lsa_shifted_spmm_transpose(lsa_ctx* ctx, const lsa_mat* A, const lsa_mat* M, int32_t nodes, const double* shifts, const lsa_vec* X, lsa_vec* Y) {
    return ss_shifted_spmm_entry(ctx, "lsa_shifted_spmm_transpose", true, A, M, nodes, shifts, X, Y);
}

}  // extern "C"
