// A family of shifted pencils C_k = A - z_k M, k < N, with exact LUs on one ordering and one analysis (shifted_sets.hip): what the
// region eigensolver (contour.hip) and stochastic forcing (stochastic.hip) factorise, group into lockstep runs, judge and release.
// Internal: not part of the C ABI.
#pragma once

#include <complex>
#include <vector>

#include "lsa_internal.h"
#include "nd_internal.h"
#include "ndlu_internal.h"

struct shifted_sets {
    const lsa_mat *A = nullptr, *M = nullptr;  // borrowed: real or complex A, real M, one pattern
    int64_t n = 0;
    int32_t N = 0;
    std::vector<std::complex<double>> z;  // the nodes
    cplx* zdev = nullptr;                 // ... and on the device, for k_shifted_spmm
    std::vector<lsa_mat*> C;              // C_k = A - z_k M (values only: A's index arrays)
    std::vector<double> normF;            // ||C_k||_F: the scale of the backward-error judgement
    std::vector<lsa_ndlu*> F;             // N factor sets, or one that is refactorised node by node
    int32_t cur = -1;                     // the node whose values F[0] holds (refactorised sets)
    // refine[dir][k]: node k's solves of that direction (0 forward, 1 adjoint) carry the refinement step
    std::vector<char> refine[2];
    double* sum_dev = nullptr;            // where ||C_k||_F^2 lands
    double seconds_factor = 0.0;          // creation, and every refactorisation since
    int analysis_reused = 0;              // the first set took the analysis the context held prepared
};

// C_k and ||C_k||_F for all nodes, then nsets factor sets (z.size(), or 1: refactorised node by node), drained.  The first set takes
// the analysis the context holds prepared (lsa_ndlu_prepare / _prepare_tree), or analyses; every further one redoes the pattern-only
// phase from the first one's forest: one ordering, one analysis, the bits of a refactorisation.  budget > 0: LSA_ERR_OOM, with the
// bytes needed and the bytes available, where nsets sets exceed that fraction of the device memory free at the call -- judged on the
// prepared analysis before anything is factorised, else on the first set's before the second.  who: the caller's name in the messages.
// A failed call releases what it made and leaves its message in the context.
int shifted_sets_create(lsa_ctx* ctx, const char* who, const lsa_mat* A, const lsa_mat* M, const std::vector<std::complex<double>>& z, size_t nsets,
                        double budget, shifted_sets** out);
void shifted_sets_free(shifted_sets* s);  // (null: nothing)

// the device bytes of one factor set on the analysis S (the figures of lsa_ndlu_prepared_memory), or -1 where they cannot be told
int64_t shifted_sets_bytes_per_set(const NdSymbolic& S);

// the factors of node k: its own set, or the one set refactorised for it (timed into seconds_factor; drains the stream)
int shifted_sets_factors(lsa_ctx* ctx, shifted_sets* s, const char* who, int32_t k, lsa_ndlu** f);

// A run of nodes whose solves go through one batched sweep: J <= kNdBatchMax of them with their factor sets.
struct shifted_run {
    int32_t J;
    int32_t node[kNdBatchMax];
    lsa_ndlu* f[kNdBatchMax];
};
// The next run from node `start` on: the nodes k with skip[k] == 0 in ascending order, until the run is full or a set is not
// nd_batch_compatible with the run's first one (a skipped node does not end a run).  Returns the node the next run starts from;
// run->J == 0: no node was left.  All N sets alive only.
int32_t shifted_sets_next_run(const shifted_sets* s, int32_t start, const std::vector<char>& skip, shifted_run* run);

// direct_solve_verdict on node k's ||C_k||_F
inline int shifted_sets_verdict(const shifted_sets* s, int32_t k, double ksp_rtol, bool refine, double res, double bnorm, double xnorm, bool* backward) {
    return direct_solve_verdict(ksp_rtol, s->normF[(size_t)k], refine, res, bnorm, xnorm, backward);
}

// Y[:, k] = (A - z_k M) X[:, k], k < N: A, M real on one pattern, X, Y n x N complex (ld n), z_dev N complex on the device
int k_shifted_spmm(lsa_ctx* ctx, const lsa_mat* A, const lsa_mat* M, int32_t N, const void* z_dev, const void* X, void* Y);
// Y[:, c] = (A - z_c M)^H X[:, c], c < N, on the pattern's transposed index (k_transpose_index) in one launch; not k_spmv_transpose's bits
int k_shifted_spmm_transpose(lsa_ctx* ctx, const lsa_mat* A, const lsa_mat* M, int32_t N, const void* z_dev, const void* X, void* Y);
// whether M has A's pattern, as far as the handles can tell without a read-back
bool sf_same_pattern(const lsa_mat* A, const lsa_mat* M);
