// The handle of stochastic forcing (stochastic.hip), shared with the trace estimator on the same factor family (stochastic_trace.hip).
// Internal: not part of the C ABI.
#pragma once

#include "shifted_sets.h"

constexpr int kSfEvents = 7;      // the boundaries of a step's six phases

typedef std::complex<double> sf_z;

struct lsa_stochastic {
    lsa_ctx* ctx = nullptr;
    int64_t n = 0;
    int32_t N = 0, ncv = 0, kind = 0;
    double ksp_rtol = 0.0;
    std::vector<double> c;           // w_k / pi
    // the pencils C_k = A - z_k M at the nodes, all N factor sets alive; refine[dir][k]: node k's solves of that direction carry the
    // refinement step
    shifted_sets* S = nullptr;
    const lsa_mat *Qf = nullptr, *Qq = nullptr;  // the weights (lsa_stochastic_set_weights; borrowed): both are M on a new handle
    lsa_stats st{};
    lsa_op_parts P{};                // what the basis reads of an operator: n, the inner product's matrix, st
    lsa_lanczos* lz = nullptr;       // the real basis and everything of a step but its operator
    lanczos_operator hook{};
    double* cdev = nullptr;          // the N coefficients w_k / pi
    // the step's vectors: the widened right-hand side; n x N blocks of the first solutions, their check products, the weighted first
    // solutions, the second solutions and their check products; a residual and a correction for refinement steps
    cplx *b = nullptr, *X1 = nullptr, *Z1 = nullptr, *TM = nullptr, *X2 = nullptr, *Z2 = nullptr, *r = nullptr, *d = nullptr;
    double *part = nullptr, *log = nullptr, *rnorms = nullptr;
    double* hlog = nullptr;          // pinned host copy of the log
    double *vdev = nullptr, *rhsdev = nullptr, *ydev = nullptr;  // lsa_stochastic_apply's vector, Q v and S v
    hipEvent_t ev[kSfEvents] = {};
    bool timed = false;              // the events of a queued step have not been read yet
    std::vector<char> used[2];       // the family's refinement flags (or all ones: force_refine) the step being judged was queued with
    bool force_refine = false, batch_forward = false, batch_adjoint = false;
    int64_t solves_adj = 0, solves_fwd = 0, refined_adj = 0, refined_fwd = 0;
    int64_t adjoint_batches = 0, forward_batches = 0;  // grouped calls of the batched sweeps with more than one set
    int64_t bytes = 0;
    double sec_solve = 0.0, sec_product = 0.0, sec_dense = 0.0;
    double sec_solve_adj = 0.0, sec_product_adj = 0.0;  // the adjoint solves' share of sec_solve, their check products' of sec_product
};

// the direction of a step's first and second solves: kind 0 solves with C^-H first, kind 1 with C^-1
inline bool sf_adjoint(const lsa_stochastic* h, int pos) { return (h->kind == 0) == (pos == 0); }
inline const lsa_mat* sf_inner(const lsa_stochastic* h) { return h->kind == 0 ? h->Qq : h->Qf; }
inline const lsa_mat* sf_middle(const lsa_stochastic* h) { return h->kind == 0 ? h->Qf : h->Qq; }
