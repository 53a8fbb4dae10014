// Resolvent (input-output) analysis of M q' = A q + M f at a real frequency omega: the optimal gains sigma_1 >= sigma_2 >= ... are the
// maxima of ||q||_M / ||f||_M over q = R M f, R = (i omega M - A)^-1, and sigma_j^2 are the largest eigenvalues of
//     W = R M R^H M = C^-1 M C^-H M,   C = A - i omega M  (the sign cancels),
// which is self-adjoint and non-negative in the M-(semi-)inner product.  So the thick-restart Lanczos iteration of lanczos.hip serves,
// with a COMPLEX basis V (n x (ncv + 1) complex128, V^H M V = I) and the same real symmetric projected matrix: alpha_j = Re h_j,
// beta_j > 0, the eigenvectors Y of T real, the restart's spike real.  This file holds the basis handle, the step and its kernels;
// the outer loop is the one of lsa_lanczos_solve (dense.hip).
//
// One step j (rhs = M v_j is left by the previous step's tail), on ONE factorisation of C (shift-invert mode 0 at sigma = i omega):
//     z = C^-H rhs                          the transposed, conjugated sweeps (ndlu_solve_adjoint_dev)
//     ca = C^H z                            for the check |rhs - ca| <= ksp_rtol |rhs|
//     tm = M z
//     w = C^-1 tm                           the forward sweeps
//     cf = C w                              for the check |tm - cf| <= ksp_rtol |tm|
//     twice:  t = M w;  h = V^H t;  w -= V h    rz_dot_kernel + rz_update_kernel
//     t = M w;  beta^2 = Re w^H t           rz_dot_kernel on the one extra column
//     v_{j+1} = w / beta;  rhs' = t / beta  rz_tail_kernel, which leaves beta^2 and both checks' sums in the step's slot
// lsa_resolvent_set_weights puts a forcing weight Q_f and a response weight Q_q (real symmetric positive semidefinite, e.g. the windowed
// D M D of lsa_csr_window) where M stands: q = R Q_f f, sigma = max ||q||_Qq / ||f||_Qf, W = C^-1 Q_f C^-H Q_q, self-adjoint in the
// Q_q-semi-inner product.  No inverse of a weight appears and the step keeps its launches: rhs = Q_q v_j, tm = Q_f z and t = Q_q w
// (rz_response, rz_forcing) replace the three uses of M; both are M on a new handle, whose bits are those of a handle without weights.
// Nothing in the step needs Re sigma = 0: a shift beta + i omega gives the discounted resolvent.
// One host synchronisation per step (the read-back of the slot).  Each direction decides about its own refinement step
// (direct_solve_enqueue with an explicit direction: the operator's own direction, and the state lsa_op_set_adjoint clears, stay).
//
// Every reduction runs in the fixed order of k_multi_dot / k_multi_axpy for complex128 (rows strided over the 256 threads of a chunk,
// real and imaginary part each through the xor tree of the wavefront, the four waves in wave order, the chunks strided over 64 lanes
// and the same tree; the columns of a row one after the other) and there are no floating-point atomics: two runs give the same bits,
// and so does the unfused form of a step (LSA_LANCZOS_FUSED=0).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "lsa_internal.h"

namespace {

constexpr int kRzThreads = 256;     // four wavefronts of 64
constexpr int kRzColTile = 8;       // basis columns per workgroup of rz_dot_kernel (k_multi_dot's tile)
constexpr int kRzMaxChunks = 2048;  // row chunks of rz_dot_kernel = partial sums per coefficient (k_multi_dot's rule)
constexpr int kRzUnroll = 8;        // basis entries of a row requested at a time by rz_update_kernel (8 x 16 bytes per lane)

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// a complex entry is moved as one 16-byte access (cplx itself is only 8-byte aligned: two 8-byte accesses otherwise); every array of
// this file is 16-byte aligned (hipMalloc, columns of 16 n bytes, slot offsets in whole complex numbers)
typedef double rz_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ cplx rz_ld(const cplx* p) {
    const rz_d2 v = *reinterpret_cast<const rz_d2*>(p);
    return cplx{v.x, v.y};
}
__device__ __forceinline__ void rz_st(cplx* p, cplx v) {
    rz_d2 o;
    o.x = v.re;
    o.y = v.im;
    *reinterpret_cast<rz_d2*>(p) = o;
}

// sum over the 64 lanes by the xor tree of blas.hip's wave_sum; every lane ends with the same value
__device__ __forceinline__ double rz_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ cplx rz_wave_sum(cplx v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        v.re += __shfl_xor(v.re, off, 64);
        v.im += __shfl_xor(v.im, off, 64);
    }
    return v;
}

// the partial sums part[0..nchunks) of one coefficient: lane k adds the chunks k, k + 64, ... in that order (eight requested at a
// time), then the tree; called by a whole wavefront
__device__ __forceinline__ cplx rz_finish_sum(const cplx* __restrict__ part, int nchunks, int lane) {
    cplx a = cplx{0.0, 0.0};
    for (int k0 = lane; k0 < nchunks; k0 += 8 * 64) {
        cplx pv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) pv[u] = (k0 + 64 * u < nchunks) ? rz_ld(part + k0 + 64 * u) : cplx{0.0, 0.0};
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (k0 + 64 * u < nchunks) a = s_add(a, pv[u]);
    }
    return rz_wave_sum(a);
}

// Partial sums of V^H t for the columns 0..ncols-1 and of w^H t (stored as column `ncols`), one pass over V: workgroup (chunk, tile)
// sums kRzColTile columns over the rows of its chunk into part[c * ldp + chunk].  The workgroups of tile 0 also sum the two inner-solve
// checks over their rows when chk_part is given: chk_part[4 chunk + 0..3] = |b1 - z1|^2, |b1|^2, |b2 - z2|^2, |b2|^2.  A full tile
// has its eight 16-byte loads of a row in flight before the first addition.
__global__ __launch_bounds__(kRzThreads) void rz_dot_kernel(int64_t n, int ncols, int64_t rows_per_block, const cplx* __restrict__ V, int64_t ldv,
                                                            const cplx* t, const cplx* w, cplx* __restrict__ part, int ldp,
                                                            const cplx* __restrict__ b1, const cplx* __restrict__ z1, const cplx* __restrict__ b2,
                                                            const cplx* __restrict__ z2, double* __restrict__ chk_part) {
    __shared__ cplx wsum[4][kRzColTile];
    __shared__ double csum[4][4];
    const int chunk = blockIdx.x;
    const int c0 = blockIdx.y * kRzColTile;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r0 = (int64_t)chunk * rows_per_block;
    const int64_t r1 = (r0 + rows_per_block < n) ? r0 + rows_per_block : n;
    // column c of the tile: a basis column, or w for the one behind the basis
    const cplx* col[kRzColTile];
#pragma unroll
    for (int c = 0; c < kRzColTile; ++c) col[c] = (c0 + c < ncols) ? V + (int64_t)(c0 + c) * ldv : w;
    const int nc = (ncols + 1 - c0 < kRzColTile) ? (ncols + 1 - c0) : kRzColTile;
    cplx acc[kRzColTile];
#pragma unroll
    for (int c = 0; c < kRzColTile; ++c) acc[c] = cplx{0.0, 0.0};
    if (nc == kRzColTile) {
        for (int64_t i = r0 + threadIdx.x; i < r1; i += kRzThreads) {
            const cplx tv = rz_ld(t + i);
            cplx v[kRzColTile];
#pragma unroll
            for (int c = 0; c < kRzColTile; ++c) v[c] = rz_ld(col[c] + i);
#pragma unroll
            for (int c = 0; c < kRzColTile; ++c) fma_conj_acc(acc[c], v[c], tv);
        }
    } else {
        for (int64_t i = r0 + threadIdx.x; i < r1; i += kRzThreads) {
            const cplx tv = rz_ld(t + i);
#pragma unroll
            for (int c = 0; c < kRzColTile; ++c)
                if (c < nc) fma_conj_acc(acc[c], rz_ld(col[c] + i), tv);
        }
    }
#pragma unroll
    for (int c = 0; c < kRzColTile; ++c) {
        const cplx s = rz_wave_sum(acc[c]);
        if (lane == 0) wsum[wave][c] = s;
    }
    const bool chk = chk_part != nullptr && blockIdx.y == 0;
    if (chk) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t r = r0 + threadIdx.x; r < r1; r += kRzThreads) {
            const cplx ba = rz_ld(b1 + r), bb = rz_ld(b2 + r);
            const cplx da = s_sub(ba, rz_ld(z1 + r)), db = s_sub(bb, rz_ld(z2 + r));
            s[0] = fma(da.im, da.im, fma(da.re, da.re, s[0]));
            s[1] = fma(ba.im, ba.im, fma(ba.re, ba.re, s[1]));
            s[2] = fma(db.im, db.im, fma(db.re, db.re, s[2]));
            s[3] = fma(bb.im, bb.im, fma(bb.re, bb.re, s[3]));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double v = rz_wave_sum(s[q]);
            if (lane == 0) csum[wave][q] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x < nc) {
        const int c = threadIdx.x;
        rz_st(part + (int64_t)(c0 + c) * ldp + chunk, s_add(s_add(s_add(wsum[0][c], wsum[1][c]), wsum[2][c]), wsum[3][c]));
    }
    if (chk && threadIdx.x >= 64 && threadIdx.x < 68) {
        const int q = threadIdx.x - 64;
        chk_part[4 * chunk + q] = ((csum[0][q] + csum[1][q]) + csum[2][q]) + csum[3][q];
    }
}

// w -= V h for the columns 0..ncols-1.  The prologue finishes h from the partial sums (rz_finish_sum: every workgroup gets the same
// bits; wave q takes the columns q, q + 4, ...); workgroup 0 writes h to h_out for the host.  Then a thread per row, the rows of a
// workgroup strided over the grid: eight entries of the row are requested at a time -- the first eight ahead of the prologue, which
// does not depend on them -- and added column after column.  The dynamic LDS holds h alone (no static LDS in front of it: 16-byte
// aligned entries).
__global__ __launch_bounds__(kRzThreads) void rz_update_kernel(int64_t n, int ncols, const cplx* __restrict__ V, int64_t ldv,
                                                               const cplx* __restrict__ part, int nchunks, int ldp, cplx* w,
                                                               cplx* __restrict__ h_out) {
    extern __shared__ __attribute__((aligned(16))) char rz_dyn[];
    cplx* hs = reinterpret_cast<cplx*>(rz_dyn);  // ncols coefficients
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * kRzThreads;
    int64_t i = (int64_t)blockIdx.x * kRzThreads + threadIdx.x;
    cplx v[kRzUnroll];
#pragma unroll
    for (int u = 0; u < kRzUnroll; ++u) v[u] = (i < n && u < ncols) ? rz_ld(V + i + (int64_t)u * ldv) : cplx{0.0, 0.0};
    for (int c = q; c < ncols; c += 4) {
        const cplx a = rz_finish_sum(part + (int64_t)c * ldp, nchunks, lane);
        if (lane == 0) {
            rz_st(hs + c, a);
            if (blockIdx.x == 0) rz_st(h_out + c, a);
        }
    }
    __syncthreads();
    bool first = true;
    for (; i < n; i += stride) {
        cplx acc = cplx{0.0, 0.0};
        for (int c0 = 0; c0 < ncols; c0 += kRzUnroll) {
            if (!(first && c0 == 0)) {
#pragma unroll
                for (int u = 0; u < kRzUnroll; ++u) v[u] = (c0 + u < ncols) ? rz_ld(V + i + (int64_t)(c0 + u) * ldv) : cplx{0.0, 0.0};
            }
#pragma unroll
            for (int u = 0; u < kRzUnroll; ++u)
                if (c0 + u < ncols) fma_acc(acc, rz_ld(hs + c0 + u), v[u]);
        }
        first = false;
        rz_st(w + i, s_sub(rz_ld(w + i), acc));
    }
}

// From the partial sums of w^H t (part[0..nchunks), rz_finish_sum): beta^2 = its real part, then v_next = w / beta and
// rhs_next = t / beta.  Workgroup 0 leaves beta^2, the imaginary part (rounding) and the four sums of the two inner-solve checks
// (chk_part, nchk quadruples) in out[0..6).  A beta^2 that is not positive and finite scales by zero: the host reads it from the slot
// and stops.
__global__ __launch_bounds__(kRzThreads) void rz_tail_kernel(int64_t n, const cplx* w, const cplx* t, const cplx* __restrict__ part, int nchunks,
                                                             cplx* vnext, cplx* rhs_next, const double* __restrict__ chk_part, int nchk,
                                                             double* __restrict__ out) {
    __shared__ double b2s;
    if (threadIdx.x < 64) {
        const cplx a = rz_finish_sum(part, nchunks, threadIdx.x);
        if (threadIdx.x == 0) b2s = a.re;
        if (blockIdx.x == 0) {
            double c[4] = {0.0, 0.0, 0.0, 0.0};
            if (chk_part)
                for (int k = threadIdx.x; k < nchk; k += 64) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) c[q] += chk_part[4 * k + q];
                }
#pragma unroll
            for (int q = 0; q < 4; ++q) c[q] = rz_wave_sum(c[q]);
            if (threadIdx.x == 0) {
                out[0] = a.re;
                out[1] = a.im;
#pragma unroll
                for (int q = 0; q < 4; ++q) out[2 + q] = c[q];
            }
        }
    }
    __syncthreads();
    const double b2 = b2s;
    const double inv = (b2 > 0.0 && b2 < 1.7e308) ? 1.0 / sqrt(b2) : 0.0;
    const int64_t stride = (int64_t)gridDim.x * kRzThreads;
    for (int64_t i = (int64_t)blockIdx.x * kRzThreads + threadIdx.x; i < n; i += stride) {
        const cplx wi = rz_ld(w + i), ti = rz_ld(t + i);
        rz_st(vnext + i, s_mul(inv, wi));
        rz_st(rhs_next + i, s_mul(inv, ti));
    }
}

// x <- alpha x (the forcing's -1 / gain)
__global__ __launch_bounds__(kRzThreads) void rz_scale_kernel(int64_t n, double alpha, const cplx* x, cplx* y) {
    const int64_t stride = (int64_t)gridDim.x * kRzThreads;
    for (int64_t i = (int64_t)blockIdx.x * kRzThreads + threadIdx.x; i < n; i += stride) rz_st(y + i, s_mul(alpha, rz_ld(x + i)));
}

int rz_check_launch(lsa_ctx* ctx, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lsa_set_error(ctx, LSA_ERR_HIP, "%s: kernel launch failed: %s", what, hipGetErrorString(e));
    return LSA_OK;
}

// the fused kernels unless LSA_LANCZOS_FUSED=0 (the switch of the real basis, read once per process): then k_multi_dot + k_multi_axpy
bool rz_fused() {
    static const bool fused = env_flag("LSA_LANCZOS_FUSED", true);
    return fused;
}

}  // namespace

struct lsa_resolvent {
    lsa_ctx* ctx = nullptr;
    lsa_op* op = nullptr;
    lsa_op_parts P{};
    int64_t n = 0;
    int32_t ncv = 0;
    // the forcing and the response weight (lsa_resolvent_set_weights; borrowed): both are the operator's M on a new handle
    const lsa_mat *Qf = nullptr, *Qq = nullptr;
    // the n x (ncv + 1) arrays: the basis, the restart's second basis (and the Ritz vectors, then the forcings) and, with a row
    // permutation, the output in the caller's numbering (on first use)
    cplx *V = nullptr, *V2 = nullptr, *xtmp = nullptr;
    int32_t* row_perm = nullptr;
    // work vectors: C^-H rhs and C^H of it, M z and the refinement's residual; W v_j, M w and C w
    cplx *za = nullptr, *ca = nullptr, *tm = nullptr, *r = nullptr, *w = nullptr, *t = nullptr, *cf = nullptr;
    cplx* rhs[2] = {nullptr, nullptr};  // M v_j of the current step / of the next one (a step that is redone finds its own intact)
    int cur = 0;
    int32_t rhs_for = -1;        // rhs[cur] holds M v_j for this j, -1: nothing
    cplx* part = nullptr;        // (ncv + 2) x kRzMaxChunks partial sums, a coefficient's chunks side by side
    double* chk_part = nullptr;  // kRzMaxChunks quadruples
    double* slot = nullptr;      // see rz_slot_doubles
    double* rnorms = nullptr;    // the two sums a refinement step's residual pass leaves (not read)
    cplx* qdev = nullptr;        // (ncv + 1)^2: the restart's and the Ritz vectors' coefficients
    double* imag2 = nullptr;     // ncv + 1: what k_columns_canonical reports (not read)
    // each direction carries its own refinement step once one of its solves missed ksp_rtol
    bool refine_adj = false, refine_fwd = false;
    int64_t solves_adj = 0, solves_fwd = 0, refined_adj = 0, refined_fwd = 0;
    std::vector<double> hslot;
    // lsa_resolvent_set_block_forcings: the forcings' adjoint solves as one block solve.  Its work vectors (M q_c and C^-H M q_c,
    // blk_cols columns each) and the three sums per column of the check are made by the first block call.
    bool block_forcings = false;
    cplx *blk_tm = nullptr, *blk_za = nullptr;
    double* blk_norms = nullptr;
    int32_t blk_cols = 0;
};

namespace {

// The slot, in doubles: h of pass 1 (ncv + 1 complex), h of pass 2 (ncv + 1 complex), then at rz_out_at: beta^2, Im w^H t, |rhs - C^H z|^2,
// |rhs|^2, |tm - C w|^2, |tm|^2, the unfused form's w^H t (complex), |z|^2 and |w|^2 of refined solves
size_t rz_out_at(int32_t ncv) { return (size_t)4 * (ncv + 1); }
size_t rz_slot_doubles(int32_t ncv) { return rz_out_at(ncv) + 10; }

void rz_free(lsa_resolvent* l) {
    for (void* p : {(void*)l->V, (void*)l->V2, (void*)l->xtmp, (void*)l->row_perm, (void*)l->za, (void*)l->ca, (void*)l->tm, (void*)l->r, (void*)l->w,
                    (void*)l->t, (void*)l->cf, (void*)l->rhs[0], (void*)l->rhs[1], (void*)l->part, (void*)l->chk_part, (void*)l->slot, (void*)l->rnorms,
                    (void*)l->qdev, (void*)l->imag2, (void*)l->blk_tm, (void*)l->blk_za, (void*)l->blk_norms})
        if (p) (void)hipFree(p);
    delete l;
}

cplx* rz_col(const lsa_resolvent* l, int32_t j) { return l->V + (size_t)j * (size_t)l->n; }

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

// M-orthogonalise l->w against the columns 0..ncols-1 (two passes), then v = w / beta into column `target` and M v into the other
// right-hand side buffer; the slot's beta^2 and check sums are read back by the caller.  chk: this step's two check pairs
// (rhs[cur] against ca, tm against cf) ride in the first reduction.
int rz_orth_tail(lsa_ctx* ctx, lsa_resolvent* l, int32_t ncols, int32_t target, bool chk) {
    const int64_t n = l->n;
    cplx* vnext = rz_col(l, target);
    cplx* rhs_next = l->rhs[l->cur ^ 1];
    const size_t h_doubles = (size_t)2 * (l->ncv + 1);
    double* out = l->slot + rz_out_at(l->ncv);
    const int tblocks = rz_grid(ctx, n, 8);
    if (rz_fused()) {
        // k_multi_dot's chunks: at most 2048 of them, whole multiples of 256 rows, at least 512 rows
        int64_t rows_per_block = ((n + kRzMaxChunks - 1) / kRzMaxChunks + kRzThreads - 1) / kRzThreads * kRzThreads;
        rows_per_block = std::max<int64_t>(rows_per_block, 2 * kRzThreads);
        const int nchunks = (int)std::max<int64_t>((n + rows_per_block - 1) / rows_per_block, 1);
        // every workgroup of the update finishes h for itself: a few hundred of them, their rows strided over the grid
        const int ublocks = rz_grid(ctx, n, 2);
        for (int pass = 0; pass < 2 && ncols > 0; ++pass) {
            LSA_CHECK(rz_response(ctx, l, l->w, l->t));
            const int tiles = (ncols + 1 + kRzColTile - 1) / kRzColTile;
            const bool c = chk && pass == 0;
            hipLaunchKernelGGL(rz_dot_kernel, dim3(nchunks, tiles), dim3(kRzThreads), 0, ctx->stream, n, ncols, rows_per_block, l->V, n, l->t, l->w,
                               l->part, nchunks, c ? l->rhs[l->cur] : nullptr, c ? l->ca : nullptr, c ? l->tm : nullptr, c ? l->cf : nullptr,
                               c ? l->chk_part : nullptr);
            hipLaunchKernelGGL(rz_update_kernel, dim3(ublocks), dim3(kRzThreads), (size_t)ncols * sizeof(cplx), ctx->stream, n, ncols, l->V, n,
                               l->part, nchunks, nchunks, l->w, (cplx*)(l->slot + (size_t)pass * h_doubles));
        }
        LSA_CHECK(rz_response(ctx, l, l->w, l->t));
        const bool c = chk && ncols == 0;
        hipLaunchKernelGGL(rz_dot_kernel, dim3(nchunks, 1), dim3(kRzThreads), 0, ctx->stream, n, 0, rows_per_block, l->V, n, l->t, l->w, l->part, nchunks,
                           c ? l->rhs[l->cur] : nullptr, c ? l->ca : nullptr, c ? l->tm : nullptr, c ? l->cf : nullptr, c ? l->chk_part : nullptr);
        hipLaunchKernelGGL(rz_tail_kernel, dim3(tblocks), dim3(kRzThreads), 0, ctx->stream, n, l->w, l->t, l->part, nchunks, vnext, rhs_next,
                           chk ? l->chk_part : nullptr, nchunks, out);
        return rz_check_launch(ctx, "resolvent step");
    }
    // the unfused form: the library's multi-dot and multi-axpy, the same tail with single partial sums
    if (chk) {
        LSA_CHECK(k_residual_norms(ctx, LSA_C128, n, l->rhs[l->cur], l->ca, l->r, l->chk_part));
        LSA_CHECK(k_residual_norms(ctx, LSA_C128, n, l->tm, l->cf, l->r, l->chk_part + 2));
    }
    for (int pass = 0; pass < 2 && ncols > 0; ++pass) {
        LSA_CHECK(rz_response(ctx, l, l->w, l->t));
        double* h = l->slot + (size_t)pass * h_doubles;
        LSA_CHECK(k_multi_dot(ctx, LSA_C128, n, ncols, l->V, n, l->t, h));
        LSA_CHECK(k_multi_axpy(ctx, LSA_C128, n, ncols, l->V, n, h, l->w, nullptr));
    }
    LSA_CHECK(rz_response(ctx, l, l->w, l->t));
    LSA_CHECK(k_multi_dot(ctx, LSA_C128, n, 1, l->w, n, l->t, out + 6));
    hipLaunchKernelGGL(rz_tail_kernel, dim3(tblocks), dim3(kRzThreads), 0, ctx->stream, n, l->w, l->t, (const cplx*)(out + 6), 1, vnext, rhs_next,
                       chk ? l->chk_part : nullptr, 1, out);
    return rz_check_launch(ctx, "resolvent step (unfused)");
}

// the slot to the host: one synchronisation
int rz_read_slot(lsa_ctx* ctx, lsa_resolvent* l) {
    const size_t bytes = rz_slot_doubles(l->ncv) * sizeof(double);
    LSA_CHECK(lsa_ensure_scratch(ctx, 0, bytes));
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(ctx->pinned, l->slot, bytes, hipMemcpyDeviceToHost, ctx->stream));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(l->hslot.data(), ctx->pinned, bytes);
    return LSA_OK;
}

// The library's judgement of a direct solve (gmres_run, lsa_lanczos_extend): within ksp_rtol, or, after the refinement step, a
// backward error within 1e-12 ||C||_F.  0: accepted (*backward says by which rule), 1: do the step again with the refinement
// step switched on, -1: diverged.
int rz_judge(const lsa_op_parts& P, bool refine, double res, double bnorm, double xnorm, bool* backward) {
    *backward = refine && res > P.ksp_rtol * bnorm && P.normF > 0.0 && res <= 1e-12 * P.normF * xnorm;
    if (res <= P.ksp_rtol * bnorm || *backward) return 0;
    return (!refine && std::isfinite(res)) ? 1 : -1;
}

void rz_book(lsa_resolvent* l, bool adjoint, bool refine, bool backward, double res, double bnorm) {
    if (backward) ++l->P.st->backward_accepted;
    stats_book_direct_solve(l->P.st, 1, refine, res, bnorm);
    ++(adjoint ? l->solves_adj : l->solves_fwd);
    if (refine) ++(adjoint ? l->refined_adj : l->refined_fwd);
}

int rz_scatter_out(lsa_ctx* ctx, lsa_resolvent* l, int32_t nvec, cplx* host) {
    const size_t vb = (size_t)l->n * sizeof(cplx);
    const cplx* src = l->V2;
    if (l->row_perm) {
        if (!l->xtmp) LSA_HIP_ALLOC(ctx, hipMalloc((void**)&l->xtmp, std::max<size_t>(vb, 16) * (size_t)(l->ncv + 1)));
        LSA_CHECK(k_scatter_rows(ctx, LSA_C128, l->n, nvec, l->row_perm, l->V2, l->xtmp));
        src = l->xtmp;
    }
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(host, src, vb * (size_t)nvec, hipMemcpyDeviceToHost, ctx->stream));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return LSA_OK;
}

// the real host matrix Y (m x k, ldy) as complex numbers for k_basis_gemm on the complex basis
int rz_basis_times_real(lsa_ctx* ctx, lsa_resolvent* l, int32_t m, int32_t k, const double* Y, int32_t ldy) {
    std::vector<cplx> Yc((size_t)m * k);
    for (int32_t c = 0; c < k; ++c)
        for (int32_t i = 0; i < m; ++i) Yc[(size_t)c * m + i] = cplx{Y[(size_t)c * ldy + i], 0.0};
    return basis_times_host_matrix(ctx, LSA_C128, l->n, m, k, l->V, Yc.data(), m, l->qdev, l->V2, 0);
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
    if (!ctx || !l || !host_v) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent: null argument");
    if (j < 0 || j > l->ncv) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent: column %d out of range", j);
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(l->w, host_v, (size_t)l->n * sizeof(cplx), hipMemcpyHostToDevice, ctx->stream));
    LSA_CHECK(rz_orth_tail(ctx, l, j, j, false));
    LSA_CHECK(rz_read_slot(ctx, l));
    const double b2 = l->hslot[rz_out_at(l->ncv)];
    if (!(b2 > 0.0) || !std::isfinite(b2))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent: v^H M v = %.3e for the injected vector: M is not positive definite on the Krylov space (or "
                                               "the vector is zero or not finite)", b2);
    l->cur ^= 1;
    l->rhs_for = j;
    return LSA_OK;
}

int resolvent_restart(lsa_ctx* ctx, lsa_resolvent* l, int32_t m, int32_t knew, const double* Y, int32_t ldy) {
    if (!ctx || !l || !Y) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent restart: null argument");
    if (m < 1 || m > l->ncv || knew < 1 || knew > m || ldy < m) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent restart: bad sizes m=%d knew=%d", m, knew);
    LSA_CHECK(rz_basis_times_real(ctx, l, m, knew, Y, ldy));
    LSA_CHECK(k_copy(ctx, LSA_C128, l->n, rz_col(l, m), l->V2 + (size_t)knew * (size_t)l->n));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    std::swap(l->V, l->V2);
    if (l->rhs_for == m) l->rhs_for = knew;  // (the same vector under its new index)
    else l->rhs_for = -1;
    return LSA_OK;
}

int resolvent_ritz_vectors(lsa_ctx* ctx, lsa_resolvent* l, int32_t m, int32_t nvec, const double* Y, int32_t ldy, cplx* Q) {
    if (!ctx || !l || !Y || !Q) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent vectors: null argument");
    if (m < 1 || m > l->ncv || nvec < 0 || nvec > l->ncv || ldy < m) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent vectors: bad sizes");
    if (nvec == 0) return LSA_OK;
    LSA_CHECK(rz_basis_times_real(ctx, l, m, nvec, Y, ldy));
    LSA_CHECK(k_columns_canonical(ctx, l->n, nvec, l->V2, l->n, 0, l->imag2));
    return rz_scatter_out(ctx, l, nvec, Q);
}

namespace {

// The forcings' first attempts as ONE adjoint block solve (lsa_resolvent_set_block_forcings, no refinement step switched on yet):
// tm_c = M q_c for all columns, z_c = C^-H tm_c in the wide passes of the transposed sweeps, then per column what
// direct_solve_enqueue and the loop of resolvent_forcings queue behind the sweeps -- the check product C^H z_c, its residual sums
// and |z_c|^2 -- and one read-back for all of them.  The columns are judged in order: an accepted one is booked and scaled as the
// loop does it; the first that misses ksp_rtol switches the refinement step on and ends the block.  *done: the columns finished;
// the loop takes the rest (every column is the loop's, bit for bit and count for count).  An allocation that fails leaves all
// columns to the loop.
int rz_forcings_block(lsa_ctx* ctx, lsa_resolvent* l, int32_t nvec, const double* gain, int32_t* done) {
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
    for (int32_t c = 0; c < nvec; ++c) LSA_CHECK(k_spmv(ctx, l->Qq, LSA_C128, l->V2 + (size_t)c * (size_t)n, l->blk_tm + (size_t)c * (size_t)n));
    LSA_CHECK(ndlu_solve_multi_adjoint_dev(ctx, l->P.nd, 1, LSA_C128, nvec, l->blk_tm, n, l->blk_za, n));
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
        const int verdict = rz_judge(l->P, false, res, bnorm, xnorm, &backward);
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
                           l->V2 + (size_t)c * (size_t)n);
        LSA_CHECK(rz_check_launch(ctx, "resolvent forcings"));
        *done = c + 1;
    }
    return LSA_OK;
}

}  // namespace

int resolvent_forcings(lsa_ctx* ctx, lsa_resolvent* l, int32_t nvec, const double* gain, cplx* F) {
    if (!ctx || !l || !gain || !F) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent forcings: null argument");
    if (nvec < 0 || nvec > l->ncv) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent forcings: bad sizes");
    const int64_t n = l->n;
    double* norms = l->slot + rz_out_at(l->ncv);  // (the step's slot is free between steps: |rhs - C^H z|^2, |rhs|^2, and |z|^2 behind them)
    int32_t first = 0;
    if (l->block_forcings && !l->refine_adj && nvec > 1) LSA_CHECK(rz_forcings_block(ctx, l, nvec, gain, &first));
    for (int32_t c = first; c < nvec; ++c) {
        if (!(gain[c] > 0.0) || !std::isfinite(gain[c]))
            return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent forcings: gain %d is %.3e: no forcing belongs to it", c, gain[c]);
        cplx* q = l->V2 + (size_t)c * (size_t)n;
        LSA_CHECK(rz_response(ctx, l, q, l->tm));
        while (true) {
            const bool refine = l->refine_adj;
            LSA_CHECK(direct_solve_enqueue(ctx, l->op, LSA_C128, l->tm, l->za, l->ca, l->r, refine, l->rnorms, 1));
            LSA_CHECK(k_residual_norms(ctx, LSA_C128, n, l->tm, l->ca, l->r, norms));
            LSA_CHECK(k_nrm2(ctx, LSA_C128, n, l->za, norms + 2));
            LSA_CHECK(rz_read_slot(ctx, l));
            const size_t at = rz_out_at(l->ncv);
            const double res = std::sqrt(l->hslot[at]), bnorm = std::sqrt(l->hslot[at + 1]), xnorm = std::sqrt(l->hslot[at + 2]);
            bool backward = false;
            const int verdict = rz_judge(l->P, refine, res, bnorm, xnorm, &backward);
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
        LSA_CHECK(rz_check_launch(ctx, "resolvent forcings"));
    }
    if (nvec == 0) return LSA_OK;
    return rz_scatter_out(ctx, l, nvec, F);
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
    l->hslot.assign(rz_slot_doubles(ncv), 0.0);
    const size_t vb = (size_t)std::max<int64_t>(l->n, 1) * sizeof(cplx);
    bool ok = hipMalloc((void**)&l->V, vb * (size_t)(ncv + 1)) == hipSuccess && hipMalloc((void**)&l->V2, vb * (size_t)(ncv + 1)) == hipSuccess;
    for (cplx** p : {&l->za, &l->ca, &l->tm, &l->r, &l->w, &l->t, &l->cf, &l->rhs[0], &l->rhs[1]}) ok = ok && hipMalloc((void**)p, vb) == hipSuccess;
    ok = ok && hipMalloc((void**)&l->part, (size_t)kRzMaxChunks * (size_t)(ncv + 2) * sizeof(cplx)) == hipSuccess &&
         hipMalloc((void**)&l->chk_part, (size_t)kRzMaxChunks * 4 * sizeof(double)) == hipSuccess &&
         hipMalloc((void**)&l->slot, rz_slot_doubles(ncv) * sizeof(double)) == hipSuccess && hipMalloc((void**)&l->rnorms, 2 * sizeof(double)) == hipSuccess &&
         hipMalloc((void**)&l->qdev, (size_t)(ncv + 1) * (size_t)(ncv + 1) * sizeof(cplx)) == hipSuccess &&
         hipMalloc((void**)&l->imag2, (size_t)(ncv + 1) * sizeof(double)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        rz_free(l);
        return lsa_set_error(ctx, LSA_ERR_OOM, "lsa_resolvent_create: out of device memory (n=%lld, ncv=%d)", (long long)P.n, ncv);
    }
    (void)hipMemsetAsync(l->slot, 0, rz_slot_doubles(ncv) * sizeof(double), ctx->stream);
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
    return basis_upload_row_permutation(ctx, "lsa_resolvent_set_row_permutation", l->n, perm, &l->row_perm);
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
    // other inner products begin as a new handle does: no right-hand side is left over, the refinement steps are off again, and a
    // start vector must follow (the basis in hand is orthonormal in the old response weight)
    l->rhs_for = -1;
    l->refine_adj = l->refine_fwd = false;
    return LSA_OK;
}

int lsa_resolvent_set_start(lsa_ctx* ctx, lsa_resolvent* l, const void* host_v) { return resolvent_inject(ctx, l, 0, (const cplx*)host_v); }

int lsa_resolvent_extend(lsa_ctx* ctx, lsa_resolvent* l, int32_t j0, int32_t j1, double* T, int32_t ldt, int32_t* breakdown) {
    if (!ctx || !l || !T) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_extend: null argument");
    if (j0 < 0 || j1 < j0 || j1 > l->ncv || ldt < j1 + 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_extend: bad step range [%d, %d) for ncv %d", j0, j1, l->ncv);
    if (breakdown) *breakdown = -1;
    const double t0 = now_s();
    const int64_t n = l->n;
    lsa_stats* st = l->P.st;
    const size_t at = rz_out_at(l->ncv), h2_at = (size_t)2 * (l->ncv + 1);
    int rc = LSA_OK;
    for (int32_t j = j0; j < j1 && rc == LSA_OK; ++j) {
        if (l->rhs_for != j) {  // (after a restart that moved another column here)
            rc = rz_response(ctx, l, rz_col(l, j), l->rhs[l->cur]);
            if (rc != LSA_OK) break;
            l->rhs_for = j;
        }
        while (true) {
            const bool ra = l->refine_adj, rf = l->refine_fwd;
            // z = C^-H rhs, ca = C^H z;  tm = M z;  w = C^-1 tm, cf = C w  (each with its direction's refinement step once switched on)
            rc = direct_solve_enqueue(ctx, l->op, LSA_C128, l->rhs[l->cur], l->za, l->ca, l->r, ra, l->rnorms, 1);
            if (rc == LSA_OK && ra) rc = k_nrm2(ctx, LSA_C128, n, l->za, l->slot + at + 8);  // for the backward-error judgement below
            if (rc == LSA_OK) rc = rz_forcing(ctx, l, l->za, l->tm);
            if (rc == LSA_OK) rc = direct_solve_enqueue(ctx, l->op, LSA_C128, l->tm, l->w, l->cf, l->r, rf, l->rnorms, 0);
            if (rc == LSA_OK && rf) rc = k_nrm2(ctx, LSA_C128, n, l->w, l->slot + at + 9);
            if (rc == LSA_OK) rc = rz_orth_tail(ctx, l, j + 1, j + 1, true);
            if (rc == LSA_OK) rc = rz_read_slot(ctx, l);
            if (rc != LSA_OK) break;
            const double res_a = std::sqrt(l->hslot[at + 2]), b_a = std::sqrt(l->hslot[at + 3]);
            const double res_f = std::sqrt(l->hslot[at + 4]), b_f = std::sqrt(l->hslot[at + 5]);
            bool back_a = false, back_f = false;
            const int va = rz_judge(l->P, ra, res_a, b_a, std::sqrt(l->hslot[at + 8]), &back_a);
            const int vf = rz_judge(l->P, rf, res_f, b_f, std::sqrt(l->hslot[at + 9]), &back_f);
            if (va == 0 && vf == 0) {
                rz_book(l, true, ra, back_a, res_a, b_a);
                rz_book(l, false, rf, back_f, res_f, b_f);
                break;
            }
            if (va < 0 || vf < 0) {
                const bool adj = va < 0;
                const double res = adj ? res_a : res_f, bn = adj ? b_a : b_f;
                rc = lsa_set_error(ctx, LSA_ERR_DIVERGED, "lsa_resolvent_extend: the %s solve of step %d left a relative residual of %.3e after its refinement "
                                                          "step (ksp_rtol %.1e) and a backward error above 1e-12 ||C||_F", adj ? "adjoint" : "forward", j,
                                   bn > 0.0 ? res / bn : res, l->P.ksp_rtol);
                break;
            }
            // from here on every solve of a direction that missed carries the refinement step; this step is done again
            if (va > 0) l->refine_adj = true;
            if (vf > 0) l->refine_fwd = true;
        }
        if (rc != LSA_OK) break;
        // alpha_j = Re h_j: W is self-adjoint in the M-inner product, the imaginary part is rounding and is dropped
        const double alpha = l->hslot[2 * (size_t)j] + l->hslot[h2_at + 2 * (size_t)j];
        const double b2 = l->hslot[at];
        if (!std::isfinite(alpha) || !std::isfinite(b2)) {
            rc = lsa_set_error(ctx, LSA_ERR_NONFINITE, "resolvent: non-finite recurrence coefficient at step %d", j);
            break;
        }
        // what is left of w after both passes, against the size of what was taken out of it (the rule of the real basis)
        double colmax = std::fabs(alpha);
        for (int32_t i = 0; i < j; ++i)
            colmax = std::max(colmax, std::hypot(l->hslot[2 * (size_t)i] + l->hslot[h2_at + 2 * (size_t)i], l->hslot[2 * (size_t)i + 1] + l->hslot[h2_at + 2 * (size_t)i + 1]));
        const double thr = 1e-14 * std::max(colmax, 1e-300);
        if (b2 < -thr * thr) {
            rc = lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_extend: w^H M w = %.3e at step %d: M is not positive semidefinite on the Krylov space", b2, j);
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

int lsa_resolvent_basis(lsa_ctx* ctx, const lsa_resolvent* l, int32_t ncols, void* host_V) {
    if (!ctx || !l || !host_V) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_basis: null argument");
    if (ncols < 0 || ncols > l->ncv + 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_basis: %d columns of %d", ncols, l->ncv + 1);
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(host_V, l->V, (size_t)l->n * (size_t)ncols * sizeof(cplx), hipMemcpyDeviceToHost, ctx->stream));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return LSA_OK;
}

}  // extern "C"
