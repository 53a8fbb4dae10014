// Thick-restart Lanczos (the symmetric variant of Krylov-Schur): the basis of the library's self-adjoint outer iterations.
//
// The symmetric-definite pencil K x = lambda M x is what SLEPc runs behind EPS_GHEP / EPS_HEP (reference: Solver/utils.py:244-270 with
// iEpsProblemType.GHEP; Elasticity/utils.py:141-155): OP = (K - sigma M)^-1 M with a real sigma is self-adjoint in the M-inner product,
// so the basis V (n x (ncv + 1) doubles) is kept M-orthonormal, V^T M V = I, the projected matrix is real symmetric, and no complex
// number is stored or moved: half of the bytes of the general path's basis, sweeps and products.  Transient growth (growth.hip) puts a
// march of solves behind the step of the same real basis; the resolvent (resolvent.hip) has complex vectors and the same real
// symmetric projected matrix (alpha_j = Re h_j, beta_j > 0, the eigenvectors Y of T real, the restart's spike real), so it owns this
// basis with complex scalars (LSA_C128: V^H Q V = I) and its two solves are the operator behind the step.  This file holds the one
// basis handle for both scalar types, the step and its kernels; the outer loop and the dense symmetric eigen-solve are
// lsa_lanczos_solve and lsa_dense_syev (dense.hip).
//
// One step j (rhs = Q v_j is left by the previous step's tail; Q: the inner product's matrix, M unless lanczos_set_inner_product gave
// another):
//     w = OP v_j from rhs                   the operator (lanczos_operator), which names the inner solves to check: pairs (b, z = C x)
//     twice:  t = Q w;  h = V^H t;  w -= V h    the dot and the update kernel: full reorthogonalisation against v_0..v_j; the first
//                                           reduction also sums |b - z|^2 and |b|^2 of the operator's checks
//     t = Q w;  beta^2 = Re w^H t           the dot kernel on the one extra column
//     v_{j+1} = w / beta;  rhs' = t / beta  the tail kernel, which also leaves beta^2 and the checks' sums in the step's slot
// Three products with Q per step, one host synchronisation (the read-back of the slot), after which the operator judges its solves:
// accepted, or the step is done again (a refinement step switched on), or the iteration fails.  For a standard problem (no M, real
// scalars only) t is w.  The default operator of a real basis is the single solve
//     w = C^-1 rhs                          the real sweeps of the exact LU (ndlu_solve_dev, float64 vectors)
//     z = C w                               for the check |rhs - z| <= ksp_rtol |rhs| (one refinement step if it fails)
// on the op's shared refinement flag.
//
// The step kernels exist per scalar type and are not one template: lz_* move 8-byte words, two rows in flight per lane, rz_* move
// 16-byte entries one row at a time (the comment of growth.hip says why a lane's rows cannot be paired into 16-byte loads of doubles).
// Every reduction runs in a fixed order (per-thread strided sums, a shuffle tree inside the wavefront -- real and imaginary part each
// -- the four wave sums in wave order, the chunks' partial sums strided over 64 lanes and the same tree) and there are no
// floating-point atomics: two runs give the same bits, and the order is that of k_multi_dot / k_multi_axpy, so the unfused form of a
// step (LSA_LANCZOS_FUSED=0) gives them too.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "lsa_internal.h"

namespace {

constexpr int kLzThreads = 256;  // four wavefronts of 64
constexpr int kLzColTile = 8;    // basis columns per workgroup of the dot kernels (k_multi_dot's tile)
constexpr int kLzUnroll = 16;    // basis entries of a row requested at a time by lz_update_kernel
constexpr int kRzUnroll = 8;     // ... by rz_update_kernel (8 x 16 bytes per lane)

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The sums of these kernels are taken in the order of the library's unfused kernels (k_multi_dot: rows strided over the 256
// threads of a chunk, xor tree over the wavefront, the four waves in wave order, the chunks strided over 64 lanes and the same
// tree; k_multi_axpy: the columns of a row one after the other), so that the fused and the unfused form of a step (LSA_LANCZOS_FUSED)
// give the same bits: a Krylov basis amplifies a difference of one rounding to 1e-8 within 40 steps, and nothing short of the same
// order keeps the two forms comparable.

// sum over the 64 lanes by the xor tree of blas.hip's wave_sum; every lane ends with the same value
__device__ __forceinline__ double lz_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ cplx lz_wave_sum(cplx v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        v.re += __shfl_xor(v.re, off, 64);
        v.im += __shfl_xor(v.im, off, 64);
    }
    return v;
}

// the partial sums part[0..nchunks) of one coefficient: lane k adds the chunks k, k + 64, ... in that order (eight requested at a
// time), then the tree; called by a whole wavefront
__device__ __forceinline__ double lz_finish_sum(const double* __restrict__ part, int nchunks, int lane) {
    double a = 0.0;
    for (int k0 = lane; k0 < nchunks; k0 += 8 * 64) {
        double pv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) pv[u] = (k0 + 64 * u < nchunks) ? part[k0 + 64 * u] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (k0 + 64 * u < nchunks) a += pv[u];
    }
    return lz_wave_sum(a);
}
__device__ __forceinline__ cplx lz_finish_sum(const cplx* __restrict__ part, int nchunks, int lane) {
    cplx a = cplx{0.0, 0.0};
    for (int k0 = lane; k0 < nchunks; k0 += 8 * 64) {
        cplx pv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) pv[u] = (k0 + 64 * u < nchunks) ? rz_ld(part + k0 + 64 * u) : cplx{0.0, 0.0};
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (k0 + 64 * u < nchunks) a = s_add(a, pv[u]);
    }
    return lz_wave_sum(a);
}

// ---- the step kernels for real scalars ---------------------------------------------------------------------------------------------
// Partial sums of V^T t for the columns 0..ncols-1 and of w^T t (stored as column `ncols`), one pass over V: workgroup
// (chunk, tile) sums kLzColTile columns over the rows of its chunk into part[c * ldp + chunk].  The workgroups of tile 0 also sum
// the inner-solve check over their rows when chk_part is given: chk_part[2 chunk] = |chk_b - chk_z|^2, [2 chunk + 1] = |chk_b|^2.
// Two rows per thread and trip, so that 2 x kLzColTile loads of V are in flight per lane before the first addition (the additions
// into a column's sum keep the order of a one-row loop).
__global__ __launch_bounds__(kLzThreads) void lz_dot_kernel(int64_t n, int ncols, int64_t rows_per_block, const double* __restrict__ V, int64_t ldv,
                                                            const double* t, const double* w, double* __restrict__ part, int ldp,
                                                            const double* __restrict__ chk_b, const double* __restrict__ chk_z,
                                                            double* __restrict__ chk_part) {
    __shared__ double wsum[4][kLzColTile];
    __shared__ double csum[4][2];
    const int chunk = blockIdx.x;
    const int c0 = blockIdx.y * kLzColTile;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r0 = (int64_t)chunk * rows_per_block;
    const int64_t r1 = (r0 + rows_per_block < n) ? r0 + rows_per_block : n;
    // column c of the tile: a basis column, or w for the one behind the basis
    const double* col[kLzColTile];
#pragma unroll
    for (int c = 0; c < kLzColTile; ++c) col[c] = (c0 + c < ncols) ? V + (int64_t)(c0 + c) * ldv : w;
    const int nc = (ncols + 1 - c0 < kLzColTile) ? (ncols + 1 - c0) : kLzColTile;
    double acc[kLzColTile];
#pragma unroll
    for (int c = 0; c < kLzColTile; ++c) acc[c] = 0.0;
    int64_t i = r0 + threadIdx.x;
    if (nc == kLzColTile) {
        for (; i + kLzThreads < r1; i += 2 * kLzThreads) {
            const double ta = t[i], tb = t[i + kLzThreads];
            double va[kLzColTile], vb[kLzColTile];
#pragma unroll
            for (int c = 0; c < kLzColTile; ++c) {
                va[c] = col[c][i];
                vb[c] = col[c][i + kLzThreads];
            }
#pragma unroll
            for (int c = 0; c < kLzColTile; ++c) {
                acc[c] = fma(va[c], ta, acc[c]);
                acc[c] = fma(vb[c], tb, acc[c]);
            }
        }
    }
    for (; i < r1; i += kLzThreads) {
        const double tv = t[i];
#pragma unroll
        for (int c = 0; c < kLzColTile; ++c)
            if (c < nc) acc[c] = fma(col[c][i], tv, acc[c]);
    }
#pragma unroll
    for (int c = 0; c < kLzColTile; ++c) {
        const double s = lz_wave_sum(acc[c]);
        if (lane == 0) wsum[wave][c] = s;
    }
    const bool chk = chk_part != nullptr && blockIdx.y == 0;
    if (chk) {
        double rw = 0.0, rb = 0.0;
        for (int64_t r = r0 + threadIdx.x; r < r1; r += kLzThreads) {
            const double b = chk_b[r], d = b - chk_z[r];
            rw = fma(d, d, rw);
            rb = fma(b, b, rb);
        }
        rw = lz_wave_sum(rw);
        rb = lz_wave_sum(rb);
        if (lane == 0) {
            csum[wave][0] = rw;
            csum[wave][1] = rb;
        }
    }
    __syncthreads();
    if (threadIdx.x < nc) {
        const int c = threadIdx.x;
        part[(int64_t)(c0 + c) * ldp + chunk] = ((wsum[0][c] + wsum[1][c]) + wsum[2][c]) + wsum[3][c];
    }
    if (chk && threadIdx.x >= 64 && threadIdx.x < 66) {
        const int q = threadIdx.x - 64;
        chk_part[2 * chunk + q] = ((csum[0][q] + csum[1][q]) + csum[2][q]) + csum[3][q];
    }
}

// w -= V h for the columns 0..ncols-1.  The prologue finishes h from the partial sums (lz_finish_sum: every workgroup gets the
// same bits; wave q takes the columns q, q + 4, ...); workgroup 0 writes h to h_out for the host.  Then a thread per row, the rows
// of a workgroup strided over the grid: sixteen entries of the row are requested at a time -- the first sixteen ahead of the
// prologue, which does not depend on them -- and added column after column.
__global__ __launch_bounds__(kLzThreads) void lz_update_kernel(int64_t n, int ncols, const double* __restrict__ V, int64_t ldv,
                                                               const double* __restrict__ part, int nchunks, int ldp, double* w,
                                                               double* __restrict__ h_out) {
    extern __shared__ double hs[];  // ncols coefficients
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * kLzThreads;
    int64_t i = (int64_t)blockIdx.x * kLzThreads + threadIdx.x;
    double v[kLzUnroll];
#pragma unroll
    for (int u = 0; u < kLzUnroll; ++u) v[u] = (i < n && u < ncols) ? V[i + (int64_t)u * ldv] : 0.0;
    for (int c = q; c < ncols; c += 4) {
        const double a = lz_finish_sum(part + (int64_t)c * ldp, nchunks, lane);
        if (lane == 0) {
            hs[c] = a;
            if (blockIdx.x == 0) h_out[c] = a;
        }
    }
    __syncthreads();
    bool first = true;
    for (; i < n; i += stride) {
        double acc = 0.0;
        for (int c0 = 0; c0 < ncols; c0 += kLzUnroll) {
            if (!(first && c0 == 0)) {
#pragma unroll
                for (int u = 0; u < kLzUnroll; ++u) v[u] = (c0 + u < ncols) ? V[i + (int64_t)(c0 + u) * ldv] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kLzUnroll; ++u)
                if (c0 + u < ncols) acc = fma(hs[c0 + u], v[u], acc);
        }
        first = false;
        w[i] -= acc;
    }
}

// From the partial sums of w^T t (part[0..nchunks), lz_finish_sum): beta^2, then v_next = w / beta and rhs_next = t / beta.
// Workgroup 0 leaves beta^2 and the two sums of the inner-solve check (chk_part, nchk pairs) in out[0..2].  A beta^2 that is not
// positive and finite scales by zero: the host reads it from the slot and stops.
__global__ __launch_bounds__(kLzThreads) void lz_tail_kernel(int64_t n, const double* w, const double* t, const double* __restrict__ part, int nchunks,
                                                             double* vnext, double* rhs_next, const double* __restrict__ chk_part, int nchk,
                                                             double* __restrict__ out) {
    __shared__ double b2s;
    if (threadIdx.x < 64) {
        const double a = lz_finish_sum(part, nchunks, threadIdx.x);
        if (threadIdx.x == 0) b2s = a;
        if (blockIdx.x == 0) {
            double c0 = 0.0, c1 = 0.0;
            if (chk_part)
                for (int k = threadIdx.x; k < nchk; k += 64) {
                    c0 += chk_part[2 * k];
                    c1 += chk_part[2 * k + 1];
                }
            c0 = lz_wave_sum(c0);
            c1 = lz_wave_sum(c1);
            if (threadIdx.x == 0) {
                out[0] = a;
                out[1] = c0;
                out[2] = c1;
            }
        }
    }
    __syncthreads();
    const double b2 = b2s;
    const double inv = (b2 > 0.0 && b2 < 1.7e308) ? 1.0 / sqrt(b2) : 0.0;
    const int64_t stride = (int64_t)gridDim.x * kLzThreads;
    for (int64_t i = (int64_t)blockIdx.x * kLzThreads + threadIdx.x; i < n; i += stride) {
        const double wi = w[i], ti = t[i];
        vnext[i] = wi * inv;
        rhs_next[i] = ti * inv;
    }
}

// Each column's entry of largest magnitude (the first of equals) made positive: one workgroup per column.
__global__ __launch_bounds__(kLzThreads) void lz_sign_kernel(int64_t n, double* X, int64_t ldx) {
    __shared__ double bm[kLzThreads];
    __shared__ long long bi[kLzThreads];
    double* x = X + (int64_t)blockIdx.x * ldx;
    double best = -1.0;
    long long at = 0;
    for (int64_t i = threadIdx.x; i < n; i += kLzThreads) {
        const double a = fabs(x[i]);
        if (a > best) best = a, at = i;
    }
    bm[threadIdx.x] = best;
    bi[threadIdx.x] = at;
    __syncthreads();
    for (int s = kLzThreads / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const double o = bm[threadIdx.x + s];
            const long long oi = bi[threadIdx.x + s];
            if (o > bm[threadIdx.x] || (o == bm[threadIdx.x] && oi < bi[threadIdx.x])) bm[threadIdx.x] = o, bi[threadIdx.x] = oi;
        }
        __syncthreads();
    }
    if (n == 0) return;
    const bool flip = x[bi[0]] < 0.0;
    __syncthreads();
    if (flip)
        for (int64_t i = threadIdx.x; i < n; i += kLzThreads) x[i] = -x[i];
}

// ---- the step kernels for complex scalars ------------------------------------------------------------------------------------------
// Partial sums of V^H t for the columns 0..ncols-1 and of w^H t (stored as column `ncols`), one pass over V: workgroup (chunk, tile)
// sums kLzColTile columns over the rows of its chunk into part[c * ldp + chunk].  The workgroups of tile 0 also sum the two inner-solve
// checks over their rows when chk_part is given: chk_part[4 chunk + 0..3] = |b1 - z1|^2, |b1|^2, |b2 - z2|^2, |b2|^2.  A full tile
// has its eight 16-byte loads of a row in flight before the first addition.
// (the body is shared by the solo kernel and the batched one: one copy of the chunking, the tiling and the order of every sum)
__device__ __forceinline__ void rz_dot_body(int64_t n, int ncols, int64_t rows_per_block, const cplx* __restrict__ V, int64_t ldv, const cplx* t,
                                            const cplx* w, cplx* __restrict__ part, int ldp, const cplx* __restrict__ b1, const cplx* __restrict__ z1,
                                            const cplx* __restrict__ b2, const cplx* __restrict__ z2, double* __restrict__ chk_part) {
    __shared__ cplx wsum[4][kLzColTile];
    __shared__ double csum[4][4];
    const int chunk = blockIdx.x;
    const int c0 = blockIdx.y * kLzColTile;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r0 = (int64_t)chunk * rows_per_block;
    const int64_t r1 = (r0 + rows_per_block < n) ? r0 + rows_per_block : n;
    // column c of the tile: a basis column, or w for the one behind the basis
    const cplx* col[kLzColTile];
#pragma unroll
    for (int c = 0; c < kLzColTile; ++c) col[c] = (c0 + c < ncols) ? V + (int64_t)(c0 + c) * ldv : w;
    const int nc = (ncols + 1 - c0 < kLzColTile) ? (ncols + 1 - c0) : kLzColTile;
    cplx acc[kLzColTile];
#pragma unroll
    for (int c = 0; c < kLzColTile; ++c) acc[c] = cplx{0.0, 0.0};
    if (nc == kLzColTile) {
        for (int64_t i = r0 + threadIdx.x; i < r1; i += kLzThreads) {
            const cplx tv = rz_ld(t + i);
            cplx v[kLzColTile];
#pragma unroll
            for (int c = 0; c < kLzColTile; ++c) v[c] = rz_ld(col[c] + i);
#pragma unroll
            for (int c = 0; c < kLzColTile; ++c) fma_conj_acc(acc[c], v[c], tv);
        }
    } else {
        for (int64_t i = r0 + threadIdx.x; i < r1; i += kLzThreads) {
            const cplx tv = rz_ld(t + i);
#pragma unroll
            for (int c = 0; c < kLzColTile; ++c)
                if (c < nc) fma_conj_acc(acc[c], rz_ld(col[c] + i), tv);
        }
    }
#pragma unroll
    for (int c = 0; c < kLzColTile; ++c) {
        const cplx s = lz_wave_sum(acc[c]);
        if (lane == 0) wsum[wave][c] = s;
    }
    const bool chk = chk_part != nullptr && blockIdx.y == 0;
    if (chk) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t r = r0 + threadIdx.x; r < r1; r += kLzThreads) {
            const cplx ba = rz_ld(b1 + r), bb = rz_ld(b2 + r);
            const cplx da = s_sub(ba, rz_ld(z1 + r)), db = s_sub(bb, rz_ld(z2 + r));
            s[0] = fma(da.im, da.im, fma(da.re, da.re, s[0]));
            s[1] = fma(ba.im, ba.im, fma(ba.re, ba.re, s[1]));
            s[2] = fma(db.im, db.im, fma(db.re, db.re, s[2]));
            s[3] = fma(bb.im, bb.im, fma(bb.re, bb.re, s[3]));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double v = lz_wave_sum(s[q]);
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

__global__ __launch_bounds__(kLzThreads) void rz_dot_kernel(int64_t n, int ncols, int64_t rows_per_block, const cplx* __restrict__ V, int64_t ldv,
                                                            const cplx* t, const cplx* w, cplx* __restrict__ part, int ldp,
                                                            const cplx* __restrict__ b1, const cplx* __restrict__ z1, const cplx* __restrict__ b2,
                                                            const cplx* __restrict__ z2, double* __restrict__ chk_part) {
    rz_dot_body(n, ncols, rows_per_block, V, ldv, t, w, part, ldp, b1, z1, b2, z2, chk_part);
}

// The batched forms of the three complex step kernels: up to kRzGroupMax problems of one n in one launch, the problem as the grid's
// last dimension, its pointers and its number of basis columns by value in the kernel arguments (the members of a lockstep group sit
// at different j after their restarts).  Each problem runs the solo kernel's body on the solo kernel's grid in the leading dimensions.
constexpr int kRzGroupMax = 16;
struct RzDotArgs {
    const cplx *V[kRzGroupMax], *t[kRzGroupMax], *w[kRzGroupMax];
    cplx* part[kRzGroupMax];
    const cplx *b1[kRzGroupMax], *z1[kRzGroupMax], *b2[kRzGroupMax], *z2[kRzGroupMax];
    double* chk_part[kRzGroupMax];
    int ncols[kRzGroupMax];
};
struct RzUpdateArgs {
    const cplx *V[kRzGroupMax], *part[kRzGroupMax];
    cplx *w[kRzGroupMax], *h_out[kRzGroupMax];
    int ncols[kRzGroupMax];
};
struct RzTailArgs {
    const cplx *w[kRzGroupMax], *t[kRzGroupMax], *part[kRzGroupMax];
    cplx *vnext[kRzGroupMax], *rhs_next[kRzGroupMax];
    const double* chk_part[kRzGroupMax];
    double* out[kRzGroupMax];
};
// (the kernel arguments of a launch are limited to 4096 bytes; the scalars beside a record take under 64)
static_assert(sizeof(RzDotArgs) + 64 <= 4096 && sizeof(RzUpdateArgs) + 64 <= 4096 && sizeof(RzTailArgs) + 64 <= 4096,
              "the arguments of a batched step kernel exceed the kernel-argument limit");
static_assert(kRzGroupMax == kKrylovGroupMax, "a lockstep group of the complex basis fills the per-problem arrays of lsa_ks_batch_info");

// grid (chunks, column tiles of the member with most columns, problems): a workgroup whose tile lies beyond its problem's ncols + 1
// columns returns before touching memory
__global__ __launch_bounds__(kLzThreads) void rz_dot_batch_kernel(int64_t n, int64_t rows_per_block, int64_t ldv, int ldp, RzDotArgs a) {
    const int z = blockIdx.z;
    const int ncols = a.ncols[z];
    if ((int)blockIdx.y * kLzColTile >= ncols + 1) return;
    rz_dot_body(n, ncols, rows_per_block, a.V[z], ldv, a.t[z], a.w[z], a.part[z], ldp, a.b1[z], a.z1[z], a.b2[z], a.z2[z], a.chk_part[z]);
}

// w -= V h for the columns 0..ncols-1.  The prologue finishes h from the partial sums (lz_finish_sum: every workgroup gets the same
// bits; wave q takes the columns q, q + 4, ...); workgroup 0 writes h to h_out for the host.  Then a thread per row, the rows of a
// workgroup strided over the grid: eight entries of the row are requested at a time -- the first eight ahead of the prologue, which
// does not depend on them -- and added column after column.  The dynamic LDS holds h alone (no static LDS in front of it: 16-byte
// aligned entries).
__device__ __forceinline__ void rz_update_body(int64_t n, int ncols, const cplx* __restrict__ V, int64_t ldv, const cplx* __restrict__ part, int nchunks,
                                               int ldp, cplx* w, cplx* __restrict__ h_out) {
    extern __shared__ __attribute__((aligned(16))) char rz_dyn[];
    cplx* hs = reinterpret_cast<cplx*>(rz_dyn);  // ncols coefficients
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * kLzThreads;
    int64_t i = (int64_t)blockIdx.x * kLzThreads + threadIdx.x;
    cplx v[kRzUnroll];
#pragma unroll
    for (int u = 0; u < kRzUnroll; ++u) v[u] = (i < n && u < ncols) ? rz_ld(V + i + (int64_t)u * ldv) : cplx{0.0, 0.0};
    for (int c = q; c < ncols; c += 4) {
        const cplx a = lz_finish_sum(part + (int64_t)c * ldp, nchunks, lane);
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

__global__ __launch_bounds__(kLzThreads) void rz_update_kernel(int64_t n, int ncols, const cplx* __restrict__ V, int64_t ldv,
                                                               const cplx* __restrict__ part, int nchunks, int ldp, cplx* w,
                                                               cplx* __restrict__ h_out) {
    rz_update_body(n, ncols, V, ldv, part, nchunks, ldp, w, h_out);
}

// grid (row workgroups, problems); the dynamic LDS holds the coefficients of the member with most columns
__global__ __launch_bounds__(kLzThreads) void rz_update_batch_kernel(int64_t n, int64_t ldv, int nchunks, int ldp, RzUpdateArgs a) {
    const int z = blockIdx.y;
    rz_update_body(n, a.ncols[z], a.V[z], ldv, a.part[z], nchunks, ldp, a.w[z], a.h_out[z]);
}

// From the partial sums of w^H t (part[0..nchunks), lz_finish_sum): beta^2 = its real part, then v_next = w / beta and
// rhs_next = t / beta.  Workgroup 0 leaves beta^2, the imaginary part (rounding) and the four sums of the two inner-solve checks
// (chk_part, nchk quadruples) in out[0..6).  A beta^2 that is not positive and finite scales by zero: the host reads it from the slot
// and stops.
__device__ __forceinline__ void rz_tail_body(int64_t n, const cplx* w, const cplx* t, const cplx* __restrict__ part, int nchunks, cplx* vnext,
                                             cplx* rhs_next, const double* __restrict__ chk_part, int nchk, double* __restrict__ out) {
    __shared__ double b2s;
    if (threadIdx.x < 64) {
        const cplx a = lz_finish_sum(part, nchunks, threadIdx.x);
        if (threadIdx.x == 0) b2s = a.re;
        if (blockIdx.x == 0) {
            double c[4] = {0.0, 0.0, 0.0, 0.0};
            if (chk_part)
                for (int k = threadIdx.x; k < nchk; k += 64) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) c[q] += chk_part[4 * k + q];
                }
#pragma unroll
            for (int q = 0; q < 4; ++q) c[q] = lz_wave_sum(c[q]);
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
    const int64_t stride = (int64_t)gridDim.x * kLzThreads;
    for (int64_t i = (int64_t)blockIdx.x * kLzThreads + threadIdx.x; i < n; i += stride) {
        const cplx wi = rz_ld(w + i), ti = rz_ld(t + i);
        rz_st(vnext + i, s_mul(inv, wi));
        rz_st(rhs_next + i, s_mul(inv, ti));
    }
}

__global__ __launch_bounds__(kLzThreads) void rz_tail_kernel(int64_t n, const cplx* w, const cplx* t, const cplx* __restrict__ part, int nchunks,
                                                             cplx* vnext, cplx* rhs_next, const double* __restrict__ chk_part, int nchk,
                                                             double* __restrict__ out) {
    rz_tail_body(n, w, t, part, nchunks, vnext, rhs_next, chk_part, nchk, out);
}

// grid (row workgroups, problems)
__global__ __launch_bounds__(kLzThreads) void rz_tail_batch_kernel(int64_t n, int nchunks, int nchk, RzTailArgs a) {
    const int z = blockIdx.y;
    rz_tail_body(n, a.w[z], a.t[z], a.part[z], nchunks, a.vnext[z], a.rhs_next[z], a.chk_part[z], nchk, a.out[z]);
}

// the fused kernels unless LSA_LANCZOS_FUSED=0 (read once per process, like LSA_KRYLOV_FUSED): then k_multi_dot + k_multi_axpy
bool lz_fused() {
    static const bool fused = env_flag("LSA_LANCZOS_FUSED", true);
    return fused;
}

}  // namespace

struct lsa_lanczos {
    lsa_ctx* ctx = nullptr;
    lsa_op* op = nullptr;
    lsa_op_parts P{};
    int64_t n = 0;
    int32_t ncv = 0;
    int dtype = LSA_F64;  // the scalar type of every vector below
    size_t es = 8;        // ... and its bytes
    const char* who = "lsa_lanczos";  // the owner's name, for the messages
    const lsa_mat* Q = nullptr;       // the inner product (lanczos_set_inner_product); null: the standard problem, t aliases w
    // the n x (ncv + 1) arrays: the basis, the restart's second basis (and the Ritz vectors) and, with a row permutation, the output in
    // the caller's numbering (on first use)
    char *V = nullptr, *V2 = nullptr;
    void* xtmp = nullptr;
    int32_t* row_perm = nullptr;
    void *w = nullptr, *t = nullptr, *z = nullptr, *r = nullptr;  // work vectors: OP v_j, Q w, and two for the operator (C w, a residual)
    void* rhs[2] = {nullptr, nullptr};  // Q v_j of the current step / of the next one (a step that is redone finds its own intact)
    int cur = 0;
    int32_t rhs_for = -1;        // rhs[cur] holds Q v_j for this j, -1: nothing
    void* part = nullptr;        // (ncv + 2) x kDotMaxChunks partial sums, a coefficient's chunks side by side
    double* chk_part = nullptr;  // kDotMaxChunks times the sums of the step's checks
    double* slot = nullptr;      // see lz_slot
    void* qdev = nullptr;        // (ncv + 1)^2: the restart's and the Ritz vectors' coefficients
    double* imag2 = nullptr;     // complex scalars: ncv + 1, what k_columns_canonical reports (not read)
    std::vector<double> hslot;
    // the operator behind a step and the checks its last enqueue named; builtin: the single solve of a real basis
    lanczos_operator builtin{};
    const lanczos_operator* hook = nullptr;
    lanczos_check chk[2] = {};
    bool refine_used = false;  // what the default operator's solve being judged was queued with
};

namespace {

// The slot, in doubles: h of pass 1 and h of pass 2 (ncv + 1 scalars each), then what the tail kernel writes at `out` -- beta^2 (complex:
// and Im w^H t, rounding), |b - z|^2 and |b|^2 per check from `chk` -- then the unfused form's w^H t (a scalar, at `wt`) and |solution|^2 of
// the checks' refined solves from `xnorm`.
struct LzSlot {
    size_t h, out, chk, wt, xnorm, doubles;
};
LzSlot lz_slot(const lsa_lanczos* l) {
    const size_t sc = l->es / sizeof(double), nchk = sc;  // doubles per scalar; one check on the real basis, two on the complex one
    LzSlot s;
    s.h = sc * (size_t)(l->ncv + 1);
    s.out = 2 * s.h;
    s.chk = s.out + sc;
    s.wt = s.chk + 2 * nchk;
    s.xnorm = s.wt + sc;
    s.doubles = s.xnorm + nchk;
    return s;
}

int lz_nchecks(const lsa_lanczos* l) { return l->dtype == LSA_C128 ? 2 : 1; }

void lz_free(lsa_lanczos* l) {
    for (void* p : {(void*)l->V, (void*)l->V2, l->xtmp, (void*)l->row_perm, l->w, l->t, l->z, l->r, l->rhs[0], l->rhs[1], l->part, (void*)l->chk_part,
                    (void*)l->slot, l->qdev, (void*)l->imag2})
        if (p) (void)hipFree(p);
    delete l;
}

void* lz_col(const lsa_lanczos* l, int32_t j) { return l->V + (size_t)j * (size_t)l->n * l->es; }

// t = Q w (or t aliases w for a standard problem)
int lz_mass(lsa_ctx* ctx, lsa_lanczos* l, const void* x, void* y) {
    if (!l->Q) return LSA_OK;
    ++l->P.st->spmv_calls;
    return k_spmv(ctx, l->Q, l->dtype, x, y);
}

int lz_grid(lsa_ctx* ctx, int64_t n, int per_cu) {
    return (int)std::max<int64_t>(std::min<int64_t>((n + kLzThreads - 1) / kLzThreads, (int64_t)ctx->num_cu * per_cu), 1);
}

// the three launches of the fused form by scalar type.  dot: ncols basis columns and w against t, the step's checks with chk
void lz_launch_dot(lsa_ctx* ctx, lsa_lanczos* l, int nchunks, int64_t rows_per_block, int ncols, const void* t, bool chk) {
    const dim3 grid(nchunks, (ncols + 1 + kLzColTile - 1) / kLzColTile);
    const lanczos_check none{}, &c0 = chk ? l->chk[0] : none, &c1 = chk ? l->chk[1] : none;
    double* chk_part = chk ? l->chk_part : nullptr;
    if (l->dtype == LSA_F64)
        hipLaunchKernelGGL(lz_dot_kernel, grid, dim3(kLzThreads), 0, ctx->stream, l->n, ncols, rows_per_block, (const double*)l->V, l->n, (const double*)t,
                           (const double*)l->w, (double*)l->part, nchunks, (const double*)c0.b, (const double*)c0.z, chk_part);
    else
        hipLaunchKernelGGL(rz_dot_kernel, grid, dim3(kLzThreads), 0, ctx->stream, l->n, ncols, rows_per_block, (const cplx*)l->V, l->n, (const cplx*)t,
                           (const cplx*)l->w, (cplx*)l->part, nchunks, (const cplx*)c0.b, (const cplx*)c0.z, (const cplx*)c1.b, (const cplx*)c1.z, chk_part);
}

// update: w -= V h from the partial sums, h to h_out.  Every workgroup finishes h for itself: a few hundred of them, their rows
// strided over the grid
void lz_launch_update(lsa_ctx* ctx, lsa_lanczos* l, int nchunks, int ncols, double* h_out) {
    const dim3 grid(lz_grid(ctx, l->n, 2));
    if (l->dtype == LSA_F64)
        hipLaunchKernelGGL(lz_update_kernel, grid, dim3(kLzThreads), (size_t)ncols * l->es, ctx->stream, l->n, ncols, (const double*)l->V, l->n,
                           (const double*)l->part, nchunks, nchunks, (double*)l->w, h_out);
    else
        hipLaunchKernelGGL(rz_update_kernel, grid, dim3(kLzThreads), (size_t)ncols * l->es, ctx->stream, l->n, ncols, (const cplx*)l->V, l->n,
                           (const cplx*)l->part, nchunks, nchunks, (cplx*)l->w, (cplx*)h_out);
}

// tail: beta^2 from nparts partial sums at part, v_next and rhs_next, the slot's tail (the checks' sums from nparts partial sums with chk)
void lz_launch_tail(lsa_ctx* ctx, lsa_lanczos* l, const void* t, const void* part, int nparts, void* vnext, void* rhs_next, bool chk, double* out) {
    const dim3 grid(lz_grid(ctx, l->n, 8));
    const double* chk_part = chk ? l->chk_part : nullptr;
    if (l->dtype == LSA_F64)
        hipLaunchKernelGGL(lz_tail_kernel, grid, dim3(kLzThreads), 0, ctx->stream, l->n, (const double*)l->w, (const double*)t, (const double*)part, nparts,
                           (double*)vnext, (double*)rhs_next, chk_part, nparts, out);
    else
        hipLaunchKernelGGL(rz_tail_kernel, grid, dim3(kLzThreads), 0, ctx->stream, l->n, (const cplx*)l->w, (const cplx*)t, (const cplx*)part, nparts,
                           (cplx*)vnext, (cplx*)rhs_next, chk_part, nparts, out);
}

// Q-orthogonalise l->w against the columns 0..ncols-1 (two passes), then v = w / beta into column `target` and Q v into the
// other right-hand side buffer; the slot's beta^2 and check sums are read back by the caller.  chk: the checks the operator named
// ride in the first reduction.
int lz_orth_tail(lsa_ctx* ctx, lsa_lanczos* l, int32_t ncols, int32_t target, bool chk) {
    const int64_t n = l->n;
    const void* t = l->Q ? l->t : l->w;
    void* vnext = lz_col(l, target);
    void* rhs_next = l->rhs[l->cur ^ 1];
    const LzSlot S = lz_slot(l);
    double* out = l->slot + S.out;
    const char* what = l->dtype == LSA_C128 ? "resolvent step" : "lanczos step";
    if (lz_fused()) {
        int64_t rows_per_block;
        const int nchunks = dot_chunks(n, &rows_per_block);
        for (int pass = 0; pass < 2 && ncols > 0; ++pass) {
            LSA_CHECK(lz_mass(ctx, l, l->w, l->t));
            lz_launch_dot(ctx, l, nchunks, rows_per_block, ncols, t, chk && pass == 0);
            lz_launch_update(ctx, l, nchunks, ncols, l->slot + (size_t)pass * S.h);
        }
        LSA_CHECK(lz_mass(ctx, l, l->w, l->t));
        lz_launch_dot(ctx, l, nchunks, rows_per_block, 0, t, chk && ncols == 0);
        lz_launch_tail(ctx, l, t, l->part, nchunks, vnext, rhs_next, chk, out);
        return lsa_check_launch(ctx, what);
    }
    // the unfused form: the library's multi-dot and multi-axpy, the same tail with single partial sums
    for (int k = 0; chk && k < lz_nchecks(l); ++k) LSA_CHECK(k_residual_norms(ctx, l->dtype, n, l->chk[k].b, l->chk[k].z, l->r, l->chk_part + 2 * k));
    for (int pass = 0; pass < 2 && ncols > 0; ++pass) {
        LSA_CHECK(lz_mass(ctx, l, l->w, l->t));
        double* h = l->slot + (size_t)pass * S.h;
        LSA_CHECK(k_multi_dot(ctx, l->dtype, n, ncols, l->V, n, t, h));
        LSA_CHECK(k_multi_axpy(ctx, l->dtype, n, ncols, l->V, n, h, l->w, nullptr));
    }
    LSA_CHECK(lz_mass(ctx, l, l->w, l->t));
    LSA_CHECK(k_multi_dot(ctx, l->dtype, n, 1, l->w, n, t, l->slot + S.wt));
    lz_launch_tail(ctx, l, t, l->slot + S.wt, 1, vnext, rhs_next, chk, out);
    return lsa_check_launch(ctx, l->dtype == LSA_C128 ? "resolvent step (unfused)" : "lanczos step (unfused)");
}

// the slot to the host: one synchronisation
int lz_read_slot(lsa_ctx* ctx, lsa_lanczos* l) {
    const size_t bytes = l->hslot.size() * sizeof(double);
    LSA_CHECK(lsa_ensure_scratch(ctx, 0, bytes));
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(ctx->pinned, l->slot, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (l->hook && l->hook->read_back) LSA_CHECK(l->hook->read_back(ctx, l->hook->self));  // (its log travels behind the same synchronisation)
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(l->hslot.data(), ctx->pinned, bytes);
    return LSA_OK;
}

// V2[:, 0:k] = V[:, 0:m] Y for the real host matrix Y (complex scalars: widened for k_basis_gemm)
int lz_basis_times_real(lsa_ctx* ctx, lsa_lanczos* l, int32_t m, int32_t k, const double* Y, int32_t ldy) {
    if (l->dtype == LSA_F64) return basis_times_host_matrix(ctx, LSA_F64, l->n, m, k, l->V, Y, ldy, l->qdev, l->V2, 0);
    std::vector<cplx> Yc((size_t)m * k);
    for (int32_t c = 0; c < k; ++c)
        for (int32_t i = 0; i < m; ++i) Yc[(size_t)c * m + i] = cplx{Y[(size_t)c * ldy + i], 0.0};
    return basis_times_host_matrix(ctx, LSA_C128, l->n, m, k, l->V, Yc.data(), m, l->qdev, l->V2, 0);
}

// ---- the default operator of a real basis: the single solve, on the op's shared refinement flag -------------------------------------
int lz_solve_enqueue(lsa_ctx* ctx, void* self, int32_t, const void* rhs, void* w, void* z, void* r, lanczos_check* chk) {
    lsa_lanczos* l = (lsa_lanczos*)self;
    const bool refine = l->refine_used = *l->P.refine;
    // (w += C^-1 (rhs - C w) with refine: takes what large factors leave behind to rounding level)
    LSA_CHECK(direct_solve_enqueue(ctx, l->op, LSA_F64, rhs, w, z, r, refine, l->chk_part));
    if (refine) LSA_CHECK(k_nrm2(ctx, LSA_F64, l->n, w, chk[0].xnorm2_dev));  // for the backward-error judgement
    chk[0].b = rhs;
    chk[0].z = z;
    chk[0].refined = refine;
    return LSA_OK;
}

int lz_solve_judge(lsa_ctx* ctx, void* self, int32_t j, const lanczos_sums* s) {
    lsa_lanczos* l = (lsa_lanczos*)self;
    const bool refine = l->refine_used;
    bool backward = false;
    const int verdict = direct_solve_verdict(l->P, refine, s[0].res, s[0].bnorm, s[0].xnorm, &backward);
    if (verdict == 0) {
        if (backward) ++l->P.st->backward_accepted;
        stats_book_direct_solve(l->P.st, 1, refine, s[0].res, s[0].bnorm);
    } else if (verdict > 0) {  // from here on every step carries the refinement step; this one is done again
        *l->P.refine = true;
    } else {
        lsa_set_error(ctx, LSA_ERR_DIVERGED, "lsa_lanczos_extend: the inner solve of step %d left a relative residual of %.3e after its refinement "
                                             "step (ksp_rtol %.1e) and a backward error above 1e-12 ||C||_F", j, s[0].bnorm > 0.0 ? s[0].res / s[0].bnorm : s[0].res,
                      l->P.ksp_rtol);
    }
    return verdict;
}

// ---- what follows a step's read-back, over the basis' own host slot: one copy for the solo loop and the lockstep rounds --------------
// the operator's judgement of the step's checked solves.  0: accepted (and booked), 1: do the step again, -1: failed (the error is set)
int lz_judge_step(lsa_ctx* ctx, lsa_lanczos* l, int32_t j) {
    const LzSlot S = lz_slot(l);
    const double* h = l->hslot.data();
    lanczos_sums sums[2];
    for (int k = 0; k < lz_nchecks(l); ++k)
        sums[k] = lanczos_sums{std::sqrt(h[S.chk + 2 * k]), std::sqrt(h[S.chk + 2 * k + 1]), l->chk[k].refined ? std::sqrt(h[S.xnorm + k]) : 0.0};
    return l->hook->judge(ctx, l->hook->self, j, sums);
}

// alpha_j and beta_j of an accepted step into T, the definiteness check and the breakdown rule; the right-hand side buffers change roles
int lz_accept_step(lsa_ctx* ctx, lsa_lanczos* l, int32_t j, double* T, int32_t ldt, bool* broke_out) {
    const bool cx = l->dtype == LSA_C128;
    const size_t sc = cx ? 2 : 1;  // doubles per scalar
    const LzSlot S = lz_slot(l);
    const double* h = l->hslot.data();
    *broke_out = false;
    // Re h_i of both passes.  alpha_j = Re h_j: OP is self-adjoint in the inner product, the imaginary part is rounding and is dropped
    auto re = [&](int32_t i) { return h[sc * (size_t)i] + h[S.h + sc * (size_t)i]; };
    const double alpha = re(j);
    const double b2 = h[S.out];
    if (!std::isfinite(alpha) || !std::isfinite(b2))
        return lsa_set_error(ctx, LSA_ERR_NONFINITE, "%s: non-finite recurrence coefficient at step %d", cx ? "resolvent" : "Lanczos", j);
    // what is left of w after both passes, against the size of what was taken out of it (the rule of the general loop's columns)
    double colmax = std::fabs(alpha);
    for (int32_t i = 0; i < j; ++i)
        colmax = std::max(colmax, cx ? std::hypot(re(i), h[2 * (size_t)i + 1] + h[S.h + 2 * (size_t)i + 1]) : std::fabs(re(i)));
    const double thr = 1e-14 * std::max(colmax, 1e-300);
    if (b2 < -thr * thr)
        return lsa_set_error(ctx, LSA_ERR_ARG, "%s_extend: w^%s M w = %.3e at step %d: M is not positive %s on the Krylov space", l->who, cx ? "H" : "T", b2, j,
                             cx ? "semidefinite" : "definite");
    const double beta = b2 > 0.0 ? std::sqrt(b2) : 0.0;
    const bool broke = beta <= thr;
    T[(size_t)j * ldt + j] = alpha;
    T[(size_t)j * ldt + j + 1] = broke ? 0.0 : beta;
    if (j + 1 < l->ncv && j + 1 < ldt) T[(size_t)(j + 1) * ldt + j] = broke ? 0.0 : beta;
    l->cur ^= 1;
    l->rhs_for = broke ? -1 : j + 1;
    *broke_out = broke;
    return LSA_OK;
}

}  // namespace

int lanczos_create_basis(lsa_ctx* ctx, lsa_op* op, int32_t ncv, int dtype, const char* who, lsa_lanczos** out) {
    lsa_op_parts P{};
    LSA_CHECK(lsa_op_get_parts(op, &P));
    return lanczos_create_basis_on(ctx, op, P, ncv, dtype, who, out);
}

int lanczos_create_basis_on(lsa_ctx* ctx, lsa_op* op, const lsa_op_parts& P, int32_t ncv, int dtype, const char* who, lsa_lanczos** out) {
    lsa_lanczos* l = new lsa_lanczos();
    l->ctx = ctx;
    l->op = op;
    l->P = P;
    l->n = P.n;
    l->ncv = ncv;
    l->dtype = dtype;
    l->es = dtype == LSA_C128 ? sizeof(cplx) : sizeof(double);
    l->who = who;
    l->Q = P.Kmul;
    l->builtin = lanczos_operator{l, 1, lz_solve_enqueue, nullptr, lz_solve_judge};
    l->hook = dtype == LSA_F64 && op ? &l->builtin : nullptr;  // (the default's single solve runs on an operator's factors)
    const LzSlot S = lz_slot(l);
    l->hslot.assign(S.doubles, 0.0);
    const size_t vb = (size_t)std::max<int64_t>(l->n, 1) * l->es, nchk = (size_t)lz_nchecks(l);
    bool ok = hipMalloc((void**)&l->V, vb * (size_t)(ncv + 1)) == hipSuccess && hipMalloc((void**)&l->V2, vb * (size_t)(ncv + 1)) == hipSuccess;
    for (void** p : {&l->w, &l->t, &l->z, &l->r, &l->rhs[0], &l->rhs[1]}) ok = ok && hipMalloc(p, vb) == hipSuccess;
    ok = ok && hipMalloc(&l->part, (size_t)kDotMaxChunks * (size_t)(ncv + 2) * l->es) == hipSuccess &&
         hipMalloc((void**)&l->chk_part, (size_t)kDotMaxChunks * 2 * nchk * sizeof(double)) == hipSuccess &&
         hipMalloc((void**)&l->slot, S.doubles * sizeof(double)) == hipSuccess &&
         hipMalloc(&l->qdev, (size_t)(ncv + 1) * (size_t)(ncv + 1) * l->es) == hipSuccess &&
         (dtype == LSA_F64 || hipMalloc((void**)&l->imag2, (size_t)(ncv + 1) * sizeof(double)) == hipSuccess);
    if (!ok) {
        (void)hipGetLastError();
        lz_free(l);
        return lsa_set_error(ctx, LSA_ERR_OOM, "%s_create: out of device memory (n=%lld, ncv=%d)", who, (long long)P.n, ncv);
    }
    (void)hipMemsetAsync(l->slot, 0, S.doubles * sizeof(double), ctx->stream);
    *out = l;
    return LSA_OK;
}

int lanczos_shape(const lsa_lanczos* l, int64_t* n, int32_t* ncv) {
    if (!l) return LSA_ERR_ARG;
    if (n) *n = l->n;
    if (ncv) *ncv = l->ncv;
    return LSA_OK;
}

int lanczos_set_operator(lsa_ctx* ctx, lsa_lanczos* l, const lanczos_operator* hook) {
    if (!hook && l->dtype == LSA_F64 && l->op) hook = &l->builtin;
    if (hook && hook->nchecks != lz_nchecks(l))
        return lsa_set_error(ctx, LSA_ERR_ARG, "%s: the operator names %d checked solves a step, the step kernels of this basis take %d", l->who, hook->nchecks,
                             lz_nchecks(l));
    l->hook = hook;
    return LSA_OK;
}

void lanczos_set_inner_product(lsa_lanczos* l, const lsa_mat* Q) {
    l->Q = Q ? Q : l->P.Kmul;
    l->rhs_for = -1;
}

void* lanczos_ritz_device(const lsa_lanczos* l) { return l->V2; }

const int32_t* lanczos_row_permutation(const lsa_lanczos* l) { return l->row_perm; }

int lanczos_ritz_to_host(lsa_ctx* ctx, lsa_lanczos* l, int32_t nvec, void* X) {
    return basis_columns_to_host(ctx, l->dtype, l->n, nvec, l->row_perm, l->V2, &l->xtmp, l->ncv + 1, X);
}

int lanczos_inject(lsa_ctx* ctx, lsa_lanczos* l, int32_t j, const void* host_v) {
    if (!ctx || !l || !host_v) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: null argument", l ? l->who : "lsa_lanczos");
    if (j < 0 || j > l->ncv) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: column %d out of range", l->who, j);
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(l->w, host_v, (size_t)l->n * l->es, hipMemcpyHostToDevice, ctx->stream));
    LSA_CHECK(lz_orth_tail(ctx, l, j, j, false));
    LSA_CHECK(lz_read_slot(ctx, l));
    const double b2 = l->hslot[lz_slot(l).out];
    if (!(b2 > 0.0) || !std::isfinite(b2))
        return lsa_set_error(ctx, LSA_ERR_ARG, "%s: v^%s M v = %.3e for the injected vector: M is not positive definite on the Krylov space (or the "
                                               "vector is zero or not finite)", l->who, l->dtype == LSA_C128 ? "H" : "T", b2);
    l->cur ^= 1;
    l->rhs_for = j;
    return LSA_OK;
}

int lanczos_restart(lsa_ctx* ctx, lsa_lanczos* l, int32_t m, int32_t knew, const double* Y, int32_t ldy) {
    if (!ctx || !l || !Y) return lsa_set_error(ctx, LSA_ERR_ARG, "%s restart: null argument", l ? l->who : "lsa_lanczos");
    if (m < 1 || m > l->ncv || knew < 1 || knew > m || ldy < m) return lsa_set_error(ctx, LSA_ERR_ARG, "%s restart: bad sizes m=%d knew=%d", l->who, m, knew);
    LSA_CHECK(lz_basis_times_real(ctx, l, m, knew, Y, ldy));
    LSA_CHECK(k_copy(ctx, l->dtype, l->n, lz_col(l, m), l->V2 + (size_t)knew * (size_t)l->n * l->es));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    std::swap(l->V, l->V2);
    if (l->rhs_for == m) l->rhs_for = knew;  // (the same vector under its new index)
    else l->rhs_for = -1;
    return LSA_OK;
}

int lanczos_ritz_vectors(lsa_ctx* ctx, lsa_lanczos* l, int32_t m, int32_t nvec, const double* Y, int32_t ldy, void* X) {
    if (!ctx || !l || !Y || !X) return lsa_set_error(ctx, LSA_ERR_ARG, "%s vectors: null argument", l ? l->who : "lsa_lanczos");
    if (m < 1 || m > l->ncv || nvec < 0 || nvec > l->ncv || ldy < m) return lsa_set_error(ctx, LSA_ERR_ARG, "%s vectors: bad sizes", l->who);
    if (nvec == 0) return LSA_OK;
    LSA_CHECK(lz_basis_times_real(ctx, l, m, nvec, Y, ldy));
    if (l->dtype == LSA_F64) {
        hipLaunchKernelGGL(lz_sign_kernel, dim3(nvec), dim3(kLzThreads), 0, ctx->stream, l->n, (double*)l->V2, l->n);
        LSA_CHECK(lsa_check_launch(ctx, "lanczos vectors"));
    } else {
        LSA_CHECK(k_columns_canonical(ctx, l->n, nvec, l->V2, l->n, 0, l->imag2));
    }
    return lanczos_ritz_to_host(ctx, l, nvec, X);
}

extern "C" {

int lsa_lanczos_create(lsa_ctx* ctx, lsa_op* op, int32_t ncv, lsa_lanczos** out) {
    if (!ctx || !op || !out || ncv < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_create: bad argument");
    lsa_op_parts P{};
    LSA_CHECK(lsa_op_get_parts(op, &P));
    if (!P.plain || ctx->nranks != 1)
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_create: needs a shift-invert operator (mode 0), forward and unprojected, on one rank");
    if (!P.nd || !P.Kfac || P.Kfac->dtype != LSA_F64 || (P.Kmul && P.Kmul->dtype != LSA_F64))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_create: needs real matrices, a real shift and the exact LU (pc_type 2) of K - sigma M");
    if ((int64_t)ncv > P.n) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_create: ncv = %d exceeds the problem size %lld", ncv, (long long)P.n);
    return lanczos_create_basis(ctx, op, ncv, LSA_F64, "lsa_lanczos", out);
}

void lsa_lanczos_destroy(lsa_lanczos* l) {
    if (!l) return;
    if (l->ctx && l->ctx->stream) (void)hipStreamSynchronize(l->ctx->stream);
    lz_free(l);
}

int lsa_lanczos_set_row_permutation(lsa_ctx* ctx, lsa_lanczos* l, const int32_t* perm) {
    if (!ctx || !l) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_set_row_permutation: null argument");
    const std::string who = std::string(l->who) + "_set_row_permutation";
    return basis_upload_row_permutation(ctx, who.c_str(), l->n, perm, &l->row_perm);
}

int lsa_lanczos_set_start(lsa_ctx* ctx, lsa_lanczos* l, const double* host_v) { return lanczos_inject(ctx, l, 0, host_v); }

int lsa_lanczos_extend(lsa_ctx* ctx, lsa_lanczos* l, int32_t j0, int32_t j1, double* T, int32_t ldt, int32_t* breakdown) {
    if (!ctx || !l || !T) return lsa_set_error(ctx, LSA_ERR_ARG, "%s_extend: null argument", l ? l->who : "lsa_lanczos");
    if (j0 < 0 || j1 < j0 || j1 > l->ncv || ldt < j1 + 1) return lsa_set_error(ctx, LSA_ERR_ARG, "%s_extend: bad step range [%d, %d) for ncv %d", l->who, j0, j1, l->ncv);
    if (!l->hook) return lsa_set_error(ctx, LSA_ERR_ARG, "%s_extend: the basis has no operator behind its step", l->who);
    if (breakdown) *breakdown = -1;
    const double t0 = now_s();
    const int nchk = lz_nchecks(l);
    const LzSlot S = lz_slot(l);
    int rc = LSA_OK;
    for (int32_t j = j0; j < j1 && rc == LSA_OK; ++j) {
        if (l->rhs_for != j) {  // (after lsa_lanczos_basis users, a restart that moved another column here, or the standard problem's first step)
            if (l->Q) rc = lz_mass(ctx, l, lz_col(l, j), l->rhs[l->cur]);
            else rc = k_copy(ctx, l->dtype, l->n, lz_col(l, j), l->rhs[l->cur]);
            if (rc != LSA_OK) break;
            l->rhs_for = j;
        }
        while (true) {
            // the operator queues w = OP v_j from rhs = Q v_j and names its checks; their sums ride in the step's first reduction and come
            // back with the slot, the step's one read-back; the operator judges
            for (int k = 0; k < nchk; ++k) l->chk[k] = lanczos_check{nullptr, nullptr, false, l->slot + S.xnorm + k};
            rc = l->hook->enqueue(ctx, l->hook->self, j, l->rhs[l->cur], l->w, l->z, l->r, l->chk);
            if (rc == LSA_OK) rc = lz_orth_tail(ctx, l, j + 1, j + 1, true);
            if (rc == LSA_OK) rc = lz_read_slot(ctx, l);
            if (rc != LSA_OK) break;
            const int verdict = lz_judge_step(ctx, l, j);
            if (verdict == 0) break;
            if (verdict < 0) {  // (the operator has set the error)
                rc = LSA_ERR_DIVERGED;
                break;
            }
        }
        if (rc != LSA_OK) break;
        bool broke = false;
        rc = lz_accept_step(ctx, l, j, T, ldt, &broke);
        if (rc != LSA_OK) break;
        if (broke) {
            if (breakdown) *breakdown = j;
            break;
        }
    }
    l->P.st->seconds_solve += now_s() - t0;
    return rc;
}

}  // extern "C"

// ---- lockstep expansion of a group of complex bases (lsa_resolvent_extend_batch, lsa_resolvent_solve_batch) -------------------------
// Bases of one n and ncv whose operator the group operator can queue for several members at once advance together: a round is one
// step of every member that still has one -- the group operator's batched launches for w_z = OP v_j(z), then per pass ONE product with
// the members' Q, ONE rz_dot_batch_kernel and ONE rz_update_batch_kernel, the last product and reduction, ONE rz_tail_batch_kernel -- and
// ONE copy of all members' slots (they lie side by side in the group's buffer) behind ONE synchronisation.  The members sit at
// different j; one that has reached j1 waits.  What follows the read-back is lz_judge_step and lz_accept_step per member over its own
// slot, the code of lsa_lanczos_extend.  A member that is not eligible, or whose solve misses ksp_rtol in a round (its operator has
// switched the refinement step on; its right-hand side of the step is intact), runs the rest of its steps through lsa_lanczos_extend
// from there, exactly as its solo expansion does.
int lanczos_group_alloc(lsa_ctx* ctx, int32_t J, lsa_lanczos* const* ls, LanczosGroupBuf* gb) {
    memset(gb, 0, sizeof *gb);
    gb->J = J;
    gb->slot_doubles = lz_slot(ls[0]).doubles;
    const size_t bytes = (size_t)J * gb->slot_doubles * sizeof(double);
    LSA_HIP_ALLOC(ctx, hipMalloc((void**)&gb->slots, bytes));
    // (the cells no kernel writes -- the unfused form's scalar, the refined solves' norms -- travel with the copy and are never looked at)
    LSA_HIP_CHECK(ctx, hipMemsetAsync(gb->slots, 0, bytes, ctx->stream));
    return LSA_OK;
}

void lanczos_group_free(LanczosGroupBuf* gb) {
    if (gb->slots) (void)hipFree(gb->slots);
    memset(gb, 0, sizeof *gb);
}

int lanczos_extend_batch(lsa_ctx* ctx, LanczosGroupBuf* gb, lsa_lanczos* const* ls, const lanczos_group_operator* gop, const uint8_t* active,
                         const int32_t* j0, int32_t j1, double* const* T, int32_t ldt, int32_t* breakdown, int32_t* status, std::string* errs,
                         lsa_ks_batch_info* info) {
    const int32_t J = gb->J;
    auto fail = [&](int32_t z, int rc) {  // member z stops with its own status and its own text, which names it
        status[z] = rc;
        lsa_name_problem(ctx, z);
        errs[z] = ctx->err;
    };
    int32_t jc[kRzGroupMax];  // the members' cursors
    bool lock[kRzGroupMax];   // still asked for the lockstep set
    int32_t lead = -1;
    for (int32_t z = 0; z < J; ++z) {
        jc[z] = j0[z];
        lock[z] = false;
        if (!active[z]) continue;
        breakdown[z] = -1;
        status[z] = LSA_OK;
        lsa_lanczos* l = ls[z];
        if (j0[z] < 0 || j1 < j0[z] || j1 > l->ncv || ldt < j1 + 1) {
            (void)lsa_set_error(ctx, LSA_ERR_ARG, "%s_extend: bad step range [%d, %d) for ncv %d", l->who, j0[z], j1, l->ncv);
            fail(z, LSA_ERR_ARG);
            continue;
        }
        bool in = l->dtype == LSA_C128 && lz_fused() && l->Q && l->hook && !l->hook->read_back && l->hslot.size() == gb->slot_doubles;
        if (in && lead >= 0) in = l->n == ls[lead]->n && l->ncv == ls[lead]->ncv;
        if (in) in = gop->eligible(gop->self, z, lead);
        if (in && lead < 0) lead = z;
        lock[z] = in;
    }
    const size_t sd = gb->slot_doubles;
    int64_t rows_per_block = 0;
    const int64_t n = lead >= 0 ? ls[lead]->n : 0;
    const int nchunks = lead >= 0 ? dot_chunks(n, &rows_per_block) : 0;
    int rc = lead >= 0 ? lsa_ensure_scratch(ctx, 0, (size_t)J * sd * sizeof(double)) : (int)LSA_OK;
    while (rc == LSA_OK) {
        // ---- the members of this round
        int32_t R = 0, idx[kRzGroupMax];
        for (int32_t z = 0; z < J; ++z)
            if (active[z] && lock[z] && status[z] == LSA_OK && breakdown[z] < 0 && jc[z] < j1) idx[R++] = z;
        if (R == 0) break;
        const double t0 = now_s();
        int32_t launches = 0;
        const lsa_mat* Qs[kRzGroupMax];
        const void *rhs[kRzGroupMax], *wc[kRzGroupMax];
        void *w[kRzGroupMax], *zz[kRzGroupMax], *t[kRzGroupMax];
        lanczos_check* chk[kRzGroupMax];
        int maxcols = 0;
        for (int32_t r = 0; r < R && rc == LSA_OK; ++r) {
            lsa_lanczos* l = ls[idx[r]];
            const int32_t j = jc[idx[r]];
            const LzSlot S = lz_slot(l);
            if (l->rhs_for != j) {  // (as in the solo loop: a restart moved another column here)
                rc = lz_mass(ctx, l, lz_col(l, j), l->rhs[l->cur]);
                l->rhs_for = j;
                if (rc == LSA_OK) ++launches;
            }
            for (int k = 0; k < 2; ++k) l->chk[k] = lanczos_check{nullptr, nullptr, false, l->slot + S.xnorm + k};
            Qs[r] = l->Q;
            rhs[r] = l->rhs[l->cur];
            w[r] = l->w, wc[r] = l->w;
            zz[r] = l->z;
            t[r] = l->t;
            chk[r] = l->chk;
            maxcols = std::max(maxcols, (int)j + 1);
        }
        if (rc == LSA_OK) rc = gop->enqueue(ctx, gop->self, R, idx, rhs, w, zz, chk, &launches);
        // ---- two passes of Gram-Schmidt in the members' inner products, the last product and reduction, the tail
        RzDotArgs da;
        RzUpdateArgs ua;
        RzTailArgs ta;
        memset(&da, 0, sizeof da);
        memset(&ua, 0, sizeof ua);
        memset(&ta, 0, sizeof ta);
        for (int32_t r = 0; r < R; ++r) {
            lsa_lanczos* l = ls[idx[r]];
            const int32_t j = jc[idx[r]];
            const LzSlot S = lz_slot(l);
            double* slot = gb->slots + (size_t)idx[r] * sd;
            da.V[r] = ua.V[r] = (const cplx*)l->V;
            da.t[r] = ta.t[r] = (const cplx*)l->t;
            da.w[r] = ta.w[r] = (const cplx*)l->w;
            ua.w[r] = (cplx*)l->w;
            da.part[r] = (cplx*)l->part;
            ua.part[r] = ta.part[r] = (const cplx*)l->part;
            da.b1[r] = (const cplx*)l->chk[0].b, da.z1[r] = (const cplx*)l->chk[0].z;
            da.b2[r] = (const cplx*)l->chk[1].b, da.z2[r] = (const cplx*)l->chk[1].z;
            da.chk_part[r] = l->chk_part;
            ta.chk_part[r] = l->chk_part;
            da.ncols[r] = ua.ncols[r] = j + 1;
            ta.vnext[r] = (cplx*)lz_col(l, j + 1);
            ta.rhs_next[r] = (cplx*)l->rhs[l->cur ^ 1];
            ta.out[r] = slot + S.out;
        }
        const dim3 threads(kLzThreads);
        for (int pass = 0; pass < 2 && rc == LSA_OK; ++pass) {
            rc = k_spmv_batch(ctx, R, Qs, LSA_C128, wc, t);
            if (rc != LSA_OK) break;
            for (int32_t r = 0; r < R; ++r) {
                ++ls[idx[r]]->P.st->spmv_calls;
                ua.h_out[r] = (cplx*)(gb->slots + (size_t)idx[r] * sd + (size_t)pass * lz_slot(ls[idx[r]]).h);
                if (pass == 1) da.chk_part[r] = nullptr;  // (the checks ride in the first reduction)
            }
            hipLaunchKernelGGL(rz_dot_batch_kernel, dim3(nchunks, (maxcols + 1 + kLzColTile - 1) / kLzColTile, R), threads, 0, ctx->stream, n, rows_per_block, n,
                               nchunks, da);
            hipLaunchKernelGGL(rz_update_batch_kernel, dim3(lz_grid(ctx, n, 2), R), threads, (size_t)maxcols * sizeof(cplx), ctx->stream, n, n, nchunks, nchunks, ua);
            launches += 3;  // (counted as they are queued: a round that fails on the way has launched what it has launched)
        }
        if (rc == LSA_OK) rc = k_spmv_batch(ctx, R, Qs, LSA_C128, wc, t);
        bool queued = false;  // the whole round, tail included
        if (rc == LSA_OK) {
            for (int32_t r = 0; r < R; ++r) da.ncols[r] = 0, da.chk_part[r] = nullptr, ++ls[idx[r]]->P.st->spmv_calls;
            hipLaunchKernelGGL(rz_dot_batch_kernel, dim3(nchunks, 1, R), threads, 0, ctx->stream, n, rows_per_block, n, nchunks, da);
            hipLaunchKernelGGL(rz_tail_batch_kernel, dim3(lz_grid(ctx, n, 8), R), threads, 0, ctx->stream, n, nchunks, nchunks, ta);
            launches += 3;
            rc = lsa_check_launch(ctx, "resolvent step (lockstep)");
            queued = rc == LSA_OK;
        }
        // ---- ONE copy of the group's slots, ONE synchronisation
        if (rc == LSA_OK && hipMemcpyAsync(ctx->pinned, gb->slots, (size_t)J * sd * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            rc = lsa_set_error(ctx, LSA_ERR_HIP, "%s: read-back of a lockstep round failed", ls[lead]->who);
        if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == LSA_OK)
            rc = lsa_set_error(ctx, LSA_ERR_HIP, "%s: a lockstep round failed on the device", ls[lead]->who);
        if (info) {
            if (queued) ++info->rounds, ++info->periods;
            info->launches += launches;
        }
        if (rc != LSA_OK) {  // the device work of the whole round is lost: an error of every member of it
            const std::string text = ctx->err;
            for (int32_t r = 0; r < R; ++r) {
                ctx->err = text;
                fail(idx[r], rc);
            }
            rc = LSA_OK;
            break;
        }
        const double share = (now_s() - t0) / R;
        for (int32_t r = 0; r < R; ++r) {
            const int32_t z = idx[r];
            lsa_lanczos* l = ls[z];
            memcpy(l->hslot.data(), (const double*)ctx->pinned + (size_t)z * sd, sd * sizeof(double));
            l->P.st->seconds_solve += share;
            const int verdict = lz_judge_step(ctx, l, jc[z]);
            if (verdict > 0) {  // (the operator has switched a refinement step on: this step and the later ones run alone)
                lock[z] = false;
                continue;
            }
            if (verdict < 0) {
                fail(z, LSA_ERR_DIVERGED);
                continue;
            }
            bool broke = false;
            const int arc = lz_accept_step(ctx, l, jc[z], T[z], ldt, &broke);
            if (arc != LSA_OK) {
                fail(z, arc);
                continue;
            }
            if (info) ++info->lockstep_steps[z];
            if (broke) breakdown[z] = jc[z];
            ++jc[z];
        }
    }
    if (rc != LSA_OK) return rc;  // (the pinned buffer could not be had: nothing was queued)
    // ---- whatever is left of each expansion, through the solo code
    for (int32_t z = 0; z < J; ++z) {
        if (!active[z] || status[z] != LSA_OK || breakdown[z] >= 0 || jc[z] >= j1) continue;
        int32_t bd = -1;
        const int xrc = lsa_lanczos_extend(ctx, ls[z], jc[z], j1, T[z], ldt, &bd);
        breakdown[z] = bd;
        if (xrc != LSA_OK) fail(z, xrc);
        else if (info) info->solo_steps[z] += (bd >= 0 ? bd + 1 : j1) - jc[z];
    }
    return LSA_OK;
}

extern "C" {

int lsa_lanczos_basis(lsa_ctx* ctx, const lsa_lanczos* l, int32_t ncols, double* host_V) {
    if (!ctx || !l || !host_V) return lsa_set_error(ctx, LSA_ERR_ARG, "%s_basis: null argument", l ? l->who : "lsa_lanczos");
    if (ncols < 0 || ncols > l->ncv + 1) return lsa_set_error(ctx, LSA_ERR_ARG, "%s_basis: %d columns of %d", l->who, ncols, l->ncv + 1);
    LSA_HIP_CHECK(ctx, hipMemcpyAsync(host_V, l->V, (size_t)l->n * (size_t)ncols * l->es, hipMemcpyDeviceToHost, ctx->stream));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return LSA_OK;
}

}  // extern "C"
