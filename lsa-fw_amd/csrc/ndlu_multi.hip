// Nested-dissection multifrontal LU, solves with a block of right-hand sides (lsa_ndlu_solve_multi and its kin): the
// sweeps of ndlu_sweeps.hip with R columns carried through every launch.  A workgroup owns the tile of rows of the packed L_t /
// U_t / T it owns there, stages the R vectors' chunks side by side in LDS, loads every factor scalar ONCE and accumulates R
// pairs of row sums from it.  Per column nothing else changes: the lane partition (LPR per level), each lane's ascending
// sequence of multiply-adds, the sub-wave sum and the order of the children's contributions are those of the solo kernels, so
// column q holds exactly the bits lsa_ndlu_solve gives for it.  (A lane's sequence sl, sl + LPR, ... runs on across chunks, so
// the chunk -- kMCH entries per column, a multiple of 256 -- is free: four complex or eight real columns of kMCH = 256 are 16 KB of LDS.)
// Columns beyond the first have sweep buffers of their own (lsa_ndlu::multi), made by the first such solve.
// The same kernels carry the R columns through J <= 16 factor sets of one analysis in one launch (the set is the grid's last
// dimension, NdMultiPtrs<R, NB>); the one-set solve is their instance of set capacity one.  The transposed systems C^-T / C^-H have
// the same form (nd_sweepT_multi_kernel): nd_sweepT_kernel with R columns carried through every launch, on the update vectors of the
// same per-column buffers, templated on the set capacity like the forward kernels.
// Every form -- forward or transposed, one set or a batch, one column or many -- is one request (NdSolve, ndlu_internal.h) to
// ndlu_solve_run at the end of this file: one dispatch on the scalar types and the direction (nd_dispatch_solve), one pass driver
// (nd_solve_passes).
#include "ndlu_sweep_parts.h"

namespace {

// what a multi-column launch gets per factor set: its factors, the first column of its right-hand sides and solutions, and the
// sweep buffers of the R columns of the pass (the column index is a compile-time constant wherever it is used)
template <int R>
struct NdMultiSet {
    const void *lfac, *ufac, *top;
    const void* rhs0;
    void* x0;
    void* ubuf[R];
    void* acc[R];
    void* xb[R];
};

// ... and per launch: NB such records by value in the kernel arguments (the set index picks one: a uniform load from the argument
// segment) and the two leading dimensions, which all sets share -- column q of a set's right-hand sides is rhs0 + q ldb, of its
// solutions x0 + q ldx.  One set is the batch of one (NB = 1, the set index a constant: lsa_ndlu_solve_multi); a batch of sets
// instantiates NB = kNdBatchMax whatever J (lsa_ndlu_solve_multi_batch).  Every set runs the same grid and tiles, so it gets the
// same bits either way.  A record with pointers to every column's right-hand side and solution (3 + 5 R of them) would not fit
// the 4 KB of kernel arguments at NB = 16, R = 8; this one (5 + 3 R) is 3712 bytes there.
template <int R, int NB>
struct NdMultiPtrs {
    NdMultiSet<R> set[NB];
    int64_t ldb, ldx;
};
// the widest instance with the largest of the other arguments beside it (nd_fwd_multi_kernel: four table pointers; the merged top
// of a batch takes its NdTop record through a pointer for this reason -- by value it is 368 bytes more), with room for the 256
// bytes of hidden arguments the compiler appends
static_assert(sizeof(NdMultiPtrs<kNdMultiMax, kNdBatchMax>) == (size_t)(5 + 3 * kNdMultiMax) * 8 * kNdBatchMax + 16, "multi-set record layout");
static_assert(sizeof(NdMultiPtrs<kNdMultiMax, kNdBatchMax>) + 4 * sizeof(void*) + 256 <= 4096, "kernel arguments of a multi-column, multi-set launch");

// the NdTop record as a launch passes it: by value for one set (as nd_top_kernel takes it), through device memory for a batch
template <int NB>
using NdTopArg = typename std::conditional<NB == 1, NdTop, const NdTop*>::type;
__device__ __forceinline__ const NdTop& nd_top_ref(const NdTop& t) { return t; }
__device__ __forceinline__ const NdTop& nd_top_ref(const NdTop* t) { return *t; }

// acc0[q] += Fa[0:cn] . vs_q, acc1[q] += Fb[0:cn] . vs_q for the R staged columns (vs_q = vs + q * kMCH): the loads and the order
// of two_row_dot, each factor scalar used R times
template <int LPR, int R, typename MT, typename VT>
__device__ __forceinline__ void two_row_dot_multi(const MT* __restrict__ Fa, const MT* __restrict__ Fb, const VT* vs, int32_t cn, int sl, VT (&acc0)[R],
                                                  VT (&acc1)[R]) {
    int32_t k = sl;
    for (; k + 3 * LPR < cn; k += 4 * LPR) {
        const MT a0 = Fa[k], a1 = Fa[k + LPR], a2 = Fa[k + 2 * LPR], a3 = Fa[k + 3 * LPR];
        const MT b0 = Fb[k], b1 = Fb[k + LPR], b2 = Fb[k + 2 * LPR], b3 = Fb[k + 3 * LPR];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const VT* v = vs + q * kMCH;
            const VT v0 = v[k], v1 = v[k + LPR], v2 = v[k + 2 * LPR], v3 = v[k + 3 * LPR];
            fma_acc(acc0[q], a0, v0);
            fma_acc(acc1[q], b0, v0);
            fma_acc(acc0[q], a1, v1);
            fma_acc(acc1[q], b1, v1);
            fma_acc(acc0[q], a2, v2);
            fma_acc(acc1[q], b2, v2);
            fma_acc(acc0[q], a3, v3);
            fma_acc(acc1[q], b3, v3);
        }
    }
    for (; k < cn; k += LPR) {
        const MT a0 = Fa[k], b0 = Fb[k];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const VT v0 = vs[q * kMCH + k];
            fma_acc(acc0[q], a0, v0);
            fma_acc(acc1[q], b0, v0);
        }
    }
}

template <int LPR, int R, typename MT, typename VT>
__device__ __forceinline__ void two_row_dot_prefetched_multi(const MT* __restrict__ Fa, const MT* __restrict__ Fb, const VT* vs, int32_t cn, int sl,
                                                             VT (&acc0)[R], VT (&acc1)[R], const MT (&pa)[4], const MT (&pb)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int32_t k = sl + j * LPR;
        if (k < cn) {
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const VT v0 = vs[q * kMCH + k];
                fma_acc(acc0[q], pa[j], v0);
                fma_acc(acc1[q], pb[j], v0);
            }
        }
    }
    if (cn > 4 * LPR) two_row_dot_multi<LPR, R>(Fa + 4 * LPR, Fb + 4 * LPR, vs + 4 * LPR, cn - 4 * LPR, sl, acc0, acc1);
}

// upward sweep, one tree level, R columns: workgroup (x = node of the level, y = tile of 512 / LPR rows of its packed L block);
// nd_fwd_tile of ndlu_sweeps.hip per column (no distributed node reaches this form)
template <typename MT, typename VT, int LPR, bool ORDERED, int R, int NB>
__global__ __launch_bounds__(256) void nd_fwd_multi_kernel(const NdSweepNode* __restrict__ lnodes, const int32_t* __restrict__ idx,
                                                           const int32_t* __restrict__ gell, const int32_t* __restrict__ cmap, NdMultiPtrs<R, NB> pp) {
    __shared__ VT vs[R * kMCH];
    const NdSweepNode nd = lnodes[blockIdx.x];
    const int32_t r0 = (int32_t)blockIdx.y * (512 / LPR);
    if (r0 >= nd.orows + nd.brow) return;
    const NdMultiSet<R>& p = pp.set[blockIdx.z];  // (NB = 1: the grid has one layer; the uniform load of the record, as for a batch)
    const VT* rhs0 = (const VT*)p.rhs0;
    VT* x0 = (VT*)p.x0;
    const int64_t ldb = pp.ldb, ldx = pp.ldx;
    const int32_t m = nd.m, f = nd.f;
    const int32_t mr = nd.orows, floc = mr + nd.brow;
    const int32_t* ix = idx + nd.idx_off;
    const int32_t* ge = gell + nd.ge_off;
    const MT* L = (const MT*)p.lfac + nd.lfac_off;
    const int tid = threadIdx.x, sw = tid / LPR, sl = tid % LPR;
    const int32_t ra = r0 + sw, rb = ra + 256 / LPR;
    const MT* La = L + (size_t)min(ra, floc - 1) * m;
    const MT* Lb = L + (size_t)min(rb, floc - 1) * m;
    VT acc0[R], acc1[R];
#pragma unroll
    for (int q = 0; q < R; ++q) acc0[q] = acc1[q] = scalar_traits<VT>::zero();
    // everything that depends only on the node record is requested first: the head of the rows, where the update entries go
    MT pa[4], pb[4];
    row_pair_prefetch<LPR>(La, Lb, min(kMCH, m), sl, pa, pb);
    const bool push = nd.acc_off >= 0;
    const int64_t slot0 = push ? nd.acc_off : 0;
    int32_t ca = 0, cb = 0;
    if (sl == 0 && nd.pacc_off >= 0) {
        if (ra >= mr && ra < floc) ca = cmap[nd.cmap_off + ra - mr];
        if (rb >= mr && rb < floc) cb = cmap[nd.cmap_off + rb - mr];
    }
    // ... then what the children added to the update entries these rows produce
    VT ua[R], ub[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        ua[q] = ub[q] = scalar_traits<VT>::zero();
        if (sl == 0) {
            const VT* slots = (const VT*)p.acc[q] + slot0;
            const VT* ubuf = (const VT*)p.ubuf[q];
            if (ra >= mr && ra < floc) {
                const int32_t jg = m + nd.brow0 + ra - mr;
                ua[q] = push ? slot_sum(slots, nd.nchild, f, jg, ua[q]) : gather_updates(ge, nd.nchild, f, jg, ubuf, ua[q]);
            }
            if (rb >= mr && rb < floc) {
                const int32_t jg = m + nd.brow0 + rb - mr;
                ub[q] = push ? slot_sum(slots, nd.nchild, f, jg, ub[q]) : gather_updates(ge, nd.nchild, f, jg, ubuf, ub[q]);
            }
        }
    }
    for (int32_t c0 = 0; c0 < m; c0 += kMCH) {
        const int32_t cn = min(kMCH, m - c0);
        if (tid < cn) {  // (kMCH = 256: one entry per thread and column)
            const int32_t src = ORDERED ? nd.own0 + c0 + tid : ix[c0 + tid];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const VT v = rhs0[q * ldb + src];
                vs[q * kMCH + tid] = push ? slot_sum((const VT*)p.acc[q] + slot0, nd.nchild, f, c0 + tid, v)
                                          : gather_updates(ge, nd.nchild, f, c0 + tid, (const VT*)p.ubuf[q], v);
            }
        }
        __syncthreads();
        if (c0 == 0) two_row_dot_prefetched_multi<LPR, R>(La, Lb, vs, cn, sl, acc0, acc1, pa, pb);
        else two_row_dot_multi<LPR, R>(La + c0, Lb + c0, vs, cn, sl, acc0, acc1);
        __syncthreads();
    }
    const bool root_push = f == m && !(nd.flags & 1);
    const int32_t xa = ra < mr ? (ORDERED ? nd.own0 + nd.orow0 + ra : ix[nd.orow0 + ra]) : 0;
    const int32_t xc = rb < mr ? (ORDERED ? nd.own0 + nd.orow0 + rb : ix[nd.orow0 + rb]) : 0;
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const VT s0 = lanes_sum<LPR>(acc0[q]), s1 = lanes_sum<LPR>(acc1[q]);
        if (sl == 0) {
            VT* x = x0 + q * ldx;
            VT* xb = (VT*)p.xb[q];
            VT* acc = (VT*)p.acc[q];
            VT* ubuf = (VT*)p.ubuf[q];
            if (ra < mr) {
                x[xa] = s0;
                if (root_push) push_down(ge, nd.nchild, f, ra, xb, s0);
            } else if (ra < floc) {
                const VT u = s_add(ua[q], s0);
                if (nd.pacc_off >= 0) acc[nd.pacc_off + ca] = u;
                else ubuf[nd.u_off + (ra - mr)] = u;
            }
            if (rb < mr) {
                x[xc] = s1;
                if (root_push) push_down(ge, nd.nchild, f, rb, xb, s1);
            } else if (rb < floc) {
                const VT u = s_add(ub[q], s1);
                if (nd.pacc_off >= 0) acc[nd.pacc_off + cb] = u;
                else ubuf[nd.u_off + (rb - mr)] = u;
            }
        }
    }
}

// downward sweep, one tree level, R columns: nd_bwd_tile per column
template <typename MT, typename VT, int LPR, bool ORDERED, int R, int NB>
__global__ __launch_bounds__(256) void nd_bwd_multi_kernel(const NdSweepNode* __restrict__ lnodes, const int32_t* __restrict__ idx,
                                                           const int32_t* __restrict__ gell, NdMultiPtrs<R, NB> pp) {
    constexpr int ROWS = 512 / LPR;
    __shared__ VT vs[R * kMCH];
    const NdSweepNode nd = lnodes[blockIdx.x];
    const int32_t r0 = (int32_t)blockIdx.y * ROWS, ty = (int32_t)blockIdx.y;
    if (r0 >= nd.m || nd.f == nd.m) return;
    const NdMultiSet<R>& p = pp.set[blockIdx.z];  // (NB = 1: the grid has one layer; the uniform load of the record, as for a batch)
    VT* x0 = (VT*)p.x0;
    const int64_t ldx = pp.ldx;
    const int32_t m = nd.m, f = nd.f, b = f - m;
    const int32_t* ix = idx + nd.idx_off;
    const int32_t* ge = gell + nd.ge_off;
    const MT* U = (const MT*)p.ufac + nd.ufac_off;
    const int tid = threadIdx.x, sw = tid / LPR, sl = tid % LPR;
    const int32_t ra = r0 + sw, rb = r0 + sw + 256 / LPR;
    const MT* Ua = U + (size_t)min(ra, m - 1) * b;
    const MT* Ub = U + (size_t)min(rb, m - 1) * b;
    const int32_t ia = ORDERED ? nd.own0 + min(ra, m - 1) : ix[min(ra, m - 1)], ib = ORDERED ? nd.own0 + min(rb, m - 1) : ix[min(rb, m - 1)];
    MT pa[4], pb[4];
    row_pair_prefetch<LPR>(Ua, Ub, min(kMCH, b), sl, pa, pb);
    // the rows' own entries are needed only at the end: issue their loads before the sweep over the boundary
    VT xa[R], xc[R], acc0[R], acc1[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const VT* x = x0 + q * ldx;
        xa[q] = x[ia];
        xc[q] = x[ib];
        acc0[q] = acc1[q] = scalar_traits<VT>::zero();
    }
    for (int32_t c0 = 0; c0 < b; c0 += kMCH) {
        const int32_t cn = min(kMCH, b - c0);
        if (tid < cn) {
#pragma unroll
            for (int q = 0; q < R; ++q) vs[q * kMCH + tid] = ((const VT*)p.xb[q])[nd.u_off + c0 + tid];
        }
        __syncthreads();
        if (c0 == 0) two_row_dot_prefetched_multi<LPR, R>(Ua, Ub, vs, cn, sl, acc0, acc1, pa, pb);
        else two_row_dot_multi<LPR, R>(Ua + c0, Ub + c0, vs, cn, sl, acc0, acc1);
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const VT s0 = lanes_sum<LPR>(acc0[q]), s1 = lanes_sum<LPR>(acc1[q]);
        if (sl == 0) {
            VT* x = x0 + q * ldx;
            VT* xb = (VT*)p.xb[q];
            if (ra < m) {
                const VT v = s_sub(xa[q], s0);
                x[ia] = v;
                push_down(ge, nd.nchild, f, ra, xb, v);
            }
            if (rb < m) {
                const VT v = s_sub(xc[q], s1);
                x[ib] = v;
                push_down(ge, nd.nchild, f, rb, xb, v);
            }
        }
    }
    if (nd.nchild > 0) {  // the boundary entries this node received, handed on to the children whose boundaries hold them
        const int32_t ntile = (m + ROWS - 1) / ROWS;
        const int64_t total = (int64_t)nd.nchild * b;
        for (int64_t e = (int64_t)ty * 256 + tid; e < total; e += (int64_t)ntile * 256) {
            const int32_t c = (int32_t)(e / b), j = (int32_t)(e - (int64_t)c * b);
            const int32_t g = ge[(size_t)c * f + m + j];
            if (g >= 0) {
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    VT* xb = (VT*)p.xb[q];
                    xb[g] = xb[nd.u_off + j];
                }
            }
        }
    }
}

// the merged top, R columns: nd_top_tile per column (8 rows of T per workgroup, a wave per row pair)
template <typename MT, typename VT, int R, int NB>
__global__ __launch_bounds__(256) void nd_top_multi_kernel(NdTopArg<NB> tpa, const int32_t* __restrict__ icmap, const int32_t* __restrict__ gell,
                                                           NdMultiPtrs<R, NB> pp) {
    constexpr int LPR = 64;
    __shared__ VT vs[R * kMCH];
    const NdTop& tp = nd_top_ref(tpa);
    const NdMultiSet<R>& p = pp.set[blockIdx.y];
    const VT* rhs0 = (const VT*)p.rhs0;
    VT* x0 = (VT*)p.x0;
    const int64_t ldb = pp.ldb, ldx = pp.ldx;
    const int32_t r0 = (int32_t)blockIdx.x * 8;
    const int32_t s = tp.s, K = tp.nchild;
    const NdTopNode& Rt = tp.node[K];
    const MT* top = (const MT*)p.top;
    const int tid = threadIdx.x, sw = tid / LPR, sl = tid % LPR;
    const int32_t ra = r0 + sw, rb = ra + 256 / LPR;
    const MT* Ta = top + (size_t)min(ra, s - 1) * s;
    const MT* Tb = top + (size_t)min(rb, s - 1) * s;
    VT acc0[R], acc1[R];
#pragma unroll
    for (int q = 0; q < R; ++q) acc0[q] = acc1[q] = scalar_traits<VT>::zero();
    MT pa[4], pb[4];
    row_pair_prefetch<LPR>(Ta, Tb, min(kMCH, s), sl, pa, pb);
    for (int32_t c0 = 0; c0 < s; c0 += kMCH) {
        const int32_t c1 = min(c0 + kMCH, s);
        const int32_t j = c0 + tid;  // (kMCH = 256: one entry per thread and column)
        if (j < c1) {
            if (j >= Rt.off) {
                const int32_t k = j - Rt.off;
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    const VT* acc = (const VT*)p.acc[q];
                    VT z = rhs0[q * ldb + Rt.own0 + k];
                    for (int32_t c = 0; c < K; ++c) {
                        const NdTopNode& nd = tp.node[c];
                        const int32_t pp = icmap[(size_t)c * Rt.m + k];
                        if (pp >= 0) z = s_add(z, slot_sum(acc + nd.acc_off, nd.nchild, nd.f, nd.m + pp, scalar_traits<VT>::zero()));
                    }
                    vs[q * kMCH + tid] = z;
                }
            } else {
                for (int32_t c = 0; c < K; ++c) {
                    const NdTopNode& nd = tp.node[c];
                    if (j < nd.off || j >= nd.off + nd.m) continue;
                    const int32_t r = j - nd.off;
#pragma unroll
                    for (int q = 0; q < R; ++q)
                        vs[q * kMCH + tid] = slot_sum((const VT*)p.acc[q] + nd.acc_off, nd.nchild, nd.f, r, rhs0[q * ldb + nd.own0 + r]);
                }
            }
        }
        __syncthreads();
        if (c0 == 0) two_row_dot_prefetched_multi<LPR, R>(Ta, Tb, vs, c1 - c0, sl, acc0, acc1, pa, pb);
        else two_row_dot_multi<LPR, R>(Ta + c0, Tb + c0, vs, c1 - c0, sl, acc0, acc1);
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const VT s0 = lanes_sum<LPR>(acc0[q]), s1 = lanes_sum<LPR>(acc1[q]);
        if (sl == 0) {
            if (ra < s) nd_top_store(tp, ra, s0, icmap, gell, x0 + q * ldx, (VT*)p.xb[q]);
            if (rb < s) nd_top_store(tp, rb, s1, icmap, gell, x0 + q * ldx, (VT*)p.xb[q]);
        }
    }
}

// x_zq = C_z^-1 b_zq for the R columns of one pass on J <= NB factor sets of one analysis: nd_sweep of ndlu_sweeps.hip for one rank
// and no distributed node, the same grids with the set as their last dimension, one launch per level and direction for all
// columns of all sets, on the tables of f[0].  Column q of set z is b[z] + q ldb -> x[z] + q ldx; column 0 runs on the
// factorisation's own sweep buffers, column q > 0 on f[z]->multi[q - 1].
template <typename MT, typename VT, bool ORDERED, int R, int NB>
int nd_sweep_multi(lsa_ctx* ctx, int32_t J, lsa_ndlu* const* f, const VT* const* b, int64_t ldb, VT* const* x, int64_t ldx) {
    hipStream_t st = ctx->stream;
    const lsa_ndlu* f0 = f[0];
    if (J < 1 || J > NB) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu: a block solve on %d factor sets, at most %d", J, NB);
    NdMultiPtrs<R, NB> p;
    memset(&p, 0, sizeof p);
    p.ldb = ldb;
    p.ldx = ldx;
    for (int32_t z = 0; z < J; ++z) {
        lsa_ndlu* g = f[z];
        NdMultiSet<R>& s = p.set[z];
        s.lfac = g->d_lfac;
        s.ufac = g->d_ufac;
        s.top = g->d_top;
        s.rhs0 = b[z];
        s.x0 = x[z];
        const size_t acc_bytes = (size_t)std::max<int64_t>(g->acc_entries, 1) * 16;
        for (int q = 0; q < R; ++q) {
            void* acc = q == 0 ? g->d_acc : g->multi[(size_t)q - 1].acc;
            int& vbytes = q == 0 ? g->acc_vbytes : g->multi[(size_t)q - 1].acc_vbytes;
            if (vbytes != (int)sizeof(VT)) {  // (the rule of nd_sweep, per copy of the slot rows)
                LSA_HIP_CHECK(ctx, hipMemsetAsync(acc, 0, acc_bytes, st));
                vbytes = (int)sizeof(VT);
            }
            s.acc[q] = acc;
            s.ubuf[q] = q == 0 ? g->d_ubuf : g->multi[(size_t)q - 1].ubuf;
            s.xb[q] = q == 0 ? g->d_xb : g->multi[(size_t)q - 1].xb;
        }
    }
    const bool top = ORDERED && f0->top.s > 0;
    for (size_t li = 0; li < f0->levels.size(); ++li) {
        const NdLevel& L = f0->levels[li];
        if (top && (int32_t)li + 1 == f0->top_level) continue;  // the root's children: inside the root's launch
        if (top && (int32_t)li == f0->top_level) {
            NdTopArg<NB> tp;
            if constexpr (NB == 1) tp = f0->top;
            else tp = f0->d_top_rec;
            hipLaunchKernelGGL((nd_top_multi_kernel<MT, VT, R, NB>), dim3((f0->top.s + 7) / 8, J), dim3(256), 0, st, tp, f0->d_top_icmap, f0->d_gell, p);
        } else if (L.fwd_tiles > 0) {
            nd_with_lpr<true>(L.sweep_rows, [&](auto lpr) {
                hipLaunchKernelGGL((nd_fwd_multi_kernel<MT, VT, decltype(lpr)::value, ORDERED, R, NB>), dim3(L.node_count, L.fwd_tiles, J), dim3(256), 0, st,
                                   f0->d_lnodes + L.node_begin, f0->d_idx, f0->d_gell, f0->d_cmap, p);
            });
        }
    }
    for (size_t l = f0->levels.size(); l-- > 0;) {
        const NdLevel& L = f0->levels[l];
        if (L.bwd_tiles > 0 && !(top && (int32_t)l + 1 == f0->top_level)) {
            nd_with_lpr<false>(L.bwd_rows, [&](auto lpr) {
                hipLaunchKernelGGL((nd_bwd_multi_kernel<MT, VT, decltype(lpr)::value, ORDERED, R, NB>), dim3(L.node_count, L.bwd_tiles, J), dim3(256), 0, st,
                                   f0->d_lnodes_bwd + L.node_begin, f0->d_idx, f0->d_gell, p);
            });
        }
    }
    LSA_HIP_CHECK(ctx, hipGetLastError());
    return LSA_OK;
}

// ---- the transposed / conjugate-transposed system, R columns: nd_sweepT_kernel of ndlu_sweeps.hip with every factor scalar
// Fk[k * ld] loaded once for all of them.  Workgroup (node of the level, tile of 64 outputs), the lane = the output column of the
// packed block, the four slices sl = tid >> 6 split the rows summed over.  Per column the arithmetic is the solo kernel's: slice sl
// of a lane adds the rows sl, sl + 4, ... in ascending order into one accumulator -- a sequence that runs on across chunks, so the
// chunk of kMCH = 256 entries gives the bits of the solo kernel's kCH --, the slices are added as (p0 + p1) + (p2 + p3), and the
// epilogue is the solo one.  No distributed node reaches this form.
// The same kernel carries the R columns through J <= NB factor sets of one analysis (the set is the grid's last dimension, its
// record picked from the launch arguments as in the forward kernels): one set is the batch of one (NB = 1, lsa_ndlu_solve_multi),
// a batch of sets instantiates NB = kNdBatchMax whatever J (lsa_ndlu_solve_multi_batch_adjoint).  Every set runs the same grid and
// tiles, so it gets the same bits either way.
template <int R>
struct NdMultiTSet {
    const void *lfac, *ufac;
    const void* rhs[R];
    void* x[R];
    void* ubuf[R];
};
// Every column keeps a pointer of its own for its right-hand side and its solution (unlike NdMultiSet: one base and a shared leading
// dimension): without the slot rows and boundary vectors of the forward sweeps the record has room for them -- 2 + 3 R pointers, 3328
// bytes at NB = 16, R = 8 -- and the one-set solve goes on staging an aliased column in that column's own buffer.
template <int R, int NB>
struct NdMultiTPtrs {
    NdMultiTSet<R> set[NB];
};
static_assert(sizeof(NdMultiTPtrs<kNdMultiMax, kNdBatchMax>) == (size_t)(2 + 3 * kNdMultiMax) * 8 * kNdBatchMax, "transposed multi-set record layout");
// the widest instance beside the kernel's three table pointers, with room for the 256 bytes of hidden arguments the compiler appends
static_assert(sizeof(NdMultiTPtrs<kNdMultiMax, kNdBatchMax>) + 3 * sizeof(void*) + 256 <= 4096, "kernel arguments of a transposed multi-column, multi-set launch");

// gather_updates for R update vectors: v[q] += the children's entries of ubuf[q] that land on front position j, the gather rows'
// entries loaded once; per column the additions of gather_updates in their order
template <int R, typename VT>
__device__ __forceinline__ void gather_updates_multi(const int32_t* __restrict__ ge, int32_t nchild, int32_t f, int32_t j, void* const (&ubuf)[R],
                                                     VT (&v)[R]) {
    int32_t c = 0;
    for (; c + 3 < nchild; c += 4) {
        const int32_t g0 = ge[(size_t)c * f + j], g1 = ge[(size_t)(c + 1) * f + j], g2 = ge[(size_t)(c + 2) * f + j], g3 = ge[(size_t)(c + 3) * f + j];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const VT* ub = (const VT*)ubuf[q];
            const VT u0 = g0 >= 0 ? ub[g0] : scalar_traits<VT>::zero(), u1 = g1 >= 0 ? ub[g1] : scalar_traits<VT>::zero();
            const VT u2 = g2 >= 0 ? ub[g2] : scalar_traits<VT>::zero(), u3 = g3 >= 0 ? ub[g3] : scalar_traits<VT>::zero();
            v[q] = s_add(s_add(s_add(s_add(v[q], u0), u1), u2), u3);
        }
    }
    int32_t g[3] = {-1, -1, -1};
    for (int i = 0; i < 3; ++i)
        if (c + i < nchild) g[i] = ge[(size_t)(c + i) * f + j];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const VT* ub = (const VT*)ubuf[q];
        VT u[3];
        for (int i = 0; i < 3; ++i) u[i] = g[i] >= 0 ? ub[g[i]] : scalar_traits<VT>::zero();
        for (int i = 0; i < 3; ++i)
            if (c + i < nchild) v[q] = s_add(v[q], u[i]);
    }
}

template <typename MT, typename VT, bool CONJ, bool DOWN, int R, int NB>
__global__ __launch_bounds__(256) void nd_sweepT_multi_kernel(const NdSweepNode* __restrict__ lnodes, const int32_t* __restrict__ idx,
                                                              const int32_t* __restrict__ gell, NdMultiTPtrs<R, NB> pp) {
    __shared__ VT vs[R * kMCH];
    __shared__ VT part[R][4][64];
    static_assert(kMCH == 256, "one staged entry per thread and column");
    static_assert(sizeof(VT) * R * (kMCH + 4 * 64) <= 64 * 1024, "LDS of a transposed multi-column tile");
    const NdSweepNode nd = lnodes[blockIdx.x];
    const int32_t m = nd.m, f = nd.f, b = f - m;
    const int32_t ncols = DOWN ? m : f;              // outputs of this sweep
    const int32_t klo = DOWN ? nd.brow0 : nd.orow0;  // rows summed over (all of them: the node is not distributed)
    const int32_t K = DOWN ? nd.brow : nd.orows;
    const int32_t c0 = (int32_t)blockIdx.y * 64;
    if (c0 >= ncols || (DOWN && b == 0)) return;
    const NdMultiTSet<R>& p = pp.set[blockIdx.z];  // (NB = 1: the grid has one layer; the uniform load of the record, as for a batch)
    const MT* __restrict__ lfac = (const MT*)p.lfac;
    const MT* __restrict__ ufac = (const MT*)p.ufac;
    const int32_t* ix = idx + nd.idx_off;
    const int32_t* ge = gell + nd.ge_off;
    const int tid = threadIdx.x, lane = tid & 63, sl = tid >> 6;
    const int32_t col = min(c0 + lane, ncols - 1);
    const MT* Fc;
    int32_t ld;
    if (DOWN) Fc = lfac + nd.lfac_off + (size_t)nd.orows * m + col, ld = m;
    else if (col < m) Fc = lfac + nd.lfac_off + col, ld = m;
    else Fc = ufac + nd.ufac_off + (col - m), ld = b;
    VT acc[R];
#pragma unroll
    for (int q = 0; q < R; ++q) acc[q] = scalar_traits<VT>::zero();
    for (int32_t k0 = 0; k0 < K; k0 += kMCH) {
        const int32_t kn = min(kMCH, K - k0);
        if (tid < kn) {  // one entry per thread and column, its index loaded once
            if (DOWN) {
                const int32_t src = ix[m + klo + k0 + tid];
#pragma unroll
                for (int q = 0; q < R; ++q) vs[q * kMCH + tid] = ((const VT*)p.x[q])[src];
            } else {
                const int32_t j = klo + k0 + tid, src = ix[j];
                VT v[R];
#pragma unroll
                for (int q = 0; q < R; ++q) v[q] = ((const VT*)p.rhs[q])[src];
                gather_updates_multi<R>(ge, nd.nchild, f, j, p.ubuf, v);
#pragma unroll
                for (int q = 0; q < R; ++q) vs[q * kMCH + tid] = v[q];
            }
        }
        __syncthreads();
        const MT* Fk = Fc + (size_t)k0 * ld;
        int32_t k = sl;
        for (; k + 12 < kn; k += 16) {
            const MT a0 = maybe_conj<CONJ>(Fk[(size_t)k * ld]), a1 = maybe_conj<CONJ>(Fk[(size_t)(k + 4) * ld]);
            const MT a2 = maybe_conj<CONJ>(Fk[(size_t)(k + 8) * ld]), a3 = maybe_conj<CONJ>(Fk[(size_t)(k + 12) * ld]);
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const VT* v = vs + q * kMCH;
                fma_acc(acc[q], a0, v[k]);
                fma_acc(acc[q], a1, v[k + 4]);
                fma_acc(acc[q], a2, v[k + 8]);
                fma_acc(acc[q], a3, v[k + 12]);
            }
        }
        for (; k < kn; k += 4) {
            const MT a0 = maybe_conj<CONJ>(Fk[(size_t)k * ld]);
#pragma unroll
            for (int q = 0; q < R; ++q) fma_acc(acc[q], a0, vs[q * kMCH + k]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < R; ++q) part[q][sl][lane] = acc[q];
    __syncthreads();
    if (sl == 0 && c0 + lane < ncols) {
        const int32_t r = c0 + lane;
        VT z[R];
#pragma unroll
        for (int q = 0; q < R; ++q) z[q] = s_add(s_add(part[q][0][lane], part[q][1][lane]), s_add(part[q][2][lane], part[q][3][lane]));
        if (DOWN || r < m) {
            const int32_t dst = ix[r];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                VT* x = (VT*)p.x[q];
                x[dst] = DOWN ? s_add(x[dst], z[q]) : z[q];
            }
        } else {
            VT u[R];
#pragma unroll
            for (int q = 0; q < R; ++q) u[q] = scalar_traits<VT>::zero();
            gather_updates_multi<R>(ge, nd.nchild, f, r, p.ubuf, u);
#pragma unroll
            for (int q = 0; q < R; ++q) ((VT*)p.ubuf[q])[nd.u_off + (r - m)] = s_sub(u[q], z[q]);
        }
    }
}

// x_zq = C_z^-T b_zq (C_z^-H b_zq with CONJ) for the R columns of one pass on J <= NB factor sets of one analysis: the launches of
// nd_sweepT for one rank and no distributed node -- all levels upward, then all levels downward, the unmerged blocks throughout (the
// transposed sweeps do not use the assembled top) --, the set as the grids' last dimension, on the tables of f[0].  The caller gave
// p the columns' right-hand sides and solutions; column 0 of a set runs on the factorisation's own update vectors, column q > 0 on
// f[z]->multi[q - 1].ubuf; the slot rows and boundary vectors of the forward sweeps are not touched.
template <typename MT, typename VT, bool CONJ, int R, int NB>
int nd_sweepT_multi(lsa_ctx* ctx, int32_t J, lsa_ndlu* const* f, NdMultiTPtrs<R, NB>& p) {
    hipStream_t st = ctx->stream;
    const lsa_ndlu* f0 = f[0];
    if (J < 1 || J > NB) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu: a transposed block solve on %d factor sets, at most %d", J, NB);
    for (int32_t z = 0; z < J; ++z) {
        NdMultiTSet<R>& s = p.set[z];
        s.lfac = f[z]->d_lfac;
        s.ufac = f[z]->d_ufac;
        for (int q = 0; q < R; ++q) s.ubuf[q] = q == 0 ? f[z]->d_ubuf : f[z]->multi[(size_t)q - 1].ubuf;
    }
    for (size_t li = 0; li < f0->levels.size(); ++li) {
        const NdLevel& L = f0->levels[li];
        if (L.fwd_tiles > 0)
            hipLaunchKernelGGL((nd_sweepT_multi_kernel<MT, VT, CONJ, false, R, NB>), dim3(L.node_count, (L.max_f + 63) / 64, J), dim3(256), 0, st,
                               f0->d_lnodes + L.node_begin, f0->d_idx, f0->d_gell, p);
    }
    for (size_t l = f0->levels.size(); l-- > 0;) {
        const NdLevel& L = f0->levels[l];
        if (L.bwd_tiles > 0)
            hipLaunchKernelGGL((nd_sweepT_multi_kernel<MT, VT, CONJ, true, R, NB>), dim3(L.node_count, (L.max_m + 63) / 64, J), dim3(256), 0, st,
                               f0->d_lnodes + L.node_begin, f0->d_idx, f0->d_gell, p);
    }
    LSA_HIP_CHECK(ctx, hipGetLastError());
    return LSA_OK;
}

// sweep buffers for passes of `want` columns; returns how many columns a pass can have (1 + the extra sets that fitted).  An
// allocation that fails narrows the passes of this and every later call; it is not an error.
int32_t nd_multi_ensure(lsa_ctx* ctx, lsa_ndlu* f, int32_t want) {
    const size_t ub = (size_t)std::max<int64_t>(f->S.u_off[(size_t)f->S.nt], 1) * 16;
    const size_t ab = (size_t)std::max<int64_t>(f->acc_entries, 1) * 16;
    const size_t tb = (size_t)std::max<int32_t>(f->S.n, 1) * 16;
    while ((int32_t)f->multi.size() + 1 < want && !f->multi_full) {
        lsa_ndlu::MultiColumn c;
        const bool ok = hipMalloc(&c.ubuf, ub) == hipSuccess && hipMalloc(&c.xb, ub) == hipSuccess && hipMalloc(&c.acc, ab) == hipSuccess &&
                        hipMalloc(&c.tmp, tb) == hipSuccess;
        // as nd_setup_buffers leaves them; the slot rows are zeroed by their first use (acc_vbytes = 0 matches no vector scalar)
        if (!ok || hipMemsetAsync(c.ubuf, 0, ub, ctx->stream) != hipSuccess || hipMemsetAsync(c.xb, 0, ub, ctx->stream) != hipSuccess) {
            (void)hipGetLastError();
            for (void* q : {c.ubuf, c.xb, c.acc, c.tmp})
                if (q) (void)hipFree(q);
            f->multi_full = true;
            break;
        }
        f->multi.push_back(c);
        f->multi_bytes += (int64_t)(2 * ub + ab + tb);
    }
    return std::min<int32_t>(want, (int32_t)f->multi.size() + 1);
}

// The widest pass for vectors of vbytes-byte scalars, from the measurement (profiles/multi_rhs.json): every
// width measured beat the solo loop per column, but eight complex columns (255 VGPRs, one wave per SIMD) took 560 us per column
// at 500 k unknowns where four take 453 (the same within 3 % at 30 k), so complex vectors stop at four and the kernels of eight
// complex columns are not built; eight real columns (as many bytes as four complex ones) are as fast as four or faster.
// LSA_ND_MULTI_WIDTH lowers it (1, 2, 4, 8; for measurements).
int32_t nd_multi_cap(size_t vbytes) {
    static const int32_t env = [] {
        const char* e = getenv("LSA_ND_MULTI_WIDTH");
        return e && *e ? std::max(1, std::min(kNdMultiMax, atoi(e))) : kNdMultiMax;
    }();
    return std::min<int32_t>(env, vbytes == 16 ? 4 : kNdMultiMax);
}

// columns of the next pass when `left` are left and a pass may have `most`: 8, 4, 2, or 1 (a solo solve)
int32_t nd_pass_width(int32_t left, int32_t most) {
    const int32_t w = std::min(left, most);
    return w >= 8 ? 8 : w >= 4 ? 4 : w >= 2 ? 2 : 1;
}

// An aliased block (B == X, ldb == ldx) is solved from a copy: the sweeps read a right-hand side after they began to write the
// solution.  The record of a launch addresses a set's columns by one base and the shared leading dimension, so the copy of a
// pass's W columns is one strided block of the set's own (lsa_ndlu::multi_stage, grown on demand), the columns ldb apart as in B.
template <typename VT>
int nd_multi_stage(lsa_ctx* ctx, lsa_ndlu* f, int32_t W, const VT* b, int64_t ldb, const VT** out) {
    const size_t need = ((size_t)(W - 1) * (size_t)ldb + (size_t)f->S.n) * sizeof(VT);
    if (f->multi_stage_bytes < (int64_t)need) {
        if (f->multi_stage) (void)hipFree(f->multi_stage);
        f->multi_stage = nullptr;
        f->multi_bytes -= f->multi_stage_bytes;
        f->multi_stage_bytes = 0;
        LSA_HIP_ALLOC(ctx, hipMalloc(&f->multi_stage, need));
        f->multi_stage_bytes = (int64_t)need;
        f->multi_bytes += (int64_t)need;
    }
    LSA_HIP_CHECK(ctx, hipMemcpy2DAsync(f->multi_stage, (size_t)ldb * sizeof(VT), b, (size_t)ldb * sizeof(VT), (size_t)f->S.n * sizeof(VT), (size_t)W,
                                        hipMemcpyDeviceToDevice, ctx->stream));
    *out = (const VT*)f->multi_stage;
    return LSA_OK;
}

// fn(std::integral_constant<int, R>) for the pass widths that are built: 8 for 8-byte vector scalars only (nd_multi_cap), 4 and 2
template <typename VT, typename F>
int nd_with_width(int32_t R, F&& fn) {
    if constexpr (sizeof(VT) == 8)
        if (R == 8) return fn(std::integral_constant<int, 8>{});
    if (R == 4) return fn(std::integral_constant<int, 4>{});
    return fn(std::integral_constant<int, 2>{});
}

// The one pass driver: the request's nrhs >= 2 columns on its J <= NB sets in passes of 8, 4 or 2 columns, the widest every set has
// buffers for (a remainder runs in narrower passes); a last single column goes through the single-column sweeps of the same capacity
// and direction.  DIR (0 N, 1 T, 2 H) supplies only its launch record and its sweep.  An aliased block is solved from a copy, as the
// form has always staged it: the forward passes and the transposed ones on a batch of sets in the set's strided stage block
// (nd_multi_stage), the transposed passes on one set column by column in the columns' own tmp buffers.
template <typename MT, typename VT, int NB, int DIR>
int nd_solve_passes(lsa_ctx* ctx, const NdSolve& rq, NdSolveInfo* info) {
    const int32_t J = rq.J;
    lsa_ndlu* const* f = rq.f;
    const int64_t ldb = rq.ldb, ldx = rq.ldx;
    // (buffers for the widest pass that will run: the first)
    const int32_t want = nd_pass_width(rq.nrhs, nd_multi_cap(sizeof(VT)));
    int32_t avail = want;
    for (int32_t z = 0; z < J; ++z) avail = std::min(avail, nd_multi_ensure(ctx, f[z], want));
    NdSolveInfo done = {0, 1};
    for (int32_t q0 = 0; q0 < rq.nrhs;) {
        const int32_t R = nd_pass_width(rq.nrhs - q0, avail);
        const VT* b[NB];
        VT* x[NB];
        for (int32_t z = 0; z < J; ++z) {
            b[z] = (const VT*)rq.B[z] + (int64_t)q0 * ldb;
            x[z] = (VT*)rq.X[z] + (int64_t)q0 * ldx;
        }
        if (R == 1) {
            LSA_CHECK(ndlu_solve_column(ctx, rq, (const void* const*)b, (void* const*)x));
            q0 += 1;
            continue;
        }
        if constexpr (DIR == 0 || NB > 1)
            for (int32_t z = 0; z < J; ++z)
                if (b[z] == x[z]) LSA_CHECK(nd_multi_stage(ctx, f[z], R, b[z], ldb, &b[z]));
        LSA_CHECK(nd_with_width<VT>(R, [&](auto width) {
            constexpr int W = decltype(width)::value;
            if constexpr (DIR == 0) {
                return f[0]->ordered ? nd_sweep_multi<MT, VT, true, W, NB>(ctx, J, f, b, ldb, x, ldx) : nd_sweep_multi<MT, VT, false, W, NB>(ctx, J, f, b, ldb, x, ldx);
            } else {
                NdMultiTPtrs<W, NB> p;
                memset(&p, 0, sizeof p);
                for (int32_t z = 0; z < J; ++z)
                    for (int q = 0; q < W; ++q) {
                        const VT* bq = b[z] + (int64_t)q * ldb;
                        VT* xq = x[z] + (int64_t)q * ldx;
                        if constexpr (NB == 1)
                            if (bq == xq) {  // in place: a tile reads the node's right-hand side while the others write its solution
                                void* tmp = q == 0 ? f[z]->d_tmp : f[z]->multi[(size_t)q - 1].tmp;
                                LSA_HIP_CHECK(ctx, hipMemcpyAsync(tmp, bq, (size_t)f[z]->S.n * sizeof(VT), hipMemcpyDeviceToDevice, ctx->stream));
                                bq = (const VT*)tmp;
                            }
                        p.set[z].rhs[q] = bq;
                        p.set[z].x[q] = xq;
                    }
                return nd_sweepT_multi<MT, VT, DIR == 2, W, NB>(ctx, J, f, p);
            }
        }));
        done.width = std::max(done.width, R);
        ++done.passes;
        q0 += R;
    }
    for (int32_t z = 0; z < J; ++z) f[z]->multi_width = done.width, f[z]->multi_passes = done.passes;
    if (info) *info = done;
    return LSA_OK;
}

}  // namespace

void ndlu_multi_free(lsa_ndlu* f) {
    for (lsa_ndlu::MultiColumn& c : f->multi)
        for (void* q : {c.ubuf, c.xb, c.acc, c.tmp})
            if (q) (void)hipFree(q);
    f->multi.clear();
    if (f->multi_stage) (void)hipFree(f->multi_stage);
    f->multi_stage = nullptr;
    f->multi_stage_bytes = 0;
    f->multi_bytes = 0;
}

// the one internal entry of the solves (NdSolve, ndlu_internal.h): one column is the single-column sweep, more go to the pass driver
int ndlu_solve_run(lsa_ctx* ctx, const NdSolve& rq, NdSolveInfo* info) {
    if (info) *info = {0, 1};
    const int32_t most = rq.sets ? kNdBatchMax : 1;
    if (rq.J < 1 || rq.J > most) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: J = %d outside [1, %d]", rq.who, rq.J, most);
    if (rq.nrhs == 1) return ndlu_solve_column(ctx, rq, rq.B, rq.X);
    return nd_dispatch_solve(ctx, rq.who, true, rq.J, rq.f, rq.trans, rq.vdtype, [&](auto mt, auto vt, auto dir) {
        using MT = decltype(mt);
        using VT = decltype(vt);
        constexpr int DIR = decltype(dir)::value;
        return rq.sets ? nd_solve_passes<MT, VT, kNdBatchMax, DIR>(ctx, rq, info) : nd_solve_passes<MT, VT, 1, DIR>(ctx, rq, info);
    });
}
