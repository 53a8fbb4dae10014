// Nested-dissection multifrontal LU, the solves: the upward and downward sweeps over the tree (one launch per level and
// direction; the root and its children as one launch where the top is merged), their exchanges over distributed nodes, the
// transposed sweeps (solo and batched alike: lsa_ndlu_solve_adjoint, lsa_ndlu_solve_batch_adjoint), and the one driver behind
// lsa_ndlu_solve, lsa_ndlu_solve_batch and the solver's inner solves.
// Layout and sweep scheme: ndlu.hip; records and tables: ndlu_internal.h.
#include "ndlu_sweep_parts.h"

namespace {

// One tile of the upward sweep: 512 / LPR rows from r0 of node nd's packed L block.  LPR lanes run along a pair of rows: 16 (32
// rows per workgroup) where the level has many tiles, 64 (8 rows) near the top of the tree, where a few tall fronts must still be
// spread over the whole chip, 4 (128 rows) on levels of thin separators.
// ORDERED: the vectors are in elimination order (own unknown r of the node = own0 + r), else through idx.
// A root (no boundary) also starts the downward sweep: its rows are final, they go to its children's boundary vectors.
template <typename MT, typename VT, int LPR, bool ORDERED>
__device__ __forceinline__ void nd_fwd_tile(const NdSweepNode& nd, int32_t r0, VT* vs, const MT* __restrict__ lfac, const int32_t* __restrict__ idx,
                                            const int32_t* __restrict__ gell, const int32_t* __restrict__ cmap, const VT* __restrict__ rhs,
                                            VT* __restrict__ x, VT* __restrict__ ubuf, VT* __restrict__ acc, VT* __restrict__ xb) {
    const int32_t m = nd.m, f = nd.f;
    // rows of the packed L on this rank: its own rows of the inverse, then its boundary rows (m and f - m of them unless the node
    // is distributed: then orows rows from orow0 and brow rows from brow0)
    const int32_t mr = nd.orows, floc = mr + nd.brow;
    const int32_t* ix = idx + nd.idx_off;
    const int32_t* ge = gell + nd.ge_off;
    const MT* L = lfac + nd.lfac_off;
    const int tid = threadIdx.x, sw = tid / LPR, sl = tid % LPR;
    const int32_t ra = r0 + sw, rb = ra + 256 / LPR;
    const MT* La = L + (size_t)min(ra, floc - 1) * m;
    const MT* Lb = L + (size_t)min(rb, floc - 1) * m;
    VT acc0 = scalar_traits<VT>::zero(), acc1 = scalar_traits<VT>::zero();
    // everything that depends only on the node record is requested first: the head of the rows, where the update entries go
    MT pa[4], pb[4];
    row_pair_prefetch<LPR>(La, Lb, min(kCH, m), sl, pa, pb);
    const bool push = nd.acc_off >= 0;
    const VT* slots = acc + (push ? nd.acc_off : 0);
    int32_t ca = 0, cb = 0;
    if (sl == 0 && nd.pacc_off >= 0) {
        if (ra >= mr && ra < floc) ca = cmap[nd.cmap_off + ra - mr];
        if (rb >= mr && rb < floc) cb = cmap[nd.cmap_off + rb - mr];
    }
    // ... then what the children added to the update entries these rows produce (front position of local row r >= mr: m + brow0 + r - mr)
    VT ua = scalar_traits<VT>::zero(), ub = scalar_traits<VT>::zero();
    if (sl == 0) {
        if (ra >= mr && ra < floc) {
            const int32_t jg = m + nd.brow0 + ra - mr;
            ua = push ? slot_sum(slots, nd.nchild, f, jg, ua) : gather_updates(ge, nd.nchild, f, jg, ubuf, ua);
        }
        if (rb >= mr && rb < floc) {
            const int32_t jg = m + nd.brow0 + rb - mr;
            ub = push ? slot_sum(slots, nd.nchild, f, jg, ub) : gather_updates(ge, nd.nchild, f, jg, ubuf, ub);
        }
    }
    for (int32_t c0 = 0; c0 < m; c0 += kCH) {
        const int32_t cn = min(kCH, m - c0);
        for (int32_t j = tid; j < cn; j += 256) {
            const VT v = rhs[ORDERED ? nd.own0 + c0 + j : ix[c0 + j]];
            vs[j] = push ? slot_sum(slots, nd.nchild, f, c0 + j, v) : gather_updates(ge, nd.nchild, f, c0 + j, ubuf, v);
        }
        __syncthreads();
        if (c0 == 0) two_row_dot_prefetched<LPR>(La, Lb, vs, cn, sl, acc0, acc1, pa, pb);
        else two_row_dot<LPR>(La + c0, Lb + c0, vs, cn, sl, acc0, acc1);
        __syncthreads();
    }
    const VT s0 = lanes_sum<LPR>(acc0), s1 = lanes_sum<LPR>(acc1);
    if (sl == 0) {
        const bool root_push = f == m && !(nd.flags & 1);
        if (ra < mr) {
            x[ORDERED ? nd.own0 + nd.orow0 + ra : ix[nd.orow0 + ra]] = s0;
            if (root_push) push_down(ge, nd.nchild, f, ra, xb, s0);
        } else if (ra < floc) {
            const VT u = s_add(ua, s0);
            if (nd.pacc_off >= 0) acc[nd.pacc_off + ca] = u;
            else ubuf[nd.u_off + (ra - mr)] = u;
        }
        if (rb < mr) {
            x[ORDERED ? nd.own0 + nd.orow0 + rb : ix[nd.orow0 + rb]] = s1;
            if (root_push) push_down(ge, nd.nchild, f, rb, xb, s1);
        } else if (rb < floc) {
            const VT u = s_add(ub, s1);
            if (nd.pacc_off >= 0) acc[nd.pacc_off + cb] = u;
            else ubuf[nd.u_off + (rb - mr)] = u;
        }
    }
}

// ---- what a sweep launch gets per problem: the factors and vectors of NB factorisations of one analysis, by value in the
// kernel arguments (the problem index picks them: a uniform load from the argument segment).  The tables are shared.  A solo
// solve is the batch of one (NB = 1: 64 bytes, the problem index a constant); lsa_ndlu_solve_batch instantiates NB = kNdBatchMax
// whatever J.  Every problem runs the same grid and tiles, so it gets the same bits either way.  The transposed sweeps
// (nd_sweepT_kernel) take the same record and read lfac, ufac, rhs, x and ubuf of it.
template <int NB>
struct NdSweepPtrs {
    const void* lfac[NB];
    const void* ufac[NB];
    const void* rhs[NB];
    void* x[NB];
    void* ubuf[NB];
    void* acc[NB];
    void* xb[NB];
    const void* top[NB];  // the assembled inverse of the top (nd_top_kernel), or null
};

// upward sweep, one tree level: workgroup (x = node of the level, y = tile of 512 / LPR rows of its packed L block, z = problem)
template <typename MT, typename VT, int LPR, bool ORDERED, int NB>
__global__ __launch_bounds__(256) void nd_fwd_kernel(const NdSweepNode* __restrict__ lnodes, const int32_t* __restrict__ idx,
                                                     const int32_t* __restrict__ gell, const int32_t* __restrict__ cmap, NdSweepPtrs<NB> p) {
    __shared__ VT vs[kCH];
    const NdSweepNode nd = lnodes[blockIdx.x];
    const int32_t r0 = (int32_t)blockIdx.y * (512 / LPR);
    if (r0 >= nd.orows + nd.brow) return;
    const int z = NB == 1 ? 0 : blockIdx.z;
    nd_fwd_tile<MT, VT, LPR, ORDERED>(nd, r0, vs, (const MT*)p.lfac[z], idx, gell, cmap, (const VT*)p.rhs[z], (VT*)p.x[z], (VT*)p.ubuf[z], (VT*)p.acc[z],
                                      (VT*)p.xb[z]);
}

// One tile of the downward sweep: x[own] -= U x[boundary] for 512 / LPR own rows from r0; the boundary vector was filled by the
// ancestors, and this tile fills the children's: the rows it finishes, and (tile `ty` of the node's `ntile`) its share of the
// boundary entries the node received.
template <typename MT, typename VT, int LPR, bool ORDERED>
__device__ __forceinline__ void nd_bwd_tile(const NdSweepNode& nd, int32_t r0, int32_t ty, VT* vs, const MT* __restrict__ ufac,
                                            const int32_t* __restrict__ idx, const int32_t* __restrict__ gell, VT* __restrict__ x,
                                            VT* __restrict__ xb) {
    constexpr int ROWS = 512 / LPR;
    const int32_t m = nd.m, f = nd.f, b = f - m;
    const int32_t* ix = idx + nd.idx_off;
    const int32_t* ge = gell + nd.ge_off;
    const MT* U = ufac + nd.ufac_off;
    const VT* bv = xb + nd.u_off;
    const int tid = threadIdx.x, sw = tid / LPR, sl = tid % LPR;
    const int32_t ra = r0 + sw, rb = r0 + sw + 256 / LPR;
    const MT* Ua = U + (size_t)min(ra, m - 1) * b;
    const MT* Ub = U + (size_t)min(rb, m - 1) * b;
    const int32_t ia = ORDERED ? nd.own0 + min(ra, m - 1) : ix[min(ra, m - 1)], ib = ORDERED ? nd.own0 + min(rb, m - 1) : ix[min(rb, m - 1)];
    MT pa[4], pb[4];
    row_pair_prefetch<LPR>(Ua, Ub, min(kCH, b), sl, pa, pb);
    // the rows' own entries are needed only at the end: issue their loads before the sweep over the boundary
    const VT xa = x[ia], xc = x[ib];
    // ... and, in the 64-lane form, where the finished rows go in the boundary vectors of up to four children: push_down would
    // load these indices after the reduction, a dependent load at the very end of the launch.  (The 16-lane form stays at the
    // 128 registers that let four of its workgroups share a CU: it leaves them to push_down.)
    constexpr bool GE = LPR == 64;
    int32_t ga[4] = {-1, -1, -1, -1}, gb[4] = {-1, -1, -1, -1};
    if constexpr (GE) {
        if (sl == 0 && nd.nchild <= 4) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c < nd.nchild && ra < m) ga[c] = ge[(size_t)c * f + ra];
                if (c < nd.nchild && rb < m) gb[c] = ge[(size_t)c * f + rb];
            }
        }
    }
    VT acc0 = scalar_traits<VT>::zero(), acc1 = scalar_traits<VT>::zero();
    for (int32_t c0 = 0; c0 < b; c0 += kCH) {
        const int32_t cn = min(kCH, b - c0);
        for (int32_t j = tid; j < cn; j += 256) vs[j] = bv[c0 + j];
        __syncthreads();
        if (c0 == 0) two_row_dot_prefetched<LPR>(Ua, Ub, vs, cn, sl, acc0, acc1, pa, pb);
        else two_row_dot<LPR>(Ua + c0, Ub + c0, vs, cn, sl, acc0, acc1);
        __syncthreads();
    }
    acc0 = lanes_sum<LPR>(acc0);
    acc1 = lanes_sum<LPR>(acc1);
    if (sl == 0) {
        if (ra < m) {
            const VT v = s_sub(xa, acc0);
            x[ia] = v;
            push_down_at<GE>(ge, nd.nchild, f, ra, ga, xb, v);
        }
        if (rb < m) {
            const VT v = s_sub(xc, acc1);
            x[ib] = v;
            push_down_at<GE>(ge, nd.nchild, f, rb, gb, xb, v);
        }
    }
    if (nd.nchild > 0) {  // the boundary entries this node received, handed on to the children whose boundaries hold them
        const int32_t ntile = (m + ROWS - 1) / ROWS;
        const int64_t total = (int64_t)nd.nchild * b;
        for (int64_t e = (int64_t)ty * 256 + tid; e < total; e += (int64_t)ntile * 256) {
            const int32_t c = (int32_t)(e / b), j = (int32_t)(e - (int64_t)c * b);
            const int32_t g = ge[(size_t)c * f + m + j];
            if (g >= 0) xb[g] = bv[j];
        }
    }
}

// downward sweep, one tree level: (node, tile, problem)
template <typename MT, typename VT, int LPR, bool ORDERED, int NB>
__global__ __launch_bounds__(256) void nd_bwd_kernel(const NdSweepNode* __restrict__ lnodes, const int32_t* __restrict__ idx,
                                                     const int32_t* __restrict__ gell, NdSweepPtrs<NB> p) {
    __shared__ VT vs[kCH];
    const NdSweepNode nd = lnodes[blockIdx.x];
    const int32_t r0 = (int32_t)blockIdx.y * (512 / LPR);
    if (r0 >= nd.m || nd.f == nd.m) return;
    const int z = NB == 1 ? 0 : blockIdx.z;
    nd_bwd_tile<MT, VT, LPR, ORDERED>(nd, r0, (int32_t)blockIdx.y, vs, (const MT*)p.ufac[z], idx, gell, (VT*)p.x[z], (VT*)p.xb[z]);
}

// One tile of the merged top: 8 rows of T from r0, a wave per row pair (the shape of nd_fwd_tile<..., 64, ...>).  Every
// workgroup stages [v_c...; z_R] from the right-hand side and the slot rows of the root's children; the sums have one order
// (a child's slot rows in rank order, the children in rank order).  Vectors in elimination order only.
template <typename MT, typename VT>
__device__ __forceinline__ void nd_top_tile(const NdTop& tp, int32_t r0, VT* vs, const MT* __restrict__ top, const int32_t* __restrict__ icmap,
                                            const int32_t* __restrict__ gell, const VT* __restrict__ rhs, VT* __restrict__ x,
                                            const VT* __restrict__ acc, VT* __restrict__ xb) {
    constexpr int LPR = 64;
    const int32_t s = tp.s, K = tp.nchild;
    const NdTopNode& R = tp.node[K];
    const int tid = threadIdx.x, sw = tid / LPR, sl = tid % LPR;
    const int32_t ra = r0 + sw, rb = ra + 256 / LPR;
    const MT* Ta = top + (size_t)min(ra, s - 1) * s;
    const MT* Tb = top + (size_t)min(rb, s - 1) * s;
    VT acc0 = scalar_traits<VT>::zero(), acc1 = scalar_traits<VT>::zero();
    MT pa[4], pb[4];
    row_pair_prefetch<LPR>(Ta, Tb, min(kCH, s), sl, pa, pb);
    // where the rows' outputs go: asked for now, needed after the reduction
    NdTopTargets ta, tb;
    if (sl == 0) {
        nd_top_targets(tp, min(ra, s - 1), icmap, gell, ta);
        nd_top_targets(tp, min(rb, s - 1), icmap, gell, tb);
    }
    for (int32_t c0 = 0; c0 < s; c0 += kCH) {
        const int32_t c1 = min(c0 + kCH, s);
        for (int32_t c = 0; c < K; ++c) {
            const NdTopNode& nd = tp.node[c];
            const VT* slots = acc + nd.acc_off;
            for (int32_t j = max(c0, nd.off) + tid; j < min(c1, nd.off + nd.m); j += 256) {
                const int32_t r = j - nd.off;
                vs[j - c0] = slot_sum(slots, nd.nchild, nd.f, r, rhs[nd.own0 + r]);
            }
        }
        for (int32_t j = max(c0, R.off) + tid; j < c1; j += 256) {
            const int32_t k = j - R.off;
            VT z = rhs[R.own0 + k];
            for (int32_t c = 0; c < K; ++c) {
                const NdTopNode& nd = tp.node[c];
                const int32_t p = icmap[(size_t)c * R.m + k];
                if (p >= 0) z = s_add(z, slot_sum(acc + nd.acc_off, nd.nchild, nd.f, nd.m + p, scalar_traits<VT>::zero()));
            }
            vs[j - c0] = z;
        }
        __syncthreads();
        if (c0 == 0) two_row_dot_prefetched<LPR>(Ta, Tb, vs, c1 - c0, sl, acc0, acc1, pa, pb);
        else two_row_dot<LPR>(Ta + c0, Tb + c0, vs, c1 - c0, sl, acc0, acc1);
        __syncthreads();
    }
    const VT s0 = lanes_sum<LPR>(acc0), s1 = lanes_sum<LPR>(acc1);
    if (sl == 0) {
        if (ra < s) nd_top_store(tp, ra, s0, ta, icmap, gell, x, xb);
        if (rb < s) nd_top_store(tp, rb, s1, tb, icmap, gell, x, xb);
    }
}

// (tile, problem)
template <typename MT, typename VT, int NB>
__global__ __launch_bounds__(256) void nd_top_kernel(NdTop tp, const int32_t* __restrict__ icmap, const int32_t* __restrict__ gell, NdSweepPtrs<NB> p) {
    __shared__ VT vs[kCH];
    const int z = NB == 1 ? 0 : blockIdx.y;
    nd_top_tile<MT, VT>(tp, (int32_t)blockIdx.x * 8, vs, (const MT*)p.top[z], icmap, gell, (const VT*)p.rhs[z], (VT*)p.x[z], (const VT*)p.acc[z],
                        (VT*)p.xb[z]);
}

// ---- downward sweep of DISTRIBUTED top nodes: a rank finishes its slice of the node's own rows (nd_bwd_kernel on a record
// that describes the slice), the slices are exchanged through the own-row buffer (pack, one in-place all-gather per level), and
// this kernel completes x and fills the boundary vectors of the node's children: entry k of child c's boundary is the parent's
// front position cmap_c[k] -- one of the parent's own rows (from the exchange buffer) or one of its boundary entries.
// grid: (distributed node of the level, 0 = the node's own rows / 1 + child, tile of 256 entries)
template <typename VT, bool ORDERED>
__global__ __launch_bounds__(256) void nd_dist_pack_kernel(const int32_t* __restrict__ dnodes, const NdNodeDev* __restrict__ nodes,
                                                           const int32_t* __restrict__ idx, int32_t rank, const VT* __restrict__ x, VT* __restrict__ xg) {
    const NdNodeDev nd = nodes[dnodes[blockIdx.x]];
    const int32_t r = (int32_t)blockIdx.y * 256 + threadIdx.x;
    if (r >= nd.orows) return;
    const int32_t j = nd.orow0 + r;
    xg[nd.xg_base + (int64_t)rank * nd.xg_stride + r] = x[ORDERED ? nd.own0 + j : idx[nd.idx_off + j]];
}

template <typename VT, bool ORDERED>
__global__ __launch_bounds__(256) void nd_dist_unpack_kernel(const int32_t* __restrict__ dnodes, const NdNodeDev* __restrict__ nodes,
                                                             const int32_t* __restrict__ child_ptr, const int32_t* __restrict__ child_idx,
                                                             const int32_t* __restrict__ cmap, const int32_t* __restrict__ idx, int32_t nranks,
                                                             VT* x, const VT* __restrict__ xg, VT* xb) {
    const int32_t t = dnodes[blockIdx.x];
    const NdNodeDev nd = nodes[t];
    const int32_t m = nd.m, b = nd.f - m;
    const int32_t ms = (m + nranks - 1) / nranks;
    const int32_t i = (int32_t)blockIdx.z * 256 + threadIdx.x;
    (void)b;
    auto own_val = [&](int32_t j) -> VT { return xg[nd.xg_base + (int64_t)(j / ms) * nd.xg_stride + j % ms]; };
    if (blockIdx.y == 0) {
        if (i >= m) return;
        x[ORDERED ? nd.own0 + i : idx[nd.idx_off + i]] = own_val(i);
        return;
    }
    const int32_t cp = child_ptr[t] + (int32_t)blockIdx.y - 1;
    if (cp >= child_ptr[t + 1]) return;
    const NdNodeDev nc = nodes[child_idx[cp]];
    if (i >= nc.f - nc.m) return;
    const int32_t p = cmap[nc.cmap_off + i];
    xb[nc.u_off + i] = p < m ? own_val(p) : xb[nd.u_off + (p - m)];
}

// ---- sweeps of the transposed / conjugate-transposed system on the same factors (the adjoint eigenproblem of
// Sensitivity/__init__.py:230-311 needs (A - sigma M)^-H without a second factorisation) --------------------------------------
// C^T has the fronts F^T, so with the stored blocks  inv = F11^-1, S1 = -F21 inv, S2 = inv F12:
//     up:    z = [inv | S2]^T v   (the columns of the packed inv and U blocks);  y[own] = z[:m];  update = v_B - z[m:]
//     down:  x[own] = y[own] + S1^T x[boundary]
// Column access of row-major blocks: 64 lanes run along a row (coalesced), four slices of the rows per workgroup.  These
// sweeps keep the pull form (gather rows + update vectors) and address the vectors through idx.
// (maybe_conj: ndlu_sweep_parts.h, shared with the multi-column form of this kernel in ndlu_multi.hip.)
// One tile: 64 outputs from c0 of node nd.  DIST: the node may be distributed (this rank's rows only, the sums go to the rank's
// slot of the partial buffer); a batch has no such node.
template <typename MT, typename VT, bool CONJ, bool DOWN, bool DIST>
__device__ __forceinline__ void nd_sweepT_tile(const NdSweepNode& nd, int32_t c0, VT* vs, VT (*part)[64], const MT* __restrict__ lfac,
                                               const MT* __restrict__ ufac, const int32_t* __restrict__ idx, const int32_t* __restrict__ gell,
                                               const VT* __restrict__ rhs, VT* __restrict__ x, VT* __restrict__ ubuf, const int64_t* __restrict__ tgoff,
                                               VT* __restrict__ pz, int64_t tg_slot, int32_t rank) {
    const int32_t m = nd.m, f = nd.f, b = f - m;
    const bool dist = DIST && (nd.flags & 1) != 0;
    const int32_t ncols = DOWN ? m : f;                         // outputs of this sweep
    const int32_t klo = DOWN ? nd.brow0 : nd.orow0;             // rows summed over: this rank's (all of them unless the node is distributed)
    const int32_t K = DOWN ? nd.brow : nd.orows;
    const int32_t* ix = idx + nd.idx_off;
    const int32_t* ge = gell + nd.ge_off;
    const int tid = threadIdx.x, lane = tid & 63, sl = tid >> 6;
    const int32_t col = min(c0 + lane, ncols - 1);
    // this lane's column: base pointer and row stride inside the packed blocks (rows = the rank's rows, local numbering)
    const MT* Fc;
    int32_t ld;
    if (DOWN) Fc = lfac + nd.lfac_off + (size_t)nd.orows * m + col, ld = m;
    else if (col < m) Fc = lfac + nd.lfac_off + col, ld = m;
    else Fc = ufac + nd.ufac_off + (col - m), ld = b;
    VT acc = scalar_traits<VT>::zero();
    for (int32_t k0 = 0; k0 < K; k0 += kCH) {
        const int32_t kn = min(kCH, K - k0);
        for (int32_t j = tid; j < kn; j += 256) {
            if (DOWN) vs[j] = x[ix[m + klo + k0 + j]];
            else vs[j] = gather_updates(ge, nd.nchild, f, klo + k0 + j, ubuf, rhs[ix[klo + k0 + j]]);
        }
        __syncthreads();
        const MT* Fk = Fc + (size_t)k0 * ld;
        int32_t k = sl;
        for (; k + 12 < kn; k += 16) {
            const MT a0 = Fk[(size_t)k * ld], a1 = Fk[(size_t)(k + 4) * ld], a2 = Fk[(size_t)(k + 8) * ld], a3 = Fk[(size_t)(k + 12) * ld];
            fma_acc(acc, maybe_conj<CONJ>(a0), vs[k]);
            fma_acc(acc, maybe_conj<CONJ>(a1), vs[k + 4]);
            fma_acc(acc, maybe_conj<CONJ>(a2), vs[k + 8]);
            fma_acc(acc, maybe_conj<CONJ>(a3), vs[k + 12]);
        }
        for (; k < kn; k += 4) fma_acc(acc, maybe_conj<CONJ>(Fk[(size_t)k * ld]), vs[k]);
        __syncthreads();
    }
    part[sl][lane] = acc;
    __syncthreads();
    if (sl == 0 && c0 + lane < ncols) {
        const VT z = s_add(s_add(part[0][lane], part[1][lane]), s_add(part[2][lane], part[3][lane]));
        const int32_t r = c0 + lane;
        if (dist) pz[(int64_t)rank * tg_slot + tgoff[blockIdx.x] + r] = z;  // summed over the ranks by nd_distT_finish_kernel
        else if (DOWN) x[ix[r]] = s_add(x[ix[r]], z);
        else if (r < m) x[ix[r]] = z;
        else ubuf[nd.u_off + (r - m)] = s_sub(gather_updates(ge, nd.nchild, f, r, ubuf, scalar_traits<VT>::zero()), z);
    }
}

// transposed sweep, one tree level: workgroup (x = node of the level, y = tile of 64 outputs, z = problem).  Of the per-problem
// pointers only lfac, ufac, rhs, x and ubuf are read; the partial-sum arguments of distributed nodes serve NB = 1 alone.
template <typename MT, typename VT, bool CONJ, bool DOWN, int NB>
__global__ __launch_bounds__(256) void nd_sweepT_kernel(const NdSweepNode* __restrict__ lnodes, const int32_t* __restrict__ idx,
                                                        const int32_t* __restrict__ gell, NdSweepPtrs<NB> p, const int64_t* __restrict__ tgoff,
                                                        VT* __restrict__ pz, int64_t tg_slot, int32_t rank) {
    __shared__ VT vs[kCH];
    __shared__ VT part[4][64];
    const NdSweepNode nd = lnodes[blockIdx.x];
    const int32_t c0 = (int32_t)blockIdx.y * 64;
    if (c0 >= (DOWN ? nd.m : nd.f) || (DOWN && nd.f == nd.m)) return;
    const int z = NB == 1 ? 0 : blockIdx.z;
    nd_sweepT_tile<MT, VT, CONJ, DOWN, NB == 1>(nd, c0, vs, part, (const MT*)p.lfac[z], (const MT*)p.ufac[z], idx, gell, (const VT*)p.rhs[z], (VT*)p.x[z],
                                                (VT*)p.ubuf[z], tgoff, pz, tg_slot, rank);
}

// The distributed nodes of a level after the exchange of their partial sums: z = the ranks' partials added in rank order (the same
// bits on every rank), then what nd_sweepT_kernel does for an ordinary node.  Upwards the node's update vector is written in the
// layout its parent's gather rows expect: entry j in the slot of the rank that owns boundary row j in the forward sweeps.
template <typename VT, bool DOWN>
__global__ __launch_bounds__(256) void nd_distT_finish_kernel(const NdSweepNode* __restrict__ lnodes, const int64_t* __restrict__ tgoff,
                                                              const int32_t* __restrict__ idx, const int32_t* __restrict__ gell,
                                                              const VT* __restrict__ pz, int64_t tg_slot, int32_t nranks, int32_t rank, int64_t ux_slot,
                                                              VT* __restrict__ x, VT* __restrict__ ubuf) {
    const NdSweepNode nd = lnodes[blockIdx.x];
    if (!(nd.flags & 1)) return;
    const int32_t m = nd.m, f = nd.f, b = f - m;
    const int32_t ncols = DOWN ? m : f;
    const int32_t r = (int32_t)blockIdx.y * 256 + threadIdx.x;
    if (r >= ncols || (DOWN && b == 0)) return;
    const int64_t off = tgoff[blockIdx.x] + r;
    VT z = scalar_traits<VT>::zero();
    for (int32_t p = 0; p < nranks; ++p) z = s_add(z, pz[(int64_t)p * tg_slot + off]);
    const int32_t* ix = idx + nd.idx_off;
    if (DOWN) {
        x[ix[r]] = s_add(x[ix[r]], z);
    } else if (r < m) {
        x[ix[r]] = z;
    } else {
        const int32_t j = r - m, w = (b + nranks - 1) / nranks, owner = j / w;
        const VT u = s_sub(gather_updates(gell + nd.ge_off, nd.nchild, f, r, ubuf, scalar_traits<VT>::zero()), z);
        ubuf[nd.u_off + (int64_t)(owner - rank) * ux_slot + (j - owner * w)] = u;
    }
}

// x_z = C_z^-1 b_z for J <= NB factorisations of one analysis: one launch per level and direction for all of them, on the
// tables of f[0].  A solo solve is J = NB = 1.  The collectives of a forest cut over ranks act on f[0] alone: a batch has one
// rank and no distributed node (nd_batch_compatible lets nothing else through the C-ABI).
template <typename MT, typename VT, bool ORDERED, int NB>
int nd_sweep(lsa_ctx* ctx, int32_t J, lsa_ndlu* const* f, const VT* const* b, VT* const* x) {
    hipStream_t st = ctx->stream;
    const lsa_ndlu* f0 = f[0];
    const NdSymbolic& S = f0->S;
    if (J < 1 || J > NB || (J > 1 && (S.nranks > 1 || S.has_dist)))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu: a batch of %d solves needs one rank, no distributed node and at most %d problems", J, NB);
    NdSweepPtrs<NB> p;
    memset(&p, 0, sizeof p);
    for (int32_t z = 0; z < J; ++z) {
        if (f[z]->acc_vbytes != (int)sizeof(VT)) {
            // the slot rows are indexed in units of the vector scalar: after a solve with the other scalar type the entries no
            // child writes no longer read zero
            LSA_HIP_CHECK(ctx, hipMemsetAsync(f[z]->d_acc, 0, (size_t)std::max<int64_t>(f[z]->acc_entries, 1) * 16, st));
            f[z]->acc_vbytes = (int)sizeof(VT);
        }
        p.lfac[z] = f[z]->d_lfac;
        p.ufac[z] = f[z]->d_ufac;
        p.rhs[z] = b[z];
        p.x[z] = x[z];
        p.ubuf[z] = f[z]->d_ubuf;
        p.acc[z] = f[z]->d_acc;
        p.xb[z] = f[z]->d_xb;
        p.top[z] = f[z]->d_top;
    }
    VT* ubuf = (VT*)f0->d_ubuf;
    const bool top = ORDERED && f0->top.s > 0;  // root and children in one launch (nd_top_kernel); their downward launch falls away
    for (size_t li = 0; li <= f0->levels.size(); ++li) {
        // subtree-parallel: the update vectors of all ranks' subtree roots, before the replicated top of the tree
        if ((int32_t)li == S.phase_b_level && S.nranks > 1 && S.xu_slot > 0) LSA_CHECK(k_allgather_inplace(ctx, ubuf, (size_t)S.xu_slot * sizeof(VT)));
        if (li == f0->levels.size()) break;
        const NdLevel& L = f0->levels[li];
        if (top && (int32_t)li + 1 == f0->top_level) continue;  // the root's children: inside the root's launch
        if (top && (int32_t)li == f0->top_level) {
            hipLaunchKernelGGL((nd_top_kernel<MT, VT, NB>), dim3((f0->top.s + 7) / 8, J), dim3(256), 0, st, f0->top, f0->d_top_icmap, f0->d_gell, p);
        } else if (L.fwd_tiles > 0) {
            nd_with_lpr<true>(L.sweep_rows, [&](auto lpr) {
                hipLaunchKernelGGL((nd_fwd_kernel<MT, VT, decltype(lpr)::value, ORDERED, NB>), dim3(L.node_count, L.fwd_tiles, J), dim3(256), 0, st,
                                   f0->d_lnodes + L.node_begin, f0->d_idx, f0->d_gell, f0->d_cmap, p);
            });
        }
        // distributed top nodes of the level: every rank produced its slice of their update entries
        if (L.dist_count > 0 && L.ux_slot > 0) LSA_CHECK(k_allgather_inplace(ctx, ubuf + L.ux_base, (size_t)L.ux_slot * sizeof(VT)));
    }
    for (size_t l = f0->levels.size(); l-- > 0;) {
        const NdLevel& L = f0->levels[l];
        if (L.bwd_tiles > 0 && !(top && (int32_t)l + 1 == f0->top_level)) {
            nd_with_lpr<false>(L.bwd_rows, [&](auto lpr) {
                hipLaunchKernelGGL((nd_bwd_kernel<MT, VT, decltype(lpr)::value, ORDERED, NB>), dim3(L.node_count, L.bwd_tiles, J), dim3(256), 0, st,
                                   f0->d_lnodes_bwd + L.node_begin, f0->d_idx, f0->d_gell, p);
            });
        }
        if (L.dist_count > 0) {
            // ... their own rows: slices -> exchange buffer -> all ranks; then x and the children's boundary vectors
            const int32_t* dn = f0->d_dist_nodes + L.dist_begin;
            VT* xg = (VT*)f0->d_xg;
            if (L.xg_slot > 0) {
                hipLaunchKernelGGL((nd_dist_pack_kernel<VT, ORDERED>), dim3(L.dist_count, (L.dist_rows + 255) / 256), dim3(256), 0, st, dn, f0->d_nodes, f0->d_idx, S.rank,
                                   (const VT*)x[0], xg);
                LSA_CHECK(k_allgather_inplace(ctx, xg + L.xg_base, (size_t)L.xg_slot * sizeof(VT)));
            }
            hipLaunchKernelGGL((nd_dist_unpack_kernel<VT, ORDERED>), dim3(L.dist_count, 1 + L.dist_children, (L.dist_rows + 255) / 256), dim3(256), 0, st, dn, f0->d_nodes,
                               f0->d_child_ptr, f0->d_child_idx, f0->d_cmap, f0->d_idx, S.nranks, x[0], (const VT*)xg, (VT*)f0->d_xb);
        }
    }
    LSA_HIP_CHECK(ctx, hipGetLastError());
    return LSA_OK;
}

// the partial-sum buffer of the transposed sweeps over distributed nodes, built by the first adjoint solve: a level's slot holds
// the f outputs of each of its distributed nodes (the downward sweep's m fit the same places)
int nd_ensure_transposed_dist(lsa_ctx* ctx, lsa_ndlu* f) {
    const NdSymbolic& S = f->S;
    if (!S.has_dist || f->d_tgoff) return LSA_OK;
    std::vector<int64_t> off(S.lvl_nodes.size(), -1);
    f->tg_slot.assign(f->levels.size(), 0);
    f->tg_slot_max = 0;
    for (size_t l = 0; l < f->levels.size(); ++l) {
        const NdLevel& L = f->levels[l];
        int64_t run = 0;
        for (int32_t q = 0; q < L.node_count; ++q) {
            const int32_t t = S.lvl_nodes[(size_t)L.node_begin + q];
            if (S.kind[(size_t)t] != 4) continue;
            off[(size_t)L.node_begin + q] = run;
            run += S.f[(size_t)t];
        }
        f->tg_slot[l] = run;
        f->tg_slot_max = std::max(f->tg_slot_max, run);
    }
    LSA_HIP_ALLOC(ctx, hipMalloc(&f->d_tg, (size_t)std::max<int64_t>(f->tg_slot_max, 1) * (size_t)S.nranks * 16));
    LSA_CHECK(upload(ctx, off, &f->d_tgoff));
    return LSA_OK;
}

// x_z = C_z^-T b_z (CONJ: C_z^-H) for J <= NB factorisations of one analysis, in the shape of nd_sweep: one launch per level and
// direction for all of them, on the tables of f[0].  A solo solve is J = NB = 1; the exchanges over distributed nodes act on f[0]
// alone.  The sweeps have no assembled top: every level is launched in both directions.
template <typename MT, typename VT, bool CONJ, int NB>
int nd_sweepT(lsa_ctx* ctx, int32_t J, lsa_ndlu* const* f, const VT* const* b, VT* const* x) {
    hipStream_t st = ctx->stream;
    lsa_ndlu* f0 = f[0];
    const NdSymbolic& S = f0->S;
    if (J < 1 || J > NB || (J > 1 && (S.nranks > 1 || S.has_dist)))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu: a batch of %d transposed solves needs one rank, no distributed node and at most %d problems", J, NB);
    NdSweepPtrs<NB> p;
    memset(&p, 0, sizeof p);
    for (int32_t z = 0; z < J; ++z) {
        p.lfac[z] = f[z]->d_lfac;
        p.ufac[z] = f[z]->d_ufac;
        p.rhs[z] = b[z];
        p.x[z] = x[z];
        p.ubuf[z] = f[z]->d_ubuf;
    }
    LSA_CHECK(nd_ensure_transposed_dist(ctx, f0));
    VT* pz = (VT*)f0->d_tg;
    VT* x0 = x[0];
    for (size_t li = 0; li <= f0->levels.size(); ++li) {
        if ((int32_t)li == S.phase_b_level && S.nranks > 1 && S.xu_slot > 0) LSA_CHECK(k_allgather_inplace(ctx, f0->d_ubuf, (size_t)S.xu_slot * sizeof(VT)));
        if (li == f0->levels.size()) break;
        const NdLevel& L = f0->levels[li];
        const int64_t slot = L.dist_count > 0 ? f0->tg_slot[li] : 0;
        if (L.fwd_tiles > 0)
            hipLaunchKernelGGL((nd_sweepT_kernel<MT, VT, CONJ, false, NB>), dim3(L.node_count, (L.max_f + 63) / 64, J), dim3(256), 0, st,
                               f0->d_lnodes + L.node_begin, f0->d_idx, f0->d_gell, p, f0->d_tgoff ? f0->d_tgoff + L.node_begin : nullptr, pz, slot, S.rank);
        if (L.dist_count > 0) {
            // the distributed nodes of the level: every rank summed over its rows; partials to all, added in rank order
            LSA_CHECK(k_allgather_inplace(ctx, pz, (size_t)slot * sizeof(VT)));
            hipLaunchKernelGGL((nd_distT_finish_kernel<VT, false>), dim3(L.node_count, (L.max_f + 255) / 256), dim3(256), 0, st, f0->d_lnodes + L.node_begin,
                               f0->d_tgoff + L.node_begin, f0->d_idx, f0->d_gell, (const VT*)pz, slot, S.nranks, S.rank, L.ux_slot, x0, (VT*)f0->d_ubuf);
        }
    }
    for (size_t l = f0->levels.size(); l-- > 0;) {
        const NdLevel& L = f0->levels[l];
        const int64_t slot = L.dist_count > 0 ? f0->tg_slot[l] : 0;
        if (L.bwd_tiles > 0 || L.dist_count > 0)
            hipLaunchKernelGGL((nd_sweepT_kernel<MT, VT, CONJ, true, NB>), dim3(L.node_count, (L.max_m + 63) / 64, J), dim3(256), 0, st,
                               f0->d_lnodes + L.node_begin, f0->d_idx, f0->d_gell, p, f0->d_tgoff ? f0->d_tgoff + L.node_begin : nullptr, pz, slot, S.rank);
        if (L.dist_count > 0) {
            LSA_CHECK(k_allgather_inplace(ctx, pz, (size_t)slot * sizeof(VT)));
            hipLaunchKernelGGL((nd_distT_finish_kernel<VT, true>), dim3(L.node_count, (L.max_m + 255) / 256), dim3(256), 0, st, f0->d_lnodes + L.node_begin,
                               f0->d_tgoff + L.node_begin, f0->d_idx, f0->d_gell, (const VT*)pz, slot, S.nranks, S.rank, L.ux_slot, x0, (VT*)f0->d_ubuf);
        }
    }
    LSA_HIP_CHECK(ctx, hipGetLastError());
    return LSA_OK;
}

// x_z = C_z^-1 b_z (trans 1: C_z^-T, 2: C_z^-H) for J problems on the sweeps of capacity NB, after an aliased right-hand side of
// each of them went to the problem's own buffer (bd: J pointers, updated)
template <int NB>
int nd_solve(lsa_ctx* ctx, const char* who, int32_t J, lsa_ndlu* const* f, int trans, int vdtype, const void** bd, void* const* x) {
    return nd_dispatch_solve(ctx, who, false, J, f, trans, vdtype, [&](auto mt, auto vt, auto dir) {
        using MT = decltype(mt);
        using VT = decltype(vt);
        constexpr int DIR = decltype(dir)::value;
        for (int32_t z = 0; z < J; ++z)
            if (bd[z] == x[z]) {
                LSA_HIP_CHECK(ctx, hipMemcpyAsync(f[z]->d_tmp, bd[z], (size_t)f[z]->S.n * sizeof(VT), hipMemcpyDeviceToDevice, ctx->stream));
                bd[z] = f[z]->d_tmp;
            }
        if constexpr (DIR != 0) return nd_sweepT<MT, VT, DIR == 2, NB>(ctx, J, f, (const VT* const*)bd, (VT* const*)x);
        else
            return f[0]->ordered ? nd_sweep<MT, VT, true, NB>(ctx, J, f, (const VT* const*)bd, (VT* const*)x)
                                 : nd_sweep<MT, VT, false, NB>(ctx, J, f, (const VT* const*)bd, (VT* const*)x);
    });
}

}  // namespace

// g can run in a batch with f: one rank, no distributed nodes, and the same analysis (pattern, constraints, forest or leaf size,
// memory plan, sweep levels), so that f's tables address g's factors and buffers as g's own do
bool nd_batch_compatible(const lsa_ndlu* f, const lsa_ndlu* g) {
    const NdSymbolic &A = f->S, &B = g->S;
    if (A.nranks != 1 || B.nranks != 1 || A.has_dist || B.has_dist) return false;
    if (f->dtype != g->dtype || f->ordered != g->ordered || A.n != B.n || A.nnz != B.nnz || A.pattern_hash != B.pattern_hash ||
        A.constraint_hash != B.constraint_hash || A.tree_hash != B.tree_hash || A.leaf_size != B.leaf_size)
        return false;
    if (f->lfac_entries != g->lfac_entries || f->ufac_entries != g->ufac_entries || f->acc_entries != g->acc_entries || f->h_lfac_off != g->h_lfac_off ||
        f->h_upd_off != g->h_upd_off || A.lvl_nodes != B.lvl_nodes || f->levels.size() != g->levels.size())
        return false;
    for (size_t l = 0; l < f->levels.size(); ++l) {
        const NdLevel &a = f->levels[l], &c = g->levels[l];
        if (a.node_begin != c.node_begin || a.node_count != c.node_count || a.fwd_tiles != c.fwd_tiles || a.bwd_tiles != c.bwd_tiles ||
            a.sweep_rows != c.sweep_rows || a.bwd_rows != c.bwd_rows || a.dist_count != 0 || c.dist_count != 0)
            return false;
    }
    if (f->top.s != g->top.s || f->top_level != g->top_level) return false;
    return true;
}

// x = C^-1 b on device pointers (b and x distinct or identical: an aliased right-hand side is copied first)
int ndlu_solve_dev(lsa_ctx* ctx, lsa_ndlu* f, int vdtype, const void* b, void* x) { return nd_solve<1>(ctx, "lsa_ndlu_solve", 1, &f, 0, vdtype, &b, &x); }

// x = C^-T b (conj == 0) or C^-H b (conj != 0) on the factors of C
int ndlu_solve_adjoint_dev(lsa_ctx* ctx, lsa_ndlu* f, int conj, int vdtype, const void* b, void* x) {
    return nd_solve<1>(ctx, "lsa_ndlu_solve_adjoint", 1, &f, conj ? 2 : 1, vdtype, &b, &x);
}

// one column of a request (ndlu_solve_run, ndlu_multi.hip): b[z] -> x[z] on the sweeps of its capacity and direction.  The sweeps
// work on a copy of the pointers, where an aliased right-hand side is replaced by the problem's own copy of it.
int ndlu_solve_column(lsa_ctx* ctx, const NdSolve& rq, const void* const* b, void* const* x) {
    const void* bd[kNdBatchMax];
    std::copy(b, b + rq.J, bd);  // (ndlu_solve_run checked J)
    return rq.sets ? nd_solve<kNdBatchMax>(ctx, rq.who, rq.J, rq.f, rq.trans, rq.vdtype, bd, x) : nd_solve<1>(ctx, rq.who, 1, rq.f, rq.trans, rq.vdtype, bd, x);
}
