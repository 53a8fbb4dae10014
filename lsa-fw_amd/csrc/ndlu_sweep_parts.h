// Nested-dissection multifrontal LU, the solves: the device pieces every sweep kernel is built from -- the sub-wave sum, the row-pair
// dot product and its prefetch, the gathers and pushes between a node and its children, the stores of the merged top -- and the
// choice of a level's tile form.  Shared by ndlu_sweeps.hip (one vector per factor set) and ndlu_multi.hip (R vectors on one).
#pragma once
#include "ndlu_internal.h"

namespace {

// sum over LPR consecutive lanes (4, 16 or 64), returned to every one of them.  DPP moves inside a row of 16 lanes (two 32-bit
// halves per double), the four row sums of a wavefront through SGPRs: a ds_bpermute butterfly is a chain of ~100-cycle steps,
// and the sweeps are chains of short kernels that end in exactly this reduction.  Fixed order: bitwise repeatable.
template <int CTRL>
__device__ __forceinline__ double dpp_mov_f64(double v) {
    const long long bits = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)((unsigned long long)bits & 0xFFFFFFFFull), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)((unsigned long long)bits >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
template <int LPR>
__device__ __forceinline__ double lanes_sum(double v) {
    static_assert(LPR == 4 || LPR == 16 || LPR == 64, "sub-wave width");
    v += dpp_mov_f64<0xB1>(v);  // quad_perm [1,0,3,2]
    v += dpp_mov_f64<0x4E>(v);  // quad_perm [2,3,0,1]: every lane of a quad holds the quad's sum
    if constexpr (LPR >= 16) {
        v += dpp_mov_f64<0x141>(v);  // row_half_mirror
        v += dpp_mov_f64<0x140>(v);  // row_mirror: every lane of a row of 16 holds the row's sum
    }
    if constexpr (LPR == 64) {
        const long long bits = __double_as_longlong(v);
        const int lo = (int)(unsigned)((unsigned long long)bits & 0xFFFFFFFFull), hi = (int)(unsigned)((unsigned long long)bits >> 32);
        double tot = 0.0;
#pragma unroll
        for (int row = 0; row < 4; ++row) {
            const unsigned l = (unsigned)__builtin_amdgcn_readlane(lo, 16 * row), h = (unsigned)__builtin_amdgcn_readlane(hi, 16 * row);
            tot += __longlong_as_double((long long)(((unsigned long long)h << 32) | l));
        }
        v = tot;
    }
    return v;
}
template <int LPR>
__device__ __forceinline__ cplx lanes_sum(cplx v) {
    return cplx{lanes_sum<LPR>(v.re), lanes_sum<LPR>(v.im)};
}

// acc0 += Fa[0:cn] . vs, acc1 += Fb[0:cn] . vs over the LPR lanes of a sub-wave; eight row loads in flight per lane (the
// sweeps are chains of short kernels: what they wait for is memory latency, not bandwidth)
template <int LPR = 16, typename MT, typename VT>
__device__ __forceinline__ void two_row_dot(const MT* __restrict__ Fa, const MT* __restrict__ Fb, const VT* vs, int32_t cn, int sl, VT& acc0,
                                            VT& acc1) {
    int32_t k = sl;
    for (; k + 3 * LPR < cn; k += 4 * LPR) {
        const MT a0 = Fa[k], a1 = Fa[k + LPR], a2 = Fa[k + 2 * LPR], a3 = Fa[k + 3 * LPR];
        const MT b0 = Fb[k], b1 = Fb[k + LPR], b2 = Fb[k + 2 * LPR], b3 = Fb[k + 3 * LPR];
        fma_acc(acc0, a0, vs[k]);
        fma_acc(acc1, b0, vs[k]);
        fma_acc(acc0, a1, vs[k + LPR]);
        fma_acc(acc1, b1, vs[k + LPR]);
        fma_acc(acc0, a2, vs[k + 2 * LPR]);
        fma_acc(acc1, b2, vs[k + 2 * LPR]);
        fma_acc(acc0, a3, vs[k + 3 * LPR]);
        fma_acc(acc1, b3, vs[k + 3 * LPR]);
    }
    for (; k < cn; k += LPR) {
        const MT a0 = Fa[k], b0 = Fb[k];
        fma_acc(acc0, a0, vs[k]);
        fma_acc(acc1, b0, vs[k]);
    }
}

// the first 4 * LPR columns of a row pair, loaded before the vector they multiply is ready (they depend on the node record only)
template <int LPR, typename MT>
__device__ __forceinline__ void row_pair_prefetch(const MT* __restrict__ Fa, const MT* __restrict__ Fb, int32_t cn, int sl, MT (&pa)[4], MT (&pb)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int32_t k = sl + q * LPR;
        pa[q] = k < cn ? Fa[k] : scalar_traits<MT>::zero();
        pb[q] = k < cn ? Fb[k] : scalar_traits<MT>::zero();
    }
}

template <int LPR, typename MT, typename VT>
__device__ __forceinline__ void two_row_dot_prefetched(const MT* __restrict__ Fa, const MT* __restrict__ Fb, const VT* vs, int32_t cn, int sl, VT& acc0,
                                                       VT& acc1, const MT (&pa)[4], const MT (&pb)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int32_t k = sl + q * LPR;
        if (k < cn) {
            fma_acc(acc0, pa[q], vs[k]);
            fma_acc(acc1, pb[q], vs[k]);
        }
    }
    if (cn > 4 * LPR) two_row_dot<LPR>(Fa + 4 * LPR, Fb + 4 * LPR, vs + 4 * LPR, cn - 4 * LPR, sl, acc0, acc1);
}

// PULL form: sum of the children's update-vector entries that land on front position j, through the per-child gather rows
// (fixed order: child rank).  Used where a child's vector arrives by all-gather (the replicated top of a forest cut over ranks)
// and by the transposed sweeps.
template <typename VT>
__device__ __forceinline__ VT gather_updates(const int32_t* __restrict__ ge, int32_t nchild, int32_t f, int32_t j, const VT* __restrict__ ubuf,
                                             VT v) {
    int32_t c = 0;
    for (; c + 3 < nchild; c += 4) {
        const int32_t g0 = ge[(size_t)c * f + j], g1 = ge[(size_t)(c + 1) * f + j], g2 = ge[(size_t)(c + 2) * f + j], g3 = ge[(size_t)(c + 3) * f + j];
        const VT u0 = g0 >= 0 ? ubuf[g0] : scalar_traits<VT>::zero(), u1 = g1 >= 0 ? ubuf[g1] : scalar_traits<VT>::zero();
        const VT u2 = g2 >= 0 ? ubuf[g2] : scalar_traits<VT>::zero(), u3 = g3 >= 0 ? ubuf[g3] : scalar_traits<VT>::zero();
        v = s_add(s_add(s_add(s_add(v, u0), u1), u2), u3);
    }
    int32_t g[3] = {-1, -1, -1};
    for (int q = 0; q < 3; ++q)
        if (c + q < nchild) g[q] = ge[(size_t)(c + q) * f + j];
    VT u[3];
    for (int q = 0; q < 3; ++q) u[q] = g[q] >= 0 ? ubuf[g[q]] : scalar_traits<VT>::zero();
    for (int q = 0; q < 3; ++q)
        if (c + q < nchild) v = s_add(v, u[q]);
    return v;
}

// PUSH form: the same sum from the node's slot rows (row c = what child c added to every front position; slots no child maps
// to were zeroed once and are never written): contiguous loads, no index in between.  Same order of additions as the pull form.
template <typename VT>
__device__ __forceinline__ VT slot_sum(const VT* __restrict__ slots, int32_t nchild, int32_t f, int32_t j, VT v) {
    int32_t c = 0;
    for (; c + 3 < nchild; c += 4) {
        const VT u0 = slots[(size_t)c * f + j], u1 = slots[(size_t)(c + 1) * f + j], u2 = slots[(size_t)(c + 2) * f + j],
                 u3 = slots[(size_t)(c + 3) * f + j];
        v = s_add(s_add(s_add(s_add(v, u0), u1), u2), u3);
    }
    VT u[3];
    for (int q = 0; q < 3; ++q) u[q] = c + q < nchild ? slots[(size_t)(c + q) * f + j] : scalar_traits<VT>::zero();
    for (int q = 0; q < 3; ++q)
        if (c + q < nchild) v = s_add(v, u[q]);
    return v;
}

// a factor scalar as the transposed sweeps use it: conjugated for C^-H on complex factors
template <bool CONJ, typename MT>
__device__ __forceinline__ MT maybe_conj(MT a) {
    if constexpr (CONJ) return s_conj(a);
    else return a;
}

// downward sweep: the value of front position j goes into the boundary vector of every child that has j in its boundary
template <typename VT>
__device__ __forceinline__ void push_down(const int32_t* __restrict__ ge, int32_t nchild, int32_t f, int32_t j, VT* __restrict__ xb, VT val) {
    for (int32_t c = 0; c < nchild; ++c) {
        const int32_t g = ge[(size_t)c * f + j];
        if (g >= 0) xb[g] = val;
    }
}

// push_down with the gather rows' entries of up to four children asked for beforehand (HAVE: g[c] = child c's entry, -1 = none)
template <bool HAVE, typename VT>
__device__ __forceinline__ void push_down_at(const int32_t* __restrict__ ge, int32_t nchild, int32_t f, int32_t j, const int32_t (&g)[4],
                                             VT* __restrict__ xb, VT val) {
    if (HAVE && nchild <= 4) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (g[c] >= 0) xb[g[c]] = val;
    } else {
        push_down(ge, nchild, f, j, xb, val);
    }
}

// ---- the merged top (NdTop, ndlu_internal.h): the root and its children in one launch
// the output of top row i (final: no downward step follows): into x, and to the boundary vectors of the grandchildren -- a row
// of child c through c's gather rows at its own position; a row of the root, for every child c that has it at boundary
// position p, through c's gather rows at m_c + p (what nd_bwd_tile hands on for a child of the root)
template <typename VT>
__device__ __forceinline__ void nd_top_store(const NdTop& tp, int32_t i, VT val, const int32_t* __restrict__ icmap, const int32_t* __restrict__ gell,
                                             VT* __restrict__ x, VT* __restrict__ xb) {
    const int32_t K = tp.nchild;
    const NdTopNode& R = tp.node[K];
    if (i >= R.off) {
        const int32_t k = i - R.off;
        x[R.own0 + k] = val;
        for (int32_t c = 0; c < K; ++c) {
            const NdTopNode& nd = tp.node[c];
            const int32_t p = icmap[(size_t)c * R.m + k];
            if (p >= 0) push_down(gell + nd.ge_off, nd.nchild, nd.f, nd.m + p, xb, val);
        }
        return;
    }
    for (int32_t c = 0; c < K; ++c) {
        const NdTopNode& nd = tp.node[c];
        if (i < nd.off || i >= nd.off + nd.m) continue;
        x[nd.own0 + i - nd.off] = val;
        push_down(gell + nd.ge_off, nd.nchild, nd.f, i - nd.off, xb, val);
    }
}

// Where nd_top_store sends the output of top row i, asked for before the row is swept (it depends on the tables alone): the
// row's place in x and its entries of the grandchildren's boundary vectors -- g[q] = -1: none.  They fit for a row of a child
// with at most eight children, and for a row of the root under at most two children of at most four children each; fits = false
// otherwise (nd_top_store then finds them after the reduction).
struct NdTopTargets {
    int32_t own;
    bool fits;
    int32_t g[8];
};

__device__ __forceinline__ void nd_top_targets(const NdTop& tp, int32_t i, const int32_t* __restrict__ icmap, const int32_t* __restrict__ gell,
                                               NdTopTargets& t) {
    const int32_t K = tp.nchild;
    const NdTopNode& R = tp.node[K];
    t.own = 0, t.fits = false;
#pragma unroll
    for (int q = 0; q < 8; ++q) t.g[q] = -1;
    if (i >= R.off) {
        const int32_t k = i - R.off;
        t.own = R.own0 + k;
        t.fits = K <= 2;
        if (!t.fits) return;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (c >= K) break;
            const NdTopNode& nd = tp.node[c];
            if (nd.nchild > 4) t.fits = false;
            const int32_t p = icmap[(size_t)c * R.m + k];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc)
                if (p >= 0 && cc < nd.nchild) t.g[4 * c + cc] = gell[nd.ge_off + (size_t)cc * nd.f + nd.m + p];
        }
        return;
    }
    for (int32_t c = 0; c < K; ++c) {
        const NdTopNode& nd = tp.node[c];
        if (i < nd.off || i >= nd.off + nd.m) continue;
        t.own = nd.own0 + i - nd.off;
        t.fits = nd.nchild <= 8;
#pragma unroll
        for (int cc = 0; cc < 8; ++cc)
            if (t.fits && cc < nd.nchild) t.g[cc] = gell[nd.ge_off + (size_t)cc * nd.f + i - nd.off];
    }
}

template <typename VT>
__device__ __forceinline__ void nd_top_store(const NdTop& tp, int32_t i, VT val, const NdTopTargets& t, const int32_t* __restrict__ icmap,
                                             const int32_t* __restrict__ gell, VT* __restrict__ x, VT* __restrict__ xb) {
    if (!t.fits) return nd_top_store(tp, i, val, icmap, gell, x, xb);
    x[t.own] = val;
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (t.g[q] >= 0) xb[t.g[q]] = val;
}

// The tile form of a level's launch from NdLevel::sweep_rows (upwards) or bwd_rows (downwards): LPR lanes per row pair, 512 / LPR
// rows per tile.  8 rows -> 64 lanes; 128 -> 4, upwards only (THIN: the downward sweep of a thin level has few, long rows and
// stays with 32-row tiles, as nd_setup_levels counted them); else 32 rows -> 16.
template <bool THIN, typename F>
void nd_with_lpr(int32_t sweep_rows, F&& launch) {
    if (sweep_rows == 8) return launch(std::integral_constant<int, 64>{});
    if constexpr (THIN)
        if (sweep_rows == 128) return launch(std::integral_constant<int, 4>{});
    launch(std::integral_constant<int, 16>{});
}

// The one place that picks a solve's instance, single columns and blocks alike: fn(factor scalar, vector scalar, direction) for the
// factor dtype, the vector dtype and trans (0 N, 1 T, 2 H) of a solve on J factorisations, behind the argument checks.  The direction
// is std::integral_constant<int, 0 | 1 | 2>; real factors never get 2 (C^H = C^T, one instance).  `block`: the multi-column sweeps,
// which have no form for a forest cut over ranks.  `who` names the entry in the message.
template <typename F>
int nd_dispatch_solve(lsa_ctx* ctx, const char* who, bool block, int32_t J, lsa_ndlu* const* f, int trans, int vdtype, F&& fn) {
    using N = std::integral_constant<int, 0>;
    using T = std::integral_constant<int, 1>;
    using H = std::integral_constant<int, 2>;
    for (int32_t z = 0; block && z < J; ++z)
        if (f[z]->S.nranks > 1 || f[z]->S.has_dist) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: the multi-column sweeps need one rank and no distributed node", who);
    if (f[0]->dtype == LSA_C128 && vdtype != LSA_C128) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: complex factors need complex vectors", who);
    if (f[0]->S.n == 0) return LSA_OK;
    if (f[0]->dtype == LSA_C128) return trans == 0 ? fn(cplx{}, cplx{}, N{}) : trans == 2 ? fn(cplx{}, cplx{}, H{}) : fn(cplx{}, cplx{}, T{});
    if (vdtype == LSA_C128) return trans == 0 ? fn(double{}, cplx{}, N{}) : fn(double{}, cplx{}, T{});
    return trans == 0 ? fn(double{}, double{}, N{}) : fn(double{}, double{}, T{});
}

}  // namespace
