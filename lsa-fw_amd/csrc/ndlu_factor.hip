// Nested-dissection multifrontal LU, the numeric factorisation: assembly and extend-add of the fronts, blocked Gauss-Jordan
// inversion of the pivot blocks (panel launches, or tournament pivoting for tall blocks), the packed factors by MFMA products,
// and the assembly of the merged top of the sweeps.  Layout and pivoting: ndlu.hip; records and tables: ndlu_internal.h.
#include "ndlu_internal.h"

#include <utility>

// every kernel launch of the numeric factorisation, counted on the host (lsa_ndlu_info: factor_launches)
#define ND_LAUNCH(f, ...)                   \
    do {                                    \
        ++(f)->factor_launches;             \
        hipLaunchKernelGGL(__VA_ARGS__);    \
    } while (0)

namespace {

template <typename T>
__global__ __launch_bounds__(256) void nd_maxabs2_kernel(int64_t nnz, const T* __restrict__ v, unsigned long long* __restrict__ out) {
    // one atomic per workgroup (an atomic per wavefront on one address serialised: 165 us for 0.9 M entries)
    __shared__ double wmax[4];
    double best = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += stride) {
        const double a = s_abs2(v[i]);
        if (a == a && a > best) best = a;
        else if (a != a) best = a;  // a NaN must reach the host (NaN > x is false: keep it by hand)
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(best, o);
        best = (best != best) ? best : (other != other) ? other : fmax(best, other);
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) best = (best != best) ? best : (wmax[w] != wmax[w]) ? wmax[w] : fmax(best, wmax[w]);
        // non-negative doubles order like their bit patterns; a NaN's pattern (0x7ff8...) is above every finite value's and infinity's
        atomicMax(out, (unsigned long long)__double_as_longlong(best));
    }
}

// test aid (LSA_ND_TEST_PERTURB): every stored factor scalar times (1 + eps), so that a solve is wrong by about eps and the
// operator layer's iterative refinement has something to do (tests/test_gpu_3d.py)
template <typename T>
__global__ void nd_scale_kernel(int64_t count, T* __restrict__ v, double factor) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) v[i] = s_mul(factor, v[i]);
}

template <typename T>
__global__ void nd_assemble_kernel(int64_t count, const T* __restrict__ val, const int32_t* __restrict__ src, const int64_t* __restrict__ dst,
                                   T* __restrict__ front) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += stride) front[dst[e]] = val[src[e]];
}

// parent front += child's update matrix (tile = 16 rows of the child's b x b update matrix in the update arena)
template <typename T>
__global__ __launch_bounds__(256) void nd_extend_add_kernel(const int32_t* __restrict__ tiles, const NdNodeDev* __restrict__ nodes,
                                                            const int32_t* __restrict__ cmap, T* __restrict__ front, const T* __restrict__ upd) {
    const int32_t c = tiles[2 * blockIdx.x], i0 = tiles[2 * blockIdx.x + 1];
    const NdNodeDev nc = nodes[c];
    const NdNodeDev np = nodes[nc.parent];
    const int32_t b = nc.f - nc.m;
    const int32_t* map = cmap + nc.cmap_off;
    const int32_t i = i0 + (threadIdx.x >> 4);
    if (i >= b) return;
    const T* src = upd + nc.upd_off + (int64_t)i * b;
    int32_t pr = map[i];
    if (pr >= np.m) {  // a boundary row of the parent: a distributed parent keeps only its own slice of them
        pr -= np.brow0;
        if (pr < np.m || pr >= np.m + np.brow) return;
    }
    T* dst = front + np.front_off + (int64_t)pr * np.f;
    for (int32_t j = threadIdx.x & 15; j < b; j += 16) {
        T* d = dst + map[j];
        *d = s_add(*d, src[j]);
    }
}

// the same for rows [row0, row0 + nrows) of child c's update matrix that arrived in the staging buffer (`src`: nrows x b,
// row-major): a distributed parent receives its children's update matrices in row chunks, one rank's chunk per launch (the
// chunks of one step may belong to different children of one parent: launches in slot order keep the sums in a fixed order)
template <typename T>
__global__ __launch_bounds__(256) void nd_extend_add_staged_kernel(const NdNodeDev* __restrict__ nodes, const int32_t* __restrict__ cmap, T* __restrict__ front,
                                                                   const T* __restrict__ src, int32_t c, int32_t row0, int32_t nrows) {
    const NdNodeDev nc = nodes[c];
    const NdNodeDev np = nodes[nc.parent];
    const int32_t b = nc.f - nc.m;
    const int32_t* map = cmap + nc.cmap_off;
    const int32_t k = (int32_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (k >= nrows) return;
    int32_t pr = map[row0 + k];
    if (pr >= np.m) {
        pr -= np.brow0;
        if (pr < np.m || pr >= np.m + np.brow) return;
    }
    const T* s = src + (int64_t)k * b;
    T* dst = front + np.front_off + (int64_t)pr * np.f;
    for (int32_t j = threadIdx.x & 15; j < b; j += 16) {
        T* d = dst + map[j];
        *d = s_add(*d, s[j]);
    }
}

// max of a 64-bit key over the wavefront, returned to every lane: DPP steps inside each row of 16 lanes (a ds_bpermute
// butterfly costs ~100 cycles per step, and the pivot searches are chains of them), then the four row maxima through SGPRs
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_mov_key(unsigned long long v) {
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(v & 0xFFFFFFFFull), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, false);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long v) {
    unsigned long long o;
    o = dpp_mov_key<0xB1>(v);  // quad_perm [1,0,3,2]
    v = o > v ? o : v;
    o = dpp_mov_key<0x4E>(v);  // quad_perm [2,3,0,1]
    v = o > v ? o : v;
    o = dpp_mov_key<0x141>(v);  // row_half_mirror
    v = o > v ? o : v;
    o = dpp_mov_key<0x140>(v);  // row_mirror: every lane of a row now holds the row's max
    v = o > v ? o : v;
    unsigned long long best = 0ull;
#pragma unroll
    for (int row = 0; row < 4; ++row) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xFFFFFFFFull), 16 * row);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 16 * row);
        const unsigned long long r = ((unsigned long long)hi << 32) | lo;
        best = r > best ? r : best;
    }
    return best;
}

__device__ __forceinline__ unsigned long long pivot_key(double mag2, int32_t row) {
    // |a|^2 with its low 16 mantissa bits replaced by (65535 - row): one unsigned max picks the largest magnitude and,
    // among magnitudes equal to 2^-36 relative, the lowest row (deterministic)
    return ((unsigned long long)__double_as_longlong(mag2) & ~0xFFFFull) | (unsigned long long)(65535 - row);
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop that cannot stay rolled.  The pivots of a panel index a
// thread's registers, and `#pragma unroll` gave up on that loop at 16 pivots (the row went to scratch memory).
template <typename F, int... J>
__device__ __forceinline__ void static_for_seq(F&& f, std::integer_sequence<int, J...>) {
    (f(std::integral_constant<int, J>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_seq(f, std::make_integer_sequence<int, N>{});
}

// ---- blocked Gauss-Jordan inversion of the pivot blocks of a level ---------------------------------------------------------
// Columns are eliminated in blocks of kNB; inside a block in panels of W columns (W = 8 for pivot blocks of up to 2048 rows,
// narrower for taller ones so that a thread's rows of the panel stay in registers).  Rows are never interchanged: a row
// that has served as a pivot is excluded from later searches (rowq), the permutation is undone by nd_unperm_kernel.
// ONE launch per panel (nd_gj_fused_kernel), grid (node, 1 + kNB / 16):
//   workgroup y = 0   thread per row (RPT rows per thread): first brings the panel's W columns up to date with the rank-W
//                     update of the PREVIOUS panel of the block, then eliminates them;
//   workgroups y >= 1 apply that previous panel's rank-W update to a tile of 16 of the block's other columns, all rows:
//                     A[i, c] = (i was a pivot row of the previous panel ? 0 : A[i, c]) + W_prev[i, :] Y_prev[:, c],  Y_prev =
//                     the previous panel's pivot rows in these columns, read before the tile is touched.
// A workgroup owns its columns for all rows, and the columns of the previous panel are read-only in the launch: no staging
// buffer, no second launch per panel (round 2: panel launch + block-update launch, 2 x 157 launches of ~12 us in the
// factorisation of the 30 k-unknown case).  After the block's last panel one launch of the tiles alone finishes the block;
// then the pivot rows' values in all other columns are staged (nd_gj_stage_kernel) and one rank-kNB product
//                   A[:, J] = (pivot row ? 0 : A[:, J]) + Wb Yb  updates the rest (nd_gj_gemm_kernel, 64 x 64 tiles):
// the columns outside a block are touched once per kNB pivots instead of once per 8 (the update of a 6 000-row pivot block
// streamed 1.1 GB per 8 pivots, and its panel did not fit the registers of one workgroup at W = 8).

// The finishing launch carries the staging in further workgroups (y >= ystage) unless LSA_ND_GJ_PANEL=8 asks for the separate
// launch: staging reads the columns outside the block, the tiles write columns inside it, and ipiv is complete when the
// last panel has ended.  Blocks of one panel have no finishing launch and keep the separate staging launch.
// Panels of 16 columns (LSA_ND_GJ_PANEL=16, where a thread holds one row): a block is two panels, the second panel's launch
// has no tiles (no block column lies outside both panels), and the finishing launch is the second panel's rank-16 update of
// the first panel's columns.  Measured slower than panels of 8 (nd_numeric), hence not the default.

// Yb[j][c] = A[pivot row of column kb + j][c], j < kw, for column c < c_hi of one node (nd_gj_stage_kernel; the
// staging workgroups of a finishing launch);  ycap = rows of staging space per unknown
template <typename T>
__device__ __forceinline__ void gj_stage_column(const NdNodeDev& nd, const T* front, const int32_t* ipiv, int32_t kb, int32_t kw, int32_t ycap,
                                                int32_t c, int32_t c_hi, T* ybuf) {
    const int32_t m = nd.m, ld = nd.f;
    const int32_t nb = min(kw, m - kb);
    if (nb <= 0 || m <= kNB || c >= min(m, c_hi)) return;
    const T* a = front + nd.front_off;
    T* yb = ybuf + (size_t)ycap * nd.piv_off;
    const int32_t* pv = ipiv + nd.piv_off + kb;
    int32_t j = 0;
    for (; j + 4 <= nb; j += 4) {  // (independent loads, issued together)
        const T v0 = a[(size_t)pv[j] * ld + c], v1 = a[(size_t)pv[j + 1] * ld + c], v2 = a[(size_t)pv[j + 2] * ld + c], v3 = a[(size_t)pv[j + 3] * ld + c];
        yb[(size_t)j * m + c] = v0;
        yb[(size_t)(j + 1) * m + c] = v1;
        yb[(size_t)(j + 2) * m + c] = v2;
        yb[(size_t)(j + 3) * m + c] = v3;
    }
    for (; j < nb; ++j) yb[(size_t)j * m + c] = a[(size_t)pv[j] * ld + c];
}

// k0 < 0: no panel in this launch (the tiles finish the block);  kprev < 0: no previous panel to apply;
// ystage > 0: workgroups y >= ystage stage the block's pivot rows in the columns [0, c_hi) into ybuf, NT columns each
template <typename T, int NT, int RPT, int W>
__global__ __launch_bounds__(NT) void nd_gj_fused_kernel(const int32_t* __restrict__ lvl_nodes, const NdNodeDev* __restrict__ nodes,
                                                         T* __restrict__ front, int32_t* __restrict__ ipiv, int32_t* __restrict__ rowq,
                                                         int32_t kb, int32_t k0, int32_t kprev, int32_t* __restrict__ flag, double tiny2,
                                                         int32_t ystage, T* __restrict__ ybuf, int32_t c_hi) {
    __shared__ unsigned long long skey[W];
    __shared__ T prow_s[2][W];
    __shared__ int32_t prows[W];
    __shared__ T yprev[W][16];
    __shared__ int32_t pprev[W];
    const int32_t t = lvl_nodes[blockIdx.x];
    const NdNodeDev nd = nodes[t];
    const int32_t m = nd.m, ld = nd.f;
    T* a = front + nd.front_off;
    const int tid = threadIdx.x, lane = tid & 63;
    if (ystage > 0 && (int32_t)blockIdx.y >= ystage) {
        gj_stage_column<T>(nd, front, ipiv, kb, kNB, kNB, ((int32_t)blockIdx.y - ystage) * NT + tid, c_hi, ybuf);
        return;
    }
    const int32_t wp = kprev >= 0 ? min(W, m - kprev) : 0;  // columns of the previous panel in this node
    if (blockIdx.y > 0) {
        // ---- tile of 16 block columns: the previous panel's rank-W update, all rows ----
        if (wp <= 0) return;
        const int32_t cb = ((int32_t)blockIdx.y - 1) * 16 + (tid & 15);
        const int32_t c = kb + cb;
        const bool mine = cb < kNB && c < m && !(c >= kprev && c < kprev + wp) && !(k0 >= 0 && c >= k0 && c < k0 + W);
        if (tid < W) pprev[tid] = tid < wp ? ipiv[nd.piv_off + kprev + tid] : -1;
        __syncthreads();
        for (int e = tid; e < 16 * W; e += NT) {  // (the column of entry e is that of thread e & 15 = tid & 15: NT is a multiple of 16)
            const int j = e >> 4;
            yprev[j][e & 15] = (mine && j < wp) ? a[(size_t)pprev[j] * ld + c] : scalar_traits<T>::zero();
        }
        __syncthreads();
        if (!mine) return;
        T y[W];
#pragma unroll
        for (int j = 0; j < W; ++j) y[j] = yprev[j][tid & 15];
        // four rows per trip, their loads issued together (a trip is a chain of dependent loads; with 64 threads a tile of a
        // 64-row pivot block would otherwise walk 16 of them one after the other)
        // (two rows at W = 16: the same number of multipliers in registers)
        constexpr int RL = NT / 16, U = W > 8 ? 2 : 4;
        for (int32_t i0 = tid >> 4; i0 < m; i0 += U * RL) {
            T cur[U], mult[U][W];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int32_t i = i0 + u * RL;
                const T* ai = a + (size_t)min(i, m - 1) * ld;
                cur[u] = ai[c];
#pragma unroll
                for (int j = 0; j < W; ++j) mult[u][j] = j < wp ? ai[kprev + j] : scalar_traits<T>::zero();
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int32_t i = i0 + u * RL;
                if (i >= m) break;
                bool is_piv = false;
#pragma unroll
                for (int j = 0; j < W; ++j) is_piv |= (i == pprev[j]);
                T acc = is_piv ? scalar_traits<T>::zero() : cur[u];
#pragma unroll
                for (int j = 0; j < W; ++j) fma_acc(acc, mult[u][j], y[j]);
                a[(size_t)i * ld + c] = acc;
            }
        }
        return;
    }
    // ---- the panel ----
    if (k0 < 0) return;
    const int32_t w = min(W, m - k0);
    if (w <= 0) return;
    int32_t* piv = ipiv + nd.piv_off;
    int32_t* rq = rowq + nd.piv_off;
    if (tid < W) {
        skey[tid] = 0ull;
        pprev[tid] = tid < wp ? piv[kprev + tid] : -1;
    }
    __syncthreads();
    if (wp > 0) {  // the previous panel's pivot rows in this panel's columns, before anything is overwritten
        for (int e = tid; e < W * W; e += NT) {
            const int j = e / W, cc = e % W;
            yprev[j][cc] = (j < wp && cc < w) ? a[(size_t)pprev[j] * ld + k0 + cc] : scalar_traits<T>::zero();
        }
    }
    T r[RPT][W];
    bool used[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const int32_t i = tid + NT * q;
        used[q] = i >= m || rq[min(i, m - 1)] >= 0;
#pragma unroll
        for (int c = 0; c < W; ++c) r[q][c] = (i < m && c < w) ? a[(size_t)i * ld + k0 + c] : scalar_traits<T>::zero();
    }
    __syncthreads();
    if (wp > 0) {
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            const int32_t i = tid + NT * q;
            if (i >= m) continue;
            bool is_piv = false;
#pragma unroll
            for (int j = 0; j < W; ++j) is_piv |= (i == pprev[j]);
            T mult[W];
#pragma unroll
            for (int j = 0; j < W; ++j) mult[j] = j < wp ? a[(size_t)i * ld + kprev + j] : scalar_traits<T>::zero();
#pragma unroll
            for (int c = 0; c < W; ++c) {
                T acc = is_piv ? scalar_traits<T>::zero() : r[q][c];
#pragma unroll
                for (int j = 0; j < W; ++j) fma_acc(acc, mult[j], yprev[j][c]);
                r[q][c] = c < w ? acc : scalar_traits<T>::zero();
            }
        }
    }
    static_for<W>([&](auto jc) {
        constexpr int jj = decltype(jc)::value;
        if (jj >= w) return;
        unsigned long long key = 0ull;
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            if (!used[q]) {
                const unsigned long long kq = pivot_key(s_abs2(r[q][jj]), tid + NT * q);
                key = kq > key ? kq : key;
            }
        }
        key = wave_max_key(key);
        if (lane == 0) atomicMax(&skey[jj], key);
        __syncthreads();
        key = skey[jj];
        const int32_t p = 65535 - (int32_t)(key & 0xFFFFull);
        if (tid == 0) {
            piv[k0 + jj] = p;
            prows[jj] = p;
            if (!(__longlong_as_double((long long)(key & ~0xFFFFull)) > tiny2) && atomicCAS(&flag[1], 0, t + 1) == 0) {
                flag[2] = k0 + jj;
                flag[3] = (int32_t)(key >> 32);  // high word of |pivot|^2
            }
        }
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            if (tid + NT * q == p) {
                T pv = r[q][jj];
                if (s_abs2(pv) == 0.0) s_from(pv, 1.0, 0.0);
                const T pinv = s_inv(pv);
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    const T v = (j == jj) ? pinv : s_mul(pinv, r[q][j]);
                    prow_s[jj & 1][j] = v;
                    r[q][j] = v;
                }
                used[q] = true;
                rq[p] = k0 + jj;
            }
        }
        __syncthreads();
        T prow[W];
#pragma unroll
        for (int j = 0; j < W; ++j) prow[j] = prow_s[jj & 1][j];
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            const int32_t i = tid + NT * q;
            if (i >= m || i == p) continue;
            const T fm = r[q][jj];
            if (s_abs2(fm) == 0.0) continue;
            const T nfm = s_sub(scalar_traits<T>::zero(), fm);
            r[q][jj] = scalar_traits<T>::zero();
#pragma unroll
            for (int j = 0; j < W; ++j) fma_acc(r[q][j], nfm, prow[j]);
        }
    });
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const int32_t i = tid + NT * q;
        if (i < m) {
#pragma unroll
            for (int j = 0; j < W; ++j)
                if (j < w) a[(size_t)i * ld + k0 + j] = r[q][j];
        }
    }
}

// Yb[j][c] = A[pivot row of column kb + j][c] for the kw columns of a finished block (or super-block, tournament path), columns
// c in [c_lo, c_hi): the rows the product below needs, staged because that product overwrites them.
// grid: (node, 256-column chunk of the window);  ycap = rows of staging space per unknown
template <typename T>
__global__ __launch_bounds__(256) void nd_gj_stage_kernel(const int32_t* __restrict__ lvl_nodes, const NdNodeDev* __restrict__ nodes,
                                                          const T* __restrict__ front, const int32_t* __restrict__ ipiv, int32_t kb, int32_t kw,
                                                          int32_t ycap, int32_t c_lo, int32_t c_hi, T* __restrict__ ybuf) {
    const NdNodeDev nd = nodes[lvl_nodes[blockIdx.x]];
    gj_stage_column<T>(nd, front, ipiv, kb, kw, ycap, c_lo + (int32_t)blockIdx.y * 256 + (int32_t)threadIdx.x, c_hi, ybuf);
}

// the columns outside the finished block: A[i, c] = (i is a pivot row of the block ? 0 : A[i, c]) + sum_j Wb[i, j] Yb[j, c]
// grid: (node, 64-row tile, 64-column tile); 4 x 4 per thread; the whole K = nb <= 32 extent in one pass through LDS
// Column windows (tournament path with look-ahead): `only` non-empty = update just the columns [only_lo, only_hi) (the next
// block's, so that its pivot search can start while the rest is updated); `skip` = leave [skip_lo, skip_hi) alone (done
// already).  ztile0 = first 64-column tile of the grid.
// INVARIANT the look-ahead relies on (launch_level_tp): while this product for block kb runs, the side stream's tournament
// for block kb + kNB may write rowq[r] for rows r that have not been pivots yet.  Such a row goes from -1 to a value
// >= kb + kNB; both read as "not a pivot row of block kb" in the test below (q >= kb && q < kb + nb), so the race cannot
// change a result.  rowq is therefore read through a plain pointer here (no __restrict__ / read-only cache path that a
// future compiler could use to assume the array does not change), and any change to rowq's encoding or to that test must
// keep the two values on the same side of it.  tests/test_gpu_ndlu.py runs the two-stream path (LSA_ND_LOOKAHEAD_MIN lowered).
template <typename T>
__global__ __launch_bounds__(256) void nd_gj_gemm_kernel(const int32_t* __restrict__ lvl_nodes, const NdNodeDev* __restrict__ nodes,
                                                         T* __restrict__ front, const int32_t* rowq, int32_t kb,
                                                         const T* __restrict__ ybuf, int32_t only_lo, int32_t only_hi, int32_t skip_lo,
                                                         int32_t skip_hi, int32_t ztile0) {
    __shared__ T Ws[kNB][kGT + 1];
    __shared__ T Ys[kNB][kGT + 1];
    const int32_t t = lvl_nodes[blockIdx.x];
    const NdNodeDev nd = nodes[t];
    const int32_t m = nd.m, ld = nd.f;
    const int32_t nb = min(kNB, m - kb);
    const int32_t row0 = (int32_t)blockIdx.y * kGT, col0 = ((int32_t)blockIdx.z + ztile0) * kGT;
    if (nb <= 0 || row0 >= m || col0 >= m) return;
    if (col0 >= kb && col0 + kGT <= kb + nb) return;  // tile inside the block
    if (only_hi > only_lo && (col0 >= only_hi || col0 + kGT <= only_lo)) return;
    if (col0 >= skip_lo && col0 + kGT <= skip_hi) return;
    T* a = front + nd.front_off;
    const T* yb = ybuf + (size_t)kNB * nd.piv_off;
    const int32_t* rq = rowq + nd.piv_off;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    for (int e = tid; e < kNB * kGT; e += 256) {
        // Ws[j][q] = Wb[row0 + q][j]: lanes along j (a row's block columns are contiguous);  Ys[j][q] = Yb[j][col0 + q]: lanes along q
        const int qa = e / kNB, ja = e - qa * kNB;
        const int32_t gr = row0 + qa;
        Ws[ja][qa] = (ja < nb && gr < m) ? a[(size_t)gr * ld + kb + ja] : scalar_traits<T>::zero();
        const int jb = e / kGT, qb = e - jb * kGT;
        const int32_t gc = col0 + qb;
        Ys[jb][qb] = (jb < nb && gc < m) ? yb[(size_t)jb * m + gc] : scalar_traits<T>::zero();
    }
    __syncthreads();
    T acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = scalar_traits<T>::zero();
    for (int k = 0; k < nb; ++k) {
        T av[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = Ws[k][ty * 4 + i];
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[j] = Ys[k][tx + 16 * j];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) fma_acc(acc[i][j], av[i], bv[j]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int32_t gr = row0 + ty * 4 + i;
        if (gr >= m) continue;
        const int32_t q = rq[gr];
        const bool is_piv = q >= kb && q < kb + nb;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int32_t gc = col0 + tx + 16 * j;
            if (gc >= m || (gc >= kb && gc < kb + nb)) continue;
            if ((gc >= skip_lo && gc < skip_hi) || (only_hi > only_lo && (gc < only_lo || gc >= only_hi))) continue;
            T* cptr = a + (size_t)gr * ld + gc;
            *cptr = is_piv ? acc[i][j] : s_add(*cptr, acc[i][j]);
        }
    }
}

// ---- tournament pivoting for tall pivot blocks --------------------------------------------------------------------------
// The panel launches above search a whole column in ONE workgroup: for a 6 000-row pivot block that is 16 dependent launch
// pairs per 32 columns, each reading its column with a stride of a front row.  Levels whose tallest pivot block has
// LSA_ND_TP_MIN rows or more choose the 32 pivot rows of a block by a tournament instead (communication-avoiding LU,
// Grigori, Demmel, Xiang 2011): every 256 rows pick their 32 best rows by Gaussian elimination with partial pivoting on
// their slice of the block's columns (thread per row, the row in registers); winners meet eight sets at a time (kTA) until one
// set is left; the last workgroup inverts the 32 x 32 pivot tile.  The block's columns then are one small product per row
// (nd_tp_colblock_kernel), and the staged rank-32 product above does the rest: 5-7 launches per 32 columns, all of them
// wide.  The pivot rows reach ipiv / rowq as with the panel launches, so everything downstream is unchanged.
constexpr int kTA = 8;  // candidate sets per workgroup in the later rounds (8 x 32 rows, thread per row)

// rows per workgroup in the first round: thread per row, or two rows per thread where 64 more registers are to be had
template <typename T>
struct tp_first {
    static constexpr int RPT = sizeof(T) == 16 ? 1 : 2;
    static constexpr int rows = 256 * RPT;
};

__host__ __device__ inline int32_t tp_sets(int32_t m, int32_t first_rows, int32_t round) {  // candidate sets of a pivot block before merge round `round`
    int32_t n = (m + first_rows - 1) / first_rows;
    for (int32_t r = 0; r < round; ++r) n = (n + kTA - 1) / kTA;
    return n;
}

template <typename T, bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void nd_tp_round_kernel(const int32_t* __restrict__ lvl_nodes, const NdNodeDev* __restrict__ nodes,
                                                          const T* __restrict__ front, int32_t* __restrict__ ipiv, int32_t* __restrict__ rowq, int32_t kb,
                                                          int32_t round, const int32_t* __restrict__ cand_in, int32_t* __restrict__ cand_out,
                                                          T* __restrict__ dinv, int32_t* __restrict__ flag, double tiny2) {
    constexpr int RPT = FIRST ? tp_first<T>::RPT : 1;
    __shared__ unsigned long long skey[2];
    __shared__ T prow_s[2][kNB];
    __shared__ int32_t sel_s[kNB];
    __shared__ T Ds[LAST ? kNB : 1][kNB + 1];
    const int32_t t = lvl_nodes[blockIdx.x];
    const NdNodeDev nd = nodes[t];
    const int32_t m = nd.m, ld = nd.f;
    const int32_t w = min(kNB, m - kb);
    if (w <= 0) return;
    const int32_t g = (int32_t)blockIdx.y;  // output set
    const int32_t nin = tp_sets(m, tp_first<T>::rows, FIRST ? 0 : round);
    if (FIRST ? g >= nin : g * kTA >= nin) return;
    const T* a = front + nd.front_off;
    const int32_t* rq = rowq + nd.piv_off;
    const int64_t coff = ((int64_t)(nd.piv_off / kTRmin) + t) * kNB;
    const int tid = threadIdx.x, lane = tid & 63;
    // (two plain arrays, not v[RPT][kNB]: the two-dimensional form ends up in scratch memory)
    int32_t row0 = -1, row1 = -1;
    T v0[kNB], v1[kNB];
    if (FIRST) {
        const int32_t i0 = g * tp_first<T>::rows + tid, i1 = i0 + 256;
        if (i0 < m && rq[i0] < 0) row0 = i0;
        if (RPT == 2 && i1 < m && rq[i1] < 0) row1 = i1;
    } else {
        const int32_t s = g * kTA + (tid >> 5);
        if (s < nin) row0 = cand_in[coff + (int64_t)s * kNB + (tid & 31)];
    }
#pragma unroll
    for (int c = 0; c < kNB; ++c) {
        v0[c] = (row0 >= 0 && c < w) ? a[(size_t)row0 * ld + kb + c] : scalar_traits<T>::zero();
        if constexpr (RPT == 2) v1[c] = (row1 >= 0 && c < w) ? a[(size_t)row1 * ld + kb + c] : scalar_traits<T>::zero();
    }
    bool alive0 = row0 >= 0, alive1 = RPT == 2 && row1 >= 0;
    if (tid < 2) skey[tid] = 0ull;
    if (tid < kNB) sel_s[tid] = -1;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kNB; ++j) {  // (no early exit: the loop must unroll for the rows to stay in registers; w is uniform)
        unsigned long long key = (alive0 && j < w) ? pivot_key(s_abs2(v0[j]), tid) : 0ull;
        if constexpr (RPT == 2) {
            const unsigned long long k1 = (alive1 && j < w) ? pivot_key(s_abs2(v1[j]), 256 + tid) : 0ull;
            key = k1 > key ? k1 : key;
        }
        key = wave_max_key(key);
        if (lane == 0 && key) atomicMax(&skey[j & 1], key);
        __syncthreads();
        key = skey[j & 1];
        if (tid == 0) skey[(j + 1) & 1] = 0ull;
        const int32_t win = 65535 - (int32_t)(key & 0xFFFFull);  // (256 *) second row + tid of the winning row
        if (key != 0ull && win == tid) {
#pragma unroll
            for (int c = 0; c < kNB; ++c) prow_s[j & 1][c] = v0[c];
            sel_s[j] = row0;
            alive0 = false;
        }
        if constexpr (RPT == 2) {
            if (key != 0ull && win == 256 + tid) {
#pragma unroll
                for (int c = 0; c < kNB; ++c) prow_s[j & 1][c] = v1[c];
                sel_s[j] = row1;
                alive1 = false;
            }
        }
        __syncthreads();
        if (key != 0ull) {
            const T pv = prow_s[j & 1][j];
            if (s_abs2(pv) > 0.0) {
                const T pinv = s_inv(pv);
                if (alive0) {
                    const T nf = s_sub(scalar_traits<T>::zero(), s_mul(v0[j], pinv));
#pragma unroll
                    for (int c = 0; c < kNB; ++c)
                        if (c > j) fma_acc(v0[c], nf, prow_s[j & 1][c]);
                }
                if constexpr (RPT == 2) {
                    if (alive1) {
                        const T nf = s_sub(scalar_traits<T>::zero(), s_mul(v1[j], pinv));
#pragma unroll
                        for (int c = 0; c < kNB; ++c)
                            if (c > j) fma_acc(v1[c], nf, prow_s[j & 1][c]);
                    }
                }
            }
        }
    }
    __syncthreads();
    if (!LAST) {
        if (tid < kNB) cand_out[coff + (int64_t)g * kNB + tid] = sel_s[tid];
        return;
    }
    // the winners are the pivot rows of columns kb .. kb + w - 1, in the order the elimination took them: invert their tile
    for (int e = tid; e < kNB * kNB; e += 256) {
        const int j = e / kNB, c = e - j * kNB;
        const int32_t pr = sel_s[j];
        T d = scalar_traits<T>::zero();
        if (j < w && c < w && pr >= 0) d = a[(size_t)pr * ld + kb + c];
        if (j == c && (j >= w || pr < 0)) s_from(d, 1.0, 0.0);
        Ds[j][c] = d;
    }
    __syncthreads();
    if (tid < w && sel_s[tid] < 0 && atomicCAS(&flag[1], 0, t + 1) == 0) {  // fewer rows left than columns: cannot happen for a square block
        flag[2] = kb + tid;
        flag[3] = 0;
    }
    for (int k = 0; k < w; ++k) {
        T rk[4], fi[4], cur[4];
        const T pv0 = Ds[k][k];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q, i = e / kNB, c = e - i * kNB;
            rk[q] = Ds[k][c];
            fi[q] = Ds[i][k];
            cur[q] = Ds[i][c];
        }
        __syncthreads();
        const double mag2 = s_abs2(pv0);
        if (tid == 0 && !(mag2 > tiny2) && atomicCAS(&flag[1], 0, t + 1) == 0) {
            flag[2] = kb + k;
            flag[3] = (int32_t)((unsigned long long)__double_as_longlong(mag2) >> 32);
        }
        T pv = pv0;
        if (mag2 == 0.0) s_from(pv, 1.0, 0.0);
        const T pinv = s_inv(pv);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q, i = e / kNB, c = e - i * kNB;
            T out;
            if (i == k) out = (c == k) ? pinv : s_mul(pinv, rk[q]);
            else if (c == k) out = s_sub(scalar_traits<T>::zero(), s_mul(fi[q], pinv));
            else out = s_sub(cur[q], s_mul(fi[q], s_mul(pinv, rk[q])));
            Ds[i][c] = out;
        }
        __syncthreads();
    }
    T* dv = dinv + (size_t)blockIdx.x * (kNB * kNB);
    for (int e = tid; e < kNB * kNB; e += 256) dv[e] = Ds[e / kNB][e % kNB];
    if (tid < w && sel_s[tid] >= 0) {
        ipiv[nd.piv_off + kb + tid] = sel_s[tid];
        rowq[nd.piv_off + sel_s[tid]] = kb + tid;
    }
}

// the block's own columns after its pivot tile is inverted:  pivot row j <- row j of D^-1,  any other row <- -A[row, K] D^-1
// grid: (node, 256-row tile), thread per row
template <typename T>
__global__ __launch_bounds__(256) void nd_tp_colblock_kernel(const int32_t* __restrict__ lvl_nodes, const NdNodeDev* __restrict__ nodes,
                                                             T* __restrict__ front, const int32_t* __restrict__ rowq, int32_t kb,
                                                             const T* __restrict__ dinv) {
    __shared__ T Ds[kNB][kNB + 1];
    const int32_t t = lvl_nodes[blockIdx.x];
    const NdNodeDev nd = nodes[t];
    const int32_t m = nd.m, ld = nd.f;
    const int32_t w = min(kNB, m - kb);
    const int32_t r0 = (int32_t)blockIdx.y * 256;
    if (w <= 0 || r0 >= m) return;
    const T* dv = dinv + (size_t)blockIdx.x * (kNB * kNB);
    for (int e = threadIdx.x; e < kNB * kNB; e += 256) Ds[e / kNB][e % kNB] = dv[e];
    __syncthreads();
    const int32_t i = r0 + threadIdx.x;
    if (i >= m) return;
    T* ai = front + nd.front_off + (size_t)i * ld + kb;
    const int32_t q = rowq[nd.piv_off + i];
    if (q >= kb && q < kb + w) {
#pragma unroll
        for (int c = 0; c < kNB; ++c)
            if (c < w) ai[c] = Ds[q - kb][c];
        return;
    }
    T x[kNB];
#pragma unroll
    for (int c = 0; c < kNB; ++c) x[c] = c < w ? ai[c] : scalar_traits<T>::zero();
#pragma unroll 4
    for (int c = 0; c < kNB; ++c) {
        if (c >= w) break;
        T acc = scalar_traits<T>::zero();
#pragma unroll
        for (int j = 0; j < kNB; ++j) fma_acc(acc, x[j], Ds[j][c]);
        ai[c] = s_sub(scalar_traits<T>::zero(), acc);
    }
}

// inverse gathered out of the eliminated block, straight into the packed factors: L[a][b] = S[p_a][q_b]  (p = pivot row of
// column a, q = its inverse)
template <typename T>
__global__ __launch_bounds__(256) void nd_unperm_kernel(const int32_t* __restrict__ tiles, const NdNodeDev* __restrict__ nodes,
                                                        T* front, const int32_t* __restrict__ ipiv,
                                                        const int32_t* __restrict__ rowq, T* __restrict__ lfac) {
    const int32_t t = tiles[2 * blockIdx.x], r0 = tiles[2 * blockIdx.x + 1];
    const NdNodeDev nd = nodes[t];
    const int32_t m = nd.m, ld = nd.f;
    const int32_t ra = r0 + (threadIdx.x >> 4);
    if (ra >= m) return;
    const T* src = front + nd.front_off + (size_t)ipiv[nd.piv_off + ra] * ld;
    const int32_t* q = rowq + nd.piv_off;
    if (nd.inv_off < 0) {
        T* dst = lfac + nd.lfac_off + (size_t)ra * m;
        for (int32_t cb = threadIdx.x & 15; cb < m; cb += 16) dst[cb] = src[q[cb]];
        return;
    }
    // a distributed node: the whole inverse into the working arena (operand of L = -F21 inv), this rank's rows also into the factors
    T* dst = front + nd.inv_off + (size_t)ra * m;
    const bool mine = ra >= nd.orow0 && ra < nd.orow0 + nd.orows;
    T* keep = lfac + nd.lfac_off + (size_t)(mine ? ra - nd.orow0 : 0) * m;
    for (int32_t cb = threadIdx.x & 15; cb < m; cb += 16) {
        const T v = src[q[cb]];
        dst[cb] = v;
        if (mine) keep[cb] = v;
    }
}

// Batched dense products of a chunk (row-major operands, 64 x 64 tiles); inv = the inverse of the node's pivot block:
//   KIND 0:  L[m:] = -F21 inv     (b x m)      KIND 1:  F22 += L[m:] F12   (b x b, in the working front)      KIND 2:  U = inv F12   (m x b)
// (a distributed top node: this rank's rows of each, see NdNodeDev)
// On the matrix cores: v_mfma_f64_16x16x4_f64, one wavefront per 32 x 32 quarter of the 64 x 64 tile
// (2 x 2 instruction tiles; complex scalars as real and imaginary planes, four instructions per complex tile product).
// A 4 x 4-per-thread FMA kernel (round 2's) reads 8 LDS values per 16 multiply-adds and is bound by the LDS array at about a third
// of the FP64 rate; here a k-step of 4 costs a wavefront 4 LDS reads for 4 (real) or 16 (complex) instructions of 64 cycles each.
// Operand maps (cdna_hip_programming.md, "Fragment layout"): lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15]; result
// register r of lane l is C[(l >> 4) + 4 r][l & 15].
// LDS images: A row-major with a row of BK + 1 doubles (16 rows x 2 k per half-wave: 32 distinct bank pairs), B k-major with a
// row of 64 + 16 doubles (two k-rows of a half-wave land 32 banks apart).  The next K-chunk's global loads are issued into
// registers before the current chunk's products (one LDS buffer, two barriers per chunk).
typedef double mfma_d4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ double plane_of(double v, int) { return v; }
__device__ __forceinline__ double plane_of(cplx v, int p) { return p == 0 ? v.re : v.im; }

template <typename T>
struct MfmaTile {
    static constexpr int BK = 16, LDAS = BK + 1, LDBS = kGT + 16, NPL = (int)(sizeof(T) / sizeof(double));
    double As[NPL][kGT * LDAS];
    double Bs[NPL][BK * LDBS];
};

// acc += A B over k in [0, K) for the 64 x 64 tile of a 256-thread workgroup: loadA(r, k) = A[tile row r][k], loadB(k, c) =
// B[k][tile column c], both zero outside their matrix.  On return wavefront w holds rows 32 (w >> 1) .., columns 32 (w & 1) ..:
// acc[plane][i][j][r] = C[32 (w >> 1) + 16 i + (lane >> 4) + 4 r][32 (w & 1) + 16 j + (lane & 15)]
template <typename T, typename FA, typename FB>
__device__ __forceinline__ void mfma_tile_product(int32_t K, FA loadA, FB loadB, MfmaTile<T>& sm, mfma_d4 (&acc)[MfmaTile<T>::NPL][2][2]) {
    constexpr int BK = MfmaTile<T>::BK, LDAS = MfmaTile<T>::LDAS, LDBS = MfmaTile<T>::LDBS, NPL = MfmaTile<T>::NPL;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = 32 * (wave >> 1), wc = 32 * (wave & 1), l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int p = 0; p < NPL; ++p)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[p][i][j] = mfma_d4{0.0, 0.0, 0.0, 0.0};
    // chunk staging: thread e = tid + 256 s;  A element (row e >> 4, k e & 15): 16 lanes along a row;  B element (k e >> 6, column e & 63)
    T pa[4], pb[4];
    auto gload = [&](int32_t kk) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int e = tid + 256 * s;
            pa[s] = loadA(e >> 4, kk + (e & 15));
            pb[s] = loadB(kk + (e >> 6), e & 63);
        }
    };
    gload(0);
    for (int32_t kk = 0; kk < K; kk += BK) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int e = tid + 256 * s;
#pragma unroll
            for (int p = 0; p < NPL; ++p) {
                sm.As[p][(e >> 4) * LDAS + (e & 15)] = plane_of(pa[s], p);
                sm.Bs[p][(e >> 6) * LDBS + (e & 63)] = plane_of(pb[s], p);
            }
        }
        __syncthreads();
        if (kk + BK < K) gload(kk + BK);
#pragma unroll
        for (int k4 = 0; k4 < BK; k4 += 4) {
            if (kk + k4 >= K) break;  // (zero-filled beyond K: skipping is only cheaper)
            double a[NPL][2], bb[NPL][2];
#pragma unroll
            for (int p = 0; p < NPL; ++p)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    a[p][i] = sm.As[p][(wr + 16 * i + l15) * LDAS + k4 + l4];
                    bb[p][i] = sm.Bs[p][(k4 + l4) * LDBS + wc + 16 * i + l15];
                }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[0][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0][i], bb[0][j], acc[0][i][j], 0, 0, 0);
                    if constexpr (NPL == 2) {
                        acc[0][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[NPL - 1][i], bb[NPL - 1][j], acc[0][i][j], 0, 0, 0);
                        acc[NPL - 1][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0][i], bb[NPL - 1][j], acc[NPL - 1][i][j], 0, 0, 0);
                        acc[NPL - 1][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[NPL - 1][i], bb[0][j], acc[NPL - 1][i][j], 0, 0, 0);
                    }
                }
        }
        __syncthreads();
    }
}

// one 64 x 64 tile (node t, tile row and column packed) of the product KIND
template <typename T, int KIND>
__device__ __forceinline__ void gemm_mfma_tile(int32_t t, int32_t packed, const NdNodeDev* __restrict__ nodes, T* __restrict__ front,
                                               T* __restrict__ lfac, T* __restrict__ ufac, MfmaTile<T>& sm) {
    constexpr int NPL = MfmaTile<T>::NPL;
    const int32_t tm = packed >> 16, tn = packed & 0xFFFF;
    const NdNodeDev nd = nodes[t];
    const int32_t m = nd.m, f = nd.f, b = f - m;
    T* F = front + nd.front_off;
    T* inv = nd.inv_off < 0 ? lfac + nd.lfac_off : front + nd.inv_off;  // the whole inverse (a distributed node: in the working arena)
    T* invrows = lfac + nd.lfac_off;                                    // this rank's own rows of it (all of them unless distributed)
    T* S1 = invrows + (size_t)nd.orows * m;
    T* S2 = ufac + nd.ufac_off;
    const T *A, *B;
    T* C;
    int32_t M, N, K, lda, ldb, ldc;
    // (a distributed top node: this rank's boundary rows of F21 / F22 and its own rows of U; F12 is whole on every rank)
    if (KIND == 0) {
        A = F + (size_t)m * f, lda = f, B = inv, ldb = m, C = S1, ldc = m, M = nd.brow, N = m, K = m;
    } else if (KIND == 1) {
        A = S1, lda = m, B = F + m, ldb = f, C = F + (size_t)m * f + m, ldc = f, M = nd.brow, N = b, K = m;
    } else {
        A = invrows, lda = m, B = F + m, ldb = f, C = S2, ldc = b, M = nd.orows, N = b, K = m;
    }
    const int32_t row0 = tm * kGT, col0 = tn * kGT;
    mfma_d4 acc[NPL][2][2];
    mfma_tile_product<T>(
        K,
        [&](int r, int32_t k) {
            const int32_t gr = row0 + r;
            return (gr < M && k < K) ? A[(size_t)gr * lda + k] : scalar_traits<T>::zero();
        },
        [&](int32_t k, int c) {
            const int32_t gc = col0 + c;
            return (k < K && gc < N) ? B[(size_t)k * ldb + gc] : scalar_traits<T>::zero();
        },
        sm, acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = 32 * (wave >> 1), wc = 32 * (wave & 1), l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int32_t gr = row0 + wr + 16 * i + l4 + 4 * r;
            if (gr >= M) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int32_t gc = col0 + wc + 16 * j + l15;
                if (gc >= N) continue;
                T v;
                s_from(v, acc[0][i][j][r], acc[NPL - 1][i][j][r]);
                T* c = C + (size_t)gr * ldc + gc;
                if (KIND == 0) *c = s_sub(scalar_traits<T>::zero(), v);
                else if (KIND == 1) *c = s_add(*c, v);
                else *c = v;
            }
        }
}

template <typename T, int KIND>
__global__ __launch_bounds__(256) void nd_gemm_mfma_kernel(const int32_t* __restrict__ tiles, const NdNodeDev* __restrict__ nodes,
                                                           T* __restrict__ front, T* __restrict__ lfac, T* __restrict__ ufac) {
    __shared__ MfmaTile<T> sm;
    gemm_mfma_tile<T, KIND>(tiles[2 * blockIdx.x], tiles[2 * blockIdx.x + 1], nodes, front, lfac, ufac, sm);
}

// kinds 0 and 2 of a chunk in one launch (both need the inverse alone; kind 1 follows, it reads kind 0's result): the first
// count0 workgroups take the tiles of kind 0, the others those of kind 2, each tile with the arithmetic of its own kernel
template <typename T>
__global__ __launch_bounds__(256) void nd_gemm_mfma_pair_kernel(const int32_t* __restrict__ tiles0, int32_t count0, const int32_t* __restrict__ tiles2,
                                                                const NdNodeDev* __restrict__ nodes, T* __restrict__ front, T* __restrict__ lfac,
                                                                T* __restrict__ ufac) {
    __shared__ MfmaTile<T> sm;
    const int32_t g = (int32_t)blockIdx.x;
    if (g < count0) gemm_mfma_tile<T, 0>(tiles0[2 * g], tiles0[2 * g + 1], nodes, front, lfac, ufac, sm);
    else gemm_mfma_tile<T, 2>(tiles2[2 * (g - count0)], tiles2[2 * (g - count0) + 1], nodes, front, lfac, ufac, sm);
}

// Gauss-Jordan, tournament path: the columns outside a finished group of kw <= kSB pivot columns [kb, kb + kw) of every node,
//          A[i, c] = (i is a pivot row of the group ? 0 : A[i, c]) + sum_j W[i, j] Y[j, c],
// W = the group's own columns (final), Y[j, :] = the row that was the pivot of column kb + j, staged BEFORE this launch
// (nd_gj_stage_kernel; stride ycap rows per unknown).  The group is one block of kNB columns -- then the window is the rest of
// its super-block -- or a whole super-block of kSB: the elimination of a block multiplies the matrix from the left by a
// matrix that differs from the identity only in the columns of its pivot rows, so does the product over the blocks of a
// super-block, and the super-block's own columns hold exactly those columns once its blocks have updated one another.  The
// rank-kNB update of a 6 700-row pivot block streamed the block through HBM once per 32 pivots (4 flops per byte: 9 TFLOP/s);
// at rank kSB = 128 the product is bound by the matrix cores.
// grid: (node, 64-row tile, 64-column tile from ztile0).  Column windows as in nd_gj_gemm_kernel, whose invariant on rowq
// holds here unchanged (rows that become pivots of a LATER block while this runs read as "not a pivot row of the group").
template <typename T>
__global__ __launch_bounds__(256) void nd_gj_update_kernel(const int32_t* __restrict__ lvl_nodes, const NdNodeDev* __restrict__ nodes,
                                                           T* __restrict__ front, const int32_t* rowq, int32_t kb, int32_t kw,
                                                           const T* __restrict__ ybuf, int32_t ycap, int32_t only_lo, int32_t only_hi,
                                                           int32_t skip_lo, int32_t skip_hi, int32_t ztile0) {
    constexpr int NPL = MfmaTile<T>::NPL;
    __shared__ MfmaTile<T> sm;
    const int32_t t = lvl_nodes[blockIdx.x];
    const NdNodeDev nd = nodes[t];
    const int32_t m = nd.m, ld = nd.f;
    const int32_t nb = min(kw, m - kb);
    const int32_t row0 = (int32_t)blockIdx.y * kGT, col0 = ((int32_t)blockIdx.z + ztile0) * kGT;
    if (nb <= 0 || row0 >= m || col0 >= m) return;
    if (col0 >= kb && col0 + kGT <= kb + nb) return;  // tile inside the group
    if (only_hi > only_lo && (col0 >= only_hi || col0 + kGT <= only_lo)) return;
    if (col0 >= skip_lo && col0 + kGT <= skip_hi) return;
    T* a = front + nd.front_off;
    const T* yb = ybuf + (size_t)ycap * nd.piv_off;
    const int32_t* rq = rowq + nd.piv_off;
    mfma_d4 acc[NPL][2][2];
    mfma_tile_product<T>(
        nb,
        [&](int r, int32_t k) {
            const int32_t gr = row0 + r;
            return (gr < m && k < nb) ? a[(size_t)gr * ld + kb + k] : scalar_traits<T>::zero();
        },
        [&](int32_t k, int c) {
            const int32_t gc = col0 + c;
            return (k < nb && gc < m) ? yb[(size_t)k * m + gc] : scalar_traits<T>::zero();
        },
        sm, acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = 32 * (wave >> 1), wc = 32 * (wave & 1), l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int32_t gr = row0 + wr + 16 * i + l4 + 4 * r;
            if (gr >= m) continue;
            const int32_t q = rq[gr];
            const bool is_piv = q >= kb && q < kb + nb;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int32_t gc = col0 + wc + 16 * j + l15;
                if (gc >= m || (gc >= kb && gc < kb + nb)) continue;
                if ((gc >= skip_lo && gc < skip_hi) || (only_hi > only_lo && (gc < only_lo || gc >= only_hi))) continue;
                T v;
                s_from(v, acc[0][i][j][r], acc[NPL - 1][i][j][r]);
                T* cptr = a + (size_t)gr * ld + gc;
                *cptr = is_piv ? v : s_add(*cptr, v);
            }
        }
}

// the update matrix leaves the working front for the update arena (tile = 16 rows of the b x b block)
template <typename T>
__global__ __launch_bounds__(256) void nd_save_update_kernel(const int32_t* __restrict__ tiles, const NdNodeDev* __restrict__ nodes,
                                                             const T* __restrict__ front, T* __restrict__ upd) {
    const int32_t t = tiles[2 * blockIdx.x], r0 = tiles[2 * blockIdx.x + 1];
    const NdNodeDev nd = nodes[t];
    const int32_t m = nd.m, f = nd.f, b = f - m;
    const int32_t r = r0 + (threadIdx.x >> 4);
    if (r >= nd.brow) return;  // (this rank's rows of the update matrix: all b of them unless the node is distributed)
    const T* src = front + nd.front_off + (size_t)(m + r) * f + m;
    T* dst = upd + nd.upd_off + (size_t)r * b;
    for (int32_t c = threadIdx.x & 15; c < b; c += 16) dst[c] = src[c];
}

// The assembly of the merged top of the sweeps (NdTop, NdTopJob: ndlu_internal.h), two launches per factorisation.
// Plain FMA tiles: 256 threads, 2 x 2 results each, K in steps of 16 through LDS.  Every entry of C is one thread's sum in
// the order of k: two factorisations of one matrix give the same T bit for bit.
template <typename T>
__global__ __launch_bounds__(256) void nd_top_gemm_kernel(const int32_t* __restrict__ tiles, const NdTopJob* __restrict__ jobs,
                                                          const int32_t* __restrict__ cmap, const T* __restrict__ lfac,
                                                          const T* __restrict__ ufac, T* top, int32_t ldc) {
    __shared__ T As[16][33], Bs[16][33];
    const NdTopJob jb = jobs[tiles[2 * blockIdx.x]];
    const int32_t tile = tiles[2 * blockIdx.x + 1], i0 = (tile >> 16) * 32, j0 = (tile & 0xFFFF) * 32;
    const T* A = (jb.a_src == 0 ? lfac : jb.a_src == 1 ? ufac : (const T*)top) + jb.a_off;
    const T* B = lfac + jb.b_off;
    const int32_t* map = cmap + jb.map_off;
    const int tid = threadIdx.x, ti = tid / 16, tj = tid % 16;
    T acc[2][2] = {{scalar_traits<T>::zero(), scalar_traits<T>::zero()}, {scalar_traits<T>::zero(), scalar_traits<T>::zero()}};
    for (int32_t k0 = 0; k0 < jb.K; k0 += 16) {
        // A tile 32 x 16 (thread: row tid / 16 and + 16, column tid % 16), B tile 16 x 32 (row tid / 32 and + 8, column tid % 32)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int32_t i = i0 + ti + 16 * h, k = k0 + tj;
            As[tj][ti + 16 * h] = i < jb.M && k < jb.K ? A[(size_t)i * jb.lda + (jb.gather == 1 ? map[k] : k)] : scalar_traits<T>::zero();
            const int32_t kb = k0 + tid / 32 + 8 * h, j = j0 + tid % 32;
            Bs[tid / 32 + 8 * h][tid % 32] = kb < jb.K && j < jb.N ? B[(size_t)(jb.gather == 2 ? map[kb] : kb) * jb.ldb + j] : scalar_traits<T>::zero();
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const T a0 = As[k][ti], a1 = As[k][ti + 16], b0 = Bs[k][tj], b1 = Bs[k][tj + 16];
            fma_acc(acc[0][0], a0, b0);
            fma_acc(acc[0][1], a0, b1);
            fma_acc(acc[1][0], a1, b0);
            fma_acc(acc[1][1], a1, b1);
        }
        __syncthreads();
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int32_t i = i0 + ti + 16 * h, j = j0 + tj + 16 * g;
            if (i >= jb.M || j >= jb.N) continue;
            const T d = jb.d_off >= 0 ? lfac[jb.d_off + (size_t)i * jb.ldd + j] : scalar_traits<T>::zero();
            top[jb.c_off + (size_t)i * ldc + j] = jb.negate ? s_sub(d, acc[h][g]) : s_add(d, acc[h][g]);
        }
}

template <typename T, int NT, int RPT, int W>
void launch_block(lsa_ctx* ctx, lsa_ndlu* f, const NdChunk& L, int32_t kb, double tiny2) {
    hipStream_t st = ctx->stream;
    const int32_t* lv = f->d_chunk_nodes + L.node_begin;
    T* front = (T*)f->d_work;
    auto active_at = [&](int32_t k) {  // nodes are sorted by own size: those that still have column k form a prefix
        return (int32_t)(std::lower_bound(L.sorted_m.begin(), L.sorted_m.end(), k, std::greater<int32_t>()) - L.sorted_m.begin());
    };
    const int32_t kend = std::min(kb + kNB, L.max_m);
    const bool others = std::min(kNB, L.max_m - kb) > W;  // the block has columns besides one panel
    constexpr bool between = 2 * W < kNB;                 // ... and block columns outside both the previous and the current panel can exist
    const bool outside = L.max_m > kNB;                   // columns outside the block exist (in the larger nodes)
    int32_t kprev = -1, active_prev = 0;
    for (int32_t k0 = kb; k0 < kend; k0 += W) {
        const int32_t active = active_at(k0);
        if (active == 0) break;
        // (the tiles of this launch serve the nodes that had the previous panel: a superset of those that have this one)
        ND_LAUNCH(f, (nd_gj_fused_kernel<T, NT, RPT, W>), dim3(std::max(active, active_prev), others && between && kprev >= 0 ? 1 + kNB / 16 : 1), dim3(NT), 0,
                  st, lv, f->d_nodes, front, f->d_ipiv, f->d_rowq, kb, k0, kprev, f->d_flag, tiny2, 0, (T*)f->d_ybuf, 0);
        kprev = k0;
        active_prev = active;
    }
    const bool finish = others && kprev >= 0;
    const bool ride = finish && outside && f->gj_panel != 8;  // the staging rides in the finishing launch
    if (finish) {  // the last panel's update of the block's other columns
        // (two panels: only the columns before the last panel are left.  The staging serves every node that has the block, the
        //  tiles those that had the last panel: a prefix of them, the others leave at wp <= 0)
        const int32_t ftiles = between ? kNB / 16 : (kprev - kb + 15) / 16;
        ND_LAUNCH(f, (nd_gj_fused_kernel<T, NT, RPT, W>), dim3(ride ? active_at(kb) : active_prev, 1 + ftiles + (ride ? (L.max_m + NT - 1) / NT : 0)), dim3(NT),
                  0, st, lv, f->d_nodes, front, f->d_ipiv, f->d_rowq, kb, -1, kprev, f->d_flag, tiny2, ride ? 1 + ftiles : 0, (T*)f->d_ybuf, L.max_m);
    }
    if (outside) {
        const int32_t active = active_at(kb);
        if (!ride)
            ND_LAUNCH(f, (nd_gj_stage_kernel<T>), dim3(active, (L.max_m + 255) / 256), dim3(256), 0, st, lv, f->d_nodes, (const T*)front, f->d_ipiv, kb, kNB, kNB,
                      0, L.max_m, (T*)f->d_ybuf);
        const int32_t tiles = (L.max_m + kGT - 1) / kGT;
        ND_LAUNCH(f, (nd_gj_gemm_kernel<T>), dim3(active, tiles, tiles), dim3(256), 0, st, lv, f->d_nodes, front, f->d_rowq, kb, (const T*)f->d_ybuf, 0, 0,
                  0, 0, 0);
    }
}

// the tournament for the block of columns starting at kb, on stream `st`: leaves D^-1 per node in d_dinv and the pivot
// rows in ipiv / rowq
template <typename T>
void launch_tournament(lsa_ndlu* f, const NdChunk& L, int32_t kb, double tiny2, hipStream_t st) {
    const int32_t* lv = f->d_chunk_nodes + L.node_begin;
    const T* front = (const T*)f->d_work;
    const int32_t active = (int32_t)(std::lower_bound(L.sorted_m.begin(), L.sorted_m.end(), kb, std::greater<int32_t>()) - L.sorted_m.begin());
    if (active == 0) return;
    int32_t sets = (L.max_m + tp_first<T>::rows - 1) / tp_first<T>::rows;
    ND_LAUNCH(f, (nd_tp_round_kernel<T, true, false>), dim3(active, sets), dim3(256), 0, st, lv, f->d_nodes, front, f->d_ipiv, f->d_rowq, kb, 0,
              (const int32_t*)nullptr, f->d_cand[0], (T*)nullptr, f->d_flag, tiny2);
    int src = 0;
    for (int32_t round = 0;; ++round) {
        const int32_t groups = (sets + kTA - 1) / kTA;
        if (groups == 1) {
            ND_LAUNCH(f, (nd_tp_round_kernel<T, false, true>), dim3(active, 1), dim3(256), 0, st, lv, f->d_nodes, front, f->d_ipiv, f->d_rowq, kb, round,
                      (const int32_t*)f->d_cand[src], (int32_t*)nullptr, (T*)f->d_dinv, f->d_flag, tiny2);
            break;
        }
        ND_LAUNCH(f, (nd_tp_round_kernel<T, false, false>), dim3(active, groups), dim3(256), 0, st, lv, f->d_nodes, front, f->d_ipiv, f->d_rowq, kb, round,
                  (const int32_t*)f->d_cand[src], f->d_cand[src ^ 1], (T*)nullptr, f->d_flag, tiny2);
        src ^= 1;
        sets = groups;
    }
}

// Gauss-Jordan of all pivot blocks of a level by tournament pivoting, with look-ahead: once block k's own columns are done
// the next block's 32 columns are updated first, and its tournament (a chain of single-workgroup launches) runs on a
// second stream underneath the rank-32 product that updates everything else.
template <typename T>
int launch_level_tp(lsa_ctx* ctx, lsa_ndlu* f, const NdChunk& L, double tiny2) {
    hipStream_t st = ctx->stream, side = f->side;
    const int32_t* lv = f->d_chunk_nodes + L.node_begin;
    T* front = (T*)f->d_work;
    auto active_at = [&](int32_t k) {
        return (int32_t)(std::lower_bound(L.sorted_m.begin(), L.sorted_m.end(), k, std::greater<int32_t>()) - L.sorted_m.begin());
    };
    // (two cross-stream hand-offs per block cost ~15 us: worth it only where the product they hide behind is long.
    // Measured: C300k 472 -> 438 ms, C160k 186 -> 183 ms; S500k, tallest pivot block 838 rows, 56 -> 59 ms without this limit)
    const int32_t ahead_min = getenv("LSA_ND_LOOKAHEAD_MIN") ? atoi(getenv("LSA_ND_LOOKAHEAD_MIN")) : 1024;
    const bool ahead = side != nullptr && L.max_m >= std::max(ahead_min, 2 * kNB + 1);
    // super-blocks of kSB columns where the pivot blocks are large (see nd_gj_update_kernel); elsewhere a "super-block" is one block
    const bool wide = L.max_m >= f->sb_min;
    const int32_t sbw = wide ? f->sb_cols : kNB, ycap = f->ycap;
    const int32_t tiles = (L.max_m + kGT - 1) / kGT;
    auto stage = [&](int32_t active, int32_t k0, int32_t kw, int32_t c_lo, int32_t c_hi) {
        ND_LAUNCH(f, (nd_gj_stage_kernel<T>), dim3(active, (c_hi - c_lo + 255) / 256), dim3(256), 0, st, lv, f->d_nodes, (const T*)front, f->d_ipiv, k0, kw,
                  ycap, c_lo, c_hi, (T*)f->d_ybuf);
    };
    auto update = [&](int32_t active, int32_t k0, int32_t kw, int32_t zt0, int32_t ztn, int32_t only_lo, int32_t only_hi, int32_t skip_lo, int32_t skip_hi) {
        ND_LAUNCH(f, (nd_gj_update_kernel<T>), dim3(active, tiles, ztn), dim3(256), 0, st, lv, f->d_nodes, front, f->d_rowq, k0, kw, (const T*)f->d_ybuf,
                  ycap, only_lo, only_hi, skip_lo, skip_hi, zt0);
    };
    launch_tournament<T>(f, L, 0, tiny2, st);
    for (int32_t sb0 = 0; sb0 < L.max_m; sb0 += sbw) {
        const int32_t sb1 = std::min(sb0 + sbw, L.max_m);
        if (active_at(sb0) == 0) break;
        for (int32_t kb = sb0; kb < sb1; kb += kNB) {
            const int32_t active = active_at(kb);
            if (active == 0) break;
            ND_LAUNCH(f, (nd_tp_colblock_kernel<T>), dim3(active, (L.max_m + 255) / 256), dim3(256), 0, st, lv, f->d_nodes, front, f->d_rowq, kb,
                      (const T*)f->d_dinv);
            if (sb1 - sb0 > kNB) {  // the super-block's other columns (earlier blocks' included), so that its next block can be searched
                stage(active, kb, kNB, sb0, sb1);
                update(active, kb, kNB, sb0 / kGT, (sb1 + kGT - 1) / kGT - sb0 / kGT, sb0, sb1, 0, 0);
                if (kb + kNB < sb1 && active_at(kb + kNB) > 0) launch_tournament<T>(f, L, kb + kNB, tiny2, st);
            }
        }
        const int32_t active = active_at(sb0), next = sb1;
        const bool has_next = next < L.max_m && active_at(next) > 0;
        if (L.max_m > sb1 - sb0) {  // columns outside the super-block exist (in the larger nodes)
            stage(active, sb0, sb1 - sb0, 0, L.max_m);
            if (has_next && ahead) {
                update(active, sb0, sb1 - sb0, next / kGT, 1, next, next + kNB, 0, 0);
                LSA_HIP_CHECK(ctx, hipEventRecord(f->ev_panel, st));
                LSA_HIP_CHECK(ctx, hipStreamWaitEvent(side, f->ev_panel, 0));
                launch_tournament<T>(f, L, next, tiny2, side);
                LSA_HIP_CHECK(ctx, hipEventRecord(f->ev_pivots, side));
                update(active, sb0, sb1 - sb0, 0, tiles, 0, 0, next, next + kNB);
                LSA_HIP_CHECK(ctx, hipStreamWaitEvent(st, f->ev_pivots, 0));
                continue;
            }
            update(active, sb0, sb1 - sb0, 0, tiles, 0, 0, 0, 0);
        }
        if (has_next) launch_tournament<T>(f, L, next, tiny2, st);
    }
    return LSA_OK;
}

template <typename T>
int nd_numeric(lsa_ctx* ctx, lsa_ndlu* f, const lsa_mat* C) {
    const NdSymbolic& S = f->S;
    hipStream_t st = ctx->stream;
    T* front = (T*)f->d_work;
    T* lfac = (T*)f->d_lfac;
    T* ufac = (T*)f->d_ufac;
    T* upd = (T*)f->d_upd;
    int rc0 = LSA_OK;
    double max2 = 0.0;
    f->factor_launches = 0;
    {
        // (a local failure up to here -- non-finite input, a HIP error -- is agreed on by all ranks before the first exchange)
        auto head = [&]() -> int {
            LSA_HIP_CHECK(ctx, hipMemsetAsync(f->d_rowq, 0xFF, (size_t)std::max<int32_t>(S.n, 1) * sizeof(int32_t), st));
            LSA_HIP_CHECK(ctx, hipMemsetAsync(f->d_flag, 0, 4 * sizeof(int32_t), st));
            LSA_HIP_CHECK(ctx, hipMemsetAsync(f->d_maxabs, 0, sizeof(unsigned long long), st));
            if (S.nnz > 0) {
                const int blocks = (int)std::min<int64_t>((S.nnz + 255) / 256, (int64_t)ctx->num_cu * 2);
                ND_LAUNCH(f, (nd_maxabs2_kernel<T>), dim3(blocks), dim3(256), 0, st, S.nnz, (const T*)C->val, f->d_maxabs);
            }
            unsigned long long mbits = 0;
            LSA_HIP_CHECK(ctx, hipMemcpyAsync(&mbits, f->d_maxabs, sizeof mbits, hipMemcpyDeviceToHost, st));
            LSA_HIP_CHECK(ctx, hipStreamSynchronize(st));
            memcpy(&max2, &mbits, sizeof max2);
            if (!std::isfinite(max2)) return lsa_set_error(ctx, LSA_ERR_NONFINITE, "lsa_ndlu: the matrix holds non-finite values");
            return LSA_OK;
        };
        // (agreed on over the ranks THIS factorisation is split over: a rank-local factorisation on a multi-rank context --
        //  a rank's diagonal block, a retry only one rank takes -- must not enter a collective the others are not in)
        rc0 = S.nranks > 1 ? k_agree_status(ctx, head()) : head();
        if (rc0 != LSA_OK) return rc0;
    }
    // (1e-15 * max|C|)^2: rounding level.  A shift next to an eigenvalue (the adjoint problem of the reference is shifted exactly at
    // a converged eigenvalue) gives legitimate pivots of 1e-12 max|C|; those solves are judged by their backward error.
    const double tiny2 = 1e-30 * max2;
    const int32_t* tl = f->d_tiles;
    bool exchanged = false;
    for (size_t ci = 0; ci < f->chunks.size(); ++ci) {
        const NdChunk& L = f->chunks[ci];
        // subtree-parallel: the ranks' subtree roots are done; every rank receives all of their update matrices
        if (L.exchange_before && f->xupd_slot > 0) {
            LSA_CHECK(k_allgather_inplace(ctx, f->d_upd, (size_t)f->xupd_slot * sizeof(T)));
            exchanged = true;
        }
        LSA_HIP_CHECK(ctx, hipMemsetAsync(f->d_work, 0, (size_t)L.work_entries * sizeof(T), st));
        if (L.asm_count > 0) {
            const int blocks = (int)std::min<int64_t>((L.asm_count + 255) / 256, (int64_t)ctx->num_cu * 16);
            ND_LAUNCH(f, (nd_assemble_kernel<T>), dim3(blocks), dim3(256), 0, st, L.asm_count, (const T*)C->val, f->d_asm_src + L.asm_begin,
                      f->d_asm_dst + L.asm_begin, front);
        }
        for (const TileList& e : L.ext)
            if (e.count > 0)
                ND_LAUNCH(f, (nd_extend_add_kernel<T>), dim3(e.count), dim3(256), 0, st, tl + 2 * e.off, f->d_nodes, f->d_cmap, front, (const T*)upd);
        // distributed top nodes: their children's update matrices, in row chunks.  Per step: every rank copies its piece (rows of
        // a distributed child it holds, or of a subtree root it owns) into its slot of the staging buffer, one in-place
        // all-gather, then every rank adds the rows it keeps -- the pivot block and F12 rows on every rank, boundary rows on
        // their owner -- slot by slot (fixed order of the sums: the replicated pivot blocks stay bitwise alike).
        for (const auto& step : L.xsteps) {
            T* stage = (T*)f->d_xstage;
            // (the slots of a step are as wide as its largest piece, not as the buffer allows: the exchange moves what travels)
            int64_t stride = 0;
            for (int r = 0; r < S.nranks; ++r) {
                const NdChunk::XPiece& pc = step[(size_t)r];
                if (pc.nrows > 0) stride = std::max(stride, (int64_t)pc.nrows * (S.f[(size_t)pc.child] - S.m[(size_t)pc.child]));
            }
            if (stride == 0) continue;
            const NdChunk::XPiece& mine = step[(size_t)S.rank];
            if (mine.nrows > 0) {
                const int32_t bc = S.f[(size_t)mine.child] - S.m[(size_t)mine.child];
                const int64_t src_off = f->chunk_node_upd_off(mine.child) + (int64_t)(mine.row0 - S.brow0[(size_t)mine.child]) * bc;
                LSA_HIP_CHECK(ctx, hipMemcpyAsync(stage + (size_t)S.rank * (size_t)stride, upd + src_off, (size_t)mine.nrows * (size_t)bc * sizeof(T),
                                                  hipMemcpyDeviceToDevice, st));
            }
            LSA_CHECK(k_allgather_inplace(ctx, stage, (size_t)stride * sizeof(T)));
            for (int r = 0; r < S.nranks; ++r) {
                const NdChunk::XPiece& pc = step[(size_t)r];
                if (pc.nrows <= 0) continue;
                ND_LAUNCH(f, (nd_extend_add_staged_kernel<T>), dim3((pc.nrows + 15) / 16), dim3(256), 0, st, f->d_nodes, f->d_cmap, front,
                          (const T*)(stage + (size_t)r * (size_t)stride), pc.child, pc.row0, pc.nrows);
            }
        }
        if (L.max_m >= f->tp_min) LSA_CHECK(launch_level_tp<T>(ctx, f, L, tiny2));
        for (int32_t kb = 0; kb < L.max_m && L.max_m < f->tp_min; kb += kNB) {
            // 16-column panels only on request: a thread holds its row of one in registers up to 512 rows (1024 threads have half the
            // registers), but a panel launch of 16 pivots takes as long as two of 8 (21-27 against 11.5-13.6 us with complex
            // factors: the pivots are a serial chain, and each one updates twice the columns), so that the default keeps 8
            if (f->gj_panel == 16 && L.max_m <= 512) {
                if (L.max_m <= 64) launch_block<T, 64, 1, 16>(ctx, f, L, kb, tiny2);
                else if (L.max_m <= 128) launch_block<T, 128, 1, 16>(ctx, f, L, kb, tiny2);
                else if (L.max_m <= 256) launch_block<T, 256, 1, 16>(ctx, f, L, kb, tiny2);
                else launch_block<T, 512, 1, 16>(ctx, f, L, kb, tiny2);
            } else if (L.max_m <= 64) launch_block<T, 64, 1, 8>(ctx, f, L, kb, tiny2);
            else if (L.max_m <= 128) launch_block<T, 128, 1, 8>(ctx, f, L, kb, tiny2);
            else if (L.max_m <= 256) launch_block<T, 256, 1, 8>(ctx, f, L, kb, tiny2);
            else if (L.max_m <= 512) launch_block<T, 512, 1, 8>(ctx, f, L, kb, tiny2);
            else if (L.max_m <= 1024) launch_block<T, 1024, 1, 8>(ctx, f, L, kb, tiny2);
            else if (L.max_m <= 2048) launch_block<T, 1024, 2, 8>(ctx, f, L, kb, tiny2);
            else if (L.max_m <= 4096) launch_block<T, 1024, 4, 4>(ctx, f, L, kb, tiny2);
            else if (L.max_m <= 8192) launch_block<T, 1024, 8, 2>(ctx, f, L, kb, tiny2);
            else launch_block<T, 1024, 16, 1>(ctx, f, L, kb, tiny2);
        }
        if (L.unperm.count > 0)
            ND_LAUNCH(f, (nd_unperm_kernel<T>), dim3(L.unperm.count), dim3(256), 0, st, tl + 2 * L.unperm.off, f->d_nodes, front, f->d_ipiv,
                      f->d_rowq, lfac);
        auto product = [&](auto kind) {
            constexpr int KIND = decltype(kind)::value;
            if (L.gemm[KIND].count == 0) return;
            ND_LAUNCH(f, (nd_gemm_mfma_kernel<T, KIND>), dim3(L.gemm[KIND].count), dim3(256), 0, st, tl + 2 * L.gemm[KIND].off, f->d_nodes, front, lfac, ufac);
        };
        if (f->gj_panel != 8 && L.gemm[0].count > 0 && L.gemm[2].count > 0) {  // S1 and S2 depend on the inverse alone: one launch
            ND_LAUNCH(f, (nd_gemm_mfma_pair_kernel<T>), dim3(L.gemm[0].count + L.gemm[2].count), dim3(256), 0, st, tl + 2 * L.gemm[0].off, (int32_t)L.gemm[0].count,
                      tl + 2 * L.gemm[2].off, f->d_nodes, front, lfac, ufac);
            product(std::integral_constant<int, 1>{});
        } else {
            product(std::integral_constant<int, 0>{});
            product(std::integral_constant<int, 1>{});
            product(std::integral_constant<int, 2>{});
        }
        if (L.save.count > 0)
            ND_LAUNCH(f, (nd_save_update_kernel<T>), dim3(L.save.count), dim3(256), 0, st, tl + 2 * L.save.off, f->d_nodes, (const T*)front, upd);
    }
    if (f->top.s > 0)  // the merged top of the sweeps, assembled from the blocks just made (the second launch reads the first one's -Q_c)
        for (int q = 0, t0 = 0; q < 2; t0 += f->top_tiles[q++])
            if (f->top_tiles[q] > 0)
                ND_LAUNCH(f, (nd_top_gemm_kernel<T>), dim3(f->top_tiles[q]), dim3(256), 0, st, f->d_top_tiles + 2 * t0, f->d_top_jobs, f->d_cmap,
                          (const T*)lfac, (const T*)ufac, (T*)f->d_top, f->top.s);
    if (!exchanged && S.nranks > 1 && f->xupd_slot > 0)  // (no replicated level: still a collective)
        LSA_CHECK(k_allgather_inplace(ctx, f->d_upd, (size_t)f->xupd_slot * sizeof(T)));
    int32_t hflag[4] = {0, 0, 0, 0};
    if (S.nranks > 1) {
        // every rank must take the same decision (a rank that returned early would leave the others in a collective):
        // the failure flags are exchanged, the first failing rank's record wins
        LSA_HIP_CHECK(ctx, hipMemcpyAsync(f->d_xflag + 4 * S.rank, f->d_flag, 4 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        LSA_CHECK(k_allgather_inplace(ctx, f->d_xflag, 4 * sizeof(int32_t)));
        std::vector<int32_t> all((size_t)4 * S.nranks, 0);
        LSA_HIP_CHECK(ctx, hipMemcpyAsync(all.data(), f->d_xflag, all.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        LSA_HIP_CHECK(ctx, hipStreamSynchronize(st));
        for (int r = 0; r < S.nranks; ++r)
            if (all[(size_t)4 * r + 1] != 0) {
                memcpy(hflag, &all[(size_t)4 * r], sizeof hflag);
                if (r != S.rank) hflag[1] = -(r + 1);  // another rank's node: no local record of it
                break;
            }
    } else {
        LSA_HIP_CHECK(ctx, hipMemcpyAsync(hflag, f->d_flag, sizeof hflag, hipMemcpyDeviceToHost, st));
        LSA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    LSA_HIP_CHECK(ctx, hipGetLastError());
    if (hflag[1] < 0)
        return lsa_set_error(ctx, LSA_ERR_ZERO_PIVOT, "lsa_ndlu: a pivot block on rank %d is singular to 1e-15 * max|C| (column %d of its node)", -hflag[1] - 1,
                             hflag[2]);
    if (hflag[1] != 0) {
        const int32_t t = hflag[1] - 1;
        const unsigned long long hi = (unsigned long long)(uint32_t)hflag[3] << 32;
        double mag2;
        memcpy(&mag2, &hi, sizeof mag2);
        return lsa_set_error(ctx, LSA_ERR_ZERO_PIVOT,
                             "lsa_ndlu: the pivot block of tree node %d (%d unknowns, front %d, level %d) is singular at its column %d: largest "
                             "candidate pivot %.3e against max|C| = %.3e (threshold 1e-15 max|C|); the matrix is singular, or needs pivoting "
                             "across fronts",
                             t, S.m[(size_t)t], S.f[(size_t)t], S.level[(size_t)t], hflag[2], std::sqrt(mag2), std::sqrt(max2));
    }
    if (const char* pe = getenv("LSA_ND_TEST_PERTURB")) {
        const double eps = atof(pe);
        if (eps != 0.0 && f->ufac_entries > 0) {
            const int blocks = (int)std::min<int64_t>((f->ufac_entries + 255) / 256, (int64_t)ctx->num_cu * 16);
            ND_LAUNCH(f, (nd_scale_kernel<T>), dim3(blocks), dim3(256), 0, st, f->ufac_entries, ufac, 1.0 + eps);
            LSA_HIP_CHECK(ctx, hipStreamSynchronize(st));
        }
    }
    return LSA_OK;
}

}  // namespace

int ndlu_numeric(lsa_ctx* ctx, lsa_ndlu* f, const lsa_mat* C) {
    return f->dtype == LSA_C128 ? nd_numeric<cplx>(ctx, f, C) : nd_numeric<double>(ctx, f, C);
}
