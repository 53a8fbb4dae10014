// Nested-dissection multifrontal LU on the device: the exact factorisation behind PreconditionerType.LU, the setting of
// the reference's cylinder runs for the ST's KSP (.examples/eigenvalues.py:100; Sensitivity/__init__.py:182,260).
//
// Layout (analysis: nd_symbolic.hip).  Tree node t owns m unknowns and has a boundary of b unknowns of its ancestors; its
// front F_t is (m + b)^2.  What stays resident in HBM after the factorisation is PACKED, m^2 + 2 m b scalars per node:
//     L_t = [ F11^-1 ; -F21 F11^-1 ]   (f x m, row-major)        U_t = F11^-1 F12   (m x b, row-major)
// so that a solve is two sweeps over the tree in which every node is ONE dense mat-vec per sweep:
//     up   (leaves -> roots):  v = b[own] + children's updates;  [y[own]; update_t - carried] = L_t v
//     down (roots -> leaves):  x[own] = y[own] - U_t x[boundary]
// The full front exists only while its node is being factored: the nodes of a tree level are factored in CHUNKS whose
// working fronts (f^2 each) share one arena; the update matrix F22 - F21 F11^-1 F12 (b^2) a node hands to its parent lives
// in a second arena from the node's chunk to its parent's (offsets from a first-fit allocator run over the chunk order at
// analysis time).  Device memory is therefore sum(m^2 + 2 m b) + one chunk's fronts + the live update matrices, not
// sum(f^2): what lets the 3D cases beyond a million unknowns fit (round 2 kept every front whole: 40-60 % dead storage).
// All nodes of a tree level run in one launch per sweep: 2 * (levels) - 1 dependent launches per solve -- two fewer where the
// root and its children are swept as one assembled inverse (NdTop below).
//
// Sweeps without index chasing: the iteration's vectors are kept in the elimination order (a node's own unknowns are
// contiguous: the caller orders the matrix by lsa_nd_order and hands the tree back), children PUSH their update entries
// into per-child slot rows of the parent (fixed slots: bitwise repeatable, no atomics) and parents push the solution
// entries a child's boundary needs into the child's boundary vector, so every gather on a kernel's critical path is a
// contiguous load whose address depends on the node record only; index tables (cmap, gell) feed stores.
//
// Pivoting: rows are chosen by magnitude inside the pivot block of each front and never physically interchanged (the
// permutation is undone once, when the inverse is gathered).  A pivot below 1e-15 * max|C| is reported as
// LSA_ERR_ZERO_PIVOT; the operator layer (solver.hip) verifies every solve against b - C x.
//
// This file: the set-up of the device tables and buffers from the analysis (nd_setup and its steps, nd_setup_top), the
// cache of the last analysis, the C-ABI.  ndlu_factor.hip: the numeric factorisation.  ndlu_sweeps.hip: the solves.
// ndlu_internal.h: the records and tables the three share.
#include "ndlu_internal.h"

namespace {

void nd_free(lsa_ndlu* f) {
    if (!f) return;
    ndlu_multi_free(f);
    for (void* p : {f->d_top, (void*)f->d_top_rec, (void*)f->d_top_icmap, (void*)f->d_top_jobs, (void*)f->d_top_tiles})
        if (p) (void)hipFree(p);
    for (void* p : {(void*)f->d_lnodes_bwd, (void*)f->d_dist_nodes, (void*)f->d_child_ptr, (void*)f->d_child_idx, f->d_xstage, f->d_xg, (void*)f->d_tgoff, f->d_tg})
        if (p) (void)hipFree(p);
    for (void* p : {(void*)f->d_nodes, (void*)f->d_lnodes, (void*)f->d_gell, (void*)f->d_idx, (void*)f->d_cmap, (void*)f->d_tiles,
                    (void*)f->d_chunk_nodes, (void*)f->d_asm_dst, (void*)f->d_asm_src, (void*)f->d_ipiv, (void*)f->d_rowq, (void*)f->d_flag, (void*)f->d_xflag, (void*)f->d_maxabs,
                    f->d_lfac, f->d_ufac, f->d_work, f->d_upd, f->d_ubuf, f->d_xb, f->d_acc, f->d_tmp, f->d_ybuf, (void*)f->d_cand[0], (void*)f->d_cand[1], f->d_dinv})
        if (p) (void)hipFree(p);
    if (f->ev_panel) (void)hipEventDestroy(f->ev_panel);
    if (f->ev_pivots) (void)hipEventDestroy(f->ev_pivots);
    if (f->side) (void)hipStreamDestroy(f->side);
    delete f;
}

// The merged top (NdTop): decided once per analysis.  Eligible: one rank, vectors in elimination order, one root that is alone
// on the last level, and the level below it holds exactly the root's children, none of them a leaf, all with slot rows; at
// most LSA_ND_TOPINV unknowns in all (0 = off).  Anything else keeps the launch per level and direction.
int nd_setup_top(lsa_ctx* ctx, lsa_ndlu* f, const std::vector<NdNodeDev>& nodes) {
    const NdSymbolic& S = f->S;
    f->top = NdTop{};
    f->top_level = -1;
    // (default: the widest top measured -- 739 / 608 / 1203 unknowns at 5 k / 30 k / 121 k unknowns, each faster per apply and per
    //  factorisation + 184 applies)
    static const int32_t limit = getenv("LSA_ND_TOPINV") && *getenv("LSA_ND_TOPINV") ? std::max(0, atoi(getenv("LSA_ND_TOPINV"))) : 1280;
    if (limit <= 0 || S.nranks != 1 || S.has_dist || !f->ordered || S.nlevels < 3) return LSA_OK;
    const int32_t lr = S.nlevels - 1;
    if (S.lvl_ptr[(size_t)lr + 1] - S.lvl_ptr[(size_t)lr] != 1) return LSA_OK;
    const int32_t R = S.lvl_nodes[(size_t)S.lvl_ptr[(size_t)lr]];
    int32_t roots = 0;
    for (int32_t t = 0; t < S.nt; ++t) roots += S.parent[(size_t)t] < 0;
    const int32_t c0 = S.child_ptr[(size_t)R], K = S.child_ptr[(size_t)R + 1] - c0, mR = S.m[(size_t)R];
    if (roots != 1 || S.parent[(size_t)R] >= 0 || S.f[(size_t)R] != mR || K < 1 || K > kTopChildren) return LSA_OK;
    if (S.lvl_ptr[(size_t)lr] - S.lvl_ptr[(size_t)lr - 1] != K) return LSA_OK;
    NdTop tp = {};
    tp.nchild = K;
    int64_t s = 0, replaced = (int64_t)mR * mR;
    for (int32_t ci = 0; ci < K; ++ci) {
        const int32_t c = S.child_idx[(size_t)c0 + ci];
        const NdNodeDev& nd = nodes[(size_t)c];
        bool on_level = false;
        for (int32_t q = S.lvl_ptr[(size_t)lr - 1]; q < S.lvl_ptr[(size_t)lr]; ++q) on_level |= S.lvl_nodes[(size_t)q] == c;
        if (!on_level || nd.nchild < 1 || nd.acc_off < 0 || nd.f <= nd.m || nd.m < 1 || S.kind[(size_t)c] == 3 || S.kind[(size_t)c] == 4) return LSA_OK;
        tp.node[ci] = NdTopNode{nd.acc_off, nd.ge_off, nd.own0, nd.m, nd.f, nd.nchild, (int32_t)s, 0};
        s += nd.m;
        replaced += (int64_t)nd.m * nd.m + 2 * (int64_t)nd.m * (nd.f - nd.m);
    }
    const NdNodeDev& nr = nodes[(size_t)R];
    tp.node[K] = NdTopNode{nr.acc_off, nr.ge_off, nr.own0, mR, mR, K, (int32_t)s, 0};
    s += mR;
    if (s > limit) return LSA_OK;
    tp.s = (int32_t)s;
    std::vector<int32_t> icmap((size_t)K * mR, -1);
    for (int32_t ci = 0; ci < K; ++ci) {
        const int32_t c = S.child_idx[(size_t)c0 + ci];
        for (int32_t p = 0; p < S.f[(size_t)c] - S.m[(size_t)c]; ++p) {
            const int32_t k = S.cmap[(size_t)S.cmap_off[(size_t)c] + p];
            if (k < 0 || k >= mR) return LSA_OK;  // (cannot happen under a root without boundary)
            icmap[(size_t)ci * mR + k] = p;
        }
    }
    // the assembly: launch 1 = inv_R, -Q_c = -U_c inv_R[cmap_c, :], P_c = inv_R[:, cmap_c] s1_c; launch 2 = the children's blocks
    std::vector<NdTopJob> jobs;
    std::vector<int32_t> tiles;
    auto add = [&](const NdTopJob& jb) {
        for (int32_t ti = 0; ti < (jb.M + 31) / 32; ++ti)
            for (int32_t tj = 0; tj < (jb.N + 31) / 32; ++tj) {
                tiles.push_back((int32_t)jobs.size());
                tiles.push_back((ti << 16) | tj);
            }
        jobs.push_back(jb);
    };
    const int64_t oR = tp.node[K].off;
    add(NdTopJob{0, 0, oR * s + oR, nr.lfac_off, mR, mR, 0, 1, 1, mR, 0, 0, 0, 0});
    for (int32_t ci = 0; ci < K; ++ci) {
        const NdNodeDev& nd = nodes[(size_t)S.child_idx[(size_t)c0 + ci]];
        const int32_t m = nd.m, b = nd.f - nd.m;
        const int64_t o = tp.node[ci].off;
        add(NdTopJob{nd.ufac_off, nr.lfac_off, o * s + oR, -1, m, mR, b, b, mR, 0, 1, 2, nd.cmap_off, 1});
        add(NdTopJob{nr.lfac_off, nd.lfac_off + (int64_t)m * m, oR * s + o, -1, mR, m, b, mR, m, 0, 0, 1, nd.cmap_off, 0});
    }
    f->top_tiles[0] = (int32_t)tiles.size() / 2;
    for (int32_t ci = 0; ci < K; ++ci)
        for (int32_t di = 0; di < K; ++di) {
            const NdNodeDev &nc = nodes[(size_t)S.child_idx[(size_t)c0 + ci]], &nd = nodes[(size_t)S.child_idx[(size_t)c0 + di]];
            add(NdTopJob{tp.node[ci].off * s + oR, nd.lfac_off + (int64_t)nd.m * nd.m, tp.node[ci].off * s + tp.node[di].off, ci == di ? nc.lfac_off : -1, nc.m,
                         nd.m, nd.f - nd.m, (int32_t)s, nd.m, nc.m, 2, 1, nd.cmap_off, 0});
        }
    f->top_tiles[1] = (int32_t)tiles.size() / 2 - f->top_tiles[0];
    LSA_CHECK(upload(ctx, icmap, &f->d_top_icmap));
    LSA_CHECK(upload(ctx, jobs, &f->d_top_jobs));
    LSA_CHECK(upload(ctx, tiles, &f->d_top_tiles));
    LSA_HIP_ALLOC(ctx, hipMalloc(&f->d_top, (size_t)(s * s) * esize(f->dtype)));
    LSA_CHECK(upload(ctx, std::vector<NdTop>(1, tp), &f->d_top_rec));
    f->top = tp;
    f->top_level = lr;
    f->top_replaced_entries = replaced;
    f->solve_launches -= 2;
    return LSA_OK;
}

// ---- nd_setup, step by step (in the order nd_setup calls them) ----

// the tile lists of all chunks share one buffer of (node or job, tile) pairs
struct TileBuffer {
    std::vector<int32_t> tiles;
    void begin(TileList& tl) {
        tl.off = (int64_t)tiles.size() / 2;
        tl.count = 0;
    }
    void push(TileList& tl, int32_t a, int32_t b) {
        tiles.push_back(a);
        tiles.push_back(b);
        ++tl.count;
    }
};

// the thresholds of the factorisation's paths, read at every set-up
void nd_setup_knobs(lsa_ndlu* f) {
    const char* e = getenv("LSA_ND_TP_MIN");
    f->tp_min = e && *e ? std::max(1, atoi(e)) : 512;  // (measured: S500k 46.4 ms at 384, 44.5 at 512, 47.2 at 640, 62.6 at 1024; 3D cases indifferent)
    const char* sbm = getenv("LSA_ND_SB_MIN");
    f->sb_min = std::max(f->tp_min, sbm && *sbm ? std::max(1, atoi(sbm)) : 1024);
    f->ycap = kNB;
    const char* sbc = getenv("LSA_ND_SB_COLS");
    f->sb_cols = sbc && *sbc ? std::min(1024, std::max(kGT, atoi(sbc) / kGT * kGT)) : kSB;
    // unset: staging in the finishing launch, S1 and S2 in one launch, 16-column panels in the instances where they measured
    // faster;  16: the same with 16-column panels in every instance that has them (up to 512 rows);  8: the launch sequence
    // before all of that (A/B runs in one library, tests/test_gpu_gj_panels.py)
    const char* gp = getenv("LSA_ND_GJ_PANEL");
    const int gpv = gp && *gp ? atoi(gp) : 0;
    f->gj_panel = gpv == 8 || gpv == 16 ? gpv : 0;
}

// whether the matrix came in elimination order (a node's own unknowns are own0, own0 + 1, ...)
bool nd_setup_ordered(const NdSymbolic& S) {
    const bool dist = S.nranks > 1;
    bool ordered = true;
    for (size_t k = 0; k < S.perm.size() && ordered; ++k) ordered = S.perm[k] == (int32_t)k || dist;
    if (dist)  // a tree given by the caller owns contiguous index ranges: own0 = the first of them (the padded layout has holes)
        for (int32_t t = 0; t < S.nt && ordered; ++t)
            for (int32_t r = 1; r < S.m[(size_t)t]; ++r)
                if (S.idx[(size_t)S.idx_off[(size_t)t] + r] != S.idx[(size_t)S.idx_off[(size_t)t]] + r) {
                    ordered = false;
                    break;
                }
    return ordered;
}

// scalars the working arena may take: a level is factored in one go while its fronts fit a quarter of what the packed factors
// leave free (LSA_ND_WORK_MB overrides); a single front always has to fit
int64_t nd_setup_budget(const NdSymbolic& S, size_t es, int64_t free_agreed) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)16 << 30;
    const int64_t after = (int64_t)free_b - S.factor_entries * (int64_t)es;
    int64_t budget = std::max<int64_t>(after / 4, (int64_t)256 << 20) / (int64_t)es;
    // (distributed top nodes: a figure every rank computes alike -- a sixth of the smallest free memory of all ranks)
    if (S.has_dist) budget = std::max<int64_t>((free_agreed > 0 ? free_agreed : (int64_t)free_b) / 6, (int64_t)256 << 20) / (int64_t)es;
    if (const char* e = getenv("LSA_ND_WORK_MB")) budget = std::max<int64_t>(atoll(e), 1) * (1 << 20) / (int64_t)es;
    return budget;
}

// the node records of the factorisation, by node id: every kept node, the other ranks' subtree roots included (they are children here)
std::vector<NdNodeDev> nd_setup_nodes(const NdSymbolic& S, const NdMemoryPlan& P) {
    std::vector<NdNodeDev> nodes((size_t)S.nt);
    for (int32_t t = 0; t < S.nt; ++t) {
        NdNodeDev& nd = nodes[(size_t)t];
        nd.front_off = P.work_off[(size_t)t];
        nd.lfac_off = P.lfac_off[(size_t)t];
        nd.ufac_off = P.ufac_off[(size_t)t];
        nd.upd_off = P.upd_off[(size_t)t];
        nd.u_off = S.u_off[(size_t)t];
        nd.ge_off = S.ge_off[(size_t)t];
        nd.acc_off = P.acc_off[(size_t)t];
        nd.pacc_off = P.pacc_off[(size_t)t];
        nd.idx_off = (int32_t)S.idx_off[(size_t)t];
        nd.cmap_off = S.cmap_off[(size_t)t];
        nd.piv_off = S.piv_off[(size_t)t];
        nd.own0 = S.m[(size_t)t] > 0 ? S.idx[(size_t)S.idx_off[(size_t)t]] : 0;
        nd.m = S.m[(size_t)t];
        nd.f = S.f[(size_t)t];
        nd.parent = S.parent[(size_t)t];
        nd.nchild = S.child_ptr[(size_t)t + 1] - S.child_ptr[(size_t)t];
        nd.brow0 = S.brow0[(size_t)t];
        nd.brow = S.brow[(size_t)t];
        nd.orow0 = S.orow0[(size_t)t];
        nd.orows = S.orows[(size_t)t];
        nd.flags = S.kind[(size_t)t] == 4 ? 1 : 0;
        nd.pad0 = 0;
        nd.xg_base = S.xg_base[(size_t)t];
        nd.xg_stride = S.xg_stride[(size_t)t];
        // (the plan's working block of a distributed node: its slice of the front at the widest slice of any rank, then the inverse)
        nd.inv_off = S.kind[(size_t)t] == 4
                         ? nd.front_off + (int64_t)(S.m[(size_t)t] + nd_slice_width(S.f[(size_t)t] - S.m[(size_t)t], S.nranks)) * S.f[(size_t)t]
                         : -1;
    }
    return nodes;
}

// the chunks of the plan (they cut the levels' node lists, S.lvl_nodes); chunk_of: per node, its chunk
std::vector<NdChunk> nd_setup_chunks(const NdSymbolic& S, const NdMemoryPlan& P, std::vector<int32_t>& chunk_of) {
    std::vector<NdChunk> chunks;
    chunk_of.assign((size_t)S.nt, -1);
    for (size_t c = 0; c + 1 < P.chunk_begin.size(); ++c) {
        NdChunk ch;
        ch.node_begin = P.chunk_begin[c];
        ch.node_count = P.chunk_begin[c + 1] - P.chunk_begin[c];
        ch.work_entries = P.chunk_work[c];
        ch.exchange_before = P.chunk_exchange_before[c] != 0;
        for (int32_t q = 0; q < ch.node_count; ++q) {
            const int32_t t = S.lvl_nodes[(size_t)ch.node_begin + q];
            ch.max_m = std::max(ch.max_m, S.m[(size_t)t]);
            ch.max_f = std::max(ch.max_f, S.f[(size_t)t]);
            ch.sorted_m.push_back(S.m[(size_t)t]);
            chunk_of[(size_t)t] = (int32_t)c;
        }
        chunks.push_back(std::move(ch));
    }
    return chunks;
}

// assembly lists by chunk: front_buffer[work offset] = values[asm_src].  Sets the chunks' ranges of the lists and uploads them.
int nd_setup_assembly(lsa_ctx* ctx, lsa_ndlu* f, const std::vector<NdNodeDev>& nodes, const std::vector<int32_t>& chunk_of) {
    NdSymbolic& S = f->S;
    std::vector<std::pair<int64_t, int32_t>> by_off;  // (offset of the node's front in the analysis' logical layout, node)
    by_off.reserve((size_t)S.nt);
    for (int32_t t = 0; t < S.nt; ++t) by_off.emplace_back(S.front_off[(size_t)t], t);
    std::sort(by_off.begin(), by_off.end());
    const size_t ne = S.asm_src.size();
    std::vector<int32_t> node_of_entry(ne);
    std::vector<int64_t> count(f->chunks.size() + 1, 0);
    for (size_t e = 0; e < ne; ++e) {
        auto it = std::upper_bound(by_off.begin(), by_off.end(), std::make_pair(S.asm_dst[e], (int32_t)0x7fffffff));
        const int32_t t = (it - 1)->second;
        node_of_entry[e] = t;
        ++count[(size_t)chunk_of[(size_t)t] + 1];
    }
    for (size_t c = 0; c < f->chunks.size(); ++c) {
        f->chunks[c].asm_begin = count[c];
        f->chunks[c].asm_count = count[c + 1];
        count[c + 1] += count[c];
    }
    std::vector<int32_t> src(ne);
    std::vector<int64_t> dst(ne);
    std::vector<int64_t> fill(count.begin(), count.end() - 1);
    for (size_t e = 0; e < ne; ++e) {
        const int32_t t = node_of_entry[e];
        const int64_t at = fill[(size_t)chunk_of[(size_t)t]]++;
        src[(size_t)at] = S.asm_src[e];
        dst[(size_t)at] = nodes[(size_t)t].front_off + (S.asm_dst[e] - S.front_off[(size_t)t]);
    }
    f->asm_count = (int64_t)ne;
    LSA_CHECK(upload(ctx, dst, &f->d_asm_dst));
    LSA_CHECK(upload(ctx, src, &f->d_asm_src));
    // (the analysis' own copies are not needed again: the refactorisations walk the device lists)
    std::vector<int32_t>().swap(S.asm_src);
    std::vector<int64_t>().swap(S.asm_dst);
    return LSA_OK;
}

// The TM x TN tiles of one large product of node t, appended to `tl` in an order made for the 8 XCDs: consecutive workgroups go
// to the XCDs in turn (launch index mod 8 labels the workgroups that share an L2), and row-major order would hand every L2 one
// tile in eight of a dozen tile rows -- each workgroup then streams its own 64 x K and K x 64 panels, 8 flops per byte from
// beyond the L2.  Here the workgroups of one label stay inside one band of tile rows and walk it in super-tiles of 8 x 16 tiles
// (about what an XCD holds in flight): at any k they share 8 + 16 panel chunks instead of reading 2 x 128.
void nd_push_xcd_order(TileBuffer& tb, TileList& tl, int32_t t, int32_t TM, int32_t TN) {
    std::vector<int32_t> seq[8];
    for (int x = 0; x < 8; ++x) {
        const int32_t r0 = (int32_t)((int64_t)TM * x / 8), r1 = (int32_t)((int64_t)TM * (x + 1) / 8);
        if (r1 <= r0) continue;
        const int32_t sh = std::min(r1 - r0, 8), sw = std::max(1, 128 / sh);
        for (int32_t rb = r0; rb < r1; rb += sh)
            for (int32_t cb = 0; cb < TN; cb += sw)
                for (int32_t r = rb; r < std::min(rb + sh, r1); ++r)
                    for (int32_t cc = cb; cc < std::min(cb + sw, TN); ++cc) seq[x].push_back((r << 16) | cc);
    }
    size_t pos[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t left = (int64_t)TM * TN; left > 0; --left) {
        int x = (int)(tl.count % 8);
        for (int tries = 0; tries < 8 && pos[x] >= seq[x].size(); ++tries) x = (x + 1) % 8;  // (a band ran out: help the next)
        tb.push(tl, t, seq[x][pos[x]++]);
    }
}

// the tile lists of one chunk's launches: extend-add, un-permutation, the three products, the update matrices' way out
void nd_setup_chunk_tiles(const NdSymbolic& S, NdChunk& c, TileBuffer& tb) {
    auto node = [&](int32_t q) { return S.lvl_nodes[(size_t)c.node_begin + q]; };
    int32_t lvl_children = 0;
    for (int32_t q = 0; q < c.node_count; ++q) lvl_children = std::max(lvl_children, S.child_ptr[(size_t)node(q) + 1] - S.child_ptr[(size_t)node(q)]);
    // extend-add: one list per child rank (children of one parent never share a launch)
    c.ext.assign((size_t)lvl_children, TileList());
    for (int32_t r = 0; r < lvl_children; ++r) {
        tb.begin(c.ext[(size_t)r]);
        for (int32_t q = 0; q < c.node_count; ++q) {
            const int32_t t = node(q);
            if (S.child_ptr[(size_t)t] + r >= S.child_ptr[(size_t)t + 1]) continue;
            const int32_t ch = S.child_idx[(size_t)S.child_ptr[(size_t)t] + r];
            // (the update matrices of a distributed node's children travel through the staging buffer, nd_setup_chunk_xsteps --
            //  except a replicated child's, which every rank holds whole)
            if (S.kind[(size_t)t] == 4 && S.kind[(size_t)ch] != 2) continue;
            const int32_t bc = S.f[(size_t)ch] - S.m[(size_t)ch];
            for (int32_t i0 = 0; i0 < bc; i0 += 16) tb.push(c.ext[(size_t)r], ch, i0);
        }
    }
    tb.begin(c.unperm);
    for (int32_t q = 0; q < c.node_count; ++q)
        for (int32_t r0 = 0; r0 < S.m[(size_t)node(q)]; r0 += 16) tb.push(c.unperm, node(q), r0);
    static const bool xcd_order = !(getenv("LSA_ND_XCD_ORDER") && atoi(getenv("LSA_ND_XCD_ORDER")) == 0);  // (A/B measurement aid)
    for (int kind = 0; kind < 3; ++kind) {
        tb.begin(c.gemm[kind]);
        for (int32_t q = 0; q < c.node_count; ++q) {
            const int32_t t = node(q);
            const int32_t m = S.m[(size_t)t], b = S.f[(size_t)t] - m;
            if (b == 0) continue;
            // (a distributed node: this rank's boundary rows of L and of the update matrix, its own rows of U)
            const int32_t M = kind == 2 ? S.orows[(size_t)t] : S.brow[(size_t)t], N = kind == 0 ? m : b;
            if (M == 0) continue;
            const int32_t TM = (M + kGT - 1) / kGT, TN = (N + kGT - 1) / kGT;
            if ((int64_t)TM * TN >= 512 && xcd_order) {
                nd_push_xcd_order(tb, c.gemm[kind], t, TM, TN);
                continue;
            }
            for (int32_t tm = 0; tm < TM; ++tm)
                for (int32_t tn = 0; tn < TN; ++tn) tb.push(c.gemm[kind], t, (tm << 16) | tn);
        }
    }
    tb.begin(c.save);
    for (int32_t q = 0; q < c.node_count; ++q) {
        const int32_t t = node(q);
        for (int32_t r0 = 0; r0 < S.brow[(size_t)t]; r0 += 16) tb.push(c.save, t, r0);
    }
}

// the row chunks that reach a chunk's distributed nodes through the staging buffer: every rank works off its own queue (its
// slice of the rows of a distributed child, all rows of a subtree root it owns), one piece per step
void nd_setup_chunk_xsteps(const NdSymbolic& S, const NdMemoryPlan& P, NdChunk& c) {
    std::vector<std::vector<NdChunk::XPiece>> queue((size_t)S.nranks);
    for (int32_t q = 0; q < c.node_count; ++q) {
        const int32_t t = S.lvl_nodes[(size_t)c.node_begin + q];
        if (S.kind[(size_t)t] != 4) continue;
        for (int32_t cp = S.child_ptr[(size_t)t]; cp < S.child_ptr[(size_t)t + 1]; ++cp) {
            const int32_t ch = S.child_idx[(size_t)cp];
            if (S.kind[(size_t)ch] == 2) continue;
            const int32_t bc = S.f[(size_t)ch] - S.m[(size_t)ch];
            if (bc == 0) continue;
            const int32_t per = (int32_t)std::max<int64_t>(1, std::min<int64_t>(P.xstage_slot / bc, 1 << 30));
            for (int r = 0; r < S.nranks; ++r) {
                int32_t lo = 0, cnt = 0;
                if (S.kind[(size_t)ch] == 4) nd_slice(bc, S.nranks, r, &lo, &cnt);
                else if (S.owner[(size_t)ch] == r) cnt = bc;
                for (int32_t r0 = lo; r0 < lo + cnt; r0 += per) {
                    NdChunk::XPiece pc;
                    pc.child = ch, pc.row0 = r0, pc.nrows = std::min(per, lo + cnt - r0);
                    queue[(size_t)r].push_back(pc);
                }
            }
        }
    }
    size_t nsteps = 0;
    for (const auto& qv : queue) nsteps = std::max(nsteps, qv.size());
    c.xsteps.assign(nsteps, std::vector<NdChunk::XPiece>((size_t)S.nranks));
    for (size_t st = 0; st < nsteps; ++st)
        for (int r = 0; r < S.nranks; ++r)
            if (st < queue[(size_t)r].size()) c.xsteps[st][(size_t)r] = queue[(size_t)r][st];
}

// the sweeps' launches: one per tree level and direction, with the tile shape of each
int nd_setup_levels(lsa_ctx* ctx, lsa_ndlu* f) {
    const NdSymbolic& S = f->S;
    f->levels.assign((size_t)S.nlevels, NdLevel());
    for (int32_t l = 0; l < S.nlevels; ++l) {
        NdLevel& L = f->levels[(size_t)l];
        L.node_begin = S.lvl_ptr[(size_t)l];
        L.node_count = S.lvl_ptr[(size_t)l + 1] - L.node_begin;
        // the sweeps wait for memory: a level whose fronts make fewer 32-row tiles than a few per CU gets 8-row tiles (64 lanes
        // along a row pair).  Upwards only where the level's pivot blocks fill those lanes: a row of the packed L has m entries, and
        // under pivot blocks narrower than `wide` the 8-row tiles are four times the workgroups (several rounds of them, half of
        // them without a row where the fronts differ in height) for one factor scalar per lane or none.  A row of the packed U
        // has f - m entries: downwards the 8-row tiles stay.
        int64_t tiles32 = 0;
        for (int32_t q = 0; q < L.node_count; ++q) {
            const int32_t t = S.lvl_nodes[(size_t)L.node_begin + q];
            tiles32 += (S.orows[(size_t)t] + S.brow[(size_t)t] + kRT - 1) / kRT;
            L.max_m = std::max(L.max_m, S.m[(size_t)t]);
            L.max_f = std::max(L.max_f, S.f[(size_t)t]);
        }
        static const int64_t few = getenv("LSA_ND_SWEEP_FEW") ? atoll(getenv("LSA_ND_SWEEP_FEW")) : 4 * (int64_t)ctx->num_cu;
        // thin separators (pivot blocks of a few dozen unknowns under fronts of a few hundred rows): the upward sweep reads
        // f short rows per node; four lanes per row pair and 128 rows per workgroup gather the node's vector 1/4 as often
        static const int32_t thin = getenv("LSA_ND_SWEEP_THIN") ? atoi(getenv("LSA_ND_SWEEP_THIN")) : 64;
        // (64-row tiles -- NP = 2 of nd_fwd_kernel -- on the leaf level of the 500 k-unknown forest, 42 000 tiles: 900 us per solve
        //  against 886 with 32-row tiles: no gain from sharing the gather, measured round 3)
        static const int32_t wide = getenv("LSA_ND_SWEEP_WIDE") ? atoi(getenv("LSA_ND_SWEEP_WIDE")) : kSweepWide;
        L.bwd_rows = tiles32 <= few ? 8 : kRT;
        L.sweep_rows = tiles32 <= few ? (L.max_m >= wide ? 8 : kRT) : (L.max_m <= thin && l > 0) ? 128 : kRT;
        for (int32_t q = 0; q < L.node_count; ++q) {
            const int32_t t = S.lvl_nodes[(size_t)L.node_begin + q];
            L.fwd_tiles = std::max(L.fwd_tiles, (S.orows[(size_t)t] + S.brow[(size_t)t] + L.sweep_rows - 1) / L.sweep_rows);
            // (the downward sweep of a thin level has few, long rows: 32-row tiles)
            if (S.f[(size_t)t] > S.m[(size_t)t]) L.bwd_tiles = std::max(L.bwd_tiles, (S.orows[(size_t)t] + L.bwd_rows - 1) / L.bwd_rows);
        }
        if (L.fwd_tiles > 65535) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu: a front of more than %d rows is not supported", 65535 * 8);
    }
    return LSA_OK;
}

// The sweeps' records, in level order, and the levels' distributed nodes with their exchange regions.  A distributed node
// differs from its factorisation record: upwards its update entries go to its rank's slot of the level's exchange region;
// downwards it appears as its slice of the own rows (the pushes to its children are nd_dist_unpack_kernel's, after the exchange)
int nd_setup_sweep_records(lsa_ctx* ctx, lsa_ndlu* f, const std::vector<NdNodeDev>& nodes) {
    const NdSymbolic& S = f->S;
    std::vector<NdSweepNode> lnodes(S.lvl_nodes.size()), bnodes(S.lvl_nodes.size());
    std::vector<int32_t> dist_nodes;
    for (size_t q = 0; q < S.lvl_nodes.size(); ++q) {
        const int32_t t = S.lvl_nodes[q];
        lnodes[q] = bnodes[q] = NdSweepNode(nodes[(size_t)t]);
        if (S.kind[(size_t)t] != 4) continue;
        lnodes[q].u_off = S.ux_base[(size_t)t] + (int64_t)S.rank * S.ux_stride[(size_t)t];
        NdSweepNode& bn = bnodes[q];
        const int32_t b = bn.f - bn.m;
        bn.idx_off += bn.orow0;
        bn.own0 += bn.orow0;
        bn.m = bn.orows;
        bn.f = bn.orows + b;
        bn.nchild = 0;
    }
    for (int32_t l = 0; l < S.nlevels; ++l) {
        NdLevel& L = f->levels[(size_t)l];
        L.dist_begin = (int32_t)dist_nodes.size();
        for (int32_t q = 0; q < L.node_count; ++q) {
            const int32_t t = S.lvl_nodes[(size_t)L.node_begin + q];
            if (S.kind[(size_t)t] != 4) continue;
            if (L.dist_count == 0) {
                L.ux_base = S.ux_base[(size_t)t], L.ux_slot = S.ux_stride[(size_t)t];
                L.xg_base = S.xg_base[(size_t)t], L.xg_slot = S.xg_stride[(size_t)t];
            }
            L.ux_base = std::min(L.ux_base, S.ux_base[(size_t)t]);
            L.xg_base = std::min(L.xg_base, S.xg_base[(size_t)t]);
            ++L.dist_count;
            dist_nodes.push_back(t);
            L.dist_children = std::max(L.dist_children, S.child_ptr[(size_t)t + 1] - S.child_ptr[(size_t)t]);
            L.dist_rows = std::max(L.dist_rows, S.m[(size_t)t]);
            for (int32_t cp = S.child_ptr[(size_t)t]; cp < S.child_ptr[(size_t)t + 1]; ++cp) {
                const int32_t ch = S.child_idx[(size_t)cp];
                L.dist_rows = std::max(L.dist_rows, S.f[(size_t)ch] - S.m[(size_t)ch]);
            }
        }
    }
    LSA_CHECK(upload(ctx, lnodes, &f->d_lnodes));
    LSA_CHECK(upload(ctx, bnodes, &f->d_lnodes_bwd));
    LSA_CHECK(upload(ctx, dist_nodes, &f->d_dist_nodes));
    LSA_CHECK(upload(ctx, S.child_ptr, &f->d_child_ptr));
    LSA_CHECK(upload(ctx, S.child_idx, &f->d_child_idx));
    if (f->xstage_slot > 0) LSA_HIP_ALLOC(ctx, hipMalloc(&f->d_xstage, (size_t)f->xstage_slot * (size_t)S.nranks * esize(f->dtype)));
    if (S.xg_entries > 0) LSA_HIP_ALLOC(ctx, hipMalloc(&f->d_xg, (size_t)S.xg_entries * 16));
    return LSA_OK;
}

// the index tables and every buffer of the factorisation and the sweeps; widest_tp: most nodes of a chunk on the tournament path
int nd_setup_buffers(lsa_ctx* ctx, lsa_ndlu* f, const std::vector<int32_t>& tiles, int32_t widest_tp) {
    const NdSymbolic& S = f->S;
    const size_t es = esize(f->dtype);
    LSA_CHECK(upload(ctx, S.gell, &f->d_gell));
    LSA_CHECK(upload(ctx, S.idx, &f->d_idx));
    LSA_CHECK(upload(ctx, S.cmap, &f->d_cmap));
    LSA_CHECK(upload(ctx, S.lvl_nodes, &f->d_chunk_nodes));  // node ids in chunk order: the chunks cut the levels' lists
    LSA_CHECK(upload(ctx, tiles, &f->d_tiles));
    const size_t nn = (size_t)std::max<int32_t>(S.n, 1);
    LSA_HIP_ALLOC(ctx, hipMalloc((void**)&f->d_ipiv, nn * sizeof(int32_t)));
    LSA_HIP_ALLOC(ctx, hipMalloc((void**)&f->d_rowq, nn * sizeof(int32_t)));
    LSA_HIP_ALLOC(ctx, hipMalloc((void**)&f->d_flag, 4 * sizeof(int32_t)));
    LSA_HIP_ALLOC(ctx, hipMalloc((void**)&f->d_maxabs, sizeof(unsigned long long)));
    LSA_HIP_ALLOC(ctx, hipMalloc(&f->d_lfac, (size_t)std::max<int64_t>(f->lfac_entries, 1) * es));
    LSA_HIP_ALLOC(ctx, hipMalloc(&f->d_ufac, (size_t)std::max<int64_t>(f->ufac_entries, 1) * es));
    LSA_HIP_ALLOC(ctx, hipMalloc(&f->d_work, (size_t)f->work_entries * es));
    LSA_HIP_ALLOC(ctx, hipMalloc(&f->d_upd, (size_t)f->upd_entries * es));
    const size_t ub = (size_t)std::max<int64_t>(S.u_off[(size_t)S.nt], 1) * 16;
    LSA_HIP_ALLOC(ctx, hipMalloc(&f->d_ubuf, ub));
    LSA_HIP_ALLOC(ctx, hipMalloc(&f->d_xb, ub));
    LSA_HIP_ALLOC(ctx, hipMalloc(&f->d_acc, (size_t)std::max<int64_t>(f->acc_entries, 1) * 16));
    // slots no child maps to are read by every solve and written by none: zero, once
    LSA_HIP_CHECK(ctx, hipMemsetAsync(f->d_acc, 0, (size_t)std::max<int64_t>(f->acc_entries, 1) * 16, ctx->stream));
    LSA_HIP_CHECK(ctx, hipMemsetAsync(f->d_ubuf, 0, ub, ctx->stream));
    LSA_HIP_CHECK(ctx, hipMemsetAsync(f->d_xb, 0, ub, ctx->stream));
    LSA_HIP_ALLOC(ctx, hipMalloc(&f->d_tmp, nn * 16));
    LSA_HIP_ALLOC(ctx, hipMalloc(&f->d_ybuf, nn * (size_t)f->ycap * es));
    if (widest_tp > 0) {
        const size_t cand = ((size_t)S.n / kTRmin + (size_t)S.nt + 1) * kNB * sizeof(int32_t);
        LSA_HIP_ALLOC(ctx, hipMalloc((void**)&f->d_cand[0], cand));
        LSA_HIP_ALLOC(ctx, hipMalloc((void**)&f->d_cand[1], cand));
        LSA_HIP_ALLOC(ctx, hipMalloc(&f->d_dinv, (size_t)widest_tp * kNB * kNB * es));
        const char* la = getenv("LSA_ND_LOOKAHEAD");
        if (!(la && *la && atoi(la) == 0)) {
            // highest priority: the tournament's few workgroups must not queue behind the thousands of the product they
            // run under
            int lo_pri = 0, hi_pri = 0;
            LSA_HIP_CHECK(ctx, hipDeviceGetStreamPriorityRange(&lo_pri, &hi_pri));
            LSA_HIP_CHECK(ctx, hipStreamCreateWithPriority(&f->side, hipStreamNonBlocking, hi_pri));
            LSA_HIP_CHECK(ctx, hipEventCreateWithFlags(&f->ev_panel, hipEventDisableTiming));
            LSA_HIP_CHECK(ctx, hipEventCreateWithFlags(&f->ev_pivots, hipEventDisableTiming));
        }
    }
    return LSA_OK;
}

// device tables, the memory plan (packed factors, chunks of working fronts, update arena) and tile lists from the analysis
// free_agreed: > 0 = the device memory every rank of a forest cut over ranks has free (the smallest of them): with distributed
// top nodes the chunks of the top levels carry collectives and must come out alike on every rank
int nd_setup(lsa_ctx* ctx, lsa_ndlu* f, int64_t free_agreed = 0) {
    NdSymbolic& S = f->S;
    nd_setup_knobs(f);
    // (the status word of the subtree-parallel form first: ranks agree on a failed set-up through it, lsa_ndlu_create_tree)
    LSA_HIP_ALLOC(ctx, hipMalloc((void**)&f->d_xflag, 4 * sizeof(int32_t) * (size_t)std::max(1, S.nranks)));
    f->ordered = nd_setup_ordered(S);
    // the memory plan (nd_symbolic.hip: host arithmetic on the analysis, also what lsa_nd_sym_memory reports)
    const int64_t budget = nd_setup_budget(S, esize(f->dtype), free_agreed);
    if (getenv("LSA_ND_TEST_OOM"))  // test aid: rehearses the one failure the operator layer answers by a leaner method
        return lsa_set_error(ctx, LSA_ERR_OOM, "lsa_ndlu: out of device memory (forced by LSA_ND_TEST_OOM)");
    NdMemoryPlan P;
    nd_memory_plan(S, budget, P);
    const std::vector<NdNodeDev> nodes = nd_setup_nodes(S, P);
    f->xstage_slot = P.xstage_slot;
    f->h_upd_off = P.upd_off;
    f->h_lfac_off = P.lfac_off;
    f->lfac_entries = P.lfac_entries;
    f->ufac_entries = P.ufac_entries;
    f->acc_entries = P.acc_entries;
    f->work_entries = P.work_entries;
    f->upd_entries = P.upd_entries;
    f->xupd_slot = P.xupd_slot;
    std::vector<int32_t> chunk_of;
    f->chunks = nd_setup_chunks(S, P, chunk_of);
    LSA_CHECK(nd_setup_assembly(ctx, f, nodes, chunk_of));
    TileBuffer tb;
    int32_t widest_tp = 0;
    for (NdChunk& c : f->chunks) {
        nd_setup_chunk_tiles(S, c, tb);
        nd_setup_chunk_xsteps(S, P, c);
        if (c.max_m > 16384 && c.max_m < f->tp_min)  // (the tournament path has no such limit)
            return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu: a pivot block of %d rows exceeds the 16 384 the panel kernels hold in registers (LSA_ND_TP_MIN = %d)",
                                 c.max_m, f->tp_min);
        if (c.max_m >= f->tp_min) widest_tp = std::max(widest_tp, c.node_count);
        if (c.max_m >= f->sb_min) f->ycap = f->sb_cols;
    }
    LSA_CHECK(nd_setup_levels(ctx, f));
    LSA_CHECK(upload(ctx, nodes, &f->d_nodes));
    LSA_CHECK(nd_setup_sweep_records(ctx, f, nodes));
    LSA_CHECK(nd_setup_buffers(ctx, f, tb.tiles, widest_tp));
    f->solve_launches = 0;
    for (const NdLevel& L : f->levels) f->solve_launches += (L.fwd_tiles > 0) + (L.bwd_tiles > 0);
    LSA_CHECK(nd_setup_top(ctx, f, nodes));
    return LSA_OK;
}

// A new factorisation object: `analyse(S, err, errlen)` fills its analysis (out of host memory there is an error like any of its
// own; `who` names the entry in that message), nd_setup makes the device tables and buffers.  *out stays null on failure.
// t0: when the caller's analysis phase began (seconds_analyse counts from there).
template <typename Analyse>
int nd_new_analysed(lsa_ctx* ctx, int dtype, const char* who, double t0, int64_t free_agreed, lsa_ndlu** out, Analyse&& analyse) {
    *out = nullptr;
    lsa_ndlu* f = new lsa_ndlu();
    f->ctx = ctx;
    f->dtype = dtype;
    char buf[256] = {0};
    int rc;
    try {
        rc = analyse(&f->S, buf, (int)sizeof buf);
    } catch (const std::bad_alloc&) {
        rc = LSA_ERR_ARG;
        snprintf(buf, sizeof buf, "%s: out of host memory in the analysis", who);
    }
    if (rc != LSA_OK) lsa_set_error(ctx, rc, "%s", buf);
    else rc = nd_setup(ctx, f, free_agreed);
    if (rc != LSA_OK) {
        nd_free(f);
        return rc;
    }
    f->seconds_analyse = now_s() - t0;
    *out = f;
    return LSA_OK;
}

}  // namespace

template <typename T>
__global__ void nd_zero_diag_kernel(int32_t n, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci, const T* __restrict__ val,
                                    int8_t* __restrict__ flags) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        int8_t z = 1;  // structurally absent counts as zero
        for (int32_t p = rp[i]; p < rp[i + 1]; ++p)
            if (ci[p] == (int32_t)i) z = s_abs2(val[p]) == 0.0 ? 1 : 0;
        flags[i] = z;
    }
}

// flags[i] = 1 where the diagonal entry of C is exactly zero (or not stored)
static int nd_zero_diagonal_flags(lsa_ctx* ctx, const lsa_mat* C, std::vector<int8_t>& flags) {
    flags.assign((size_t)std::max<int32_t>(C->n, 1), 0);
    int8_t* d = nullptr;
    LSA_HIP_ALLOC(ctx, hipMalloc((void**)&d, flags.size()));
    const int blocks = std::max(1, std::min((C->n + 255) / 256, ctx->num_cu * 8));
    if (C->dtype == LSA_C128) hipLaunchKernelGGL((nd_zero_diag_kernel<cplx>), dim3(blocks), dim3(256), 0, ctx->stream, C->n, C->rp, C->ci, (const cplx*)C->val, d);
    else hipLaunchKernelGGL((nd_zero_diag_kernel<double>), dim3(blocks), dim3(256), 0, ctx->stream, C->n, C->rp, C->ci, (const double*)C->val, d);
    const hipError_t e = hipMemcpyAsync(flags.data(), d, flags.size(), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d);
    if (e != hipSuccess || e2 != hipSuccess) return lsa_set_error(ctx, LSA_ERR_HIP, "lsa_ndlu: reading the diagonal failed");
    flags.resize((size_t)C->n);
    return LSA_OK;
}

// the last destroyed factorisation of a context is kept (analysis, tables, buffers): a shift sweep refactorises the
// same pattern once per sigma (.examples/eigenvalues.py:97-108)
extern "C" void lsa_ndlu_drop_cache(lsa_ctx* ctx) {
    if (ctx && ctx->nd_cache) {
        nd_free(ctx->nd_cache);
        ctx->nd_cache = nullptr;
    }
}

extern "C" {

int lsa_ndlu_refactor(lsa_ctx* ctx, lsa_ndlu* f, const lsa_mat* C) {
    if (!ctx || !f || !C) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_refactor: null argument");
    if (C->n != f->S.n || C->n != C->ncols || C->nnz != f->S.nnz || C->dtype != f->dtype)
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_refactor: the matrix does not match the analysed pattern");
    const double t0 = now_s();
    const int rc = ndlu_numeric(ctx, f, C);
    f->seconds_numeric = now_s() - t0;
    return rc;
}

// nd_pattern_hash of a matrix's host pattern, kept with the (shared) pattern
static uint64_t mat_pattern_hash(const lsa_mat* P) {
    if (!P->h_hash) P->h_hash = std::make_shared<uint64_t>(0);
    if (*P->h_hash == 0) {
        const uint64_t h = nd_pattern_hash(P->n, P->h_rp.data(), P->h_ci.data());
        *P->h_hash = h ? h : 1;
    }
    return *P->h_hash;
}

// analysis + device tables + buffers for the pattern of P and factors of type `dtype`; taken from the context's cache
// when the parked factorisation matches
// (strict: the parked analysis must also have been made for the same set of constraint unknowns)
static int nd_symbolic_phase(lsa_ctx* ctx, const lsa_mat* P, int dtype, int32_t leaf_size, const int8_t* constraint, bool strict,
                             lsa_ndlu** out) {
    *out = nullptr;
    if (P->n != P->ncols || P->row0 != 0) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu: needs a square, unsharded matrix");
    if ((int64_t)P->h_rp.size() != (int64_t)P->n + 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu: the matrix has no host copy of its pattern");
    if (leaf_size <= 0) leaf_size = nd_default_leaf(P->n);
    const double t0 = now_s();
    // same pattern as the parked factorisation: only the numbers change
    if (ctx->nd_cache) {
        lsa_ndlu* c = ctx->nd_cache;
        const uint64_t want = strict && constraint ? nd_constraint_hash(P->n, constraint) : 0;
        // (an analysis parked with the caller's tree -- lsa_ndlu_prepare_tree -- stands for its pattern whatever the leaf size)
        if (c->S.n == P->n && c->S.nnz == P->nnz && c->dtype == dtype && c->S.nranks == 1 && (c->S.tree_hash != 0 || c->S.leaf_size == leaf_size) &&
            (!strict || c->S.constraint_hash == want) &&
            c->S.pattern_hash == mat_pattern_hash(P)) {
            ctx->nd_cache = nullptr;
            c->seconds_analyse = 0.0;
            *out = c;
            return LSA_OK;
        }
        lsa_ndlu_drop_cache(ctx);
    }
    return nd_new_analysed(ctx, dtype, "lsa_ndlu", t0, 0, out, [&](NdSymbolic* S, char* err, int errlen) {
        return nd_analyse(P->n, P->h_rp.data(), P->h_ci.data(), leaf_size, constraint, S, err, errlen);
    });
}

int lsa_ndlu_prepare(lsa_ctx* ctx, const lsa_mat* P, int dtype, int32_t leaf_size, const int8_t* constraint) {
    if (!ctx || !P || (dtype != LSA_F64 && dtype != LSA_C128)) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_prepare: bad argument");
    lsa_ndlu* f = nullptr;
    LSA_CHECK(nd_symbolic_phase(ctx, P, dtype, leaf_size, constraint, true, &f));
    lsa_ndlu_drop_cache(ctx);
    ctx->nd_cache = f;  // the next lsa_ndlu_create on this pattern only runs the numeric phase
    return LSA_OK;
}

int lsa_ndlu_prepare_tree(lsa_ctx* ctx, const lsa_mat* P, int dtype, int32_t ntree, const int32_t* first, const int32_t* size, const int32_t* parent) {
    if (!ctx || !P || (dtype != LSA_F64 && dtype != LSA_C128) || ntree < 0 || (ntree > 0 && (!first || !size || !parent)))
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_prepare_tree: bad argument");
    if (P->n != P->ncols || P->row0 != 0) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_prepare_tree: needs a square, unsharded matrix");
    if ((int64_t)P->h_rp.size() != (int64_t)P->n + 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_prepare_tree: the matrix has no host copy of its pattern");
    const double t0 = now_s();
    lsa_ndlu_drop_cache(ctx);
    lsa_ndlu* f = nullptr;
    LSA_CHECK(nd_new_analysed(ctx, dtype, "lsa_ndlu_prepare_tree", t0, 0, &f, [&](NdSymbolic* S, char* err, int errlen) {
        return nd_analyse_tree(P->n, P->h_rp.data(), P->h_ci.data(), ntree, first, size, parent, nullptr, 0, 1, S, err, errlen);
    }));
    ctx->nd_cache = f;
    return LSA_OK;
}

int lsa_ndlu_create(lsa_ctx* ctx, const lsa_mat* C, int32_t leaf_size, lsa_ndlu** out) {
    if (!ctx || !C || !out) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_create: null argument");
    *out = nullptr;
    lsa_ndlu* f = nullptr;
    LSA_CHECK(nd_symbolic_phase(ctx, C, C->dtype, leaf_size, nullptr, false, &f));
    int rc = lsa_ndlu_refactor(ctx, f, C);
    if (rc == LSA_ERR_ZERO_PIVOT && f->S.constraint_hash == 0) {
        // A pivot block is singular although pivots are searched over its whole columns.  On saddle-point matrices that is
        // a leaf holding more constraint (zero-diagonal) unknowns than its interior supports: analyse again with those
        // unknowns eliminated after their neighbours, once.  The new analysis replaces the old one for this pattern.
        std::vector<int8_t> flags;
        const int frc = nd_zero_diagonal_flags(ctx, C, flags);
        bool any = false;
        for (int8_t v : flags) any |= v != 0;
        if (frc == LSA_OK && any) {
            const std::string first = ctx->err;
            const int32_t leaf = f->S.leaf_size;
            nd_free(f);
            f = nullptr;
            LSA_CHECK(nd_symbolic_phase(ctx, C, C->dtype, leaf, flags.data(), true, &f));
            rc = lsa_ndlu_refactor(ctx, f, C);
            if (rc == LSA_ERR_ZERO_PIVOT) lsa_set_error(ctx, rc, "%s (also with the zero-diagonal unknowns eliminated last; first attempt: %s)", std::string(ctx->err).c_str(), first.c_str());
        }
    }
    if (rc != LSA_OK) {
        nd_free(f);
        return rc;
    }
    *out = f;
    return LSA_OK;
}

int lsa_ndlu_create_tree(lsa_ctx* ctx, const lsa_mat* C, int32_t ntree, const int32_t* first, const int32_t* size, const int32_t* parent,
                         const int32_t* owner, lsa_ndlu** out) {
    if (!ctx || !C || !out || ntree < 0) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_create_tree: bad argument");
    *out = nullptr;
    if (C->n != C->ncols || C->row0 != 0) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_create_tree: needs the whole square matrix (every rank holds it)");
    if ((int64_t)C->h_rp.size() != (int64_t)C->n + 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_create_tree: the matrix has no host copy of its pattern");
    const double t0 = now_s();
    lsa_ndlu* f = nullptr;
    int setup_rc = LSA_OK;
    // the free device memory the plan may count on, agreed over the ranks (collective: entered by every rank, first thing)
    int64_t free_agreed = 0;
    if (ctx->nranks > 1) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)16 << 30;
        if (ctx->nd_cache) {  // (what a parked factorisation holds comes back when it is dropped or reused)
            const lsa_ndlu* c = ctx->nd_cache;
            free_b += (size_t)(c->lfac_entries + c->ufac_entries + c->work_entries + c->upd_entries) * esize(c->dtype);
        }
        free_agreed = (int64_t)free_b;
        LSA_CHECK(k_agree_min_i64(ctx, &free_agreed));
    }
    // the parked factorisation, if it was made for this pattern, this tree and this rank
    if (ctx->nd_cache) {
        lsa_ndlu* c = ctx->nd_cache;
        if (c->S.tree_hash == nd_tree_hash(ntree, first, size, parent, owner, ctx->rank, ctx->nranks) && c->S.n == C->n && c->S.nnz == C->nnz && c->dtype == C->dtype &&
            c->S.pattern_hash == mat_pattern_hash(C)) {
            f = c;
            ctx->nd_cache = nullptr;
            f->seconds_analyse = 0.0;
        } else {
            lsa_ndlu_drop_cache(ctx);
        }
    }
    if (!f)
        setup_rc = nd_new_analysed(ctx, C->dtype, "lsa_ndlu_create_tree", t0, free_agreed, &f, [&](NdSymbolic* S, char* err, int errlen) {
            return nd_analyse_tree(C->n, C->h_rp.data(), C->h_ci.data(), ntree, first, size, parent, owner, ctx->rank, ctx->nranks, S, err, errlen);
        });
    // Collective agreement on the set-up (out of device memory for this rank's buffers -- their sizes differ from rank to
    // rank --, a limit of the kernels, out of host memory in the analysis): no rank enters the exchanges of the numeric
    // phase alone.
    setup_rc = k_agree_status(ctx, setup_rc);
    if (setup_rc != LSA_OK) {
        nd_free(f);  // (a set-up that failed on another rank only)
        return setup_rc;
    }
    const int rc = lsa_ndlu_refactor(ctx, f, C);
    if (rc != LSA_OK) {
        nd_free(f);
        return rc;
    }
    *out = f;
    return LSA_OK;
}

void lsa_ndlu_destroy(lsa_ndlu* f) {
    if (!f) return;
    lsa_ctx* ctx = f->ctx;
    if (ctx && ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx && !getenv("LSA_ND_NO_CACHE")) {
        lsa_ndlu_drop_cache(ctx);
        ctx->nd_cache = f;
        return;
    }
    nd_free(f);
}

int lsa_ndlu_solve(lsa_ctx* ctx, lsa_ndlu* f, const lsa_vec* b, lsa_vec* x) {
    if (!ctx || !f || !b || !x) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_solve: null argument");
    if (b->n != f->S.n || x->n != f->S.n || b->dtype != x->dtype) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_solve: shape/dtype mismatch");
    LSA_CHECK(ndlu_solve_dev(ctx, f, b->dtype, b->d, x->d));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return LSA_OK;
}

// what the rules of every solve on J factor sets share (`who` names the entry in the messages, `unit` a member), in the order the
// entries have always applied them: the head -- nothing null, J in range --, then per member that it is there and, behind the
// entry's own rules for its vectors, that it is of the analysis of the first
static int nd_sets_head(lsa_ctx* ctx, const char* who, int32_t J, lsa_ndlu* const* f, const lsa_vec* const* b, lsa_vec* const* x) {
    if (!ctx || !f || !b || !x) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: null argument", who);
    if (J < 1 || J > kNdBatchMax) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: J = %d outside [1, %d]", who, J, kNdBatchMax);
    return LSA_OK;
}
static int nd_member_there(lsa_ctx* ctx, const char* who, const char* unit, int32_t z, lsa_ndlu* const* f, const lsa_vec* const* b, lsa_vec* const* x) {
    if (!f[z] || !b[z] || !x[z]) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: null argument (%s %d)", who, unit, z);
    return LSA_OK;
}
static int nd_member_compatible(lsa_ctx* ctx, const char* who, int32_t z, lsa_ndlu* const* f) {
    if (!nd_batch_compatible(f[0], f[z])) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: factorisation %d is not of the same analysis as factorisation 0", who, z);
    return LSA_OK;
}

// one column on each of J problems, forward or transposed: checked, queued and awaited
static int nd_batch_solve(lsa_ctx* ctx, const char* who, int32_t J, lsa_ndlu* const* f, int trans, const lsa_vec* const* b, lsa_vec* const* x) {
    const void* bd[kNdBatchMax];
    void* xd[kNdBatchMax];
    LSA_CHECK(nd_sets_head(ctx, who, J, f, b, x));
    for (int32_t z = 0; z < J; ++z) {
        LSA_CHECK(nd_member_there(ctx, who, "problem", z, f, b, x));
        if (b[z]->n != f[z]->S.n || x[z]->n != f[z]->S.n || b[z]->dtype != x[z]->dtype || x[z]->dtype != x[0]->dtype)
            return lsa_set_error(ctx, LSA_ERR_ARG, "%s: shape/dtype mismatch (problem %d)", who, z);
        LSA_CHECK(nd_member_compatible(ctx, who, z, f));
        bd[z] = b[z]->d;
        xd[z] = x[z]->d;
        for (int32_t y = 0; y < z; ++y)
            if (f[y] == f[z] || xd[y] == xd[z] || xd[y] == bd[z] || bd[y] == xd[z])
                return lsa_set_error(ctx, LSA_ERR_ARG, "%s: problems %d and %d share a factorisation or an output", who, y, z);
    }
    const NdSolve rq = {J, f, true, trans, x[0]->dtype, 1, bd, 0, xd, 0, who};
    LSA_CHECK(ndlu_solve_run(ctx, rq));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return LSA_OK;
}

int lsa_ndlu_solve_batch(lsa_ctx* ctx, int32_t J, lsa_ndlu* const* f, const lsa_vec* const* b, lsa_vec* const* x) {
    return nd_batch_solve(ctx, "lsa_ndlu_solve_batch", J, f, 0, b, x);
}

int lsa_ndlu_solve_batch_adjoint(lsa_ctx* ctx, int32_t J, lsa_ndlu* const* f, int conj, const lsa_vec* const* b, lsa_vec* const* x) {
    return nd_batch_solve(ctx, "lsa_ndlu_solve_batch_adjoint", J, f, conj ? 2 : 1, b, x);
}

int lsa_ndlu_solve_adjoint(lsa_ctx* ctx, lsa_ndlu* f, int conj, const lsa_vec* b, lsa_vec* x) {
    if (!ctx || !f || !b || !x) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_solve_adjoint: null argument");
    if (b->n != f->S.n || x->n != f->S.n || b->dtype != x->dtype) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_solve_adjoint: shape/dtype mismatch");
    LSA_CHECK(ndlu_solve_adjoint_dev(ctx, f, conj, b->dtype, b->d, x->d));
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return LSA_OK;
}

int lsa_ndlu_solve_time(lsa_ctx* ctx, lsa_ndlu* f, const lsa_vec* b, lsa_vec* x, int iters, double* avg_ms) {
    if (!ctx || !f || !b || !x || !avg_ms || iters < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_solve_time: bad argument");
    if (b->n != f->S.n || x->n != f->S.n || b->dtype != x->dtype || b->d == x->d) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_solve_time: shape/dtype mismatch");
    return lsa_time_runs(ctx, false, iters, avg_ms, [&] { return ndlu_solve_dev(ctx, f, b->dtype, b->d, x->d); });
}

// shape, dtype and overlap rules of a block solve; `who` names the entry in the message
static int nd_multi_check(lsa_ctx* ctx, const char* who, const lsa_ndlu* f, int trans, int32_t nrhs, const lsa_vec* B, int64_t ldb, const lsa_vec* X,
                          int64_t ldx) {
    if (!ctx || !f || !B || !X) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: null argument", who);
    const int64_t n = f->S.n;
    if (trans < 0 || trans > 2) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: trans = %d is none of 0 (N), 1 (T), 2 (H)", who, trans);
    if (nrhs < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: nrhs = %d, need at least one column", who, nrhs);
    if (ldb < n || ldx < n) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: leading dimensions %lld / %lld below n = %lld", who, (long long)ldb, (long long)ldx, (long long)n);
    if (B->dtype != X->dtype) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: B and X differ in dtype", who);
    if (f->dtype == LSA_C128 && B->dtype != LSA_C128) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: complex factors need complex vectors", who);
    const int64_t need_b = ldb * (int64_t)(nrhs - 1) + n, need_x = ldx * (int64_t)(nrhs - 1) + n;
    if (B->n < need_b || X->n < need_x)
        return lsa_set_error(ctx, LSA_ERR_ARG, "%s: a block of %d columns needs %lld / %lld entries, B and X hold %lld / %lld", who, nrhs, (long long)need_b,
                             (long long)need_x, (long long)B->n, (long long)X->n);
    if (!(B->d == X->d && ldb == ldx)) {  // in place is the one overlap a solve can honour
        const char *b0 = (const char*)B->d, *x0 = (const char*)X->d;
        const size_t es = esize(B->dtype);
        if (b0 < x0 + (size_t)need_x * es && x0 < b0 + (size_t)need_b * es) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: B and X overlap (in place needs B == X and ldb == ldx)", who);
    }
    return LSA_OK;
}

// the rules of a block solve on J factor sets: what they share with the single-column batch, those of nd_multi_check for every
// set's blocks, and between sets no shared factorisation or X and no overlap but ONE B read by several; the device pointers.
// `refused`: the trans a forward entry was given (the transposed form has entries of its own: it goes on refusing trans != 0).
static int nd_multi_batch_check(lsa_ctx* ctx, const char* who, int32_t J, lsa_ndlu* const* f, int refused, int32_t nrhs, const lsa_vec* const* B, int64_t ldb,
                                lsa_vec* const* X, int64_t ldx, const void** bd, void** xd) {
    LSA_CHECK(nd_sets_head(ctx, who, J, f, B, X));
    if (refused != 0) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: trans = %d: the transposed form of the block solve on a batch of factor sets is not built", who, refused);
    for (int32_t z = 0; z < J; ++z) {
        LSA_CHECK(nd_member_there(ctx, who, "set", z, f, B, X));
        LSA_CHECK(nd_member_compatible(ctx, who, z, f));
        bd[z] = B[z]->d;
        xd[z] = X[z]->d;
        if (X[z]->dtype != X[0]->dtype) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: the vectors of set %d differ in dtype from those of set 0", who, z);
        LSA_CHECK(nd_multi_check(ctx, who, f[z], 0, nrhs, B[z], ldb, X[z], ldx));
    }
    const size_t es = esize(X[0]->dtype);
    const int64_t n = f[0]->S.n;
    const size_t span_b = (size_t)(ldb * (int64_t)(nrhs - 1) + n) * es, span_x = (size_t)(ldx * (int64_t)(nrhs - 1) + n) * es;
    auto overlap = [](const void* a, size_t na, const void* b, size_t nb) { return (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na; };
    for (int32_t z = 0; z < J; ++z)
        for (int32_t y = 0; y < z; ++y) {
            if (f[y] == f[z]) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: sets %d and %d share a factorisation", who, y, z);
            if (overlap(xd[y], span_x, xd[z], span_x)) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: sets %d and %d share an X or their X overlap", who, y, z);
            if (overlap(xd[y], span_x, bd[z], span_b) || overlap(bd[y], span_b, xd[z], span_x))
                return lsa_set_error(ctx, LSA_ERR_ARG, "%s: the X of one of the sets %d and %d overlaps the B of the other", who, y, z);
            if (bd[y] != bd[z] && overlap(bd[y], span_b, bd[z], span_b))
                return lsa_set_error(ctx, LSA_ERR_ARG, "%s: the B of sets %d and %d overlap (several sets may read ONE B)", who, y, z);
        }
    return LSA_OK;
}

// lsa_ndlu_solve_multi and, with avg_ms, its timed form: the checked block solve queued once and awaited, or queued once (the first
// call makes the per-column buffers) and then timed over iters repetitions
static int nd_multi_solve(lsa_ctx* ctx, const char* who, lsa_ndlu* f, int trans, int32_t nrhs, const lsa_vec* B, int64_t ldb, lsa_vec* X, int64_t ldx, int iters,
                          double* avg_ms) {
    LSA_CHECK(nd_multi_check(ctx, who, f, trans, nrhs, B, ldb, X, ldx));
    if (avg_ms && B->d == X->d) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: repeated solves need B and X apart", who);
    const void* bd = B->d;
    void* xd = X->d;
    const NdSolve rq = {1, &f, false, trans, B->dtype, nrhs, &bd, ldb, &xd, ldx, who};
    const bool block = f->S.nranks == 1 && !f->S.has_dist && (trans == 0 || f->multi_transposed);
    auto run = [&] {
        if (nrhs == 1 || block) return ndlu_solve_run(ctx, rq);
        // a forest cut over ranks, distributed nodes, the transposed systems unless lsa_ndlu_set_multi_transposed: column by column
        // (the one writer of the two fields beside ndlu_solve_run)
        f->multi_width = 1, f->multi_passes = 0;
        const size_t es = esize(B->dtype);
        for (int32_t q = 0; q < nrhs; ++q) {
            const void* b = (const char*)bd + (size_t)q * (size_t)ldb * es;
            void* x = (char*)xd + (size_t)q * (size_t)ldx * es;
            LSA_CHECK(trans == 0 ? ndlu_solve_dev(ctx, f, B->dtype, b, x) : ndlu_solve_adjoint_dev(ctx, f, trans == 2, B->dtype, b, x));
        }
        return (int)LSA_OK;
    };
    if (avg_ms) return lsa_time_runs(ctx, true, iters, avg_ms, run);
    LSA_CHECK(run());
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return LSA_OK;
}

int lsa_ndlu_solve_multi(lsa_ctx* ctx, lsa_ndlu* f, int trans, int32_t nrhs, const lsa_vec* B, int64_t ldb, lsa_vec* X, int64_t ldx) {
    return nd_multi_solve(ctx, "lsa_ndlu_solve_multi", f, trans, nrhs, B, ldb, X, ldx, 0, nullptr);
}

int lsa_ndlu_solve_multi_time(lsa_ctx* ctx, lsa_ndlu* f, int trans, int32_t nrhs, const lsa_vec* B, int64_t ldb, lsa_vec* X, int64_t ldx, int iters,
                              double* avg_ms) {
    if (!avg_ms || iters < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_solve_multi_time: bad argument");
    return nd_multi_solve(ctx, "lsa_ndlu_solve_multi_time", f, trans, nrhs, B, ldb, X, ldx, iters, avg_ms);
}

// the block solve on J sets and, with avg_ms, its timed form.  `trans`: what the entry was given -- the forward entries refuse all but 0
// (nd_multi_batch_check), the transposed ones say 1 or 2 through `adjoint`.
static int nd_multi_batch_solve(lsa_ctx* ctx, const char* who, bool adjoint, int32_t J, lsa_ndlu* const* f, int trans, int32_t nrhs, const lsa_vec* const* B,
                                int64_t ldb, lsa_vec* const* X, int64_t ldx, int iters, double* avg_ms) {
    const void* bd[kNdBatchMax];
    void* xd[kNdBatchMax];
    LSA_CHECK(nd_multi_batch_check(ctx, who, J, f, adjoint ? 0 : trans, nrhs, B, ldb, X, ldx, bd, xd));
    for (int32_t z = 0; avg_ms && z < J; ++z)
        if (bd[z] == xd[z]) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: repeated solves need B and X apart (set %d)", who, z);
    const NdSolve rq = {J, f, true, trans, X[0]->dtype, nrhs, bd, ldb, xd, ldx, who};
    auto run = [&] { return ndlu_solve_run(ctx, rq); };
    if (avg_ms) return lsa_time_runs(ctx, true, iters, avg_ms, run);
    LSA_CHECK(run());
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return LSA_OK;
}

int lsa_ndlu_solve_multi_batch(lsa_ctx* ctx, int32_t J, lsa_ndlu* const* f, int trans, int32_t nrhs, const lsa_vec* const* B, int64_t ldb, lsa_vec* const* X,
                               int64_t ldx) {
    return nd_multi_batch_solve(ctx, "lsa_ndlu_solve_multi_batch", false, J, f, trans, nrhs, B, ldb, X, ldx, 0, nullptr);
}

int lsa_ndlu_solve_multi_batch_time(lsa_ctx* ctx, int32_t J, lsa_ndlu* const* f, int trans, int32_t nrhs, const lsa_vec* const* B, int64_t ldb, lsa_vec* const* X,
                                    int64_t ldx, int iters, double* avg_ms) {
    if (!avg_ms || iters < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_solve_multi_batch_time: bad argument");
    return nd_multi_batch_solve(ctx, "lsa_ndlu_solve_multi_batch_time", false, J, f, trans, nrhs, B, ldb, X, ldx, iters, avg_ms);
}

int lsa_ndlu_solve_multi_batch_adjoint(lsa_ctx* ctx, int32_t J, lsa_ndlu* const* f, int conj, int32_t nrhs, const lsa_vec* const* B, int64_t ldb,
                                       lsa_vec* const* X, int64_t ldx) {
    return nd_multi_batch_solve(ctx, "lsa_ndlu_solve_multi_batch_adjoint", true, J, f, conj ? 2 : 1, nrhs, B, ldb, X, ldx, 0, nullptr);
}

int lsa_ndlu_solve_multi_batch_adjoint_time(lsa_ctx* ctx, int32_t J, lsa_ndlu* const* f, int conj, int32_t nrhs, const lsa_vec* const* B, int64_t ldb,
                                            lsa_vec* const* X, int64_t ldx, int iters, double* avg_ms) {
    if (!avg_ms || iters < 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_solve_multi_batch_adjoint_time: bad argument");
    return nd_multi_batch_solve(ctx, "lsa_ndlu_solve_multi_batch_adjoint_time", true, J, f, conj ? 2 : 1, nrhs, B, ldb, X, ldx, iters, avg_ms);
}

int lsa_ndlu_set_multi_transposed(lsa_ctx* ctx, lsa_ndlu* f, int on) {
    if (!ctx || !f) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_set_multi_transposed: null argument");
    f->multi_transposed = on != 0;
    return LSA_OK;
}

int lsa_ndlu_multi_info(const lsa_ndlu* f, int32_t* width, int64_t* extra_bytes, int32_t* launches_per_pass) {
    if (!f) return LSA_ERR_ARG;
    if (width) *width = f->multi_width;
    if (extra_bytes) *extra_bytes = f->multi_bytes;
    if (launches_per_pass) *launches_per_pass = f->solve_launches;
    return LSA_OK;
}

// Inertia of a REAL SYMMETRIC C from its factorisation: the multifrontal elimination is a block congruence C = L D L^T with D
// the pivot blocks (however each of them was inverted), so inertia(C) = sum over the tree nodes of the inertia of their pivot
// blocks = of the inverses the factors hold (first m rows of the packed L).  The blocks come to the host one by one
// (lsa_dense_sym_inertia: Bunch-Kaufman, O(m^3) each): meant for the interval sweep behind iEpsWhich.ALL on Hermitian
// problems (Solver/utils.py:248-254), whose pivot blocks are a few hundred rows, not for the 3D fronts of the flow problems.
int lsa_ndlu_inertia(lsa_ctx* ctx, lsa_ndlu* f, int64_t* negative, int64_t* zero, int64_t* positive) {
    if (!ctx || !f || !negative || !zero || !positive) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_inertia: null argument");
    if (f->dtype != LSA_F64) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_inertia: needs real factors (a real symmetric matrix)");
    if (f->S.nranks != 1) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_inertia: not available for a forest cut over ranks");
    *negative = *zero = *positive = 0;
    const NdSymbolic& S = f->S;
    std::vector<double> blk;
    LSA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (int32_t t = 0; t < S.nt; ++t) {
        const int32_t m = S.m[(size_t)t];
        if (m <= 0) continue;
        blk.resize((size_t)m * m);
        // (the plan's offset of the node's packed L: recomputed as nd_memory_plan lays it out -- f x m scalars per node, in node order)
        LSA_HIP_CHECK(ctx, hipMemcpy(blk.data(), (const double*)f->d_lfac + f->h_lfac_off[(size_t)t], (size_t)m * m * sizeof(double), hipMemcpyDeviceToHost));
        int64_t ng = 0, ze = 0, ps = 0;
        const int rc = lsa_dense_sym_inertia(m, blk.data(), m, 1e-13, &ng, &ze, &ps);
        if (rc != LSA_OK) return lsa_set_error(ctx, rc, "lsa_ndlu_inertia: the pivot block of tree node %d holds non-finite values", t);
        *negative += ng;
        *zero += ze;
        *positive += ps;
    }
    return LSA_OK;
}

int lsa_ndlu_prepared_memory(lsa_ctx* ctx, int64_t* out) {
    if (!ctx || !out) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_prepared_memory: null argument");
    const lsa_ndlu* c = ctx->nd_cache;
    if (!c) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_ndlu_prepared_memory: the context holds no prepared analysis");
    return nd_memory_report(c->S, (int32_t)esize(c->dtype), 0, out, nullptr, nullptr, nullptr);
}

int lsa_ndlu_sweep_level(const lsa_ndlu* f, int32_t level, int32_t* nodes, int32_t* max_pivot, int32_t* fwd_rows, int32_t* bwd_rows, int32_t* fwd_tiles,
                         int32_t* bwd_tiles) {
    if (!f || level < 0 || (size_t)level >= f->levels.size()) return LSA_ERR_ARG;
    const NdLevel& L = f->levels[(size_t)level];
    if (nodes) *nodes = L.node_count;
    if (max_pivot) *max_pivot = L.max_m;
    if (fwd_rows) *fwd_rows = L.sweep_rows;
    if (bwd_rows) *bwd_rows = L.bwd_rows;
    if (fwd_tiles) *fwd_tiles = L.fwd_tiles;
    if (bwd_tiles) *bwd_tiles = L.bwd_tiles;
    return LSA_OK;
}

int lsa_ndlu_info(const lsa_ndlu* f, int32_t* ntree, int32_t* nlevels, int32_t* max_front, int64_t* factor_entries, int64_t* front_entries,
                  int64_t* apply_bytes, int32_t* apply_launches, double* seconds_analyse, double* seconds_numeric, int32_t* factor_launches) {
    if (!f) return LSA_ERR_ARG;
    const NdSymbolic& S = f->S;
    if (ntree) *ntree = S.nt;
    if (nlevels) *nlevels = S.nlevels;
    if (max_front) {
        int32_t mf = 0;
        for (int32_t v : S.f) mf = std::max(mf, v);
        *max_front = mf;
    }
    if (factor_entries) *factor_entries = S.factor_entries;
    if (front_entries) *front_entries = f->lfac_entries + f->ufac_entries + f->work_entries + f->upd_entries;  // scalars of the device buffers
    // one solve reads every factor scalar once, the right-hand side once, and reads + writes the solution and the update vectors
    // (with the merged top: its s^2 scalars instead of the packed blocks of the root and its children)
    const int64_t swept = S.factor_entries - f->top_replaced_entries * (f->top.s > 0) + (int64_t)f->top.s * f->top.s;
    if (apply_bytes) *apply_bytes = swept * (int64_t)esize(f->dtype) + 16 * (3 * (int64_t)S.n + 2 * S.u_off[(size_t)S.nt]);
    if (apply_launches) *apply_launches = f->solve_launches;
    if (seconds_analyse) *seconds_analyse = f->seconds_analyse;
    if (seconds_numeric) *seconds_numeric = f->seconds_numeric;
    if (factor_launches) *factor_launches = f->factor_launches;
    return LSA_OK;
}

}  // extern "C"
