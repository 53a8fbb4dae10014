"""CPU suite: the top of the elimination forest as one assembled inverse (``nd_top_kernel`` in ``csrc/ndlu_sweeps.hip``,
``nd_top_gemm_kernel`` in ``csrc/ndlu_factor.hip``), checked in numpy on the analysis tables.

The root R and its children c are three dependent steps of the emulated walk (children upward, root, children downward).
With the blocks a factorisation leaves -- ``inv_t``, ``s1_t = -F21 inv_t``, ``U_t = inv_t F12`` -- they are one product
``[x_c...; x_R] = T [v_c...; z_R]``:

    T[R, R] = inv_R                     T[R, c] = inv_R[:, cmap_c] s1_c
    T[c, R] = -U_c inv_R[cmap_c, :]     T[c, d] = [c == d] inv_c + T[c, R][:, cmap_d] s1_d

Here T is built by exactly these products (in the two stages of the device assembly: the second reads the first one's
``T[c, R]``), put in place of the three steps of ``nd_emulation.Emulated.solve``, and held to the two bounds
``tests/test_gpu_ndlu.py`` puts on a solve.  ``top_plan`` is the eligibility rule of ``nd_setup_top`` on the exported tables."""

import numpy as np
import pytest
import scipy.sparse as sp

import helpers  # noqa: F401  (sys.path)
import lsa_hip
from nd_emulation import Emulated
from synthetic import fem

TOP_LIMIT = 1280  # the library's default LSA_ND_TOPINV
MAX_CHILDREN = 8


def top_plan(t: dict, limit: int = TOP_LIMIT):
    """(root, children in rank order, s) if the forest's top is merged, else None: one root alone on the last level, the level
    below it holds exactly the root's children, none of them a leaf, and at most ``limit`` unknowns in all."""
    parent, lvl_ptr, lvl_nodes = t["parent"], t["lvl_ptr"], t["lvl_nodes"]
    m = np.diff(t["node_start"])
    nl = len(lvl_ptr) - 1
    if limit <= 0 or nl < 3 or np.count_nonzero(parent < 0) != 1:
        return None
    last = lvl_nodes[lvl_ptr[nl - 1]:lvl_ptr[nl]]
    if len(last) != 1 or parent[last[0]] >= 0:
        return None
    R = int(last[0])
    K = [int(c) for c in np.flatnonzero(parent == R)]
    below = sorted(int(c) for c in lvl_nodes[lvl_ptr[nl - 2]:lvl_ptr[nl - 1]])
    if not K or len(K) > MAX_CHILDREN or below != K:
        return None
    if any(not np.any(parent == c) for c in K):  # a leaf among them
        return None
    s = int(m[R] + m[K].sum())
    return (R, K, s) if s <= limit else None


def assemble_top(em: Emulated, R: int, K: list):
    """T and the offsets of its blocks, from the packed blocks of the factored fronts."""
    t, m, b = em.t, em.m, em.b
    mR = int(m[R])
    assert b[R] == 0
    invR = em.F(R)[:mR, :mR]
    cm = {c: t["cmap"][em.u_off[c]:em.u_off[c] + int(b[c])] for c in K}
    off = np.concatenate([[0], np.cumsum([m[c] for c in K])]).astype(int)
    oR, s = int(off[-1]), int(off[-1]) + mR
    T = np.zeros((s, s), dtype=em.front.dtype)
    T[oR:, oR:] = invR
    for i, c in enumerate(K):  # stage 1
        mc = int(m[c])
        T[off[i]:off[i + 1], oR:] = -(em.F(c)[:mc, mc:] @ invR[cm[c], :])
        T[oR:, off[i]:off[i + 1]] = invR[:, cm[c]] @ em.F(c)[mc:, :mc]
    for i, c in enumerate(K):  # stage 2
        for j, d in enumerate(K):
            md = int(m[d])
            blk = T[off[i]:off[i + 1], oR:][:, cm[d]] @ em.F(d)[md:, :md]
            if c == d:
                blk = em.F(c)[:md, :md] + blk
            T[off[i]:off[i + 1], off[j]:off[j + 1]] = blk
    return T, off, cm


def solve_with_top(em: Emulated, rhs: np.ndarray, R: int, K: list) -> np.ndarray:
    """``Emulated.solve`` with the steps of R and K replaced by one product with T."""
    t, m, b = em.t, em.m, em.b
    T, off, cm = assemble_top(em, R, K)
    mR, oR = int(m[R]), int(off[-1])
    x = np.zeros_like(rhs, dtype=np.result_type(rhs.dtype, em.front.dtype))
    ubuf = np.zeros(int(em.u_off[-1]), dtype=x.dtype)
    nl = len(t["lvl_ptr"]) - 1
    top = set(K) | {R}

    def gathered(node):
        gp = t["gptr"][em.g_off[node]:em.g_off[node + 1]]
        return np.array([ubuf[t["gidx"][gp[j]:gp[j + 1]]].sum() for j in range(int(em.f[node]))])

    def ix(node):
        return t["idx"][em.idx_off[node]:em.idx_off[node + 1]]

    for lv in range(nl):
        for node in t["lvl_nodes"][t["lvl_ptr"][lv]:t["lvl_ptr"][lv + 1]]:
            node = int(node)
            if node in top:
                continue
            mm = int(m[node])
            g = gathered(node)
            out = em.F(node)[:, :mm] @ (rhs[ix(node)[:mm]] + g[:mm])
            x[ix(node)[:mm]] = out[:mm]
            ubuf[em.u_off[node]:em.u_off[node + 1]] = g[mm:] + out[mm:]
    z = np.zeros(T.shape[0], dtype=x.dtype)
    zR = rhs[ix(R)[:mR]].astype(x.dtype)
    for i, c in enumerate(K):  # children in rank order: the sums have one order
        g = gathered(c)
        z[off[i]:off[i + 1]] = rhs[ix(c)[:int(m[c])]] + g[:int(m[c])]
        assert len(np.unique(cm[c])) == len(cm[c]) and cm[c].max() < mR
        zR[cm[c]] += g[int(m[c]):]
    z[oR:] = zR
    xt = T @ z
    for i, c in enumerate(K):
        x[ix(c)[:int(m[c])]] = xt[off[i]:off[i + 1]]
    x[ix(R)[:mR]] = xt[oR:]
    for lv in range(nl - 1, -1, -1):
        for node in t["lvl_nodes"][t["lvl_ptr"][lv]:t["lvl_ptr"][lv + 1]]:
            node = int(node)
            if node in top or b[node] == 0:
                continue
            mm = int(m[node])
            x[ix(node)[:mm]] -= em.F(node)[:mm, mm:] @ x[ix(node)[mm:]]
    return x


def _shifted(es, sigma):
    C = sp.csr_matrix((es.A.data - sigma * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
    C.sort_indices()
    return C


# S5k: the root has four children; S30k (the benchmark's matrix): two.  Complex factors (the shift of the cylinder runs) and real factors.
@pytest.mark.parametrize("case,children", [("S5k", 4), ("S30k", 2)])
@pytest.mark.parametrize("sigma", [fem.SIGMA_RE50, 0.05], ids=["complex", "real"])
def test_assembled_top_equals_the_three_steps(case, children, sigma):
    es = fem.cylinder_case(case)
    C = _shifted(es, sigma)
    assert np.iscomplexobj(C.data) == np.iscomplexobj(sigma)
    t = lsa_hip.NdAnalysis(C, 0).export_tables()
    plan = top_plan(t)
    assert plan is not None, "the forest of this case must be eligible"
    R, K, s = plan
    assert len(K) == children and s == int(np.diff(t["node_start"])[[R] + K].sum())
    em = Emulated(t, C.data)
    rng = np.random.default_rng(0)
    for rhs in (rng.standard_normal(es.n), rng.standard_normal(es.n) + 1j * rng.standard_normal(es.n)):
        xw = em.solve(rhs)
        x = solve_with_top(em, rhs, R, K)
        d = np.linalg.norm(x - xw) / np.linalg.norm(xw)
        r = np.linalg.norm(C @ x - rhs) / np.linalg.norm(rhs)
        print(f"{case} s={s} children={len(K)} {x.dtype}: |x - x_walk|/|x_walk| = {d:.2e}, |b - C x|/|b| = {r:.2e}")
        assert d <= 1e-10
        assert r <= 1e-12


def test_forests_that_must_be_refused():
    # a 3D forest: the root's children do not all sit on the level under it
    es = fem.cube_case("C40k")
    t = lsa_hip.NdAnalysis(_shifted(es, fem.SIGMA_CUBE), 0).export_tables()
    root = int(np.flatnonzero(t["parent"] < 0)[0])
    lv = np.empty(len(t["parent"]), dtype=np.int64)
    for l in range(len(t["lvl_ptr"]) - 1):
        lv[t["lvl_nodes"][t["lvl_ptr"][l]:t["lvl_ptr"][l + 1]]] = l
    assert np.count_nonzero(t["parent"] < 0) == 1 and len(set(lv[t["parent"] == root].tolist())) > 1
    assert top_plan(t, limit=1 << 30) is None
    # two roots: two copies of one pattern side by side
    C = _shifted(fem.cylinder_case("S2k"), fem.SIGMA_RE50)
    t2 = lsa_hip.NdAnalysis(sp.block_diag([C, C], format="csr"), 0).export_tables()
    assert np.count_nonzero(t2["parent"] < 0) == 2
    assert top_plan(t2, limit=1 << 30) is None
    # the limit itself, and the switch
    t5 = lsa_hip.NdAnalysis(_shifted(fem.cylinder_case("S5k"), fem.SIGMA_RE50), 0).export_tables()
    s = top_plan(t5)[2]
    assert top_plan(t5, limit=s) is not None and top_plan(t5, limit=s - 1) is None and top_plan(t5, limit=0) is None
