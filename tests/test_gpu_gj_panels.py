"""GPU suite: the Gauss-Jordan panels of the exact LU at 16 columns (``nd_gj_fused_kernel<T, NT, 1, 16>``, staging in the finishing
launch, S1 and S2 in one launch: ``csrc/ndlu_factor.hip``) against the 8-column launch sequence (``LSA_ND_GJ_PANEL=8``) and against
LAPACK / SuperLU; the library's default (knob unset: the regrouped launches, the panel width chosen by instance) runs beside
both.  The knob is read at every set-up of a factorisation, and a factorisation parked in the context keeps the
one it was set up with: every test switches the parking off (``LSA_ND_NO_CACHE``).

Small dense matrices inside hand-made forests: the panel and block edges, every workgroup size up to 512 rows, pivots off the
diagonal, nodes of one launch that end at different places of a block.  The matrices are strictly diagonally dominant
before their rows are moved (entries in [-1, 1], dominant entries n + 1), so that LAPACK's own solution has a residual of a
few 1e-16 and a forward error far below the 1e-10 asked of the device (checked on the host when these cases were chosen:
residual <= 6e-16 and condition number <= 1.8 for every dense case here, so a forward error of about 1e-15; SuperLU's
residual on the S5k matrix is 3e-15)."""

import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

SIGMA = 0.018 + 0.7379601143282424j
SIZES = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 96, 129, 257]
RES_BOUND, ERR_BOUND, AGREE_BOUND = 1e-12, 1e-10, 1e-10  # (tests/test_gpu_topinv.py: its SuperLU comparison)
WIDTHS = ("16", "8", "")  # the knob: 16-column panels wherever they exist, the earlier launch sequence, unset (the default)


@functools.lru_cache(maxsize=None)
def _dense_case(m, shift, kind):
    """(matrix, right-hand side, LAPACK's solution) of one node: kind 'c' complex factors, 'r' real factors and a real
    vector, 'rc' real factors and a complex vector; rows moved down cyclically by `shift`."""
    rng = np.random.default_rng(1000 * m + shift)
    A = rng.uniform(-1.0, 1.0, (m, m))
    if kind == "c":
        A = A + 1j * rng.uniform(-1.0, 1.0, (m, m))
    A = A + (m + 1.0) * np.eye(m)
    A = np.roll(A, shift % m, axis=0)
    b = rng.standard_normal(m)
    if kind != "r":
        b = b + 1j * rng.standard_normal(m)
    for a in (A, b):
        a.setflags(write=False)
    return A, b, np.linalg.solve(A, b)


def _factor(ctx, monkeypatch, width, M, tree):
    import lsa_hip

    monkeypatch.setenv("LSA_ND_NO_CACHE", "1")
    if width:
        monkeypatch.setenv("LSA_ND_GJ_PANEL", width)
    else:
        monkeypatch.delenv("LSA_ND_GJ_PANEL", raising=False)
    M = sp.csr_matrix(M)
    M.sort_indices()
    dM = lsa_hip.CsrMatrix.from_scipy(ctx, M)
    return dM, lsa_hip.NdLu(ctx, dM, tree=tree)


def _solve(ctx, f, b):
    import lsa_hip

    dx = lsa_hip.DeviceVector(ctx, len(b), b.dtype)
    f.solve(lsa_hip.DeviceVector.from_numpy(ctx, np.array(b)), dx)
    return dx.numpy()


def _check(label, A, b, xref, xs):
    """The bounds of cases 1-3 and 5: every width against the reference, and the widths against one another."""
    for width, x in xs.items():
        res = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
        err = np.linalg.norm(x - xref) / np.linalg.norm(xref)
        print(f"{label} panel {width or 'default'}: |b - C x|/|b| = {res:.2e}, |x - x_ref|/|x_ref| = {err:.2e}")
        assert res <= RES_BOUND
        assert err <= ERR_BOUND
    for width in ("16", ""):
        d = np.linalg.norm(xs[width] - xs["8"]) / np.linalg.norm(xs["8"])
        print(f"{label}: |x_{width or 'default'} - x_8|/|x_8| = {d:.2e}")
        assert d <= AGREE_BOUND


def _one_node(hip_ctx, monkeypatch, m, shift, kind):
    A, b, xref = _dense_case(m, shift, kind)
    tree = {"first": [0], "size": [m], "parent": [-1]}
    xs = {}
    for width in WIDTHS:
        _, f = _factor(hip_ctx, monkeypatch, width, A, tree)
        xs[width] = _solve(hip_ctx, f, b)
        assert xs[width].dtype == b.dtype
    _check(f"m = {m}, rows moved by {shift}, {kind}", A, b, xref, xs)


@pytest.mark.parametrize("kind", ["c", "r", "rc"])
@pytest.mark.parametrize("m", SIZES)
def test_one_node_at_the_panel_and_block_edges(hip_ctx, monkeypatch, m, kind):
    _one_node(hip_ctx, monkeypatch, m, 0, kind)


@pytest.mark.parametrize("kind", ["c", "r", "rc"])
@pytest.mark.parametrize("shift", [9, 17])
@pytest.mark.parametrize("m", SIZES)
def test_one_node_with_every_pivot_off_the_diagonal(hip_ctx, monkeypatch, m, shift, kind):
    """Rows moved cyclically by 9 and by 17: the pivot of a column lies in another panel or another wavefront's rows."""
    _one_node(hip_ctx, monkeypatch, m, shift, kind)


@functools.lru_cache(maxsize=None)
def _two_level_case(kind):
    """A root of 40 unknowns under children of 70, 33, 16 and 5: dense blocks, dense coupling of every child to the root,
    none between children.  The children share a level: its launches serve nodes with and without a second panel, with and
    without a finishing tile, with and without columns outside the block."""
    sizes = [70, 33, 16, 5, 40]
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32)
    n = int(sum(sizes))
    rng = np.random.default_rng(77)
    mask = np.zeros((n, n), bool)
    for f0, s in zip(first, sizes):
        mask[f0:f0 + s, f0:f0 + s] = True
    mask[first[-1]:, :] = True
    mask[:, first[-1]:] = True
    A = rng.uniform(-1.0, 1.0, (n, n))
    if kind == "c":
        A = A + 1j * rng.uniform(-1.0, 1.0, (n, n))
    A = np.where(mask, A, 0.0) + (n + 1.0) * np.eye(n)
    b = rng.standard_normal(n)
    if kind != "r":
        b = b + 1j * rng.standard_normal(n)
    tree = {"first": first, "size": np.array(sizes, np.int32), "parent": np.array([4, 4, 4, 4, -1], np.int32)}
    return A, b, np.linalg.solve(A, b), tree


@pytest.mark.parametrize("kind", ["c", "r", "rc"])
def test_two_levels_whose_nodes_end_at_different_places_in_a_block(hip_ctx, monkeypatch, kind):
    A, b, xref, tree = _two_level_case(kind)
    xs, launches = {}, {}
    for width in WIDTHS:
        _, f = _factor(hip_ctx, monkeypatch, width, A, tree)
        xs[width] = _solve(hip_ctx, f, b)
        launches[width] = f.info()["factor_launches"]
    _check(f"two levels, {kind}", A, b, xref, xs)
    print("kernel launches of the factorisation:", launches)
    assert 0 < launches["16"] < launches["8"] and 0 < launches[""] < launches["8"]


@pytest.mark.parametrize("kind", ["c", "r"])
@pytest.mark.parametrize("width", WIDTHS)
def test_singular_pivot_block_is_reported_at_both_widths(hip_ctx, monkeypatch, width, kind):
    """m = 24 whose column 12 is zero: the rank drops in the second half of a 16-column panel (the second panel of 8).  The
    elimination runs to its end on a substitute pivot and reports the column; the context works afterwards."""
    import lsa_hip

    A, b, xref = _dense_case(24, 0, kind)
    S = np.array(A)
    S[:, 12] = 0.0
    with pytest.raises(lsa_hip.LsaError, match=r"LSA_ERR_ZERO_PIVOT.*column 12") as exc:
        _factor(hip_ctx, monkeypatch, width, S, {"first": [0], "size": [24], "parent": [-1]})
    assert exc.value.status == lsa_hip.LSA_ERR_ZERO_PIVOT
    _, f = _factor(hip_ctx, monkeypatch, width, A, {"first": [0], "size": [24], "parent": [-1]})
    x = _solve(hip_ctx, f, b)
    assert np.linalg.norm(x - xref) <= ERR_BOUND * np.linalg.norm(xref)


@functools.lru_cache(maxsize=None)
def _s5k():
    import lsa_hip
    from synthetic import fem

    es = fem.cylinder_case("S5k")
    C = sp.csr_matrix((es.A.data - SIGMA * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
    o = lsa_hip.nd_order(C, 0)
    Cp = C[o["perm"]][:, o["perm"]].tocsr()
    Cp.sort_indices()
    rng = np.random.default_rng(21)
    b = rng.standard_normal(es.n) + 1j * rng.standard_normal(es.n)
    b.setflags(write=False)
    xref = spla.splu(Cp.tocsc()).solve(np.array(b))
    return Cp, b, xref, {"first": o["first"], "size": o["size"], "parent": o["parent"]}


def test_s5k_determinism_and_launch_count_at_both_widths(hip_ctx, monkeypatch):
    """Two factorisations of one matrix give the same bits (seen through the solution of one right-hand side), a refactorisation
    those of a fresh one, the widths agree to 1e-10, and 16-column panels take fewer kernel launches."""
    Cp, b, xref, tree = _s5k()
    xs, launches = {}, {}
    for width in WIDTHS:
        dC, f = _factor(hip_ctx, monkeypatch, width, Cp, tree)
        x = _solve(hip_ctx, f, b)
        launches[width] = f.info()["factor_launches"]
        _, g = _factor(hip_ctx, monkeypatch, width, Cp, tree)
        assert np.array_equal(_solve(hip_ctx, g, b), x)  # factored twice
        f.refactor(dC)
        assert f.info()["factor_launches"] == launches[width]
        assert np.array_equal(_solve(hip_ctx, f, b), x)  # refactored
        xs[width] = x
    _check("S5k", Cp, b, xref, xs)
    print("kernel launches of the factorisation:", launches)
    assert 0 < launches["16"] < launches["8"] and 0 < launches[""] < launches["8"]
