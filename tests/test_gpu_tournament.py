"""GPU suite: the tournament path of the exact LU (``launch_level_tp`` in ``csrc/ndlu_factor.hip``: ``nd_tp_round_kernel`` in its
three instances, ``nd_tp_colblock_kernel``, the staged rank-32 / super-block updates, the look-ahead on a second stream)
held to the accuracy of partial pivoting, on hand-made dense forests at every edge of the path.

References (``tests/tournament_reference.py``, checked on the CPU by ``tests/test_tournament_cpu.py``): an extended-precision
solution of every system (LAPACK plus one step of refinement with a longdouble residual) and the numpy walk of the
tournament.  eta = |b - A x| / (|A|_F |x| + |b|).

Bounds, none of them taken from what the device gives:

* planted family and the forest (one entry of modulus 1 to 2 per column at a random row, everything else 1e-6; condition
  number <= 2.1; the only correct pivot of a column is its planted row): eta <= 1e-14, forward error <= 1e-12.  The walk is
  at 2e-17 and 9e-16; a tournament that loses one merge group is at 1e-11 and 5e-10
  (test_tournament_cpu.py::test_a_tournament_that_loses_its_second_merge_group_misses_the_planted_bounds).
* Gaussian family (condition numbers 5e2 to 4e3): eta of ``solve`` and of both adjoint solves <= 10 x the eta of the walk
  (mode "tournament") on the same matrix and right-hand side, computed in the test; forward error <= cond(A) 64 u.  FMA
  contraction and another order of summation move eta by a small factor, LAPACK lies within 2 x of the walk, and pivots
  chosen inside the diagonal tile only lie 66 x to 9e4 x away on these very matrices (test_tournament_cpu.py).

Every case asserts (a) both bounds for ``solve``, (b) the same for A^T and A^H through ``solve_adjoint``, (c) that a second
factorisation and a ``refactor`` give the same bits, (d) the solution's dtype.

Measured on the MI355X (eta of solve / A^T / A^H; the walk; LAPACK):

    case            device (solve / A^T / A^H)      walk     LAPACK   cond
    complex  257    4.9e-16 / 4.1e-16 / 4.0e-16     4.3e-16  3.3e-16  8.8e2
    complex  600    8.2e-16 / 6.2e-16 / 6.1e-16     7.2e-16  4.0e-16  1.9e3
    complex 1100    8.6e-16 / 6.8e-16 / 7.2e-16     7.6e-16  4.6e-16  2.5e3
    complex 2080    1.0e-15 / 9.5e-16 / 9.3e-16     8.9e-16  6.6e-16  3.8e3
    real     257    2.2e-16 / 1.6e-16 / 1.6e-16     1.9e-16  1.4e-16  5.0e2
    real     600    3.8e-16 / 3.0e-16 / 3.0e-16     3.9e-16  2.4e-16  1.5e3
    real    1100    4.4e-16 / 3.8e-16 / 3.8e-16     4.1e-16  3.4e-16  1.8e3

(one node, plain tournament; in super-blocks the largest is 1.5e-15, complex m = 600 at 128 columns, twice the walk's.)  The
planted cases and the forest come out at eta <= 5e-17 and a forward error <= 1.2e-15.  With the first round's candidates
taken from the diagonal tile only (a scratch build, not kept) every planted case from m = 33 on lands at eta 6e-12 to 8e-5
and every Gaussian case at 7 x to 9000 x the walk's eta, while the FEM tests of tests/test_gpu_ndlu.py still pass.

The knobs are read at every set-up of a factorisation, and a factorisation parked in the context keeps the ones it was set
up with: every test switches the parking off (``LSA_ND_NO_CACHE``)."""

import numpy as np
import pytest
import scipy.sparse as sp

import tournament_reference as tr
from tournament_reference import GAUSSIAN, PLANTED_C, PLANTED_R, PLANTED_R_MIDDLE

pytestmark = pytest.mark.gpu

KNOBS = ("LSA_ND_TP_MIN", "LSA_ND_SB_MIN", "LSA_ND_SB_COLS", "LSA_ND_LOOKAHEAD_MIN")
FORCED = {"LSA_ND_TP_MIN": "1", "LSA_ND_SB_MIN": "100000", "LSA_ND_LOOKAHEAD_MIN": "100000"}  # one node, plain tournament
PLANTED_ETA, PLANTED_ERR = 1e-14, 1e-12
TRANS = {"N": lambda A: A, "T": lambda A: A.T, "H": lambda A: A.conj().T}


def _device_matrix(ctx, M):
    import lsa_hip

    M = sp.csr_matrix(M)
    M.sort_indices()
    return lsa_hip.CsrMatrix.from_scipy(ctx, M)


def _factor(ctx, monkeypatch, env, dM, tree):
    """``env``: the knobs of the tournament path; a knob that is not named is unset."""
    import lsa_hip

    monkeypatch.setenv("LSA_ND_NO_CACHE", "1")
    for k in KNOBS:
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)
    return lsa_hip.NdLu(ctx, dM, tree=tree)


def _solve(ctx, f, b, trans="N"):
    import lsa_hip

    dx = lsa_hip.DeviceVector(ctx, len(b), b.dtype)
    db = lsa_hip.DeviceVector.from_numpy(ctx, np.array(b))
    if trans == "N":
        f.solve(db, dx)
    else:
        f.solve_adjoint(db, dx, conj=trans == "H")
    return dx.numpy()


def _tree(c):
    return getattr(c, "tree", None) or {"first": [0], "size": [c.A.shape[0]], "parent": [-1]}


def _bounds(c):
    """(eta bound, forward error bound) of a case"""
    if c.family == "gaussian":
        return 10.0 * c.eta_walk, c.cond * 64 * tr.U
    return PLANTED_ETA, PLANTED_ERR


def _run(ctx, monkeypatch, env, c, label):
    """Factor and solve one case under ``env``; assert (a) to (d); return the three solutions and the kernel launches of the
    factorisation."""
    dM = _device_matrix(ctx, c.A)
    f = _factor(ctx, monkeypatch, env, dM, _tree(c))
    xs = {t: _solve(ctx, f, c.b, t) for t in TRANS}
    launches = f.info()["factor_launches"]
    g = _factor(ctx, monkeypatch, env, dM, _tree(c))
    again = {t: _solve(ctx, g, c.b, t) for t in TRANS}
    del g
    f.refactor(dM)
    redone = {t: _solve(ctx, f, c.b, t) for t in TRANS}
    eta_bound, err_bound = _bounds(c)
    etas = {}
    for t, op in TRANS.items():
        etas[t] = tr.eta(op(c.A), xs[t], c.b)
        err = tr.forward_error(xs[t], c.ref[t])
        print(f"{label} {t}: eta = {etas[t]:.2e} (bound {eta_bound:.2e}), forward error = {err:.2e} (bound {err_bound:.2e})")
    if c.family == "gaussian":
        print(f"{label}: | device eta {etas['N']:.1e} / {etas['T']:.1e} / {etas['H']:.1e} | walk {c.eta_walk:.1e} | LAPACK {c.eta_lapack:.1e} |"
              f" cond {c.cond:.1e}")
    for t, op in TRANS.items():
        assert xs[t].dtype == c.b.dtype  # (d)
        assert etas[t] <= eta_bound  # (a), (b)
        assert tr.forward_error(xs[t], c.ref[t]) <= err_bound
        assert np.array_equal(again[t], xs[t])  # (c) factored twice
        assert np.array_equal(redone[t], xs[t])  # (c) refactored
    return xs, launches


# ---- one node, the tournament forced onto every size --------------------------------------------------------------------------


@pytest.mark.parametrize("m,kind", [(m, "c") for m in PLANTED_C] + [(m, k) for m in PLANTED_R for k in ("r", "rc")] + [(PLANTED_R_MIDDLE, "r")])
def test_one_node_planted_pivots(hip_ctx, monkeypatch, m, kind):
    """The planted family at the edges of the path: a last column block of w < 32 columns (every m that is no multiple of 32,
    m < 32 included), the set boundaries 256 / 257 (complex) and 512 / 513 (real), sets whose rows are all taken before the last
    blocks (m = 288: the 32 rows of the second set), the merge-group boundary of 8 / 9 sets (m = 2048 / 2049 complex) and the
    middle merge round ``nd_tp_round_kernel<T, false, false>`` (m = 2049, 2080 complex; m = 4128 real).  The 32 pivots of every
    column block are scattered over all sets; a result inside the bounds has found every one of them."""
    c = tr.case("planted", m, kind)
    _run(hip_ctx, monkeypatch, FORCED, c, f"planted m = {m} {kind}")


@pytest.mark.parametrize("m,kind", GAUSSIAN + [(257, "rc"), (600, "rc")])
def test_one_node_gaussian_within_ten_times_the_walk(hip_ctx, monkeypatch, m, kind):
    """Matrices on which the choice of pivot rows decides the answer: the device's eta against the walk's."""
    c = tr.case("gaussian", m, kind)
    _run(hip_ctx, monkeypatch, FORCED, c, f"gaussian m = {m} {kind}")


@pytest.mark.parametrize("kind", ["c", "r"])
def test_zero_pivot_is_reported_with_its_column(hip_ctx, monkeypatch, kind):
    """Planted, m = 300, one column zeroed: first the first column whose planted row lies in rows 256 .. 299 (the second set of
    complex factors; real factors hold all 300 rows in one set) and that is outside the last block, then column 293 of the
    last, partial block (columns 288 .. 299).  The elimination runs to its end on a substitute pivot and names the column;
    the context factors the intact matrix afterwards.  (After tests/test_gpu_gj_panels.py::
    test_singular_pivot_block_is_reported_at_both_widths.)"""
    import lsa_hip

    c = tr.case("planted", 300, kind)
    tree = _tree(c)
    second_set = next(j for j in range(288) if c.perm[j] >= 256)
    for col in (second_set, 293):
        S = np.array(c.A)
        S[:, col] = 0.0
        with pytest.raises(lsa_hip.LsaError, match=rf"LSA_ERR_ZERO_PIVOT.*column {col}\b") as exc:
            _factor(hip_ctx, monkeypatch, FORCED, _device_matrix(hip_ctx, S), tree)
        assert exc.value.status == lsa_hip.LSA_ERR_ZERO_PIVOT
        _run(hip_ctx, monkeypatch, FORCED, c, f"planted m = 300 {kind} after a zero pivot in column {col}")


# ---- one level whose nodes differ in height ------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["c", "r"])
def test_one_level_with_mixed_heights(hip_ctx, monkeypatch, kind):
    """The forest of ``tournament_reference.forest``: children of 600, 300, 257, 40 and 5 unknowns under a root of 530, every
    node's own block planted, couplings of 1e-6 between every child and the root, none between children.  With
    ``LSA_ND_TP_MIN=64`` the children's level is a tournament level: the nodes of 40 and 5 rows ride in the launches of the
    node of 600 (they leave after their last block, their sets beyond the first are empty), as the small nodes of a
    production level do.  The same forest on the panel path (``LSA_ND_TP_MIN=100000``) agrees to 1e-12 relative."""
    c = tr.case("forest", 0, kind)
    xs, launches = _run(hip_ctx, monkeypatch, {"LSA_ND_TP_MIN": "64"}, c, f"forest {kind}, tournament")
    xp, launches_panels = _run(hip_ctx, monkeypatch, {"LSA_ND_TP_MIN": "100000"}, c, f"forest {kind}, panels")
    print(f"forest {kind}: kernel launches of the factorisation: tournament {launches}, panels {launches_panels}")
    assert launches != launches_panels  # the knob reached the factorisation: two different launch sequences were compared
    for t in TRANS:
        d = np.linalg.norm(xs[t] - xp[t]) / np.linalg.norm(xp[t])
        print(f"forest {kind} {t}: |x_tournament - x_panels| / |x_panels| = {d:.2e}")
        assert d <= 1e-12


# ---- super-blocks and look-ahead ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("family,m,kind", [("forest", 0, "c"), ("forest", 0, "r"), ("gaussian", 257, "c"), ("gaussian", 257, "r"),
                                           ("gaussian", 600, "c"), ("gaussian", 600, "r")])
def test_super_blocks_and_look_ahead(hip_ctx, monkeypatch, family, m, kind):
    """Super-blocks of 64, 128 (the default: ``LSA_ND_SB_COLS`` unset) and 192 columns from 130 rows on, each without and with
    the second-stream look-ahead (``LSA_ND_LOOKAHEAD_MIN`` = 100000 / 131): partial last super-blocks at every width (257 =
    4 x 64 + 1 = 2 x 128 + 1 = 192 + 65; 600 = 9 x 64 + 24 = 4 x 128 + 88 = 3 x 192 + 24; the forest's 530, 300 and 257
    alike, its nodes of 40 and 5 rows ending inside the first super-block).  The bounds hold at every setting; the
    look-ahead changes which stream runs the tournament, not one bit of the result; widths differ in their order of
    summation and agree to 10 x the eta bound, measured as eta is: |A (x - x')| / (|A|_F |x'| + |b|) (the relative difference
    of the solutions is printed beside it)."""
    c = tr.case(family, m, kind)
    eta_bound, _ = _bounds(c)
    heights = [max(tr.FOREST_SIZES[:-1]), tr.FOREST_SIZES[-1]] if family == "forest" else [m]  # the tallest pivot block of every level
    xs, launches = {}, {}
    for cols in ("64", "", "192"):
        for ahead in ("100000", "131"):
            env = {"LSA_ND_TP_MIN": "64", "LSA_ND_SB_MIN": "130", "LSA_ND_LOOKAHEAD_MIN": ahead}
            if cols:
                env["LSA_ND_SB_COLS"] = cols
            label = f"{family} {m} {kind}, super-blocks of {cols or 'default'}, look-ahead from {ahead}"
            xs[cols, ahead], launches[cols, ahead] = _run(hip_ctx, monkeypatch, env, c, label)
        for t in TRANS:
            assert np.array_equal(xs[cols, "131"][t], xs[cols, "100000"][t])
        # with the look-ahead the update after a super-block that has a successor is two launches (the next block's 32 columns
        # first): one more launch per super-block but the last of every level, which shows that LSA_ND_SB_COLS and
        # LSA_ND_LOOKAHEAD_MIN both reached the factorisation
        successors = sum(-(-h // int(cols or 128)) - 1 for h in heights)
        assert launches[cols, "131"] - launches[cols, "100000"] == successors
    print(f"{family} {m} {kind}: kernel launches of the factorisation: {launches}")
    for cols in ("64", "192"):
        for t, op in TRANS.items():
            x, y = xs[cols, "131"][t], xs["", "131"][t]
            A = op(c.A)
            d_eta = np.linalg.norm(A @ (x - y)) / (np.linalg.norm(A, "fro") * np.linalg.norm(y) + np.linalg.norm(c.b))
            d_rel = np.linalg.norm(x - y) / np.linalg.norm(y)
            print(f"{family} {m} {kind} {t}: super-blocks of {cols} against the default: eta of the difference {d_eta:.2e} "
                  f"(bound {10 * eta_bound:.2e}), |x - x'| / |x'| = {d_rel:.2e}")
            assert d_eta <= 10 * eta_bound
