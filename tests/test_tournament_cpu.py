"""The numpy walk of the tournament path (``tests/tournament_reference.py``) checked against LAPACK and extended precision,
and the input families of ``tests/test_gpu_tournament.py`` checked for what that file relies on.  No GPU, no library.

Sizes: the lists of ``tournament_reference`` are the ones the GPU file runs, so that every property is shown on the very
matrices the device sees."""

import numpy as np
import pytest
import scipy.linalg as sla

import tournament_reference as tr

U = tr.U
PLANTED_ALL = [(m, True) for m in tr.PLANTED_C] + [(m, False) for m in tr.PLANTED_R + [tr.PLANTED_R_MIDDLE]]
GAUSSIAN = tr.GAUSSIAN


def _lapack_panel_pivots(panel):
    """rows that LAPACK's partial pivoting takes for the columns of an m x w panel, in order"""
    _, swaps = sla.lu_factor(panel)
    rows = np.arange(panel.shape[0])
    for j in range(panel.shape[1]):
        rows[[j, swaps[j]]] = rows[[swaps[j], j]]
    return rows[:panel.shape[1]]


def _textbook_panel_pivots(panel):
    """the same by the textbook loop, the pivot the entry of largest modulus (rows swapped, one column at a time)"""
    P = np.array(panel)
    rows = np.arange(P.shape[0])
    for j in range(P.shape[1]):
        p = j + int(np.argmax(np.abs(P[j:, j])))
        P[[j, p]], rows[[j, p]] = P[[p, j]], rows[[p, j]]
        P[j + 1:, j + 1:] -= np.outer(P[j + 1:, j] / P[j, j], P[j, j + 1:])
    return rows[:P.shape[1]]


@pytest.mark.parametrize("m,cplx", [(33, True), (255, True), (256, True), (33, False), (300, False), (511, False), (512, False)])
def test_a_single_set_picks_the_rows_of_lapacks_partial_pivoting(m, cplx):
    """One set holds all rows (complex m <= 256, real m <= 512): the tournament of the first column block is partial pivoting
    on that 32-column panel, so its rows are those of ``scipy.linalg.lu_factor``, in the same order (the last round picks
    again among the first round's 32 winners and must confirm them).

    Complex factors: LAPACK's ``izamax`` ranks by |re| + |im|, the device and the walk by the modulus, so on a general complex
    panel the two rightly differ (seen here at the second pivot of m = 33).  LAPACK is therefore asked about a complex panel on
    which both measures rank alike -- exp(0.7 i) times the real Gaussian panel: one common phase, which the elimination
    keeps -- and the general complex Gaussian panel is compared with the textbook loop that pivots by modulus."""
    A, _ = tr.gaussian(m, cplx)
    assert m <= tr.first_rows(A.dtype)
    every = np.ones(m, bool)
    if cplx:
        got = tr.pivot_rows(A, every, 0, tr.NB, "tournament")
        assert np.array_equal(got, _textbook_panel_pivots(A[:, :tr.NB]))
        A = np.exp(0.7j) * tr.gaussian(m, False)[0]
    got = tr.pivot_rows(A, every, 0, tr.NB, "tournament")
    assert np.array_equal(got, _lapack_panel_pivots(A[:, :tr.NB]))
    assert np.array_equal(got, _textbook_panel_pivots(A[:, :tr.NB]))
    assert np.array_equal(got, tr.pivot_rows(A, every, 0, tr.NB, "block"))


@pytest.mark.parametrize("m,cplx", PLANTED_ALL)
def test_planted_pivots_are_found_exactly(m, cplx):
    """The walk returns ``perm`` at every size of the GPU list, and its inverse satisfies max |A inverse - I| <=
    64 u (sqrt(m) cond + 1) with cond <= 2.1.  (Column j of the inverse solves A x = e_j; a backward error eta gives a
    residual of at most eta (|A|_F |x| + 1) <= eta (sqrt(m) cond_2(A) + 1) in the 2-norm, which bounds every entry;
    eta = 64 u allows eight times the 8 u that the walk and LAPACK show on these families.  Measured: 2e-16 to 5e-16.)"""
    A, b, perm = tr.planted(m, cplx)
    inverse, piv = tr.invert(A)
    assert np.array_equal(piv, perm)
    defect = np.abs(A @ inverse - np.eye(m)).max()
    e = tr.eta(A, inverse @ b, b)
    print(f"planted m = {m} {'complex' if cplx else 'real'}: max |A inverse - I| = {defect:.2e}, eta = {e:.2e}")
    assert defect <= 64 * U * (np.sqrt(m) * 2.1 + 1.0)
    assert e <= 1e-14  # the planted bound of the GPU tests, on the reference


def test_a_tournament_that_loses_its_second_merge_group_misses_the_planted_bounds(monkeypatch):
    """The planted family tells a broken tournament from a whole one: rows past the first eight sets never reach the merge
    (m = 2080 complex: sets 8 and 9 are lost), and both planted bounds of the GPU tests are missed by orders of magnitude."""
    A, b, perm = tr.planted(2080, True)
    whole = tr.pivot_rows

    def broken(A, free, kb, w, mode):
        kept = free.copy()
        kept[tr.TA * tr.first_rows(A.dtype):] = False
        return whole(A, kept if kept.sum() >= w else free, kb, w, mode)

    monkeypatch.setattr(tr, "pivot_rows", broken)
    inverse, piv = tr.invert(A)
    assert not np.array_equal(piv, perm)
    x = inverse @ b
    e, err = tr.eta(A, x, b), tr.forward_error(x, tr.ExtSolver(A).solve(b))
    print(f"second merge group lost: eta = {e:.2e}, forward error = {err:.2e}")
    assert e > 100 * 1e-14 and err > 100 * 1e-12


@pytest.mark.parametrize("m,kind", GAUSSIAN)
def test_gaussian_cases_modes_discrimination_and_inverse(m, kind):
    """On every Gaussian case of the GPU file:

    * modes "tournament" and "block" solve to a forward error within cond(A) 64 u of the extended-precision solution;
    * eta of mode "tile" is at least 30 times eta of mode "tournament" -- a condition on the INPUT: it shows that the case
      tells pivoting inside the diagonal tile from a tournament, with the factor 10 of the GPU bound three times inside;
    * max |A inverse - I| <= 64 u (sqrt(m) cond_2(A) + 1) for modes "tournament" and "block" (derivation: see
      test_planted_pivots_are_found_exactly).
    """
    c = tr.case("gaussian", m, kind)
    A, b = c.A, c.b
    etas = {}
    for mode in ("tournament", "block", "tile"):
        inverse = c.inverse if mode == "tournament" else tr.invert(A, mode)[0]
        x = inverse @ b
        etas[mode] = tr.eta(A, x, b)
        err = tr.forward_error(x, c.ref["N"])
        defect = np.abs(A @ inverse - np.eye(m)).max()
        print(f"gaussian m = {m} {kind} {mode}: eta = {etas[mode]:.2e}, forward error = {err:.2e} (cond = {c.cond:.1e}), "
              f"max |A inverse - I| = {defect:.2e}")
        if mode != "tile":
            assert err <= c.cond * 64 * U
            assert defect <= 64 * U * (np.sqrt(m) * c.cond + 1.0)
    print(f"gaussian m = {m} {kind}: eta LAPACK = {c.eta_lapack:.2e}, tile / tournament = {etas['tile'] / etas['tournament']:.0f}")
    assert etas["tile"] >= 30 * etas["tournament"]
    assert etas["tournament"] <= 4 * c.eta_lapack and etas["block"] <= 4 * c.eta_lapack  # (the issue saw them within 2 x)


@pytest.mark.parametrize("cplx", [True, False])
def test_forest_case_keeps_its_planted_pivots_and_its_reference_meets_the_planted_bound(cplx):
    """The two-level forest of the GPU file: a dense LAPACK solve of the whole matrix has eta <= 1e-14 and a forward error <=
    1e-12 (the planted bounds), and the root's Schur complement -- its block minus C_rt A_t^-1 C_tr over the children --
    still has the root's planted rows as the walk's pivots."""
    c = tr.case("forest", 0, "c" if cplx else "r")
    A, b, perm = c.A, c.b, c.perm
    x = np.linalg.solve(A, b)
    e, err = tr.eta(A, x, b), tr.forward_error(x, c.ref["N"])
    print(f"forest {'complex' if cplx else 'real'}: LAPACK eta = {e:.2e}, forward error = {err:.2e}")
    assert e <= 1e-14 and err <= 1e-12
    first, size = c.tree["first"], c.tree["size"]
    r0 = int(first[-1])
    S = np.array(A[r0:, r0:])
    for f0, s in zip(first[:-1], size[:-1]):
        own = slice(int(f0), int(f0 + s))
        inverse, piv = tr.invert(A[own, own])
        assert np.array_equal(piv + f0, perm[own])
        S -= A[r0:, own] @ inverse @ A[own, r0:]
    assert np.array_equal(tr.invert(S)[1] + r0, perm[r0:])
