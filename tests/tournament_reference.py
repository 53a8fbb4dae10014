"""numpy walk of the tournament path of the exact LU (``launch_level_tp`` in ``csrc/ndlu_factor.hip``): one pivot block
inverted as the device inverts it (test infrastructure: no GPU, no import of the library; never imported by the product).

The walk, per block of ``NB`` = 32 columns (the last one may be narrower, w < 32):

* first round (``nd_tp_round_kernel<T, true, false>``): the rows are cut into sets of consecutive rows, 256 per set with
  complex factors and 512 with real ones; only rows that are no pivot rows yet take part.  Every set picks up to w rows by
  Gaussian elimination with partial pivoting on its slice of the block's columns: the largest ``|a|^2`` of the column among
  the rows still alive, ties to the lowest row, the row eliminated from the others;
* merge rounds (``<T, false, false>``, ``<T, false, true>``): the winners of ``TA`` = 8 sets meet and pick again, from the
  entries of the matrix as they stand (not from the eliminated copies), until one set is left;
* the w x w tile of the winners is inverted by Gauss-Jordan in the order the last elimination took the rows, with no further
  pivoting (``numpy.linalg.inv`` would pivot again);
* the rest of the block (``nd_tp_colblock_kernel``): pivot rows <- rows of D^-1, other rows <- -A[:, K] D^-1; then the
  rank-w update of all other columns (``nd_gj_stage_kernel`` + ``nd_gj_update_kernel``): other rows += W A[pivot rows],
  pivot rows <- D^-1 A[pivot rows];
* at the end ``L[a][b] = S[p_a][q_b]`` (``nd_unperm_kernel``): p_a the pivot row of column a, q its inverse.

Super-blocks and the look-ahead change the order in which the device applies these updates, not what is computed: the
walk has one order only.

Ties.  The device compares ``|a|^2`` with its low 16 mantissa bits replaced by the row (``pivot_key``): magnitudes within
2^-36 relative count as equal and go to the lowest row of a first-round set (in a merge round: to the earliest candidate).
The walk compares ``|a|^2`` exactly.  The two agree on inputs whose leading candidates are not that close; the families
below are such inputs: a planted pivot leads its column by a factor of 1e6, and two of some hundred Gaussian entries lie
within 2^-36 relative of one another with a probability of about 1e-8 per pick, 1e-3 over all picks of all cases here;
where a tie only reorders rows that lose anyway nothing changes at all.

Modes: ``"tournament"`` as above; ``"block"`` = partial pivoting over all free rows of the pivot block (what the
tournament approximates); ``"tile"`` = pivots taken inside the block's 32 x 32 diagonal tile only (the degraded behaviour
DESIGN.md records: two digits lost).

Input families, all seeded (``planted``, ``gaussian``, ``forest``), an extended-precision solve (``ExtSolver``) and the cases
the CPU and GPU tests share (``case``)."""

from __future__ import annotations

import functools

import numpy as np
import scipy.linalg as sla

from extended_reference import LD, matmul_ext

NB = 32  # columns of a block (kNB)
TA = 8  # candidate sets that meet in one merge workgroup (kTA)
SMALL = 1e-6
U = 2.0**-53

# the sizes of tests/test_gpu_tournament.py (tests/test_tournament_cpu.py checks the references on the same ones)
PLANTED_C = [1, 5, 31, 32, 33, 255, 256, 257, 288, 513, 2048, 2049, 2080]  # set edges 256/257, merge groups 8/9 sets (2048/2049)
PLANTED_R = [1, 33, 511, 512, 513, 1025]  # set edges 512/513
PLANTED_R_MIDDLE = 4128  # 9 first-round sets of 512 real rows: the middle merge round, a last block of 0 < w < 32
GAUSSIAN = [(257, "c"), (600, "c"), (1100, "c"), (2080, "c"), (257, "r"), (600, "r"), (1100, "r")]


def first_rows(dtype) -> int:
    """rows of a first-round set (``tp_first<T>::rows``)"""
    return 256 if np.dtype(dtype).kind == "c" else 512


def select(V, rows, w):
    """Up to w of ``rows`` by Gaussian elimination with partial pivoting on ``V`` (one row of w entries per candidate, in the
    order the device's threads hold them), in the order the elimination takes them.  ``V`` is not changed."""
    V = np.array(V[:, :w])
    alive = np.ones(len(rows), bool)
    taken = []
    for j in range(min(w, len(rows))):
        mag = np.where(alive, V[:, j].real ** 2 + V[:, j].imag ** 2, -1.0)
        p = int(np.argmax(mag))  # (the first of equal maxima: the lowest row, the earliest candidate)
        taken.append(int(rows[p]))
        alive[p] = False
        if mag[p] > 0.0:
            nf = np.where(alive, -V[:, j] / V[p, j], 0.0)
            V[:, j + 1:] += np.outer(nf, V[p, j + 1:])
    return taken


def pivot_rows(A, free, kb, w, mode):
    """The pivot rows of columns kb .. kb + w - 1 of the working matrix ``A``, in elimination order."""
    m = A.shape[0]
    if mode == "tile":
        rows = np.arange(kb, kb + w)
        return select(A[rows, kb:kb + w], rows, w)
    if mode == "block":
        rows = np.flatnonzero(free)
        return select(A[rows, kb:kb + w], rows, w)
    assert mode == "tournament", mode
    fr = first_rows(A.dtype)
    sets = []
    for s0 in range(0, m, fr):
        rows = s0 + np.flatnonzero(free[s0:s0 + fr])
        sets.append(select(A[rows, kb:kb + w], rows, w))
    while True:  # (a block with one first-round set still passes through the last round, as on the device)
        merged = []
        for g in range(0, len(sets), TA):
            rows = np.array(sum(sets[g:g + TA], []), dtype=np.int64)
            merged.append(select(A[rows, kb:kb + w], rows, w))
        sets = merged
        if len(sets) == 1:
            return sets[0]


def tile_inverse(D):
    """Gauss-Jordan in place, the pivots down the diagonal in the order given (the last workgroup of the tournament)."""
    D = np.array(D)
    for k in range(len(D)):
        pinv = 1.0 / D[k, k]
        rk = pinv * D[k, :]
        fi = D[:, k].copy()
        D -= np.outer(fi, rk)
        D[:, k] = -fi * pinv
        D[k, :] = rk
        D[k, k] = pinv
    return D


def invert(A0, mode="tournament"):
    """(inverse, pivot rows) of one pivot block.  ``pivot rows[j]`` = the row whose entry was the pivot of column j."""
    A = np.array(A0)
    m = A.shape[0]
    assert A.shape == (m, m)
    free = np.ones(m, bool)
    piv = np.empty(m, np.int64)
    for kb in range(0, m, NB):
        w = min(NB, m - kb)
        sel = np.array(pivot_rows(A, free, kb, w, mode), dtype=np.int64)
        assert len(sel) == w, "fewer free rows than columns"
        piv[kb:kb + w] = sel
        free[sel] = False
        Dinv = tile_inverse(A[sel, kb:kb + w])
        W = -A[:, kb:kb + w] @ Dinv  # (m x w; its pivot rows are replaced below)
        W[sel] = 0.0
        P = A[sel, :]  # (w x m) the pivot rows before the update
        P[:, kb:kb + w] = 0.0
        A += W @ P
        A[sel, :] = Dinv @ P
        A[:, kb:kb + w] = W
        A[sel, kb:kb + w] = Dinv
    q = np.empty(m, np.int64)
    q[piv] = np.arange(m)
    return A[np.ix_(piv, q)], piv


def eta(A, x, b):
    """|b - A x| / (|A|_F |x| + |b|), the normwise backward error of x (2-norms of the vectors)"""
    return float(np.linalg.norm(b - A @ x) / (np.linalg.norm(A, "fro") * np.linalg.norm(x) + np.linalg.norm(b)))


# ---- input families -------------------------------------------------------------------------------------------------


def _rhs(rng, m, cplx):
    b = rng.standard_normal(m)
    return b + 1j * rng.standard_normal(m) if cplx else b


def planted_block(rng, m, cplx):
    """An m x m block whose entries are SMALL * uniform(-1, 1) (+ i the same for complex) except one entry per column j, in
    row ``perm[j]`` of a random permutation, of modulus uniform in [1, 2] and random sign or phase.  The only correct pivot of
    column j is row ``perm[j]``; every correct multiplier is at most 2e-6 (no growth); condition number <= 2.1."""
    B = SMALL * rng.uniform(-1.0, 1.0, (m, m))
    if cplx:
        B = B + 1j * SMALL * rng.uniform(-1.0, 1.0, (m, m))
    perm = rng.permutation(m)
    mod = rng.uniform(1.0, 2.0, m)
    B[perm, np.arange(m)] = mod * np.exp(2j * np.pi * rng.random(m)) if cplx else mod * rng.choice([-1.0, 1.0], m)
    return B, perm


def planted(m, cplx, b_cplx=None):
    """(A, b, perm) of the planted family; ``b_cplx`` = a complex right-hand side (default: as the matrix)."""
    rng = np.random.default_rng(7000 + 2 * m + int(cplx))
    A, perm = planted_block(rng, m, cplx)
    b = _rhs(rng, m, cplx if b_cplx is None else b_cplx)
    return A, b, perm


def gaussian(m, cplx, b_cplx=None):
    """(A, b) with standard normal entries (+ i normal for complex); condition numbers of 1e3 to 1e4 at the sizes used.
    The seeds are chosen so that pivoting inside the diagonal tile costs every case of the GPU tests a factor of 30 or more
    in eta (tests/test_tournament_cpu.py asserts it; with the base 9000 the complex case m = 257 lost only a factor of 10)."""
    rng = np.random.default_rng(9500 + 2 * m + int(cplx))
    A = rng.standard_normal((m, m))
    if cplx:
        A = A + 1j * rng.standard_normal((m, m))
    b = _rhs(rng, m, cplx if b_cplx is None else b_cplx)
    return A, b


FOREST_SIZES = [600, 300, 257, 40, 5, 530]  # five children and, last, their parent


def forest(cplx):
    """(A, b, perm, tree): five children of 600, 300, 257, 40 and 5 unknowns under a root of 530, in the shape of
    ``test_gpu_gj_panels._two_level_case``: every node's own block is a planted block (its pivots inside its own rows: no
    pivot crosses a front), every child is coupled to the root by dense blocks of SMALL * uniform(-1, 1) entries in both
    directions, children are not coupled to one another.  The root needs no rescaling to keep its planted pivots: a child
    of s unknowns changes the root's block by C_rt A_t^-1 C_tr, entries of at most s * 1e-12, against off-pivot entries of
    1e-6 and pivots of 1 to 2 (tests/test_tournament_cpu.py checks the Schur complement's pivots with the walk).
    ``perm[j]`` = the row of column j's planted entry, over the whole matrix."""
    sizes = FOREST_SIZES
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32)
    n, r0 = int(sum(sizes)), int(first[-1])
    rng = np.random.default_rng(4100 + int(cplx))
    A = np.zeros((n, n), np.complex128 if cplx else np.float64)
    perm = np.empty(n, np.int64)

    def small(shape):
        c = SMALL * rng.uniform(-1.0, 1.0, shape)
        return c + 1j * SMALL * rng.uniform(-1.0, 1.0, shape) if cplx else c

    for f0, s in zip(first, sizes):
        A[f0:f0 + s, f0:f0 + s], p = planted_block(rng, s, cplx)
        perm[f0:f0 + s] = f0 + p
        if f0 != r0:
            A[f0:f0 + s, r0:] = small((s, n - r0))
            A[r0:, f0:f0 + s] = small((n - r0, s))
    b = _rhs(rng, n, cplx)
    nt = len(sizes)
    tree = {"first": first, "size": np.array(sizes, np.int32), "parent": np.array([nt - 1] * (nt - 1) + [-1], np.int32)}
    return A, b, perm, tree


# ---- extended-precision solutions -------------------------------------------------------------------------------------


class ExtSolver:
    """Solutions of ``op(A) x = b`` in ``np.longdouble``: LAPACK's solution plus one step of iterative refinement whose residual
    is formed in longdouble (tests/extended_reference.py).  With cond(A) u << 1 the refined solution's relative error is about
    (cond(A) u)^2 + 2^-64 cond(A): far below anything a double-precision solve reaches."""

    def __init__(self, A):
        self.A = np.asarray(A)
        self.lu = sla.lu_factor(self.A)

    def solve(self, b, trans="N"):
        """``trans``: "N", "T" or "H".  Returns (re, im) longdouble parts (im None for a real system)."""
        A = {"N": self.A, "T": self.A.T, "H": self.A.conj().T}[trans]
        t = {"N": 0, "T": 1, "H": 2}[trans]
        x0 = sla.lu_solve(self.lu, b, trans=t)
        ax = matmul_ext(A, x0[:, None])
        rr = np.asarray(b).real.astype(LD) - ax.re[:, 0]
        cplx = ax.im is not None
        r = rr.astype(np.float64)
        if cplx:
            ri = np.asarray(b).imag.astype(LD) - ax.im[:, 0]
            r = r + 1j * ri.astype(np.float64)
        d = sla.lu_solve(self.lu, r, trans=t)
        return x0.real.astype(LD) + d.real.astype(LD), (x0.imag.astype(LD) + d.imag.astype(LD)) if cplx else None


def forward_error(x, ref):
    """|x - ref| / |ref| with the difference taken in longdouble; ``ref`` = the (re, im) parts of :meth:`ExtSolver.solve`."""
    re, im = ref
    x = np.asarray(x)
    d2 = np.sum((x.real.astype(LD) - re) ** 2)
    n2 = np.sum(re**2)
    if im is not None:
        d2 += np.sum((x.imag.astype(LD) - im) ** 2)
        n2 += np.sum(im**2)
    else:
        d2 += np.sum(x.imag.astype(LD) ** 2)
    return float(np.sqrt(d2 / n2))


# ---- the cases the CPU and the GPU tests share (computed once per process, read-only) --------------------------------------


class Case:
    """One matrix with its right-hand side and everything the bounds need.  ``ref[trans]`` = the extended-precision solution of
    op(A) x = b; for the Gaussian family also ``inverse`` (the walk's, mode "tournament"), ``eta_walk`` and ``eta_lapack``
    for this right-hand side and ``cond`` (2-norm)."""


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _base(family, m, cplx):
    c = Case()
    if family == "planted":
        c.A, _, c.perm = planted(m, cplx)
    elif family == "forest":
        c.A, _, c.perm, c.tree = forest(cplx)
    else:
        c.A, _ = gaussian(m, cplx)
        c.inverse, c.piv = invert(c.A)
        c.cond = float(np.linalg.cond(c.A))
        _freeze(c.inverse)
    _freeze(c.A)
    c.solver = ExtSolver(c.A) if m <= 2500 else None  # (the one larger case is solved once and its factors dropped)
    return c


@functools.lru_cache(maxsize=None)
def case(family, m, kind):
    """``kind``: 'c' complex matrix and vector, 'r' real matrix and vector, 'rc' real matrix and complex vector."""
    base = _base(family, m, kind == "c")
    c = Case()
    c.__dict__.update(base.__dict__)
    c.family, c.m, c.kind = family, m, kind
    c.b = {"planted": lambda: planted(m, kind == "c", kind != "r")[1], "forest": lambda: forest(kind == "c")[1],
           "gaussian": lambda: gaussian(m, kind == "c", kind != "r")[1]}[family]()
    _freeze(c.b)
    solver = base.solver or ExtSolver(c.A)
    c.ref = {t: solver.solve(c.b, t) for t in (("N", "T", "H") if kind == "c" else ("N", "T"))}
    if kind != "c":
        c.ref["H"] = c.ref["T"]
    if family == "gaussian":
        c.eta_walk = eta(c.A, c.inverse @ c.b, c.b)
        c.eta_lapack = eta(c.A, sla.lu_solve(solver.lu, c.b), c.b)
    c.solver = None
    return c
