"""Linear solves with a kept factorisation: one Jacobian-like matrix, several right-hand sides, then new values.

The shape of the reference's Newton loop (``Solver/nonlinear.py:48``: one ``iKSP`` built for the Jacobian and reused by every
step) and of its cached linear solvers (``Solver/linear.py``), on the HIP path: ``Solver.utils.iKSP`` orders, analyses and
factors at the first solve, keeps the exact LU, and a matrix with the same pattern only refactors.

    python lsa-fw_amd/examples/linear_solves.py [--case S5k] [--rhs 6]

The matrix is the synthetic cylinder operator shifted off its spectrum (``A + 0.5 M``: a Jacobian-like saddle-point matrix),
the second one the same pattern at another shift.
"""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np
import scipy.sparse as sp

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "lsa-fw_amd")]

from Solver.utils import KSPType, PreconditionerType, iKSP  # noqa: E402
from synthetic import fem  # noqa: E402


def jacobian(es, shift: float) -> sp.csr_matrix:
    return sp.csr_matrix((es.A.data + shift * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="S5k")
    ap.add_argument("--rhs", type=int, default=6)
    args = ap.parse_args()
    es = fem.cylinder_case(args.case)
    J = jacobian(es, 0.5)
    rng = np.random.default_rng(0)
    B = rng.standard_normal((es.n, args.rhs))

    ksp = iKSP(J)
    ksp.set_type(KSPType.PREONLY)
    ksp.set_preconditioner(PreconditionerType.LU)
    ksp.set_tolerances(rtol=1e-10)

    t0 = time.time()
    x = ksp.solve(B[:, 0]).as_array()  # orders, analyses, factors
    print(f"first solve {time.time() - t0:.3f} s: |b - J x|/|b| = {np.linalg.norm(B[:, 0] - J @ x) / np.linalg.norm(B[:, 0]):.1e}, stats {ksp.stats}")
    t0 = time.time()
    for q in range(1, args.rhs):  # the kept factors, one sweep per right-hand side
        ksp.solve(B[:, q])
    print(f"{args.rhs - 1} further solves {time.time() - t0:.3f} s, stats {ksp.stats}")
    t0 = time.time()
    X = ksp.solve_many(B)  # all right-hand sides in one block solve: every factor scalar read once per pass
    print(f"block solve of {args.rhs} columns {time.time() - t0:.3f} s: |B - J X|/|B| = {np.linalg.norm(B - J @ X) / np.linalg.norm(B):.1e}, "
          f"pass width {ksp.stats['multi_width']}")

    # the adjoint systems J^H Y = B on the same factors (sensitivities): column by column by default, in the wide passes of the
    # block solve above with block_adjoint -- the same bits either way
    t0 = time.time()
    Y = ksp.solve_many(B, adjoint=True)
    t1 = time.time()
    ksp.block_adjoint = True
    Yb = ksp.solve_many(B, adjoint=True)
    print(f"adjoint block solve {t1 - t0:.3f} s column by column, {time.time() - t1:.3f} s with block_adjoint (pass width {ksp.stats['multi_width']}): "
          f"|B - J^H Y|/|B| = {np.linalg.norm(B - J.conj().T @ Yb) / np.linalg.norm(B):.1e}, same bits: {np.array_equal(Y, Yb)}")

    J2 = jacobian(es, 0.7)  # the next Newton step's Jacobian: the same pattern, new values
    ksp.set_operators(J2)
    t0 = time.time()
    X2 = ksp.solve_many(B)
    print(f"refactor + block solve {time.time() - t0:.3f} s: |B - J2 X|/|B| = {np.linalg.norm(B - J2 @ X2) / np.linalg.norm(B):.1e}, stats {ksp.stats}")
    ksp.reset()


if __name__ == "__main__":
    main()
