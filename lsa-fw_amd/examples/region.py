"""All eigenvalues of a synthetic cylinder case inside a region of the complex plane, with a statement of completeness
(``RegionEigenSolver``): the question "is anything in this part of the plane, and is that all of it?" that a Krylov-Schur run at a
target cannot answer.

    python lsa-fw_amd/examples/region.py [--case S5k] [--region A B C D] [--ellipse RE IM RX RY] [--nodes 16] [--subspace 48]
                                          [--two-sided]

``--region A B C D`` is the rectangle ``A < Re < B``, ``C < Im < D`` (the arguments of ``set_interval_complex``), solved on its
circumscribing ellipse; the default is the circle of radius 0.12 about the least stable eigenvalue 0.018 + 0.738j of the wake at
Re = 50.  The spectrum is dense: when the run reports a full subspace, raise ``--subspace`` (the printed estimate helps) or shrink the
region.  ``--two-sided`` adds the left phase on the same factor sets and prints every eigenvalue with its condition number ``kappa``
and its left residual.  Needs an AMD GPU (there is no CPU fallback).
"""

from __future__ import annotations

import argparse
import logging
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "lsa-fw_amd")]

from Solver.region import Ellipse, Rectangle, RegionConfig, RegionEigenSolver  # noqa: E402
from synthetic import fem  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="S5k")
    ap.add_argument("--region", type=float, nargs=4, metavar=("A", "B", "C", "D"))
    ap.add_argument("--ellipse", type=float, nargs=4, metavar=("RE", "IM", "RX", "RY"))
    ap.add_argument("--nodes", type=int, default=16)
    ap.add_argument("--subspace", type=int, default=48)
    ap.add_argument("--atol", type=float, default=1e-10)
    ap.add_argument("--max-it", type=int, default=20)
    ap.add_argument("--batch-nodes", action="store_true", help="solve every iteration's block on all nodes in lockstep (same bytes; one more block per node)")
    ap.add_argument("--two-sided", action="store_true", help="also the left phase: left eigenvectors, and kappa and the left residual of every eigenvalue")
    args = ap.parse_args()
    logging.basicConfig(level=logging.WARNING)
    if args.region is not None:
        region = Rectangle(*args.region)
    elif args.ellipse is not None:
        region = Ellipse(complex(args.ellipse[0], args.ellipse[1]), args.ellipse[2], args.ellipse[3])
    else:
        region = Ellipse(complex(fem.SIGMA_RE50), 0.12, 0.12)
    es = fem.cylinder_case(args.case)
    rs = RegionEigenSolver(es.A, es.M, RegionConfig(nodes=args.nodes, subspace=args.subspace, atol=args.atol, max_it=args.max_it,
                                                     batch_nodes=args.batch_nodes, two_sided=args.two_sided))
    res = rs.solve(region)
    st = res.stats
    print(f"{args.case}: n = {es.n}; {region}")
    print(f"{res.count} eigenvalues inside, complete = {res.complete}; {res.iterations} iterations, rank {st['rank']}, estimate of the count inside "
          f"the ellipse {res.estimate:.1f}; factors {'kept' if st['factors_kept'] else 'refactorised per node'}")
    print(f"seconds: factor {st['seconds_factor']:.4f}, block solves {st['seconds_solve']:.4f}, products {st['seconds_product']:.4f}, "
          f"Gram {st['seconds_gram']:.4f}, host dense {st['seconds_dense']:.4f}, total {st['seconds_total']:.4f}; {st['block_solves']} column solves, "
          f"{st['refined_solves']} refined" + (f"; nodes in lockstep: {st['batched_groups']} batched groups, {st['batched_columns']} column solves"
                                                if st["batch_nodes"] else ""))
    if args.two_sided:
        lt = st["left"]
        print(f"left phase: {lt['iterations']} iterations, {lt['block_solves']} column solves ({lt['refined_solves']} refined, {lt['batched_columns']} in "
              f"lockstep), block solves {lt['seconds_solve']:.4f} s; left_complete = {res.left_complete}")
    for i, (lam, r) in enumerate(zip(res.eigenvalues, res.residuals)):
        left = f"   kappa {res.condition_numbers[i]:.3e}   left residual {res.left_residuals[i]:.2e}" if res.left_complete else ""
        print(f"  {lam.real:+.12f} {lam.imag:+.12f}j   residual {r:.2e}" + left)
    rs.release()


if __name__ == "__main__":
    main()
