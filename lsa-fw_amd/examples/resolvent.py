"""Gain curve of a synthetic cylinder case: the optimal gains sigma_1(omega) >= sigma_2(omega) >= ... of the linearised flow at
Re = 50 over a list of frequencies, on ONE context, ordering and LU analysis (``ResolventSolver.sweep``).

    python lsa-fw_amd/examples/resolvent.py [--case S5k] [--modes 3] [--omegas 0 0.2 0.4 0.6 0.738 0.9 1.2]

The wake is marginally stable and strongly non-normal: the least stable eigenvalue sits at 0.018 + 0.738j, and the gains around
omega = 0.74 -- and, larger still, at low frequencies -- say how much a harmonic forcing is amplified, which the eigenvalues alone
understate.  Needs an AMD GPU (there is no CPU fallback).
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "lsa-fw_amd")]

from Solver.resolvent import ResolventConfig, ResolventSolver  # noqa: E402
from synthetic import fem  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="S5k")
    ap.add_argument("--modes", type=int, default=3)
    ap.add_argument("--ncv", type=int, default=24)
    ap.add_argument("--omegas", type=float, nargs="+", default=[0.2, 0.4, 0.6, float(fem.SIGMA_RE50.imag), 0.9, 1.2])
    args = ap.parse_args()
    es = fem.cylinder_case(args.case)
    rs = ResolventSolver(es.A, es.M, ResolventConfig(num_modes=args.modes, ncv=args.ncv, atol=1e-8))
    print(f"{args.case}: n = {es.n}")
    print("   omega   " + "".join(f"sigma_{j + 1:<8d}" for j in range(args.modes)) + "applies restarts  factor s   steps s  analysis reused")
    for res in rs.sweep(args.omegas):
        st = res.stats
        print(f"{res.omega:8.4f}   " + "".join(f"{g:<14.6f}" for g in res.gains) + f"{st['applies']:7d} {st['restarts']:8d} "
              f"{st['seconds_factor']:9.4f} {st['seconds_expand']:9.4f}  {st['analysis_reused']}")
    best = res  # the last frequency's leading pair: R M f_1 = sigma_1 q_1
    print(f"omega = {best.omega}: leading response and forcing of length {best.responses.shape[0]}, sigma_1 = {best.gains[0]:.6f}")
    rs.release()


if __name__ == "__main__":
    main()
