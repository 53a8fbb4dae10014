"""Growth curve of a synthetic cylinder case: the optimal energy gains G_1(T) >= G_2(T) >= ... of the linearised flow at Re = 50 over
a list of horizons, on ONE factorisation of A - sigma M (``TransientGrowthSolver.sweep``).

    python lsa-fw_amd/examples/transient_growth.py [--case S5k] [--modes 2] [--dt 0.25] [--scheme euler] [--horizons 1 2 4 10 20]
                                                   [--response-window X0 X1]

``--scheme euler`` (the default) marches by implicit Euler, first order in dt; ``--scheme sdirk2`` by the L-stable two-stage SDIRK
method, second order: within 0.3 % of the flow's gains at dt = 0.5, where Euler at dt = 0.25 is 24 % low at T = 10.

The flow is stable -- the leading eigenvalue has real part -0.018 -- and strongly non-normal: a well chosen perturbation still grows
(G(4) = 2.2, G(20) = 3.5 on S2k under implicit Euler at dt = 0.25; 2.55 at T = 4 under SDIRK2) before it decays, which the eigenvalues alone do not say.  The Dirichlet rows of the pair are left
out of the flow (``constrained="auto"``).  ``--response-window X0 X1`` measures the response in the energy of the dofs with
X0 <= x <= X1 only (``G = max ||q(T)||_Q^2 / ||q(0)||_M^2``, ``Q = D M D``): on a long domain the whole-domain gain depends on where the
mesh ends.  Needs an AMD GPU (there is no CPU fallback).
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "lsa-fw_amd")]

from Solver.growth import TransientGrowthConfig, TransientGrowthSolver  # noqa: E402
from synthetic import fem  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="S5k")
    ap.add_argument("--modes", type=int, default=2)
    ap.add_argument("--ncv", type=int, default=12)
    ap.add_argument("--dt", type=float, default=0.25)
    ap.add_argument("--scheme", choices=("euler", "sdirk2"), default="euler")
    ap.add_argument("--horizons", type=float, nargs="+", default=[1.0, 2.0, 4.0, 10.0, 20.0])
    ap.add_argument("--response-window", type=float, nargs=2, metavar=("X0", "X1"), default=None)
    args = ap.parse_args()
    es = fem.cylinder_case(args.case)
    window = None
    if args.response_window is not None:
        x, _ = es.dof_xy()
        window = ((x >= args.response_window[0]) & (x <= args.response_window[1])).astype(float)
    tg = TransientGrowthSolver(es.A, es.M, TransientGrowthConfig(dt=args.dt, num_modes=args.modes, ncv=args.ncv, atol=1e-8, scheme=args.scheme),
                               response_window=window)
    print(f"{args.case}: n = {es.n}, {tg.constrained.size} constrained dofs left out, dt = {args.dt}, scheme {args.scheme}")
    print("       T  steps   " + "".join(f"G_{j + 1:<12d}" for j in range(args.modes)) + "applies restarts  factor s   steps s  factorisation reused")
    for res in tg.sweep(args.horizons):
        st = res.stats
        print(f"{res.horizon:8.3f} {res.steps:6d}   " + "".join(f"{g:<14.6f}" for g in res.gains) + f"{st['applies']:7d} {st['restarts']:8d} "
              f"{st['seconds_factor']:9.4f} {st['seconds_expand']:9.4f}  {st['factorisation_reused']}")
    peak = int(res.energy[0].argmax())  # the last horizon's leading initial condition: its energy along the march
    print(f"T = {res.horizon}: the leading perturbation's energy peaks at t = {res.times[peak]:.3f} with {res.energy[0, peak]:.6f}")
    if window is not None:
        print(f"T = {res.horizon}: energy inside the window {res.response_energy[0]:.6f} of {res.energy[0, -1]:.6f} in the whole domain")
    tg.release()


if __name__ == "__main__":
    main()
