"""Gain curve of a synthetic cylinder case: the optimal gains sigma_1(omega) >= sigma_2(omega) >= ... of the linearised flow at
Re = 50 over a list of frequencies, on ONE context, ordering and LU analysis (``ResolventSolver.sweep``).

    python lsa-fw_amd/examples/resolvent.py [--case S5k] [--modes 3] [--omegas 0 0.2 0.4 0.6 0.738 0.9 1.2]
                                            [--forcing-window X0 X1 [Y0 Y1]] [--response-window X0 X1] [--discount B]
                                            [--norm-map RE0 RE1 NRE IM0 IM1 NIM] [--lockstep J]

The wake is marginally stable and strongly non-normal: the least stable eigenvalue sits at 0.018 + 0.738j, and the gains around
omega = 0.74 -- and, larger still, at low frequencies -- say how much a harmonic forcing is amplified, which the eigenvalues alone
understate.  ``--forcing-window`` confines the forcing to a box and ``--response-window`` measures the response in a strip
(``sigma = max ||q||_Qq / ||f||_Qf``, ``Q = D M D`` with the 0/1 window ``D``): what is published for long domains, where the whole-domain
gain depends on where the mesh ends.  ``--discount B`` shifts to ``((B + i omega) M - A)^-1``, the discounted resolvent for an unstable
base flow, and ``--norm-map`` prints ``sigma_1(z)`` on a grid of complex points: ``1 / sigma_1`` is the epsilon-level of the energy-norm
pseudospectrum.  ``--lockstep J`` advances up to J (at most 16) frequencies, or map points off the real axis, together: one batched
launch per launch of a solo step, the same numbers.  Needs an AMD GPU (there is no CPU fallback).
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "lsa-fw_amd")]

import numpy as np  # noqa: E402

from Solver.resolvent import ResolventConfig, ResolventSolver  # noqa: E402
from synthetic import fem  # noqa: E402


def box_window(es, box):
    """The 0/1 window of the dofs inside ``box`` = (x0, x1[, y0, y1]); ``None`` for no box."""
    if box is None:
        return None
    if len(box) not in (2, 4):
        raise SystemExit("a window is X0 X1 or X0 X1 Y0 Y1")
    x, y = es.dof_xy()
    inside = (x >= box[0]) & (x <= box[1])
    if len(box) == 4:
        inside &= (y >= box[2]) & (y <= box[3])
    return inside.astype(float)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="S5k")
    ap.add_argument("--modes", type=int, default=3)
    ap.add_argument("--ncv", type=int, default=24)
    ap.add_argument("--omegas", type=float, nargs="+", default=[0.2, 0.4, 0.6, float(fem.SIGMA_RE50.imag), 0.9, 1.2])
    ap.add_argument("--forcing-window", type=float, nargs="+", metavar="X", default=None)
    ap.add_argument("--response-window", type=float, nargs=2, metavar=("X0", "X1"), default=None)
    ap.add_argument("--discount", type=float, default=0.0)
    ap.add_argument("--norm-map", type=float, nargs=6, metavar=("RE0", "RE1", "NRE", "IM0", "IM1", "NIM"), default=None)
    ap.add_argument("--lockstep", type=int, default=0, metavar="J", help="advance up to J frequencies (or map points) together")
    args = ap.parse_args()
    es = fem.cylinder_case(args.case)
    rs = ResolventSolver(es.A, es.M, ResolventConfig(num_modes=args.modes, ncv=args.ncv, atol=1e-8), forcing_window=box_window(es, args.forcing_window),
                         response_window=box_window(es, args.response_window), discount=args.discount)
    print(f"{args.case}: n = {es.n}, discount {args.discount}")
    if args.norm_map is not None:
        re0, re1, nre, im0, im1, nim = args.norm_map
        re, im = np.linspace(re0, re1, int(nre)), np.linspace(im0, im1, int(nim))
        pts = re[None, :] + 1j * im[:, None]
        sigma1 = rs.norm_map(pts, warm_start=False, lockstep=True, max_batch=args.lockstep) if args.lockstep else rs.norm_map(pts)
        print("sigma_1(z), rows Im z, columns Re z:   " + "".join(f"{r:<12.4f}" for r in re))
        for w, row in zip(im, sigma1):
            print(f"{w:36.4f}   " + "".join(f"{g:<12.4e}" for g in row))
        rs.release()
        return
    print("   omega   " + "".join(f"sigma_{j + 1:<8d}" for j in range(args.modes)) + "applies restarts  factor s   steps s  analysis reused")
    for res in (rs.sweep(args.omegas, lockstep=True, max_batch=args.lockstep) if args.lockstep else rs.sweep(args.omegas)):
        st = res.stats
        print(f"{res.omega:8.4f}   " + "".join(f"{g:<14.6f}" for g in res.gains) + f"{st['applies']:7d} {st['restarts']:8d} "
              f"{st['seconds_factor']:9.4f} {st['seconds_expand']:9.4f}  {st['analysis_reused']}")
    best = res  # the last frequency's leading pair: R M f_1 = sigma_1 q_1
    print(f"omega = {best.omega}: leading response and forcing of length {best.responses.shape[0]}, sigma_1 = {best.gains[0]:.6f}")
    rs.release()


if __name__ == "__main__":
    main()
