"""Response of a synthetic cylinder case to stochastic forcing: the variance the linearised flow at Re = 50 sustains under forcing
that is white in time, the structures that carry it (EOFs) or feed it (stochastic optimals), and where in frequency each mode's
variance comes from, on a frequency quadrature (``StochasticForcingSolver``).

    python lsa-fw_amd/examples/stochastic_forcing.py [--case S5k] [--modes 4] [--nodes 8 16] [--band 0 1.5] [--scale S]
                                                     [--kind eofs|optimals] [--discount B] [--response-window X0 X1] [--batch-adjoint]
                                                     [--trace P]

The numbers are those of the QUADRATURE operator ``(1 / pi) sum_k w_k Re W(i omega_k)``, not of the integral: give several ``--nodes`` and
compare.  The wake has sharp resonances (the least stable eigenvalue sits at 0.018 + 0.738j), so the leading variances move a lot
between 8 and 16 nodes while their sum over all modes does not; ``--discount B`` evaluates at ``B + i omega`` and smooths the integrand.
``--scale S`` integrates over the whole axis through ``omega = S tan(theta)`` instead of the band.  ``--batch-adjoint`` sends the adjoint
solves of a step through the batched transposed sweeps (the same numbers, bit for bit).  ``--trace P`` adds the total variance (the
sum over ALL modes) estimated by ``P`` block probes on the same factor sets, its standard error, and the cumulative share of it the
leading modes carry: the figure that says whether four modes explain the flow or nearly nothing.  Needs an AMD GPU (there is no CPU
fallback).
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "lsa-fw_amd")]

import numpy as np  # noqa: E402

from Solver.stochastic import StochasticConfig, StochasticForcingSolver  # noqa: E402
from synthetic import fem  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="S5k")
    ap.add_argument("--modes", type=int, default=4)
    ap.add_argument("--ncv", type=int, default=24)
    ap.add_argument("--nodes", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--band", type=float, nargs=2, metavar=("A", "B"), default=[0.0, 1.5])
    ap.add_argument("--scale", type=float, default=None, help="the whole axis through omega = S tan(theta) instead of --band")
    ap.add_argument("--kind", choices=("eofs", "optimals"), default="eofs")
    ap.add_argument("--discount", type=float, default=0.0)
    ap.add_argument("--response-window", type=float, nargs=2, metavar=("X0", "X1"), default=None)
    ap.add_argument("--batch-adjoint", action="store_true", help="the adjoint solves of a step through the batched transposed sweeps (same bits)")
    ap.add_argument("--trace", type=int, default=None, metavar="P", help="the total variance and the captured fractions from P block probes")
    args = ap.parse_args()
    es = fem.cylinder_case(args.case)
    window = None
    if args.response_window is not None:
        x, _ = es.dof_xy()
        window = ((x >= args.response_window[0]) & (x <= args.response_window[1])).astype(float)
    print(f"{args.case}: n = {es.n}, kind {args.kind}, discount {args.discount}")
    for nodes in args.nodes:
        sf = StochasticForcingSolver(es.A, es.M, StochasticConfig(num_modes=args.modes, ncv=args.ncv, atol=1e-8, nodes=nodes), response_window=window,
                                     discount=args.discount, batch_adjoint=args.batch_adjoint)
        where = dict(band=(0.0, np.inf), scale=args.scale) if args.scale is not None else dict(band=tuple(args.band))
        res = sf.solve(**where, kind=args.kind, trace=args.trace)
        sf.release()
        st = res.stats
        print(f"nodes = {nodes}: variances " + " ".join(f"{v:.6f}" for v in res.variances) + f"   ({st['applies']} applies, {st['restarts']} restarts, "
              f"{st['adjoint_batches']} batched adjoint sweeps, factor {st['seconds_factor']:.3f} s, steps {st['seconds_expand']:.3f} s)")
        print("    omega      " + "".join(f"mode {j + 1:<9d}" for j in range(len(res.variances))))
        for k, om in enumerate(res.omegas):
            print(f"{om:10.4f}   " + "".join(f"{res.spectrum[j, k]:<14.6f}" for j in range(len(res.variances))))
        if res.total_variance is not None:
            print(f"    total variance {res.total_variance:.4f} +- {res.total_variance_stderr:.4f} ({args.trace} probes, {st['trace']['solves_adjoint'] + st['trace']['solves_forward']} "
                  f"solves in {st['trace']['seconds_solve']:.3f} s); captured " + " ".join(f"{100 * c:.2f}%" for c in res.captured)
                  + "  (+- " + " ".join(f"{100 * e:.2f}" for e in res.captured_stderr) + ")")


if __name__ == "__main__":
    main()
