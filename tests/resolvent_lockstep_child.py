"""Child process of tests/test_gpu_resolvent_lockstep.py: switches read once per process (LSA_LANCZOS_FUSED) are set by the parent in
the environment.  Solves three S2k frequencies alone and as one lockstep group and prints one JSON line: whether every member equals
its solo solve byte for byte, and the group's counters."""

import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
for p in (str(ROOT), str(ROOT / "lsa-fw_amd"), str(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main() -> None:
    import lsa_hip
    import resolvent_reference as ref
    from test_lanczos_cpu import on_shared_pattern

    omegas, nev, ncv, tol = (0.4, 0.8, 1.6), 3, 12, 1e-10
    A, M = on_shared_pattern(*ref.case("S2k"))
    v0 = ref.start_vector(A.shape[0])
    ctx = lsa_hip.Context(0)
    dA, dM = lsa_hip.CsrMatrix.from_scipy(ctx, A), lsa_hip.CsrMatrix.from_scipy(ctx, M)

    def open_basis(w):
        op = lsa_hip.ShiftInvertOperator(ctx, dA, dM, 1j * w, mode=0, pc_type=2, ksp_rtol=1e-12)
        return lsa_hip.ResolventBasis(ctx, op, ncv), op

    solo = []
    for w in omegas:
        b, op = open_basis(w)
        solo.append(b.solve(nev, tol, 500, v0=v0, max_out=nev))
        del b, op
    objs = [open_basis(w) for w in omegas]
    res, info = lsa_hip.ResolventBasis.solve_batch([o[0] for o in objs], nev, tol, 500, v0s=v0, max_out=nev)
    same = all(r[k].tobytes() == s[k].tobytes() for r, s in zip(res, solo) for k in ("theta", "gains", "responses", "forcings", "estimates"))
    same = same and all(r["applies"] == s["applies"] and r["restarts"] == s["restarts"] for r, s in zip(res, solo))
    del objs
    print(json.dumps({"same": bool(same), "info": info, "applies": [int(r["applies"]) for r in res], "gains": [float(np.max(r["gains"])) for r in res]}))
    ctx.close()


if __name__ == "__main__":
    main()
