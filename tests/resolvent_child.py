"""Child-process side of ``tests/test_gpu_resolvent.py``: one job in a fresh process (its own device context, its own reading of the
environment knobs), results into an ``.npz`` file.  Usage: ``python resolvent_child.py <job> <case> <ncv> <out.npz>``."""

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "lsa-fw_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def basis_job(case, ncv, out):
    """``ncv`` steps on W of the case at the target frequency from a seeded start: T and the ncv + 1 basis vectors."""
    import lsa_hip
    import resolvent_reference as ref
    from test_lanczos_cpu import on_shared_pattern

    A, M = on_shared_pattern(*ref.case(case))
    ctx = lsa_hip.Context(0)
    dA, dM = lsa_hip.CsrMatrix.from_scipy(ctx, A), lsa_hip.CsrMatrix.from_scipy(ctx, M)
    op = lsa_hip.ShiftInvertOperator(ctx, dA, dM, 1j * ref.OMEGA_TARGET, mode=0, pc_type=2, ksp_rtol=1e-12)
    basis = lsa_hip.ResolventBasis(ctx, op, ncv)
    basis.set_start(ref.start_vector(A.shape[0]))
    T = np.zeros((ncv + 1, ncv), order="F")
    bd = basis.extend(0, ncv, T)
    V = basis.basis(ncv + 1)
    np.savez(out, T=T, V=V, bd=bd)
    del basis, op, dA, dM
    ctx.close()


def solve_job(case, ncv, out):
    """The case at the target frequency through the front end, six modes: gains, responses, forcings."""
    import resolvent_reference as ref
    from Solver.resolvent import ResolventConfig, ResolventSolver

    A, M = ref.case(case)
    rs = ResolventSolver(A, M, ResolventConfig(num_modes=6, ncv=ncv, atol=1e-10))
    res = rs.solve(ref.OMEGA_TARGET)
    np.savez(out, gains=res.gains, responses=res.responses, forcings=res.forcings, restarts=res.stats["restarts"])
    rs.release()


if __name__ == "__main__":
    {"basis": basis_job, "solve": solve_job}[sys.argv[1]](sys.argv[2], int(sys.argv[3]), sys.argv[4])
