"""Child-process side of ``tests/test_gpu_weighted.py``: one job in a fresh process (its own device context, its own reading of the
environment knobs), results into an ``.npz`` file.  Usage: ``python weighted_child.py <job> <case> <ncv> <out.npz>``."""

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "lsa-fw_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def basis_job(case, ncv, out):
    """``ncv`` steps on the weighted W of the case at the target frequency, both windows set through ``lsa_csr_window`` and
    ``lsa_resolvent_set_weights``, from a seeded start: T and the ncv + 1 basis vectors."""
    import lsa_hip
    import resolvent_reference as rref
    import weighted_reference as ref
    from test_lanczos_cpu import on_shared_pattern

    A, M = on_shared_pattern(*ref.case(case))
    ctx = lsa_hip.Context(0)
    dA, dM = lsa_hip.CsrMatrix.from_scipy(ctx, A), lsa_hip.CsrMatrix.from_scipy(ctx, M)
    Qf, Qq = dM.windowed(ref.window(case, *ref.OMEGA_F)), dM.windowed(ref.window(case, *ref.OMEGA_Q))
    op = lsa_hip.ShiftInvertOperator(ctx, dA, dM, 1j * ref.OMEGA_TARGET, mode=0, pc_type=2, ksp_rtol=1e-12)
    basis = lsa_hip.ResolventBasis(ctx, op, ncv)
    basis.set_weights(Qf, Qq)
    basis.set_start(rref.start_vector(A.shape[0]))
    T = np.zeros((ncv + 1, ncv), order="F")
    bd = basis.extend(0, ncv, T)
    V = basis.basis(ncv + 1)
    np.savez(out, T=T, V=V, bd=bd)
    del basis, op, Qf, Qq, dA, dM
    ctx.close()


def solve_job(case, ncv, out):
    """The case at the target frequency through the front end with both windows, four modes: gains, responses, forcings."""
    import weighted_reference as ref
    from Solver.resolvent import ResolventConfig, ResolventSolver

    A, M = ref.case(case)
    rs = ResolventSolver(A, M, ResolventConfig(num_modes=4, ncv=ncv, atol=1e-10), forcing_window=ref.window(case, *ref.OMEGA_F),
                         response_window=ref.window(case, *ref.OMEGA_Q))
    res = rs.solve(ref.OMEGA_TARGET)
    np.savez(out, gains=res.gains, responses=res.responses, forcings=res.forcings, restarts=res.stats["restarts"])
    rs.release()


def growth_job(case, ncv, out):
    """The case over 16 implicit-Euler steps through the front end with the response window, three modes: every output."""
    import growth_reference as gref
    import weighted_reference as ref
    from Solver.growth import TransientGrowthConfig, TransientGrowthSolver

    A, M = ref.case(case)
    tg = TransientGrowthSolver(A, M, TransientGrowthConfig(dt=gref.DT, num_modes=3, ncv=ncv, atol=1e-10), response_window=ref.window(case, *ref.OMEGA_Q))
    res = tg.solve(16 * gref.DT)
    np.savez(out, gains=res.gains, initial=res.initial, responses=res.responses, energy=res.energy, response_energy=res.response_energy,
             estimates=res.estimates)
    tg.release()


if __name__ == "__main__":
    {"basis": basis_job, "solve": solve_job, "growth": growth_job}[sys.argv[1]](sys.argv[2], int(sys.argv[3]), sys.argv[4])
