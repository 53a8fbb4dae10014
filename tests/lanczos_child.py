"""Child-process side of ``tests/test_gpu_lanczos.py``: one job in a fresh process (its own device context, its own reading of the
environment knobs), results into an ``.npz`` file.  Usage: ``python lanczos_child.py <job> <out.npz>``."""

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "lsa-fw_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def basis_job(out):
    """40 Lanczos steps on the 32 x 32 interior pencil from a seeded start: T and the 41 basis vectors."""
    import lsa_hip
    from test_lanczos_cpu import interior_membrane, on_shared_pattern

    K, M = on_shared_pattern(*interior_membrane(32, 32, 2.0, 2.0))
    ctx = lsa_hip.Context(0)
    dK, dM = lsa_hip.CsrMatrix.from_scipy(ctx, K), lsa_hip.CsrMatrix.from_scipy(ctx, M)
    op = lsa_hip.ShiftInvertOperator(ctx, dK, dM, 10.0, mode=0, pc_type=2, ksp_rtol=1e-12)
    basis = lsa_hip.LanczosBasis(ctx, op, 40)
    basis.set_start(np.random.default_rng(0).standard_normal(K.shape[0]))
    T = np.zeros((41, 40), order="F")
    bd = basis.extend(0, 40, T)
    V = basis.basis(41)
    np.savez(out, T=T, V=V, bd=bd)
    del basis, op, dK, dM
    ctx.close()


def solve_job(out):
    """The 128 x 128 interior pencil through ``EigenSolver(..., symmetric=True)``: eigenvalues and vectors."""
    from test_gpu_lanczos import symmetric_solver
    from test_lanczos_cpu import interior_membrane

    K, M = interior_membrane(128, 128, 2.0, 2.0)
    es = symmetric_solver(K, M, 10.0, 12, 40, True)
    es.solve()
    s = es.solver
    k = s.get_num_converged()
    np.savez(out, lam=np.array([s.get_eigenvalue(i) for i in range(k)]), X=np.column_stack([s.get_eigenvector_array(i) for i in range(k)]))


if __name__ == "__main__":
    {"basis": basis_job, "solve": solve_job}[sys.argv[1]](sys.argv[2])
