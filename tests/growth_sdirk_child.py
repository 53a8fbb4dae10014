"""Child-process side of ``tests/test_gpu_growth_sdirk.py``: the basis job of ``growth_child.py`` under the SDIRK2 scheme, in a fresh
process (its own device context, its own reading of the environment knobs), results into an ``.npz`` file.
Usage: ``python growth_sdirk_child.py <case> <ncv> <nsteps> <out.npz>``."""

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "lsa-fw_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def basis_job(case, ncv, nsteps, out):
    """``ncv`` steps on W of the case over ``nsteps`` SDIRK2 time steps of dt = 0.5 from a seeded start: T and the ncv + 1 basis vectors."""
    import growth_reference as ref
    import growth_sdirk_reference as sref
    import lsa_hip
    from test_lanczos_cpu import on_shared_pattern

    A, M = on_shared_pattern(*ref.case(case))
    ctx = lsa_hip.Context(0)
    dA, dM = lsa_hip.CsrMatrix.from_scipy(ctx, A), lsa_hip.CsrMatrix.from_scipy(ctx, M)
    op = lsa_hip.ShiftInvertOperator(ctx, dA, dM, 1.0 / (sref.GAMMA * sref.DT), mode=0, pc_type=2, ksp_rtol=1e-12)
    basis = lsa_hip.GrowthBasis(ctx, op, ncv, nsteps, ref.keep_mask(case), scheme="sdirk2")
    basis.set_start(ref.start_vector(A.shape[0]))
    T = np.zeros((ncv + 1, ncv), order="F")
    bd = basis.extend(0, ncv, T)
    V = basis.basis(ncv + 1)
    np.savez(out, T=T, V=V, bd=bd)
    del basis, op, dA, dM
    ctx.close()


if __name__ == "__main__":
    basis_job(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
