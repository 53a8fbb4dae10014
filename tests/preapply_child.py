"""Child process of tests/test_gpu_preapply.py: ``LSA_KRYLOV_PREAPPLY`` and the other switches of the Krylov steps are read once per
process, so every setting runs here.

usage: preapply_child.py ROOT MODE CASE OUT.npz   -> one JSON line (the counters); eigenvalues and eigenvectors in OUT.npz

MODE: base | mask | two | maxit | reuse (k = 6, ncv = 24, complex shift, on a cylinder case)."""

import json
import sys

sys.path[:0] = [sys.argv[1], sys.argv[1] + "/lsa-fw_amd"]
import numpy as np  # noqa: E402

from synthetic import fem  # noqa: E402
from Solver.eigen import EigenSolver, EigensolverConfig  # noqa: E402
from Solver.utils import PreconditionerType, iSTType  # noqa: E402

mode, case, out = sys.argv[2], sys.argv[3], sys.argv[4]
es = fem.cylinder_case(case)
SIGMA = fem.SIGMA_RE50
SIGMA2 = SIGMA + (0.01 + 0.02j)
COUNTERS = ("op_applies", "spmv_calls", "sptrsv_calls", "krylov_restarts", "refined_solves")


def solver(sigma, max_it=500, **kw):
    s = EigenSolver(es.A, es.M, EigensolverConfig(num_eig=6, atol=1e-10, ncv=24, max_it=max_it), check_hermitian=False, **kw)
    s.solver.set_st_type(iSTType.SINVERT)
    s.solver.set_target(sigma)
    s.solver.set_st_pc_type(PreconditionerType.LU)
    return s


def pairs(eps):
    n = eps.get_num_converged()
    lam = np.array([complex(eps.get_eigenvalue(i)) for i in range(n)])
    X = np.column_stack([eps.get_eigenvector_array(i) for i in range(n)]) if n else np.zeros((es.n, 0), complex)
    return lam, np.ascontiguousarray(X)


def counters(eps):
    return {name: int(eps.stats[name]) for name in COUNTERS}


arrays, record = {}, {}
if mode in ("base", "maxit"):
    s = solver(SIGMA, max_it=1 if mode == "maxit" else 500)
    s.solve()
    arrays["lam"], arrays["X"] = pairs(s.solver)
    record = counters(s.solver)
elif mode == "mask":
    from Solver.eigen2 import ArpackEigenSolver, ShiftInvertConfig

    lam, V, res = ArpackEigenSolver(ShiftInvertConfig(sigma=SIGMA, k=6, tol=1e-10, ncv=24), es.A, es.M, dofs_u=es.dofs_u, dofs_p=es.dofs_p).solve()
    arrays["lam"], arrays["X"] = np.asarray(lam), np.ascontiguousarray(V)
elif mode == "two":
    s = solver(SIGMA, two_sided=True)
    s.solve()
    arrays["lam"], arrays["X"] = pairs(s.solver)
    mu, Z = s.solver.get_adjoint_eigenpairs()
    arrays["mu"], arrays["Z"] = np.asarray(mu), np.ascontiguousarray(Z)
    st = dict(s.solver.stats)
    left = st.pop("left")
    record = {name: int(st[name]) for name in COUNTERS}
    record.update({"left_" + name: int(left[name]) for name in COUNTERS if name in left})
elif mode == "reuse":
    s = solver(SIGMA)
    s.solve()
    s.solver.set_target(SIGMA2)
    s.solve()
    arrays["lam"], arrays["X"] = pairs(s.solver)
    record = counters(s.solver)
    s.solver.release()
    f = solver(SIGMA2)
    f.solve()
    arrays["lam_fresh"], arrays["X_fresh"] = pairs(f.solver)
    record.update({"fresh_" + k: v for k, v in counters(f.solver).items()})
else:
    raise SystemExit(f"unknown mode {mode}")
np.savez(out, **arrays)
print(json.dumps(record))
