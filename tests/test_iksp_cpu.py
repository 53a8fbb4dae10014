"""``Solver.utils.iKSP`` without a GPU: the surface of the reference's class, and the argument errors that are raised before
any device call."""

import inspect

import numpy as np
import pytest
import scipy.sparse as sp

# the public methods of the reference's iKSP (Solver/utils.py:331-419) with their parameters and defaults, plus the
# extensions solve_many / stats
SURFACE = {
    "set_operators": [("A", inspect.Parameter.empty), ("P", None)],
    "set_type": [("ksp_type", inspect.Parameter.empty)],
    "get_type": [],
    "set_tolerances": [("tol", 1e-12), ("max_it", 1000), ("rtol", 1e-8)],
    "set_preconditioner": [("pc_type", inspect.Parameter.empty)],
    "set_initial_guess_nonzero": [("flag", inspect.Parameter.empty)],
    "set_from_options": [("prefix", None)],
    "solve": [("b", inspect.Parameter.empty), ("x", None)],
    "get_solution": [],
    "get_residual_norm": [],
    "get_iteration_number": [],
    "reset": [],
    "solve_many": [("B", inspect.Parameter.empty), ("adjoint", False)],
}


def _params(fn):
    return [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[1:]]


def test_surface_matches_the_reference_class():
    import Solver
    from Solver.utils import iKSP

    assert Solver.iKSP is iKSP
    public = {name for name, v in vars(iKSP).items() if not name.startswith("_") and callable(v)}
    assert public == set(SURFACE)
    for name, want in SURFACE.items():
        assert _params(getattr(iKSP, name)) == want, name
    assert isinstance(vars(iKSP)["raw"], property) and isinstance(vars(iKSP)["stats"], property)
    init = inspect.signature(iKSP.__init__).parameters
    assert [(p.name, p.default, p.kind) for p in list(init.values())[1:]] == [
        ("A", None, inspect.Parameter.POSITIONAL_OR_KEYWORD), ("comm", None, inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("device", 0, inspect.Parameter.KEYWORD_ONLY)]


def test_configuration_needs_no_gpu_and_argument_errors_come_first(monkeypatch):
    import lsa_hip
    from FEM.utils import iPETScMatrix
    from Solver.utils import KSPType, PreconditionerType, iKSP

    opened = []
    monkeypatch.setattr(lsa_hip, "Context", lambda *a, **k: opened.append(a) or (_ for _ in ()).throw(AssertionError("a context was opened")))
    A = sp.random(12, 12, density=0.3, format="csr", random_state=1) + 4.0 * sp.identity(12, format="csr")
    ksp = iKSP()
    ksp.set_operators(iPETScMatrix(A))
    ksp = iKSP(A, comm=None, device=0)
    ksp.set_type(KSPType.PREONLY)
    ksp.set_preconditioner(PreconditionerType.LU)
    ksp.set_tolerances(tol=1e-14, max_it=50, rtol=1e-9)
    ksp.set_initial_guess_nonzero(True)
    ksp.set_from_options()
    ksp.set_from_options(prefix="ns_")
    ksp.set_operators(A, A)  # P = A is the default of PETSc
    assert ksp.get_type() == "preonly" and ksp.raw.getType() == "preonly" and ksp.raw.getPC().getType() == "lu"
    assert ksp.raw.getIterationNumber() == 0 and ksp.raw.getResidualNorm() == 0.0
    assert ksp.stats == {"analyses": 0, "factorisations": 0, "refactorisations": 0, "solves": 0, "columns": 0, "multi_width": 0}
    for bad in (KSPType.CG, KSPType.BICGSTAB, KSPType.FGMRES):
        with pytest.raises(ValueError, match="KSP type not supported."):
            ksp.set_type(bad)
    with pytest.raises(NotImplementedError):
        ksp.set_operators(A, sp.identity(12, format="csr"))
    with pytest.raises(ValueError, match=r"Operator A must be square, got shape \(3, 4\)"):
        ksp.set_operators(sp.csr_matrix(np.ones((3, 4))))
    with pytest.raises(ValueError, match=r"Operator A must be square"):
        iKSP(sp.csr_matrix(np.ones((3, 4))))
    with pytest.raises(ValueError, match=r"Right-hand side has shape \(11,\), expected \(12,\)"):
        ksp.solve(np.ones(11))
    with pytest.raises(ValueError):
        ksp.solve_many(np.ones((11, 2)))
    with pytest.raises(ValueError):
        ksp.solve_many(np.ones(12))
    ksp.reset()  # nothing to free: still no device work
    assert opened == []


def test_solve_without_a_gpu_raises_the_no_cpu_fallback_error():
    """On a device index no machine has, so that the test sees the error of a machine without a GPU wherever it runs."""
    from Solver.utils import KSPType, PreconditionerType, iKSP

    A = sp.identity(10, format="csr") * 2.0
    for ksp_type, pc in ((KSPType.PREONLY, PreconditionerType.LU), (KSPType.GMRES, PreconditionerType.NONE)):
        ksp = iKSP(A, device=4096)
        ksp.set_type(ksp_type)
        ksp.set_preconditioner(pc)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ksp.solve(np.ones(10))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ksp.solve_many(np.ones((10, 3)))
