"""CPU suite: what the four analysis front ends on the exact LU refuse in their constructors, word for word, and that a good pencil
opens nothing.  The expected texts are the ones the constructors raised before they shared ``Solver/exact_lu.py``."""

import numpy as np
import pytest
import scipy.sparse as sp

from Solver.growth import TransientGrowthConfig, TransientGrowthSolver
from Solver.region import RegionConfig, RegionEigenSolver
from Solver.resolvent import ResolventSolver
from Solver.stochastic import StochasticConfig, StochasticForcingSolver
from Solver.utils import PreconditionerType

N = 6
A = (sp.diags([np.arange(1.0, N + 1)], [0]) + 0.5 * sp.diags([np.ones(N - 1)], [1]) + 0.25 * sp.diags([np.ones(N - 1)], [-1])).tocsr()
M = (sp.diags([np.full(N, 2.0)], [0]) + 0.5 * sp.diags([np.ones(N - 1)], [1]) + 0.5 * sp.diags([np.ones(N - 1)], [-1])).tocsr()
SKEW = (M + sp.csr_matrix(([1.0], ([0], [1])), shape=M.shape)).tocsr()

FRONT_ENDS = {
    "resolvent": lambda A, M, **kw: ResolventSolver(A, M, **kw),
    "growth": lambda A, M, **kw: TransientGrowthSolver(A, M, TransientGrowthConfig(dt=0.5, num_modes=1, ncv=4), **kw),
    "stochastic": lambda A, M, **kw: StochasticForcingSolver(A, M, StochasticConfig(num_modes=2, ncv=5), **kw),
    "region": lambda A, M, **kw: RegionEigenSolver(A, M, RegionConfig(subspace=4), **kw),
}
CASES = {
    "no_A": lambda f: f(None, M),
    "no_M": lambda f: f(A, None),
    "complex_M": lambda f: f(A, M.astype(np.complex128)),
    "complex_A": lambda f: f(A.astype(np.complex128), M),
    "complex_both": lambda f: f(A.astype(np.complex128), M.astype(np.complex128)),
    "skew_M": lambda f: f(A, SKEW),
    "layout": lambda f: f(A, M, layout="sharded"),
    "ilu": lambda f: f(A, M, pc_type=PreconditionerType.ILU),
    "ilu_levels": lambda f: f(A, M, ilu_levels=1),
    "chol_levels": lambda f: f(A, M, pc_type=PreconditionerType.CHOLESKY, ilu_levels=2),
    "shape": lambda f: f(A, sp.identity(N + 1, format="csr")),
    # two rules broken at once: the same one wins
    "layout_and_ilu": lambda f: f(A, M, layout="sharded", pc_type=PreconditionerType.ILU),
    "skew_and_layout": lambda f: f(A, SKEW, layout="sharded"),
}

# (front end, case) -> None (accepted) or (exception type, the whole message), recorded from the constructors as they were
EXPECTED = {
    ("resolvent", "no_A"): (ValueError, 'Operator A is required.'),
    ("resolvent", "no_M"): (ValueError, 'Resolvent analysis needs M: the gains are measured in the M-inner product'),
    ("resolvent", "complex_M"): (ValueError, 'Resolvent analysis needs a real M (the M-inner product); M is complex'),
    ("resolvent", "complex_A"): None,
    ("resolvent", "complex_both"): (ValueError, 'Resolvent analysis needs a real M (the M-inner product); M is complex'),
    ("resolvent", "skew_M"): (ValueError, 'Resolvent analysis needs a symmetric M; its relative symmetry defect is 2.649e-01'),
    ("resolvent", "layout"): (NotImplementedError, "Resolvent analysis runs on one GPU; the layout is 'sharded'"),
    ("resolvent", "ilu"): (NotImplementedError, 'Resolvent analysis needs the exact LU (PreconditionerType.LU): both inner solves of a step run on its factors; the preconditioner is ILU'),
    ("resolvent", "ilu_levels"): (NotImplementedError, 'Resolvent analysis needs the exact LU (PreconditionerType.LU): both inner solves of a step run on its factors; the preconditioner is LU with ILU level 1'),
    ("resolvent", "chol_levels"): (NotImplementedError, 'Resolvent analysis needs the exact LU (PreconditionerType.LU): both inner solves of a step run on its factors; the preconditioner is CHOLESKY with ILU level 2'),
    ("resolvent", "shape"): (ValueError, "Operator M shape (7, 7) does not match A's shape (6, 6)"),
    ("resolvent", "layout_and_ilu"): (NotImplementedError, "Resolvent analysis runs on one GPU; the layout is 'sharded'"),
    ("resolvent", "skew_and_layout"): (ValueError, 'Resolvent analysis needs a symmetric M; its relative symmetry defect is 2.649e-01'),
    ("growth", "no_A"): (ValueError, 'Operator A is required.'),
    ("growth", "no_M"): (ValueError, 'Transient growth needs M: the energy is measured in the M-inner product'),
    ("growth", "complex_M"): (ValueError, 'Transient growth needs real A and M (a real march on real factors); M is complex'),
    ("growth", "complex_A"): (ValueError, 'Transient growth needs real A and M (a real march on real factors); A is complex'),
    ("growth", "complex_both"): (ValueError, 'Transient growth needs real A and M (a real march on real factors); A is complex'),
    ("growth", "skew_M"): (ValueError, 'Transient growth needs a symmetric M; its relative symmetry defect is 2.649e-01'),
    ("growth", "layout"): (NotImplementedError, "Transient growth runs on one GPU; the layout is 'sharded'"),
    ("growth", "ilu"): (NotImplementedError, 'Transient growth needs the exact LU (PreconditionerType.LU): every solve of the march runs on its factors; the preconditioner is ILU'),
    ("growth", "ilu_levels"): (NotImplementedError, 'Transient growth needs the exact LU (PreconditionerType.LU): every solve of the march runs on its factors; the preconditioner is LU with ILU level 1'),
    ("growth", "chol_levels"): (NotImplementedError, 'Transient growth needs the exact LU (PreconditionerType.LU): every solve of the march runs on its factors; the preconditioner is CHOLESKY with ILU level 2'),
    ("growth", "shape"): (ValueError, "Operator M shape (7, 7) does not match A's shape (6, 6)"),
    ("growth", "layout_and_ilu"): (NotImplementedError, "Transient growth runs on one GPU; the layout is 'sharded'"),
    ("growth", "skew_and_layout"): (ValueError, 'Transient growth needs a symmetric M; its relative symmetry defect is 2.649e-01'),
    ("stochastic", "no_A"): (ValueError, 'Operator A is required.'),
    ("stochastic", "no_M"): (ValueError, 'Stochastic forcing needs M: the variance is measured in the M-inner product'),
    ("stochastic", "complex_M"): (ValueError, 'Stochastic forcing needs a real M (the M-inner product); M is complex'),
    ("stochastic", "complex_A"): (ValueError, 'Stochastic forcing needs a real A: the quadrature over omega >= 0 stands for the whole axis only for a real pencil'),
    ("stochastic", "complex_both"): (ValueError, 'Stochastic forcing needs a real A: the quadrature over omega >= 0 stands for the whole axis only for a real pencil'),
    ("stochastic", "skew_M"): (ValueError, 'Stochastic forcing needs a symmetric M; its relative symmetry defect is 2.649e-01'),
    ("stochastic", "layout"): (NotImplementedError, "Stochastic forcing runs on one GPU; the layout is 'sharded'"),
    ("stochastic", "ilu"): (NotImplementedError, 'Stochastic forcing needs the exact LU (PreconditionerType.LU): every node of the quadrature is a pair of solves on its factors; the preconditioner is ILU'),
    ("stochastic", "ilu_levels"): (NotImplementedError, 'Stochastic forcing needs the exact LU (PreconditionerType.LU): every node of the quadrature is a pair of solves on its factors; the preconditioner is LU with ILU level 1'),
    ("stochastic", "chol_levels"): (NotImplementedError, 'Stochastic forcing needs the exact LU (PreconditionerType.LU): every node of the quadrature is a pair of solves on its factors; the preconditioner is CHOLESKY with ILU level 2'),
    ("stochastic", "shape"): (ValueError, "Operator M shape (7, 7) does not match A's shape (6, 6)"),
    ("stochastic", "layout_and_ilu"): (NotImplementedError, "Stochastic forcing runs on one GPU; the layout is 'sharded'"),
    ("stochastic", "skew_and_layout"): (ValueError, 'Stochastic forcing needs a symmetric M; its relative symmetry defect is 2.649e-01'),
    ("region", "no_A"): (ValueError, 'Operator A is required.'),
    ("region", "no_M"): (ValueError, 'The region eigensolver needs M: the contour integral is that of the pencil (A, M)'),
    ("region", "complex_M"): (ValueError, 'The region eigensolver needs a real M; M is complex'),
    ("region", "complex_A"): None,
    ("region", "complex_both"): (ValueError, 'The region eigensolver needs a real M; M is complex'),
    ("region", "skew_M"): None,
    ("region", "layout"): (NotImplementedError, "The region eigensolver runs on one GPU; the layout is 'sharded'"),
    ("region", "ilu"): (NotImplementedError, 'The region eigensolver needs the exact LU (PreconditionerType.LU): every node of the contour is a block solve on its factors; the preconditioner is ILU'),
    ("region", "ilu_levels"): (NotImplementedError, 'The region eigensolver needs the exact LU (PreconditionerType.LU): every node of the contour is a block solve on its factors; the preconditioner is LU with ILU level 1'),
    ("region", "chol_levels"): (NotImplementedError, 'The region eigensolver needs the exact LU (PreconditionerType.LU): every node of the contour is a block solve on its factors; the preconditioner is CHOLESKY with ILU level 2'),
    ("region", "shape"): (ValueError, "Operator M shape (7, 7) does not match A's shape (6, 6)"),
    ("region", "layout_and_ilu"): (NotImplementedError, "The region eigensolver runs on one GPU; the layout is 'sharded'"),
    ("region", "skew_and_layout"): (NotImplementedError, "The region eigensolver runs on one GPU; the layout is 'sharded'"),
}


@pytest.mark.parametrize("front_end", sorted(FRONT_ENDS))
def test_constructor_refusals_word_for_word(front_end):
    make = FRONT_ENDS[front_end]
    for case, attempt in CASES.items():
        want = EXPECTED[front_end, case]
        if want is None:
            assert attempt(make).solver.prepared is None, case
            continue
        with pytest.raises(want[0]) as info:
            attempt(make)
        assert type(info.value) is want[0] and str(info.value) == want[1], (case, str(info.value))


def test_growth_names_its_missing_config_after_a_missing_operator():
    text = "Transient growth needs a TransientGrowthConfig: the time step dt has no default"
    for args, want in (((None, M, None), "Operator A is required."), ((A, None, None), "Transient growth needs M: the energy is measured in the M-inner product"),
                       ((A, M, None), text), ((A, sp.identity(N + 1, format="csr"), None), text)):
        with pytest.raises(ValueError) as info:
            TransientGrowthSolver(*args)
        assert str(info.value) == want


@pytest.mark.parametrize("front_end", sorted(FRONT_ENDS))
def test_a_good_pencil_opens_nothing(front_end, monkeypatch):
    import lsa_hip
    from Solver.utils import iEpsSolver

    monkeypatch.setattr(lsa_hip, "Context", lambda *a, **k: pytest.fail("a context was opened"))
    s = FRONT_ENDS[front_end](A, M)
    assert isinstance(s.solver, iEpsSolver) and s.solver.prepared is None and s.solver._prepared is None
    assert [X.as_scipy_array().shape for X in s.solver.operators] == [(N, N), (N, N)]
    v = s.solver.start_vector(N)
    assert v.shape == (N,) and v.dtype == np.complex128 and v is s.solver._start_vector(N)
    s.release()
    assert s.solver.prepared is None
    dims = s.solver.raw.getDimensions()
    assert dims[:2] == {"resolvent": (3, 24), "growth": (1, 4), "stochastic": (2, 5), "region": (1, None)}[front_end]


def test_the_window_and_weight_helpers_are_still_importable_from_resolvent():
    from Solver import exact_lu
    from Solver.resolvent import checked_side, checked_weight, checked_window, device_weight, shared_pattern

    for f in (checked_side, checked_weight, checked_window, device_weight, shared_pattern):
        assert f is getattr(exact_lu, f.__name__)
    assert checked_side("response", None, None, M) is None
    kind, d = checked_side("response", np.ones(N), None, M)
    assert kind == "window" and d.dtype == np.float64
    assert shared_pattern(A, M).nnz == A.nnz
