"""LSA-FW Solver package, eigen path and the kept linear solver (drop-in for ``/root/reference/Solver``'s ``eigen`` and ``utils`` modules)."""

from .eigen import EigenSolver, EigensolverConfig, solve_batch  # noqa: F401
from .utils import KSPType, PreconditionerType, iEpsProblemType, iEpsSolver, iEpsWhich, iKSP, iSTType  # noqa: F401
