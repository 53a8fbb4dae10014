"""Transposed block solves without a GPU: the two new C-ABI entries (``lsa_ndlu_set_multi_transposed``,
``lsa_resolvent_set_block_forcings``) in header, library and binding, and the switches of the front ends that reach them
(``NdLu.set_multi_transposed``, ``iKSP.block_adjoint``, ``ResolventSolver(block_forcings=...)``), none of which opens a context."""

import ctypes
import inspect

import scipy.sparse as sp

from test_abi import declared_functions
from test_iksp_cpu import SURFACE

NEW_ENTRIES = ("lsa_ndlu_set_multi_transposed", "lsa_resolvent_set_block_forcings")


def test_header_library_and_binding_have_the_new_entries():
    import lsa_hip

    lib = lsa_hip.load_library()
    declared = declared_functions()
    for name in NEW_ENTRIES:
        assert name in declared, f"{name} is not declared in include/lsa_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        restype, argtypes = lsa_hip.SIGNATURES[name]
        assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    for cls, method in ((lsa_hip.NdLu, "set_multi_transposed"), (lsa_hip.ResolventBasis, "set_block_forcings")):
        params = list(inspect.signature(getattr(cls, method)).parameters.values())
        assert [p.name for p in params] == ["self", "on"], (cls, method)


def test_iksp_block_adjoint_is_a_property_and_the_callables_stay():
    from Solver.utils import iKSP

    assert isinstance(vars(iKSP)["block_adjoint"], property) and vars(iKSP)["block_adjoint"].fset is not None
    public = {name for name, v in vars(iKSP).items() if not name.startswith("_") and callable(v)}
    assert public == set(SURFACE)
    assert iKSP().block_adjoint is False


def test_resolvent_solver_has_block_forcings_keyword_only():
    from Solver.resolvent import ResolventSolver

    p = inspect.signature(ResolventSolver.__init__).parameters["block_forcings"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_the_switches_need_no_gpu(monkeypatch):
    import lsa_hip
    from Solver.resolvent import ResolventConfig, ResolventSolver
    from Solver.utils import KSPType, PreconditionerType, iKSP

    opened = []
    monkeypatch.setattr(lsa_hip, "Context", lambda *a, **k: opened.append(a) or (_ for _ in ()).throw(AssertionError("a context was opened")))
    A = (sp.random(12, 12, density=0.3, format="csr", random_state=1) + 4.0 * sp.identity(12, format="csr")).tocsr()
    ksp = iKSP(A)
    ksp.set_type(KSPType.PREONLY)
    ksp.set_preconditioner(PreconditionerType.LU)
    ksp.block_adjoint = True
    assert ksp.block_adjoint is True
    ksp.block_adjoint = 0
    assert ksp.block_adjoint is False
    assert ksp.stats["multi_width"] == 0
    M = sp.identity(12, format="csr")
    for flag in (True, False):
        rs = ResolventSolver(A, M, ResolventConfig(num_modes=2, ncv=6), block_forcings=flag)
        assert rs._block_forcings is flag
    assert ResolventSolver(A, M, ResolventConfig(num_modes=2, ncv=6))._block_forcings is False
    assert opened == []
