"""CPU suite: the transposed block solve on a batch of factor sets and the transposed block product are declared, exported and bound;
``NdLu.solve_multi_batch_adjoint`` refuses bad lists before the library (or a context) is touched; the forward entry goes on refusing
``trans``."""

import ctypes
import re
from pathlib import Path

import pytest

import lsa_hip

HEADER = Path(__file__).resolve().parents[1] / "include" / "lsa_hip.h"


class Fake:
    def __init__(self, ctx):
        self.ctx, self.handle, self.n = ctx, ctypes.c_void_p(1), 10


def test_symbols_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    lib = lsa_hip.load_library()
    for name, nargs in (("lsa_ndlu_solve_multi_batch_adjoint", 9), ("lsa_ndlu_solve_multi_batch_adjoint_time", 11), ("lsa_spmm_transpose", 8)):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(lib, name), name
        restype, argtypes = lsa_hip.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs, name
    # the transposed entries take `conj` where the forward ones take `trans`, and are otherwise the forward ones
    assert lsa_hip.SIGNATURES["lsa_ndlu_solve_multi_batch_adjoint"] == lsa_hip.SIGNATURES["lsa_ndlu_solve_multi_batch"]
    assert lsa_hip.SIGNATURES["lsa_ndlu_solve_multi_batch_adjoint_time"] == lsa_hip.SIGNATURES["lsa_ndlu_solve_multi_batch_time"]


@pytest.mark.parametrize("entry", ["solve_multi_batch_adjoint", "time_solve_multi_batch_adjoint"])
def test_argument_errors_need_no_context(entry):
    """``J`` outside 1..16 and list lengths that differ: ``ValueError`` before anything of the library (or of the factorisations: they
    are ``None`` here) is touched; then factorisations and vectors of two contexts."""
    call = getattr(lsa_hip.NdLu, entry)
    extra = (3,) if entry.startswith("time") else ()
    with pytest.raises(ValueError, match="between 1 and 16"):
        call([], [], [], 4, *extra)
    with pytest.raises(ValueError, match="between 1 and 16"):
        call([None] * 17, [None] * 17, [None] * 17, 4, *extra)
    with pytest.raises(ValueError, match="as many blocks"):
        call([None] * 3, [None] * 2, [None] * 3, 4, *extra)
    with pytest.raises(ValueError, match="as many blocks"):
        call([None] * 3, [None] * 3, [None] * 4, 4, *extra, conj=False)
    f = [Fake(object()) for _ in range(2)]  # (contexts without a library: reaching for it would be an AttributeError)
    with pytest.raises(ValueError, match="one context"):
        call(f, f, f, 4, *extra)


def test_forward_entry_still_refuses_trans():
    for trans in ("T", "H"):
        with pytest.raises(ValueError, match="transposed form .* is not built"):
            lsa_hip.NdLu.solve_multi_batch([None] * 3, [None] * 3, [None] * 3, 4, trans=trans)
