"""CPU suite: the batched transposed entry points are declared, exported and bound; the stochastic front end accepts and stores
``batch_adjoint``; ``NdLu.solve_batch`` and ``CsrMatrix.spmv_transpose_batch`` reject bad input before any device is touched."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import lsa_hip

HEADER = Path(__file__).resolve().parents[1] / "include" / "lsa_hip.h"


def _pair(n=30):
    A = sp.csr_matrix(sp.random(n, n, density=0.2, random_state=1, format="csr") - 2.0 * sp.eye(n, format="csr"))
    A.sort_indices()
    M = sp.csr_matrix((np.zeros(A.nnz), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    M.setdiag(1.0)
    return A, M


class Fake:
    def __init__(self, ctx):
        self.ctx, self.handle = ctx, ctypes.c_void_p(1)


def test_batched_transposed_symbols_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    lib = lsa_hip.load_library()
    for name, nargs in (("lsa_ndlu_solve_batch_adjoint", 6), ("lsa_spmv_transpose_batch", 6), ("lsa_stochastic_set_batch_adjoint", 3)):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(lib, name), name
        restype, argtypes = lsa_hip.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs, name
    fields = [name for name, _ in lsa_hip.lsa_stochastic_stats._fields_]
    struct = re.search(r"typedef struct \{([^}]*)\} lsa_stochastic_stats;", text).group(1)
    declared = re.findall(r"(\w+);", struct)
    assert fields == declared and fields[-5:-2] == ["batch_adjoint", "adjoint_batches", "forward_batches"]


@pytest.mark.parametrize("on", [False, True])
def test_front_end_accepts_and_stores_batch_adjoint(on):
    from Solver.stochastic import StochasticForcingSolver

    sf = StochasticForcingSolver(*_pair(), batch_adjoint=on)
    assert sf._batch_adjoint is on and sf._batch_forward is True
    assert sf.solver._prepared is None  # nothing was prepared: no context was opened
    assert StochasticForcingSolver(*_pair())._batch_adjoint is False  # the default stays off


@pytest.mark.parametrize("bad", ["X", "n", "", None, 1])
def test_solve_batch_rejects_a_bad_trans_before_the_library(bad):
    f = [Fake(object())]  # (a context without a library: reaching for it would be an AttributeError)
    with pytest.raises(ValueError, match="trans must be"):
        lsa_hip.NdLu.solve_batch(f, f, f, trans=bad)
    with pytest.raises(ValueError, match="trans must be"):
        lsa_hip.NdLu.solve_batch([], [], [], trans=bad)


@pytest.mark.parametrize("trans", ["N", "T", "H"])
def test_solve_batch_checks_its_lists_for_every_trans(trans):
    ctx = object()
    f = [Fake(ctx) for _ in range(17)]
    with pytest.raises(ValueError, match="at most 16"):
        lsa_hip.NdLu.solve_batch(f, f, f, trans=trans)
    with pytest.raises(ValueError, match="as many"):
        lsa_hip.NdLu.solve_batch(f[:2], f[:1], f[:2], trans=trans)
    with pytest.raises(ValueError, match="one context"):
        lsa_hip.NdLu.solve_batch([f[0], Fake(object())], f[:2], f[:2], trans=trans)


def test_spmv_transpose_batch_checks_its_lists_on_the_host():
    ctx = object()
    f = [Fake(ctx) for _ in range(3)]
    with pytest.raises(ValueError, match="as many"):
        lsa_hip.CsrMatrix.spmv_transpose_batch([], [], [])
    with pytest.raises(ValueError, match="as many"):
        lsa_hip.CsrMatrix.spmv_transpose_batch(f[:2], f[:1], f[:2])
    with pytest.raises(ValueError, match="one context"):
        lsa_hip.CsrMatrix.spmv_transpose_batch([f[0], Fake(object())], f[:2], f[:2])
