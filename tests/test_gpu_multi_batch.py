"""GPU tests of the block solve on a batch of factor sets (``lsa_ndlu_solve_multi_batch``, ``NdLu.solve_multi_batch``): R columns on J
factor sets of one analysis in one launch per tree level and direction.  Every column of every set holds, bit for bit, what
``lsa_ndlu_solve_multi`` gives on that set alone and what ``lsa_ndlu_solve`` gives column by column.  Factor sets as in
``test_gpu_batch_adjoint.py``: S5k at several Reynolds numbers (one pattern, other values), S2k (n = 1953, a multiple of no tile) at
distinct shifts."""

import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

REYNOLDS = tuple(range(40, 91, 5))
TARGETS = ((-0.03 + 0.7197388769374216j), 0.7316769290210628j, (0.018 + 0.7379601143282424j))
PAD = 3           # every block has ld = n + PAD
FILL = 7.0        # what X holds before a solve: the rows between the columns must keep it

_CASES = {}
_FACTORS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_factors():
    yield
    _FACTORS.clear()


def _case(name, re):
    from synthetic import fem

    if (name, re) not in _CASES:
        _CASES[(name, re)] = fem.cylinder_case(name, re=float(re))
    return _CASES[(name, re)]


def _factors(hip_ctx, name, res, targets):
    """``[(NdLu, device C, host C)]``, one factorisation per (Reynolds number, shift); made once per module."""
    import lsa_hip

    key = (name, tuple(res), tuple(targets))
    if key not in _FACTORS:
        out = []
        for re_, sigma in zip(res, targets):
            es = _case(name, re_)
            C = sp.csr_matrix((es.A.data - sigma * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
            dC = lsa_hip.CsrMatrix.from_scipy(hip_ctx, C)
            out.append((lsa_hip.NdLu(hip_ctx, dC, 0), dC, C))
        _FACTORS[key] = out
    return _FACTORS[key]


def _sets(hip_ctx, J, shifts):
    if shifts == "complex_S2k":
        return _factors(hip_ctx, "S2k", REYNOLDS[:1] * J, tuple(TARGETS[0] + 0.01 * j * (1 + 1j) for j in range(J)))
    targets = TARGETS[:J] if shifts == "complex" else tuple(0.05 + 0.01 * j for j in range(J))
    return _factors(hip_ctx, "S5k", REYNOLDS[:J], targets)


def _columns(n, nrhs, vdtype, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, nrhs)) + 1j * rng.standard_normal((n, nrhs))
    return np.asfortranarray(B.real.copy() if vdtype is np.float64 else B)


def _upload(hip_ctx, cols, fill):
    """The n x nrhs block as one device vector of (n + PAD) nrhs entries, ``fill`` in the rows between the columns."""
    import lsa_hip

    n, nrhs = cols.shape
    flat = np.full((n + PAD, nrhs), fill, dtype=cols.dtype, order="F")
    flat[:n] = cols
    return lsa_hip.DeviceVector.from_numpy(hip_ctx, flat.reshape(-1, order="F"))


def _download(dv, n, nrhs):
    flat = dv.numpy().reshape((n + PAD, nrhs), order="F")
    return flat[:n], flat[n:]


def _references(hip_ctx, fs, Bs, vdtype):
    """Per set: the block through ``solve_multi`` on that set alone, and through ``solve`` column by column."""
    import lsa_hip

    multi, solo = [], []
    for (f, _, _), B in zip(fs, Bs):
        n, nrhs = B.shape
        dX = _upload(hip_ctx, np.zeros_like(B), FILL)
        f.solve_multi(_upload(hip_ctx, B, np.nan), dX, nrhs, ldb=n + PAD, ldx=n + PAD)
        multi.append(_download(dX, n, nrhs)[0].copy())
        cols = np.empty_like(B)
        for q in range(nrhs):
            x = lsa_hip.DeviceVector(hip_ctx, n, vdtype)
            f.solve(lsa_hip.DeviceVector.from_numpy(hip_ctx, np.ascontiguousarray(B[:, q])), x)
            cols[:, q] = x.numpy()
        solo.append(cols)
    return multi, solo


def _assert_blocks(dXs, refs, n, nrhs, pad_is_nan=False):
    for z, (dX, (multi, solo)) in enumerate(zip(dXs, refs)):
        X, pad = _download(dX, n, nrhs)
        for q in range(nrhs):
            assert np.array_equal(X[:, q], multi[:, q]), f"set {z}, column {q}: not the bits of solve_multi on the set alone"
            assert np.array_equal(X[:, q], solo[:, q]), f"set {z}, column {q}: not the bits of solve"
        assert np.all(np.isnan(pad.real)) if pad_is_nan else np.all(pad == FILL), f"set {z}: the rows between the columns were written"


@pytest.mark.parametrize("J,shifts,vdtype,nrhs", [(3, "complex", np.complex128, 2), (3, "complex", np.complex128, 4),
                                                  (3, "complex", np.complex128, 5), (3, "complex", np.complex128, 7),
                                                  (16, "complex_S2k", np.complex128, 4), (1, "complex_S2k", np.complex128, 4),
                                                  (3, "real", np.complex128, 5), (3, "real", np.float64, 8), (3, "real", np.float64, 9)])
def test_block_batch_equals_solo_block_and_column_solves(hip_ctx, J, shifts, vdtype, nrhs):
    """The cases of the issue: complex factors on S5k at three Reynolds numbers with one pass (2), the full width (4), 4 + 1 (the
    remainder through the batched solo sweep) and 4 + 2 + 1 columns; sixteen shifts of S2k (the last pointer slot); one set; real
    factors with complex (4 + 1) and real vectors (8, 8 + 1).  ``ld = n + 3`` with NaN between the columns of B (never read: a NaN
    would spread) and a fill value between those of X (kept).  Then all sets reading ONE B, in place, and a second time."""
    import lsa_hip

    fs = _sets(hip_ctx, J, shifts)
    factors = [f for f, _, _ in fs]
    n = fs[0][1].shape[0]
    ld = n + PAD
    Bs = [_columns(n, nrhs, vdtype, seed=100 * nrhs + z) for z in range(J)]
    refs = list(zip(*_references(hip_ctx, fs, Bs, vdtype)))
    shared_refs = list(zip(*_references(hip_ctx, fs, [Bs[0]] * J, vdtype)))

    def fresh_x():
        return [_upload(hip_ctx, np.zeros_like(Bs[0]), FILL) for _ in range(J)]

    dBs = [_upload(hip_ctx, B, np.nan) for B in Bs]
    dXs = fresh_x()
    lsa_hip.NdLu.solve_multi_batch(factors, dBs, dXs, nrhs, ldb=ld, ldx=ld)
    _assert_blocks(dXs, refs, n, nrhs)
    for f in factors:
        assert f.multi_info()["width"] == (8 if vdtype is np.float64 else 4 if nrhs >= 4 else 2)
    # all sets read ONE B
    dXs = fresh_x()
    lsa_hip.NdLu.solve_multi_batch(factors, [dBs[0]] * J, dXs, nrhs, ldb=ld, ldx=ld)
    _assert_blocks(dXs, shared_refs, n, nrhs)
    # in place: X = B, one block per set
    lsa_hip.NdLu.solve_multi_batch(factors, dBs, dBs, nrhs, ldb=ld, ldx=ld)
    _assert_blocks(dBs, refs, n, nrhs, pad_is_nan=True)
    # a second time on fresh blocks
    dBs = [_upload(hip_ctx, B, np.nan) for B in Bs]
    dXs = fresh_x()
    lsa_hip.NdLu.solve_multi_batch(factors, dBs, dXs, nrhs, ldb=ld, ldx=ld)
    _assert_blocks(dXs, refs, n, nrhs)


def test_block_batch_residual_against_superlu(hip_ctx):
    """An anchor that does not pass through the solo kernel: J = 3 complex sets, 4 columns; the host residual ``||C_z x - b||_2`` of
    every column is at most 10 x the residual ``scipy.sparse.linalg.splu(C_z)`` leaves for the same column (the rule and margin of
    ``test_batched_adjoint_residual_against_superlu``: two backward-stable eliminations with different pivot orders; ten covers their
    growth factors and admits no wrong block)."""
    import lsa_hip

    fs = _sets(hip_ctx, 3, "complex")
    n, nrhs, ld = fs[0][1].shape[0], 4, fs[0][1].shape[0] + PAD
    Bs = [_columns(n, nrhs, np.complex128, seed=40 + z) for z in range(3)]
    dXs = [_upload(hip_ctx, np.zeros_like(B), FILL) for B in Bs]
    lsa_hip.NdLu.solve_multi_batch([f for f, _, _ in fs], [_upload(hip_ctx, B, np.nan) for B in Bs], dXs, nrhs, ldb=ld, ldx=ld)
    for z, ((_, _, C), B, dX) in enumerate(zip(fs, Bs, dXs)):
        X = _download(dX, n, nrhs)[0]
        lu = spla.splu(sp.csc_matrix(C))
        for q in range(nrhs):
            ours = float(np.linalg.norm(C @ X[:, q] - B[:, q]))
            theirs = float(np.linalg.norm(C @ lu.solve(B[:, q]) - B[:, q]))
            print(f"set {z} column {q}: ||C x - b||_2 = {ours:.3e} (block-batch sweeps), {theirs:.3e} (SuperLU); ||b||_2 = {np.linalg.norm(B[:, q]):.3e}")
            assert np.isfinite(ours) and ours <= 10.0 * theirs


def test_neighbouring_solves_keep_their_bits(hip_ctx):
    """The sweep buffers are shared: after a batched block solve, a solo ``solve``, a ``solve_batch`` and a ``solve_multi(trans="H")`` on
    the same sets return what they returned before it."""
    import lsa_hip

    fs = _sets(hip_ctx, 3, "complex")
    factors = [f for f, _, _ in fs]
    n, nrhs, ld = fs[0][1].shape[0], 4, fs[0][1].shape[0] + PAD
    B = _columns(n, nrhs, np.complex128, seed=77)
    col = lambda q: lsa_hip.DeviceVector.from_numpy(hip_ctx, np.ascontiguousarray(B[:, q]))  # noqa: E731

    def neighbours():
        x = lsa_hip.DeviceVector(hip_ctx, n, np.complex128)
        factors[1].solve(col(0), x)
        xs = [lsa_hip.DeviceVector(hip_ctx, n, np.complex128) for _ in range(3)]
        lsa_hip.NdLu.solve_batch(factors, [col(z) for z in range(3)], xs)
        dX = _upload(hip_ctx, np.zeros_like(B), FILL)
        factors[2].solve_multi(_upload(hip_ctx, B, np.nan), dX, nrhs, ldb=ld, ldx=ld, trans="H")
        return [x.numpy()] + [v.numpy() for v in xs] + [dX.numpy()]

    before = neighbours()
    dXs = [_upload(hip_ctx, np.zeros_like(B), FILL) for _ in range(3)]
    lsa_hip.NdLu.solve_multi_batch(factors, [_upload(hip_ctx, B, np.nan)] * 3, dXs, nrhs, ldb=ld, ldx=ld)
    after = neighbours()
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()


def test_block_batch_arguments_are_refused(hip_ctx):
    """Each refusal is ``LSA_ERR_ARG`` (a ``ValueError``) naming its condition, and X is left untouched."""
    import lsa_hip

    fs = _sets(hip_ctx, 3, "complex")
    factors = [f for f, _, _ in fs]
    other = _sets(hip_ctx, 1, "complex_S2k")[0][0]
    n, nrhs = fs[0][1].shape[0], 4
    B = _columns(n, nrhs, np.complex128, seed=5)
    block = lambda: lsa_hip.DeviceVector.from_numpy(hip_ctx, np.full(n * nrhs, FILL + 0j))  # noqa: E731
    dB = lsa_hip.DeviceVector.from_numpy(hip_ctx, B.reshape(-1, order="F"))
    xs = [block() for _ in range(3)]

    def refused(match, fl, bl, xl, cols=nrhs, lib_trans=0, **kw):
        with pytest.raises(ValueError, match=match):
            if lib_trans:  # (the binding refuses trans itself: the library's own refusal through the raw entry point)
                J = len(fl)
                arr = lambda objs: (ctypes.c_void_p * J)(*[o.handle.value for o in objs])  # noqa: E731
                hip_ctx.check(hip_ctx._lib.lsa_ndlu_solve_multi_batch(hip_ctx.handle, J, arr(fl), lib_trans, cols, arr(bl), n, arr(xl), n))
            else:
                lsa_hip.NdLu.solve_multi_batch(fl, bl, xl, cols, **kw)
        for x in set(xl):
            assert np.all(x.numpy() == FILL), "a refused call wrote X"

    # J = 17 reaches the library only through the raw entry point: the binding refuses it first
    with pytest.raises(ValueError, match="between 1 and 16"):
        lsa_hip.NdLu.solve_multi_batch([factors[0]] * 17, [dB] * 17, [xs[0]] * 17, nrhs)
    J17 = 17
    arr17 = lambda o: (ctypes.c_void_p * J17)(*[o.handle.value] * J17)  # noqa: E731
    with pytest.raises(ValueError, match=r"J = 17 outside \[1, 16\]"):
        hip_ctx.check(hip_ctx._lib.lsa_ndlu_solve_multi_batch(hip_ctx.handle, J17, arr17(factors[0]), 0, nrhs, arr17(dB), n, arr17(xs[0]), n))
    assert np.all(xs[0].numpy() == FILL)
    n2 = other.n
    x_other = lsa_hip.DeviceVector.from_numpy(hip_ctx, np.full(n * nrhs, FILL + 0j))
    assert n2 < n
    refused("not of the same analysis", [factors[0], other], [dB, dB], [xs[0], x_other])
    refused("share a factorisation", [factors[0], factors[0]], [dB, dB], xs[:2])
    refused("share an X", factors[:2], [dB, dB], [xs[0], xs[0]])
    short = lsa_hip.DeviceVector.from_numpy(hip_ctx, np.full(n * nrhs - 1, FILL + 0j))
    refused("needs .* entries", factors[:2], [dB, dB], [xs[0], short])
    refused("below n", factors[:2], [dB, dB], xs[:2], ldb=n - 1)
    rB = lsa_hip.DeviceVector.from_numpy(hip_ctx, np.full(n * nrhs, 1.0))
    rxs = [lsa_hip.DeviceVector.from_numpy(hip_ctx, np.full(n * nrhs, FILL)) for _ in range(2)]
    refused("complex factors need complex vectors", factors[:2], [rB, rB], rxs)
    refused("transposed form .* is not built", factors[:2], [dB, dB], xs[:2], lib_trans=2)
