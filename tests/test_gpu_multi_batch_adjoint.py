"""GPU tests of the transposed block solve on a batch of factor sets (``lsa_ndlu_solve_multi_batch_adjoint``,
``NdLu.solve_multi_batch_adjoint``): R columns on J factor sets of one analysis in one launch per tree level and direction of the
transposed sweeps (``nd_sweepT_multi_kernel<..., R, NB>`` of ``csrc/ndlu_multi.hip``).  Every column of every set holds, bit for bit,
what ``lsa_ndlu_solve_adjoint`` gives for it on that set alone.  Factor sets as in ``test_gpu_multi_batch.py``: S5k at several
Reynolds numbers (one pattern, other values), S2k (n = 1953, a multiple of no tile) at distinct shifts; and S30k, the smallest
synthetic cylinder case whose forest has a node of more than one tile of outputs and more than one staged chunk of summed rows."""

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

REYNOLDS = tuple(range(40, 91, 5))
TARGETS = ((-0.03 + 0.7197388769374216j), 0.7316769290210628j, (0.018 + 0.7379601143282424j))
PAD = 3           # every block has ld = n + PAD
FILL = 7.0        # what X holds before a solve: the rows between the columns must keep it
TILE = 64         # outputs of one workgroup of the transposed sweeps

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
            if complex(sigma).imag == 0.0:
                C = sp.csr_matrix(C.real)
            dC = lsa_hip.CsrMatrix.from_scipy(hip_ctx, C)
            out.append((lsa_hip.NdLu(hip_ctx, dC, 0), dC, C))
        _FACTORS[key] = out
    return _FACTORS[key]


def _sets(hip_ctx, J, shifts):
    if shifts == "complex_S2k":
        return _factors(hip_ctx, "S2k", REYNOLDS[:1] * J, tuple(TARGETS[0] + 0.01 * j * (1 + 1j) for j in range(J)))
    if shifts == "complex_S30k":
        return _factors(hip_ctx, "S30k", (50,) * J, TARGETS[:J])
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


def _solo_adjoint(hip_ctx, fs, Bs, vdtype, conj):
    """Per set: the block through ``solve_adjoint``, column by column."""
    import lsa_hip

    out = []
    for (f, _, _), B in zip(fs, Bs):
        n, nrhs = B.shape
        cols = np.empty_like(B)
        for q in range(nrhs):
            x = lsa_hip.DeviceVector(hip_ctx, n, vdtype)
            f.solve_adjoint(lsa_hip.DeviceVector.from_numpy(hip_ctx, np.ascontiguousarray(B[:, q])), x, conj=conj)
            cols[:, q] = x.numpy()
        out.append(cols)
    return out


def _assert_blocks(dXs, refs, n, nrhs, pad_is_nan=False):
    for z, (dX, solo) in enumerate(zip(dXs, refs)):
        X, pad = _download(dX, n, nrhs)
        for q in range(nrhs):
            assert np.array_equal(X[:, q], solo[:, q]), f"set {z}, column {q}: not the bits of solve_adjoint"
        assert np.all(np.isnan(pad.real)) if pad_is_nan else np.all(pad == FILL), f"set {z}: the rows between the columns were written"


def _width(nrhs, vdtype):
    most = 8 if vdtype is np.float64 else 4
    return most if nrhs >= most else 4 if nrhs >= 4 else 2


@pytest.mark.parametrize("J,shifts,vdtype,nrhs,conj", [
    (3, "complex", np.complex128, 2, True), (3, "complex", np.complex128, 2, False),
    (3, "complex", np.complex128, 4, True), (3, "complex", np.complex128, 4, False),
    (3, "complex", np.complex128, 5, True), (3, "complex", np.complex128, 5, False), (3, "complex", np.complex128, 1, True),
    (16, "complex_S2k", np.complex128, 4, True), (16, "complex_S2k", np.complex128, 5, False),
    (1, "complex_S2k", np.complex128, 4, True), (1, "complex_S2k", np.complex128, 2, False),
    (3, "complex_S30k", np.complex128, 5, True),
    (3, "real", np.float64, 8, False), (3, "real", np.float64, 7, True),
    (3, "real", np.complex128, 4, True), (1, "real", np.complex128, 4, False)])
def test_adjoint_block_batch_equals_solo_adjoint_solves(hip_ctx, J, shifts, vdtype, nrhs, conj):
    """J in {1, 3, 16}; complex sets with 2 (one narrow pass), 4 (the full width), 5 = 4 + 1 columns (the remainder through the
    batched solo transposed sweep) and one column (that sweep alone); real sets with real vectors (8; 7 = 4 + 2 + 1) and with complex vectors (4); ``conj`` on and off;
    S30k for the node of two tiles and two chunks.  ``ld = n + 3`` with NaN between the columns of B (never read: a NaN would spread)
    and a fill value between those of X (kept).  Then all sets reading ONE B, and in place."""
    import lsa_hip

    fs = _sets(hip_ctx, J, shifts)
    factors = [f for f, _, _ in fs]
    n = fs[0][1].shape[0]
    ld = n + PAD
    Bs = [_columns(n, nrhs, vdtype, seed=100 * nrhs + z) for z in range(J)]
    refs = _solo_adjoint(hip_ctx, fs, Bs, vdtype, conj)
    shared_refs = _solo_adjoint(hip_ctx, fs, [Bs[0]] * J, vdtype, conj)

    def fresh_x():
        return [_upload(hip_ctx, np.zeros_like(Bs[0]), FILL) for _ in range(J)]

    dBs = [_upload(hip_ctx, B, np.nan) for B in Bs]
    dXs = fresh_x()
    lsa_hip.NdLu.solve_multi_batch_adjoint(factors, dBs, dXs, nrhs, conj=conj, ldb=ld, ldx=ld)
    _assert_blocks(dXs, refs, n, nrhs)
    for f in factors:
        assert nrhs == 1 or f.multi_info()["width"] == _width(nrhs, vdtype)  # (one column is lsa_ndlu_solve_batch_adjoint: no pass)
    # all sets read ONE B
    dXs = fresh_x()
    lsa_hip.NdLu.solve_multi_batch_adjoint(factors, [dBs[0]] * J, dXs, nrhs, conj=conj, ldb=ld, ldx=ld)
    _assert_blocks(dXs, shared_refs, n, nrhs)
    # in place: X = B, one block per set
    lsa_hip.NdLu.solve_multi_batch_adjoint(factors, dBs, dBs, nrhs, conj=conj, ldb=ld, ldx=ld)
    _assert_blocks(dBs, refs, n, nrhs, pad_is_nan=True)


def test_s30k_has_a_node_of_two_tiles_and_two_chunks():
    """From the analysis: S30k has a node whose upward transposed sweep has more than 64 outputs (its front) and sums over more than
    ``NDLU_MULTI_CHUNK`` = 256 rows (its pivot block), and one whose downward sweep has more than 64 outputs (pivot block) and sums over
    more than 256 rows (boundary): two tiles and two staged chunks in either direction.  S5k, the next smaller cylinder case, has none."""
    import lsa_hip

    def shapes(name):
        es = _case(name, 50)
        C = sp.csr_matrix((es.A.data - TARGETS[0] * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
        e = lsa_hip.NdAnalysis(C, 0).export()  # (the analysis NdLu(ctx, C, 0) runs: the library's own dissection)
        f = np.asarray(e["front_size"])
        m = np.diff(np.asarray(e["node_start"]))
        return f, m

    f, m = shapes("S30k")
    up = (f > TILE) & (m > lsa_hip.NDLU_MULTI_CHUNK)
    down = (m > TILE) & (f - m > lsa_hip.NDLU_MULTI_CHUNK)
    print(f"S30k: widest pivot block {int(m.max())}, widest boundary {int((f - m).max())}; nodes with two tiles and two chunks: {int(up.sum())} upward, {int(down.sum())} downward")
    assert lsa_hip.NDLU_MULTI_CHUNK == 256
    assert up.any() and down.any()
    f5, m5 = shapes("S5k")
    assert not ((f5 > TILE) & (m5 > lsa_hip.NDLU_MULTI_CHUNK)).any()


def test_adjoint_block_batch_residual_against_superlu(hip_ctx):
    """An anchor that does not pass through the solo kernel: one complex set of a batch of three, 4 columns; the host residual
    ``||C^H x - b||_2`` of every column is at most 10 x the residual ``scipy.sparse.linalg.splu(C^H)`` leaves for the same column (the
    rule and margin of ``test_block_batch_residual_against_superlu``: two backward-stable eliminations with different pivot orders; ten
    covers their growth factors and admits no wrong block)."""
    import lsa_hip

    fs = _sets(hip_ctx, 3, "complex")
    n, nrhs, ld = fs[0][1].shape[0], 4, fs[0][1].shape[0] + PAD
    Bs = [_columns(n, nrhs, np.complex128, seed=40 + z) for z in range(3)]
    dXs = [_upload(hip_ctx, np.zeros_like(B), FILL) for B in Bs]
    lsa_hip.NdLu.solve_multi_batch_adjoint([f for f, _, _ in fs], [_upload(hip_ctx, B, np.nan) for B in Bs], dXs, nrhs, conj=True, ldb=ld, ldx=ld)
    z = 1
    CH = sp.csc_matrix(fs[z][2].conj().T)
    X = _download(dXs[z], n, nrhs)[0]
    lu = spla.splu(CH)
    for q in range(nrhs):
        ours = float(np.linalg.norm(CH @ X[:, q] - Bs[z][:, q]))
        theirs = float(np.linalg.norm(CH @ lu.solve(Bs[z][:, q]) - Bs[z][:, q]))
        print(f"set {z} column {q}: ||C^H x - b||_2 = {ours:.3e} (block-batch transposed sweeps), {theirs:.3e} (SuperLU); ||b||_2 = {np.linalg.norm(Bs[z][:, q]):.3e}")
        assert np.isfinite(ours) and ours <= 10.0 * theirs


def test_forward_and_adjoint_block_batches_share_buffers_and_keep_their_bits(hip_ctx):
    """The update vectors of the per-column buffers serve both directions: a forward block-batch solve, the adjoint one, and the
    forward one again -- the third returns the bytes of the first, and the adjoint one the bits of ``solve_adjoint``."""
    import lsa_hip

    fs = _sets(hip_ctx, 3, "complex")
    factors = [f for f, _, _ in fs]
    n, nrhs, ld = fs[0][1].shape[0], 5, fs[0][1].shape[0] + PAD
    Bs = [_columns(n, nrhs, np.complex128, seed=60 + z) for z in range(3)]
    refs = _solo_adjoint(hip_ctx, fs, Bs, np.complex128, True)

    def forward():
        dXs = [_upload(hip_ctx, np.zeros_like(B), FILL) for B in Bs]
        lsa_hip.NdLu.solve_multi_batch(factors, [_upload(hip_ctx, B, np.nan) for B in Bs], dXs, nrhs, ldb=ld, ldx=ld)
        return [dX.numpy() for dX in dXs]

    first = forward()
    dXs = [_upload(hip_ctx, np.zeros_like(B), FILL) for B in Bs]
    lsa_hip.NdLu.solve_multi_batch_adjoint(factors, [_upload(hip_ctx, B, np.nan) for B in Bs], dXs, nrhs, conj=True, ldb=ld, ldx=ld)
    _assert_blocks(dXs, refs, n, nrhs)
    third = forward()
    for a, b in zip(first, third):
        assert a.tobytes() == b.tobytes()


def test_adjoint_block_batch_ignores_the_transposed_switch(hip_ctx):
    """``lsa_ndlu_set_multi_transposed`` belongs to ``solve_multi``: off (the default) the batch entry still runs its wide passes."""
    import lsa_hip

    fs = _sets(hip_ctx, 3, "complex")
    factors = [f for f, _, _ in fs]
    n, nrhs = fs[0][1].shape[0], 4
    B = _columns(n, nrhs, np.complex128, seed=3)
    for f in factors:
        f.set_multi_transposed(False)
    dB = lsa_hip.DeviceVector.from_numpy(hip_ctx, B.reshape(-1, order="F"))
    dXs = [lsa_hip.DeviceVector(hip_ctx, n * nrhs, np.complex128) for _ in range(3)]
    lsa_hip.NdLu.solve_multi_batch_adjoint(factors, [dB] * 3, dXs, nrhs)
    assert all(f.multi_info()["width"] == 4 for f in factors)
    ms = lsa_hip.NdLu.time_solve_multi_batch_adjoint(factors, [dB] * 3, dXs, nrhs, iters=2)
    assert ms > 0.0
    refs = _solo_adjoint(hip_ctx, fs, [B] * 3, np.complex128, True)
    for dX, ref in zip(dXs, refs):
        assert np.array_equal(dX.numpy().reshape((n, nrhs), order="F"), ref)


def test_adjoint_block_batch_arguments_are_refused(hip_ctx):
    """Each refusal is ``LSA_ERR_ARG`` (a ``ValueError``) naming its condition, and X is left untouched."""
    import ctypes

    import lsa_hip

    fs = _sets(hip_ctx, 3, "complex")
    factors = [f for f, _, _ in fs]
    other = _sets(hip_ctx, 1, "complex_S2k")[0][0]
    n, nrhs = fs[0][1].shape[0], 4
    B = _columns(n, nrhs, np.complex128, seed=5)
    block = lambda: lsa_hip.DeviceVector.from_numpy(hip_ctx, np.full(n * nrhs, FILL + 0j))  # noqa: E731
    dB = lsa_hip.DeviceVector.from_numpy(hip_ctx, B.reshape(-1, order="F"))
    xs = [block() for _ in range(3)]

    def refused(match, fl, bl, xl, cols=nrhs, **kw):
        with pytest.raises(ValueError, match=match):
            lsa_hip.NdLu.solve_multi_batch_adjoint(fl, bl, xl, cols, **kw)
        for x in set(xl):
            assert np.all(x.numpy() == FILL), "a refused call wrote X"

    # J = 17 reaches the library only through the raw entry point: the binding refuses it first
    with pytest.raises(ValueError, match="between 1 and 16"):
        lsa_hip.NdLu.solve_multi_batch_adjoint([factors[0]] * 17, [dB] * 17, [xs[0]] * 17, nrhs)
    J17 = 17
    arr17 = lambda o: (ctypes.c_void_p * J17)(*[o.handle.value] * J17)  # noqa: E731
    with pytest.raises(ValueError, match=r"lsa_ndlu_solve_multi_batch_adjoint: J = 17 outside \[1, 16\]"):
        hip_ctx.check(hip_ctx._lib.lsa_ndlu_solve_multi_batch_adjoint(hip_ctx.handle, J17, arr17(factors[0]), 1, nrhs, arr17(dB), n, arr17(xs[0]), n))
    assert np.all(xs[0].numpy() == FILL)
    x_other = block()
    assert other.n < n
    refused("not of the same analysis", [factors[0], other], [dB, dB], [xs[0], x_other])
    refused("share a factorisation", [factors[0], factors[0]], [dB, dB], xs[:2])
    refused("share an X", factors[:2], [dB, dB], [xs[0], xs[0]])
    refused("overlaps the B of the other", factors[:2], [dB, xs[0]], [xs[0], xs[1]])
    short = lsa_hip.DeviceVector.from_numpy(hip_ctx, np.full(n * nrhs - 1, FILL + 0j))
    refused("needs .* entries", factors[:2], [dB, dB], [xs[0], short])
    refused("below n", factors[:2], [dB, dB], xs[:2], ldb=n - 1)
    refused("in place needs B == X and ldb == ldx", factors[:1], [xs[0]], [xs[0]], cols=2, ldb=n, ldx=n + 1)
    refused("at least one column", factors[:2], [dB, dB], xs[:2], cols=0)
    rB = lsa_hip.DeviceVector.from_numpy(hip_ctx, np.full(n * nrhs, 1.0))
    rxs = [lsa_hip.DeviceVector.from_numpy(hip_ctx, np.full(n * nrhs, FILL)) for _ in range(2)]
    refused("complex factors need complex vectors", factors[:2], [rB, rB], rxs)
