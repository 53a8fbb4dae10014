"""GPU suite: every form ``lsa_spmv`` can dispatch to, against an extended-precision product, component by component.

The default dispatch runs ``spmv_group_kernel`` only for matrices of 4 Mi entries or more, so the kernel-level tests of
``test_gpu_kernels.py`` all exercise ``spmv_subwave_kernel``.  Here the variant word (``LSA_SPMV_VARIANT``, read on every
call) forces each form on matrices of a few thousand rows: row groups at every lanes-per-row count, with 16-bit indices,
with XCD chunks and with a grid-stride pass; the ungrouped sub-wave forms at every lanes-per-row count, non-temporal,
XCD rows, two rows per sub-wave and 16-bit indices; and the transposed pull kernel.  Every case

  * asserts on ``matvec_info(dtype)["kernel"]`` that the intended kernel and template arguments were chosen,
  * starts from an output full of NaN (a row never written fails), runs twice and requires identical bytes (the kernels add
    in a fixed order),
  * requires ``|y_i - ref_i| <= 2 (L_i + 3) u sum_j |a_ij| |x_j|`` for every row i (``extended_reference.bound``): derived,
    not measured; a row without entries has bound 0 and must come back as exactly 0,

at all three scalar pairings (real * real, real * complex, complex * complex)."""

import numpy as np
import pytest
import scipy.sparse as sp

import extended_reference as xr

pytestmark = pytest.mark.gpu

PAIRINGS = [(False, False), (False, True), (True, True)]
GROUPS, C16, XCD_GROUPS, NO_GROUPS = 0x2000, 0x800, 0x8000, 0x4000
NT, XCD_ROWS, TWO_ROWS = 0x100, 0x200, 0x400
ONE_WG_PER_CU = 1 << 16  # grid capped at one workgroup per compute unit: the kernels' grid-stride loops go round more than once


def _library_groups(A):
    """The row groups ``ensure_groups`` forms (restated): consecutive rows with one column pattern, at most four."""
    rp, ci = A.indptr, A.indices
    sizes, cur = [], 1
    for r in range(1, A.shape[0]):
        a0, a1, b1 = rp[r - 1], rp[r], rp[r + 1]
        if cur < 4 and a1 - a0 == b1 - a1 and np.array_equal(ci[a0:a1], ci[a1:b1]):
            cur += 1
        else:
            sizes.append(cur)
            cur = 1
    sizes.append(cur)
    return sizes


def _distinct_columns(rng, ncols, l):
    """l distinct columns in random order"""
    if 4 * l > ncols:
        return rng.choice(ncols, size=l, replace=False)
    while True:
        draw = rng.integers(0, ncols, size=2 * l + 8)
        _, first = np.unique(draw, return_index=True)
        if first.size >= l:
            return draw[np.sort(first)[:l]]


def _grouped_matrix(seed, ngroups, len_lo, len_hi, ncols=None):
    """Real CSR matrix of consecutive row groups (1 to 4 rows with one column set, values differing per row), stored with
    UNSORTED columns inside every row.  In front of the random groups: a run of 9 identical rows (4 + 4 + 1 for the library),
    three empty rows, two rows of length 1, and two rows of 300 entries (longer than 4 x 64 lanes).  Exactly ``ngroups``
    groups by the library's rule; about one entry in nine is an explicit zero."""
    rng = np.random.default_rng(seed)
    special = [(9, 23), (3, 0), (2, 1), (2, 300)]  # (rows, entries per row); 9 rows make 3 groups
    nspecial = 3 + 1 + 1 + 1
    sizes = rng.choice([1, 2, 3, 4], size=ngroups - nspecial, p=[0.3, 0.3, 0.2, 0.2])  # mean 2.3 >= the library's threshold 1.5
    lens = rng.integers(len_lo, len_hi + 1, size=sizes.size)
    blocks = special + list(zip(sizes.tolist(), lens.tolist()))
    n = int(sum(g for g, _ in blocks))
    ncols = n if ncols is None else ncols
    assert n == ncols and max(l for _, l in blocks) <= ncols
    indptr, indices = [0], []
    prev = None
    for g, l in blocks:
        while True:
            cols = _distinct_columns(rng, ncols, l)  # unsorted
            if l == 0 or prev is None or not np.array_equal(np.sort(cols), prev):
                break
        prev = np.sort(cols)
        for _ in range(g):
            indices.append(cols)
            indptr.append(indptr[-1] + l)
    indices = np.concatenate(indices).astype(np.int32)
    data = rng.standard_normal(indices.size)
    data[rng.random(indices.size) < 1.0 / 9.0] = 0.0
    A = sp.csr_matrix((data, indices, np.asarray(indptr, dtype=np.int32)), shape=(n, ncols))
    S = A.copy()
    S.sort_indices()
    got = _library_groups(S)
    assert len(got) == ngroups and got[:6] == [4, 4, 1, 3, 2, 2], (len(got), got[:6])
    assert not A.has_sorted_indices
    return A


def _imag_like(A, seed):
    """complex matrix on A's pattern: A's values as real parts, seeded normal imaginary parts (explicit zeros stay zeros)"""
    rng = np.random.default_rng(seed)
    C = A.astype(np.complex128)
    C.data = A.data + 1j * rng.standard_normal(A.nnz) * (A.data != 0.0)
    return C


class _Case:
    """One matrix with its device copies, vectors and extended references, built once per module."""

    def __init__(self, ctx, name, A):
        self.ctx, self.name = ctx, name
        self.A = {False: A, True: _imag_like(A, 77)}
        rng = np.random.default_rng(sum(map(ord, name)))
        xre, xim = rng.standard_normal(A.shape[1]), rng.standard_normal(A.shape[1])
        self.x = {False: xre, True: xre + 1j * xim}
        self.sizes = _library_groups(self._sorted(A))
        self.ngroups = len(self.sizes)
        self._dev, self._ref = {}, {}

    @staticmethod
    def _sorted(A):
        S = A.copy()
        S.sort_indices()
        return S

    def fresh_device_matrix(self, mat_c):
        """a new upload: the group table and the 16-bit indices are built lazily on first use and kept with the matrix, so
        every variant gets a matrix that has not seen another one"""
        import lsa_hip

        return lsa_hip.CsrMatrix.from_scipy(self.ctx, self.A[mat_c])

    def ref(self, mat_c, vec_c, trans=None):
        key = (mat_c, vec_c, trans)
        if key not in self._ref:
            self._ref[key] = xr.spmv_ext(self.A[mat_c], self.x[vec_c], trans)
        return self._ref[key]


_CASES = {}


def _case(ctx, name):
    if name not in _CASES:
        if name == "grouped512":
            A = _grouped_matrix(1, 512, 1, 40)
        elif name == "grouped511":
            A = _grouped_matrix(2, 511, 1, 40)
        elif name == "grouped513":
            A = _grouped_matrix(3, 513, 1, 40)
        elif name == "grouped1000":
            A = _grouped_matrix(4, 1003, 1, 40)
        elif name == "grouped8300":  # 8300 x 16 lanes / 256 = 519 workgroups wanted, 256 compute units
            A = _grouped_matrix(5, 8300, 1, 24)
        elif name == "rows90":  # about 90 entries per row, as on a 3D Taylor-Hood mesh: the automatic choice is 32 lanes per row
            A = _grouped_matrix(6, 201, 80, 100)
            assert 48.0 < A.nnz / A.shape[0] <= 96.0
        elif name == "taylor_hood":
            from synthetic import fem

            A = fem.cylinder_case("S2k").A.tocsr()
        else:
            raise KeyError(name)
        _CASES[name] = _Case(ctx, name, A)
    return _CASES[name]


def _nan_vector(ctx, n, cplx):
    import lsa_hip

    fill = np.full(n, np.nan + 1j * np.nan if cplx else np.nan, dtype=np.complex128 if cplx else np.float64)
    return lsa_hip.DeviceVector.from_numpy(ctx, fill)


def _tn(c):
    return "cplx" if c else "double"


def _check_product(got, again, ref, what):
    assert got.tobytes() == again.tobytes(), f"{what}: two runs differ"
    err, bnd = ref.error(got), ref.bound()
    bad = np.flatnonzero(~(err <= bnd))  # (NaN compares false: a row never written is bad)
    assert bad.size == 0, f"{what}: {bad.size} rows outside the bound, first {bad[:5]}, error {err[bad[:5]]}, bound {bnd[bad[:5]]}, length {ref.lengths[bad[:5]]}"
    empty = ref.lengths == 0
    assert np.all(got[empty] == 0), f"{what}: rows without entries must be exactly 0"


def _run_form(ctx, monkeypatch, case, variant, expect):
    """``expect(mt, vt)`` -> the kernel string ``matvec_info`` must report"""
    import lsa_hip

    monkeypatch.setenv("LSA_SPMV_VARIANT", str(variant))
    for mat_c, vec_c in PAIRINGS:
        dA = case.fresh_device_matrix(mat_c)
        what = f"{case.name} variant {variant:#x} {_tn(mat_c)}*{_tn(vec_c)}"
        kernel = dA.matvec_info(np.complex128 if vec_c else np.float64)["kernel"]
        assert kernel == expect(_tn(mat_c), _tn(vec_c)), what
        dx = lsa_hip.DeviceVector.from_numpy(ctx, case.x[vec_c])
        y1, y2 = _nan_vector(ctx, dA.shape[0], vec_c), _nan_vector(ctx, dA.shape[0], vec_c)
        dA.matvec(dx, y1)
        dA.matvec(dx, y2)
        _check_product(y1.numpy(), y2.numpy(), case.ref(mat_c, vec_c), what)


@pytest.mark.parametrize("name", ["grouped513", "taylor_hood", "rows90"])
@pytest.mark.parametrize("lpr", [4, 8, 16, 32, 64])
def test_grouped_every_lanes_per_row(hip_ctx, monkeypatch, name, lpr):
    case = _case(hip_ctx, name)
    assert (case.ngroups * lpr) % 256 != 0  # the last workgroup is not full
    _run_form(hip_ctx, monkeypatch, case, GROUPS | lpr, lambda mt, vt: f"spmv_group_kernel<{mt},{vt},{lpr},false,false>")


def test_grouped_automatic_lanes_per_row(hip_ctx, monkeypatch):
    """no lane count in the variant word: chosen from the mean row length (32 at about 90 entries per row, 16 on Taylor-Hood 2D)"""
    _run_form(hip_ctx, monkeypatch, _case(hip_ctx, "rows90"), GROUPS, lambda mt, vt: f"spmv_group_kernel<{mt},{vt},32,false,false>")
    _run_form(hip_ctx, monkeypatch, _case(hip_ctx, "taylor_hood"), GROUPS, lambda mt, vt: f"spmv_group_kernel<{mt},{vt},16,false,false>")


@pytest.mark.parametrize("name", ["grouped512", "taylor_hood"])
def test_grouped_16bit_indices(hip_ctx, monkeypatch, name):
    _run_form(hip_ctx, monkeypatch, _case(hip_ctx, name), GROUPS | C16 | 16, lambda mt, vt: f"spmv_group_kernel<{mt},{vt},16,true,false>")
    # XCD chunks are not combined with 16-bit indices: the 16-bit form runs, and the report says so
    _run_form(hip_ctx, monkeypatch, _case(hip_ctx, name), GROUPS | C16 | XCD_GROUPS | 16, lambda mt, vt: f"spmv_group_kernel<{mt},{vt},16,true,false>")


@pytest.mark.parametrize("name,xcd", [("grouped511", False), ("grouped512", True), ("grouped513", True), ("grouped1000", True), ("taylor_hood", True)])
def test_grouped_xcd_chunks(hip_ctx, monkeypatch, name, xcd):
    """the XCD-chunked form runs from 8 x 64 groups on; below, the plain grouped form runs and ``lsa_spmv_info`` reports that"""
    case = _case(hip_ctx, name)
    assert (case.ngroups >= 512) == xcd
    flag = "true" if xcd else "false"
    _run_form(hip_ctx, monkeypatch, case, GROUPS | XCD_GROUPS | 16, lambda mt, vt: f"spmv_group_kernel<{mt},{vt},16,false,{flag}>")
    if name == "grouped1000":
        _run_form(hip_ctx, monkeypatch, case, GROUPS | XCD_GROUPS | 64, lambda mt, vt: f"spmv_group_kernel<{mt},{vt},64,false,true>")
        _run_form(hip_ctx, monkeypatch, case, GROUPS | XCD_GROUPS | 4, lambda mt, vt: f"spmv_group_kernel<{mt},{vt},4,false,true>")


def test_grid_stride_passes(hip_ctx, monkeypatch):
    """One workgroup per compute unit and 8300 groups / 19 000 rows: every kernel's outer loop goes round more than once
    (8300 x 16 / 256 = 519 workgroups of groups and 19 000 x 16 / 256 = 1180 of rows wanted, 256 compute units)."""
    case = _case(hip_ctx, "grouped8300")
    assert case.ngroups * 16 // 256 > 2 * 256 and case.A[False].shape[0] * 4 // 256 > 256
    cap = ONE_WG_PER_CU
    _run_form(hip_ctx, monkeypatch, case, cap | GROUPS | 16, lambda mt, vt: f"spmv_group_kernel<{mt},{vt},16,false,false>")
    _run_form(hip_ctx, monkeypatch, case, cap | GROUPS | 64, lambda mt, vt: f"spmv_group_kernel<{mt},{vt},64,false,false>")
    _run_form(hip_ctx, monkeypatch, case, cap | GROUPS | C16 | 16, lambda mt, vt: f"spmv_group_kernel<{mt},{vt},16,true,false>")
    _run_form(hip_ctx, monkeypatch, case, cap | GROUPS | XCD_GROUPS | 16, lambda mt, vt: f"spmv_group_kernel<{mt},{vt},16,false,true>")
    _run_form(hip_ctx, monkeypatch, case, cap | 16, lambda mt, vt: f"spmv_subwave_kernel<{mt},{vt},16>")
    _run_form(hip_ctx, monkeypatch, case, cap | 4, lambda mt, vt: f"spmv_subwave_kernel<{mt},{vt},4>")
    _run_form(hip_ctx, monkeypatch, case, cap | TWO_ROWS | 16, lambda mt, vt: f"spmv_subwave2_kernel<{mt},{vt},16>")
    _run_form(hip_ctx, monkeypatch, case, cap | XCD_ROWS | 16, lambda mt, vt: f"spmv_xcd_kernel<{mt},{vt},16>")
    _run_form(hip_ctx, monkeypatch, case, cap | C16 | 16, lambda mt, vt: f"spmv_subwave16_kernel<{mt},{vt},16>")
    _run_form(hip_ctx, monkeypatch, case, cap | NT | 16, lambda mt, vt: f"spmv_subwave_kernel<{mt},{vt},16,true>")


@pytest.mark.parametrize("name", ["grouped513", "taylor_hood", "rows90"])
@pytest.mark.parametrize("lpr", [4, 8, 16, 32, 64])
def test_ungrouped_every_lanes_per_row(hip_ctx, monkeypatch, name, lpr):
    case = _case(hip_ctx, name)
    _run_form(hip_ctx, monkeypatch, case, lpr, lambda mt, vt: f"spmv_subwave_kernel<{mt},{vt},{lpr}>")
    _run_form(hip_ctx, monkeypatch, case, NO_GROUPS | lpr, lambda mt, vt: f"spmv_subwave_kernel<{mt},{vt},{lpr}>")


@pytest.mark.parametrize("name", ["grouped513", "taylor_hood"])
@pytest.mark.parametrize("lpr", [4, 16, 64])
def test_ungrouped_forms(hip_ctx, monkeypatch, name, lpr):
    """non-temporal matrix loads, XCD-contiguous row chunks, two rows per sub-wave, 16-bit indices, and the non-temporal
    instances of the XCD and two-row kernels; row groups are never combined with these (the variant word asks for both)"""
    case = _case(hip_ctx, name)
    assert case.A[False].shape[0] >= 8 * 256 // lpr
    run = lambda variant, expect: _run_form(hip_ctx, monkeypatch, case, variant | lpr, expect)  # noqa: E731
    run(NT, lambda mt, vt: f"spmv_subwave_kernel<{mt},{vt},{lpr},true>")
    run(XCD_ROWS, lambda mt, vt: f"spmv_xcd_kernel<{mt},{vt},{lpr}>")
    run(TWO_ROWS, lambda mt, vt: f"spmv_subwave2_kernel<{mt},{vt},{lpr}>")
    run(C16, lambda mt, vt: f"spmv_subwave16_kernel<{mt},{vt},{lpr}>")
    run(NT | XCD_ROWS, lambda mt, vt: f"spmv_xcd_kernel<{mt},{vt},{lpr},true>")
    run(NT | TWO_ROWS, lambda mt, vt: f"spmv_subwave2_kernel<{mt},{vt},{lpr},true>")
    run(GROUPS | NT, lambda mt, vt: f"spmv_subwave_kernel<{mt},{vt},{lpr},true>")
    run(GROUPS | TWO_ROWS, lambda mt, vt: f"spmv_subwave2_kernel<{mt},{vt},{lpr}>")


def test_xcd_rows_needs_eight_workgroups_of_rows(hip_ctx, monkeypatch):
    """fewer than 8 x 256 / LPR rows: the plain sub-wave kernel runs, and the report says so"""
    case = _case(hip_ctx, "rows90")
    n = case.A[False].shape[0]
    assert 8 * 256 // 16 <= n < 8 * 256 // 4
    _run_form(hip_ctx, monkeypatch, case, XCD_ROWS | 4, lambda mt, vt: f"spmv_subwave_kernel<{mt},{vt},4>")
    _run_form(hip_ctx, monkeypatch, case, XCD_ROWS | 16, lambda mt, vt: f"spmv_xcd_kernel<{mt},{vt},16>")


def test_default_dispatch_of_small_matrices(hip_ctx, monkeypatch):
    """no variant word: matrices below 4 Mi entries run the plain sub-wave kernel (what the other suites measure)"""
    monkeypatch.delenv("LSA_SPMV_VARIANT", raising=False)
    _run_form(hip_ctx, monkeypatch, _case(hip_ctx, "taylor_hood"), 0, lambda mt, vt: f"spmv_subwave_kernel<{mt},{vt},16>")
    _run_form(hip_ctx, monkeypatch, _case(hip_ctx, "rows90"), 0, lambda mt, vt: f"spmv_subwave_kernel<{mt},{vt},32>")


def _transpose_matrix():
    """300 x 300: random pattern, columns 7 and 150..159 empty, column 40 with an entry in 200 rows (more than 64, more than
    4 x 16 lanes), explicit zeros"""
    rng = np.random.default_rng(21)
    n = 300
    A = sp.random(n, n, density=0.03, random_state=22, format="lil", data_rvs=rng.standard_normal)
    A[rng.choice(n, size=200, replace=False), 40] = rng.standard_normal(200)
    A = sp.csc_matrix(A)
    for c in [7] + list(range(150, 160)):
        A.data[A.indptr[c] : A.indptr[c + 1]] = 0.0
    A.eliminate_zeros()
    A = sp.csr_matrix(A)
    A.data[::11] = 0.0  # explicit zeros stay in the pattern
    return A


@pytest.mark.parametrize("mat_c,vec_c", PAIRINGS)
@pytest.mark.parametrize("conj", [True, False])
def test_transposed_product(hip_ctx, mat_c, vec_c, conj):
    import lsa_hip

    if "transpose" not in _CASES:
        _CASES["transpose"] = _Case(hip_ctx, "transpose", _transpose_matrix())
    case = _CASES["transpose"]
    counts = np.bincount(case.A[False].indices, minlength=300)
    assert counts[7] == 0 and np.all(counts[150:160] == 0) and counts[40] > 64
    dA = case.fresh_device_matrix(mat_c)
    dx = lsa_hip.DeviceVector.from_numpy(hip_ctx, case.x[vec_c])
    y1, y2 = _nan_vector(hip_ctx, 300, vec_c), _nan_vector(hip_ctx, 300, vec_c)
    dA.rmatvec(dx, y1, conj=conj)
    dA.rmatvec(dx, y2, conj=conj)
    ref = case.ref(mat_c, vec_c, "H" if conj else "T")
    _check_product(y1.numpy(), y2.numpy(), ref, f"transpose conj={conj} {_tn(mat_c)}*{_tn(vec_c)}")
