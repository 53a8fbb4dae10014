"""CPU suite: what the four Lanczos-type handles of the binding (``LanczosBasis``, ``ResolventBasis``, ``GrowthBasis``,
``StochasticBasis``) send to the library and hand back, against a recording stand-in for the context.  No GPU and no library: every
``lsa_*`` entry is a callable that records its arguments and returns 0.  The assertions are about behaviour (names called, what the
pointers hold, the options, the results' keys and layout, the handle's lifetime), not about how the classes are put together."""

import ctypes
import gc
from types import SimpleNamespace

import numpy as np
import pytest

import lsa_hip

N, NCV, HANDLE = 5, 4, 0xBEEF
RESULT = dict(nconv=1, nout=2, restarts=3, op_applies=17, next_unconverged=0.125, seconds_expand=0.5, seconds_dense=0.25, seconds_restart=0.75)
TAIL = {"nconv": 1, "restarts": 3, "applies": 17, "next_unconverged": 0.125, "seconds_expand": 0.5, "seconds_dense": 0.25, "seconds_restart": 0.75}
DTYPES = {"lanczos": np.float64, "resolvent": np.complex128, "growth": np.float64, "stochastic": np.float64}
OTHERS = ("adjoint_solves", "forward_solves", "refined_adjoint", "refined_forward")
COUNTERS = {"resolvent": OTHERS, "stochastic": OTHERS, "growth": ("forward_solves", "transposed_solves", "refined_forward", "refined_transposed")}
KEYS = {"resolvent": {"theta", "gains", "responses", "forcings", "estimates"},
        "growth": {"gains", "initial", "responses", "energy", "response_energy", "estimates"},
        "stochastic": {"variances", "modes", "estimates"}}


def _read(pointer, dtype, count):
    """What a ``c_void_p`` argument points at, copied while the caller's array is alive."""
    dtype = np.dtype(dtype)
    return np.frombuffer((ctypes.c_char * (dtype.itemsize * count)).from_address(pointer.value), dtype=dtype).copy()


class _Lib:
    def __init__(self, owner):
        self._owner = owner

    def __getattr__(self, name):
        if not name.startswith("lsa_"):
            raise AttributeError(name)
        owner = self._owner

        def entry(*args):
            owner.calls.append((name, args))
            prefix = name.split("_")[1]
            if name.endswith("_create"):
                if owner.fail_create:
                    return -1
                args[-1]._obj.value = HANDLE
            elif name.endswith("_set_row_permutation"):
                owner.seen.append(None if args[2] is None else _read(args[2], np.int32, N))
            elif name.endswith("_set_start"):
                owner.seen.append(_read(args[2], DTYPES[prefix], N))
            elif name.endswith("_solve"):
                owner.seen.append(None if args[3] is None else _read(args[3], DTYPES[prefix], N))
                res = next(a._obj for a in args if isinstance(getattr(a, "_obj", None), lsa_hip.lsa_ks_result))
                for key, value in RESULT.items():
                    setattr(res, key, value)
                if isinstance(args[-1], ctypes.c_void_p):  # the four solve counters
                    (ctypes.c_int64 * 4).from_address(args[-1].value)[:] = [1, 2, 3, 4]
            return 0

        return entry


class _Context:
    """The members of ``lsa_hip.Context`` the handle classes use."""

    def __init__(self):
        self.calls, self.seen, self.fail_create = [], [], False
        self._lib = _Lib(self)
        self.handle = ctypes.c_void_p(0xC0DE)

    def check(self, rc):
        if rc != 0:
            raise ValueError(f"status {rc}")

    def names(self):
        return [name for name, _ in self.calls]


def _make(prefix, ctx, **kw):
    op = SimpleNamespace(n=N, handle=ctypes.c_void_p(7))
    if prefix == "lanczos":
        return lsa_hip.LanczosBasis(ctx, op, NCV)
    if prefix == "resolvent":
        return lsa_hip.ResolventBasis(ctx, op, NCV)
    if prefix == "growth":
        return lsa_hip.GrowthBasis(ctx, op, NCV, 3, **kw)
    mat = SimpleNamespace(shape=(N, N), handle=ctypes.c_void_p(9))
    return lsa_hip.StochasticBasis(ctx, mat, mat, [0.5j, 1.5j], [1.0, 2.0], NCV)


def _solve(prefix, obj, **kw):
    if prefix == "lanczos":
        return obj.solve(2, 1e-9, 7, 3, 0.25, seed=11, **kw)
    return obj.solve(2, 1e-9, 7, seed=11, **kw)


def _options(ctx):
    name, args = next(c for c in ctx.calls if c[0].endswith("_solve"))
    return args[2]._obj


PREFIXES = sorted(DTYPES)


@pytest.mark.parametrize("prefix", PREFIXES)
def test_every_call_goes_to_the_class_own_prefix(prefix):
    ctx = _Context()
    obj = _make(prefix, ctx)
    obj.set_row_permutation(np.arange(N))
    if prefix != "stochastic":
        obj.set_start(np.ones(N))
        assert obj.extend(0, 2, np.zeros((NCV + 1, NCV), order="F")) == -1
        obj.basis(2)
    _solve(prefix, obj)
    assert ctx.calls and all(name.startswith(f"lsa_{prefix}_") for name in ctx.names()), ctx.names()
    # (every entry but the handle's own queries and its destructor takes the context first, then the handle)
    for name, args in ctx.calls:
        if not name.endswith("_create"):
            assert args[0] is ctx.handle and args[1].value == HANDLE, name


@pytest.mark.parametrize("prefix", PREFIXES)
def test_row_permutation_is_a_contiguous_int32_pointer_or_none(prefix):
    ctx = _Context()
    obj = _make(prefix, ctx)
    perm = np.arange(2 * N, dtype=np.int64)[::-2] // 2  # neither int32 nor contiguous: N-1 .. 0
    obj.set_row_permutation(perm)
    obj.set_row_permutation(None)
    assert ctx.names()[-2:] == [f"lsa_{prefix}_set_row_permutation"] * 2
    assert isinstance(ctx.calls[-2][1][2], ctypes.c_void_p) and np.array_equal(ctx.seen[0], np.arange(N)[::-1])
    assert ctx.calls[-1][1][2] is None and ctx.seen[1] is None


@pytest.mark.parametrize("prefix", PREFIXES)
def test_start_vector_check_and_dtype(prefix):
    ctx = _Context()
    obj = _make(prefix, ctx)
    text = f"start vector must have shape ({N},)"
    v = np.arange(1.0, N + 1.0)
    for bad in (np.ones(N + 1), np.ones((N, 1))):
        with pytest.raises(ValueError) as info:
            _solve(prefix, obj, v0=bad)
        assert str(info.value) == text
        if prefix != "stochastic":
            with pytest.raises(ValueError) as info:
                obj.set_start(bad)
            assert str(info.value) == text
    assert not any(name.endswith(("_solve", "_set_start")) for name in ctx.names())  # refused before the library is called
    _solve(prefix, obj, v0=v[::-1][::-1].astype(np.float32))
    if prefix != "stochastic":
        obj.set_start(list(v))
    for got in ctx.seen:
        assert got.dtype == DTYPES[prefix] and np.array_equal(got, v)
    ctx.seen.clear()
    _solve(prefix, obj)
    assert ctx.seen == [None]  # no start vector: a null pointer


@pytest.mark.parametrize("prefix", PREFIXES)
def test_options_struct(prefix):
    ctx = _Context()
    _solve(prefix, _make(prefix, ctx))
    o = _options(ctx)
    assert (o.nev, o.max_restarts, o.tol, o.seed, o.keep_fraction, o.transform) == (2, 7, 1e-9, 11, 0.5, 0)
    assert list(o.antishift) == [0.0, 0.0]
    if prefix == "lanczos":
        assert o.which == 3 and list(o.sigma) == [0.25, 0.0] and list(o.target) == [0.25, 0.0]  # (no target: the shift)
        ctx.calls.clear()
        _make(prefix, ctx).solve(2, 1e-9, 7, 3, 0.25, target=0.5)
        o = _options(ctx)
        assert list(o.sigma) == [0.25, 0.0] and list(o.target) == [0.5, 0.0] and o.seed == 0
    else:
        assert o.which == 0 and list(o.sigma) == [0.0, 0.0] and list(o.target) == [0.0, 0.0]


@pytest.mark.parametrize("prefix", PREFIXES)
def test_result_keys_counters_and_layout(prefix):
    ctx = _Context()
    obj = _make(prefix, ctx)
    out = _solve(prefix, obj)
    dt = DTYPES[prefix]
    if prefix == "lanczos":
        assert type(out).__name__ == "KrylovSchurResult"
        assert (out.nconv, out.restarts, out.op_applies) == (1, 3, 17)
        assert out.history == [{k: v for k, v in TAIL.items() if k not in ("restarts", "applies")}]
        assert out.theta.shape == out.lam.shape == out.residuals.shape == (2,) and out.theta.dtype == out.lam.dtype == np.float64
        blocks = [out.vectors]
        assert obj.solve(2, 1e-9, 7, 3, 0.25, vectors=False).vectors.shape == (N, 0)
    else:
        assert set(out) == KEYS[prefix] | set(TAIL) | set(COUNTERS[prefix])
        assert {k: out[k] for k in TAIL} == TAIL
        assert all(type(out[k]) is int for k in ("nconv", "restarts", "applies") + COUNTERS[prefix])
        assert [out[k] for k in COUNTERS[prefix]] == [1, 2, 3, 4]
        blocks = [out[k] for k in ("responses", "forcings", "initial", "modes") if k in out]
        for k in KEYS[prefix] - {"responses", "forcings", "initial", "modes", "energy"}:
            assert out[k].shape == (2,) and out[k].dtype == np.float64, k
    if prefix == "resolvent":
        assert out["adjoint_solves"] == 1 and out["forward_solves"] == 2
        assert len(blocks) == 2 and obj.solve(2, 1e-9, 7, forcings=False)["forcings"] is None
    if prefix == "growth":
        assert out["forward_solves"] == 1 and out["transposed_solves"] == 2
        assert out["energy"].shape == (2, 4)  # nsteps + 1 columns
    for X in blocks:
        assert X.shape == (N, 2) and X.dtype == dt and X.flags.f_contiguous
    # max_out is clipped to ncv; the library is told how many columns the arrays hold
    _solve(prefix, obj, max_out=99)
    assert [a for a in ctx.calls[-1 if prefix != "growth" else -2][1] if isinstance(a, int)][0] == NCV


def test_step_methods_only_where_the_library_has_them():
    for name in ("set_start", "extend", "basis"):
        assert not hasattr(lsa_hip.StochasticBasis, name)
        for cls in (lsa_hip.LanczosBasis, lsa_hip.ResolventBasis, lsa_hip.GrowthBasis):
            assert callable(getattr(cls, name))


@pytest.mark.parametrize("prefix", ["lanczos", "resolvent", "growth"])
def test_extend_and_basis(prefix):
    ctx = _Context()
    obj = _make(prefix, ctx)
    T = np.zeros((NCV + 1, NCV), order="F")
    assert obj.extend(1, 3, T) == -1
    name, args = ctx.calls[-1]
    assert name == f"lsa_{prefix}_extend" and args[2:4] == (1, 3) and args[4].value == T.ctypes.data and args[5] == NCV + 1
    with pytest.raises(AssertionError):
        obj.extend(0, 1, np.zeros((NCV + 1, NCV)))  # C order is refused
    V = obj.basis(3)
    assert V.shape == (N, 3) and V.dtype == DTYPES[prefix] and V.flags.f_contiguous
    assert ctx.calls[-1][0] == f"lsa_{prefix}_basis" and ctx.calls[-1][1][2] == 3


@pytest.mark.parametrize("prefix", ["lanczos", "resolvent", "growth"])
def test_basis_bytes_follow_the_scalar_and_the_permutation(prefix):
    obj = _make(prefix, _Context())
    size = np.dtype(DTYPES[prefix]).itemsize
    assert obj.basis_bytes == size * N * (NCV + 1) * 2
    obj.set_row_permutation(np.arange(N))
    assert obj.basis_bytes == size * N * (NCV + 1) * 3
    obj.set_row_permutation(None)
    assert obj.basis_bytes == size * N * (NCV + 1) * 2


@pytest.mark.parametrize("prefix", PREFIXES)
def test_destroyed_once_and_only_with_a_handle(prefix):
    ctx = _Context()
    obj = _make(prefix, ctx)
    del obj
    gc.collect()
    destroyed = [args for name, args in ctx.calls if name == f"lsa_{prefix}_destroy"]
    assert len(destroyed) == 1 and len(destroyed[0]) == 1 and destroyed[0][0].value == HANDLE
    # a context that is closed already: the handle went with it, nothing is called
    ctx = _Context()
    obj = _make(prefix, ctx)
    ctx.handle = None
    del obj
    gc.collect()
    assert not any(name.endswith("_destroy") for name in ctx.names())
    # a constructor that raised before the handle existed
    ctx = _Context()
    ctx.fail_create = True
    try:
        _make(prefix, ctx)
    except ValueError:
        pass
    else:
        pytest.fail("the refused create did not raise")
    gc.collect()
    assert ctx.names() == [f"lsa_{prefix}_create"]


def test_growth_scheme_refused_before_anything_is_called():
    ctx = _Context()
    try:
        _make("growth", ctx, scheme="rk4")
    except ValueError as exc:
        assert "scheme must be one of" in str(exc)
    else:
        pytest.fail("the unknown scheme did not raise")
    gc.collect()
    assert ctx.calls == []
