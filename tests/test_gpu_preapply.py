"""GPU suite: the next cycle's first inner solve queued under the host's Schur form, and the restart that does not wait for the
stream (``LSA_KRYLOV_PREAPPLY``, ``preapply_enqueue`` / ``krylov_restart_queued`` in ``csrc/solver.hip``), against the queueing
order it replaces (``LSA_KRYLOV_PREAPPLY=0``).  The same kernels run on the same inputs, so everything is compared bit for bit.
The switches are read once per process: every setting runs in a child (tests/preapply_child.py)."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = str(Path(__file__).resolve().parents[1])
KNOBS = ("LSA_KRYLOV_PREAPPLY", "LSA_KRYLOV_DELAYED", "LSA_KRYLOV_TAIL", "LSA_ND_TEST_PERTURB", "LSA_KS_DRIVER")


def _child(mode, case, out, preapply, extra=None):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env["LSA_KRYLOV_PREAPPLY"] = preapply
    env.update(extra or {})
    p = subprocess.run([sys.executable, str(Path(ROOT) / "tests" / "preapply_child.py"), ROOT, mode, case, str(out)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    return r, dict(np.load(out))


def _pair(tmp_path, mode, case, extra=None):
    off = _child(mode, case, tmp_path / "off.npz", "0", extra)
    on = _child(mode, case, tmp_path / "on.npz", "1", extra)
    print(mode, case, extra, "off", off[0], "on", on[0])
    assert on[0] == off[0]  # op_applies, spmv_calls, sptrsv_calls, krylov_restarts, refined_solves
    assert set(on[1]) == set(off[1])
    for name in on[1]:
        assert on[1][name].shape == off[1][name].shape and on[1][name].tobytes() == off[1][name].tobytes(), name
    return on


@pytest.mark.parametrize("case", ["S2k", "S5k"])
def test_same_bits_and_counters_over_several_restarts(tmp_path, case):
    counters, arrays = _pair(tmp_path, "base", case)
    assert counters["krylov_restarts"] >= 3 and len(arrays["lam"]) >= 6 and counters["refined_solves"] == 0


@pytest.mark.parametrize("mode,extra", [("mask", None),                                # projection mask: no tail form, nothing queued ahead
                                        ("base", {"LSA_KRYLOV_DELAYED": "0"}),         # CGS2 steps
                                        ("base", {"LSA_KRYLOV_TAIL": "0"}),            # DCGS2 without the tail form
                                        ("base", {"LSA_ND_TEST_PERTURB": "1e-7"}),     # the first check misses: refinement from then on
                                        ("two", None),                                 # set_adjoint between the phases
                                        ("maxit", None)])                              # the solve ends by max_restarts
def test_same_bits_where_the_apply_ahead_must_not_be_taken(tmp_path, mode, extra):
    counters, arrays = _pair(tmp_path, mode, "S2k", extra)
    if extra and "LSA_ND_TEST_PERTURB" in extra:
        assert counters["refined_solves"] > 0
    if mode == "maxit":
        assert counters["krylov_restarts"] == 1
    if mode == "two":
        assert len(arrays["mu"]) >= 6


def test_second_solve_on_a_solver_is_a_fresh_solver_s(tmp_path):
    """Two targets on one solver: nothing queued ahead in the first solve survives into the second."""
    counters, arrays = _pair(tmp_path, "reuse", "S2k")
    assert len(arrays["lam"]) >= 6 and counters["krylov_restarts"] >= 1
    assert arrays["lam"].tobytes() == arrays["lam_fresh"].tobytes() and arrays["X"].tobytes() == arrays["X_fresh"].tobytes()
