"""GPU suite: the tile shape of a level of the LU sweeps, chosen per direction (``nd_setup_levels`` in ``csrc/ndlu.hip``): upwards
a level with few tiles takes the 8-row tiles (64 lanes along a row pair) only where its pivot blocks are at least
``LSA_ND_SWEEP_WIDE`` wide, downwards it keeps them.  The shape changes a row's lane partition, so the solutions of two settings
differ at rounding level; within a setting the solo, batched and multi-column solves read the same shapes and agree bit for bit.
The knob is read once per process: every setting runs in a child (tests/sweep_shapes_child.py)."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = str(Path(__file__).resolve().parents[1])
CASES = ("S2k", "S5k", "C2k")
WIDE = 512  # kSweepWide
# the default; 8-row tiles wherever a level has few tiles, both ways (the rule before there was a width); never upwards
KNOBS = (None, "0", "100000")
_RUNS = {}


@pytest.fixture(scope="module")
def runs_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("sweep_shapes")


def _child(case, knob, tmp):
    key = (case, knob)
    if key not in _RUNS:
        env = {k: v for k, v in os.environ.items() if k != "LSA_ND_SWEEP_WIDE"}
        if knob is not None:
            env["LSA_ND_SWEEP_WIDE"] = knob
        out = tmp / f"{case}_{knob}.npz"
        p = subprocess.run([sys.executable, str(Path(ROOT) / "tests" / "sweep_shapes_child.py"), ROOT, case, str(out)], env=env, capture_output=True,
                           text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        r["arrays"] = dict(np.load(out))
        _RUNS[key] = r
    return _RUNS[key]


@pytest.mark.parametrize("knob", KNOBS, ids=lambda k: "default" if k is None else k)
@pytest.mark.parametrize("case", CASES)
def test_shapes_are_reported_and_every_path_reads_them(runs_dir, case, knob):
    """The reported shapes follow the rule; residuals against the scipy matrix at the bound of the top-inverse tests; a repeated
    solve, a batch of three shifts and a block of four columns hold the solo solves' bits."""
    run = _child(case, knob, runs_dir)
    wide = WIDE if knob is None else int(knob)
    for c in run["configs"]:
        shapes = [(lv["max_pivot"], lv["fwd_rows"], lv["bwd_rows"]) for lv in c["levels"]]
        print(f"{case} wide {wide} {c['order']} sigma {c['sigma']} vectors {c['vectors']}: (widest pivot block, rows up, rows down) per level {shapes}, "
              f"|b - C x|/|b| = {c['residual']:.2e}")
        for lv in c["levels"]:
            assert lv["bwd_rows"] in (8, 32) and lv["fwd_rows"] in (8, 32, 128)
            assert (lv["fwd_rows"] == 8) == (lv["bwd_rows"] == 8 and lv["max_pivot"] >= wide), lv
            if lv["fwd_rows"] == 128:
                assert lv["bwd_rows"] == 32
        assert c["repeat_same"] and c["multi_same"]
        assert c["residual"] <= 1e-12
    assert run["configs"][0]["batch_same"] and run["configs"][0]["batch_residual"] <= 1e-12


@pytest.mark.parametrize("case", CASES)
def test_the_settings_differ_in_shape_and_agree_in_the_solution(runs_dir, case):
    """Each case has a level whose upward shape the width decides (else the test would compare a setting with itself); the
    solutions agree to 1e-10 relative, the distance the top-inverse tests allow between two forms of one solve."""
    runs = [_child(case, k, runs_dir) for k in KNOBS]
    rows = [[[lv["fwd_rows"] for lv in c["levels"]] for c in r["configs"]] for r in runs]
    assert rows[1] != rows[2]
    assert [[lv["bwd_rows"] for lv in c["levels"]] for c in runs[1]["configs"]] == [[lv["bwd_rows"] for lv in c["levels"]] for c in runs[2]["configs"]]
    for name, a in runs[0]["arrays"].items():
        for r, knob in zip(runs[1:], KNOBS[1:]):
            d = np.linalg.norm(r["arrays"][name] - a) / np.linalg.norm(a)
            print(f"{case} {name}: |x(wide {knob}) - x(default)|/|x(default)| = {d:.2e}")
            assert d <= 1e-10
