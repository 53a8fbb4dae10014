"""GPU suite: the root of the elimination forest and its children swept as one assembled inverse (``nd_top_kernel`` in
``csrc/ndlu_sweeps.hip``, ``nd_top_gemm_kernel`` in ``csrc/ndlu_factor.hip``) against the launch per level and direction it replaces (``LSA_ND_TOPINV=0``).
The knob is read once per process: every setting runs in a child (tests/topinv_child.py)."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

ROOT = str(Path(__file__).resolve().parents[1])
SIGMA = 0.018 + 0.7379601143282424j


def _child(case, sigma, vectors, out, knob):
    env = {k: v for k, v in os.environ.items() if k != "LSA_ND_TOPINV"}
    if knob is not None:
        env["LSA_ND_TOPINV"] = knob
    p = subprocess.run([sys.executable, str(Path(ROOT) / "tests" / "topinv_child.py"), ROOT, case, repr(complex(sigma).real), repr(complex(sigma).imag),
                        vectors, str(out)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    r.update(np.load(out))
    return r


def _matrix(case, sigma, perm):
    from synthetic import fem

    es = fem.cube_case(case) if case.startswith("C") else fem.cylinder_case(case)
    C = sp.csr_matrix((es.A.data - sigma * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
    if complex(sigma).imag == 0.0:
        C = sp.csr_matrix(C.real)
    return C[perm][:, perm].tocsc()


def _eligible(case, sigma, limit):
    import lsa_hip
    from synthetic import fem
    from test_topinv_cpu import top_plan

    es = fem.cube_case(case) if case.startswith("C") else fem.cylinder_case(case)
    C = sp.csr_matrix((es.A.data - sigma * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
    C.sort_indices()
    zd = C.diagonal() == 0  # (the 3D cases: constraint unknowns are eliminated after their neighbours, as in the child)
    flags = zd if (zd.any() and C.nnz > 60 * es.n) else None
    return top_plan(lsa_hip.NdAnalysis(C, 0, constraint=flags).export_tables(), limit) is not None


# S5k (four children under the root) and S30k (two; the benchmark's matrix) with complex factors; a real shift with real and
# with complex vectors
@pytest.mark.parametrize("case,sigma,vectors", [("S5k", SIGMA, "c"), ("S30k", SIGMA, "c"), ("S5k", 0.05, "r"), ("S5k", 0.05, "c")])
def test_merged_top_against_the_three_launches(tmp_path, case, sigma, vectors):
    from test_topinv_cpu import TOP_LIMIT

    off = _child(case, sigma, vectors, tmp_path / "off.npz", "0")
    on = _child(case, sigma, vectors, tmp_path / "on.npz", None)
    assert _eligible(case, sigma, TOP_LIMIT)
    assert on["launches"] == off["launches"] - 2
    assert on["bytes"] != off["bytes"]
    assert np.array_equal(on["b"], off["b"]) and np.array_equal(on["perm"], off["perm"])
    b = on["b"]
    for key, sig in (("x", complex(sigma)), ("x_second", complex(*on["sigma_second"]))):
        C = _matrix(case, sig, on["perm"])
        xref = spla.splu(C.astype(np.complex128)).solve(b.astype(np.complex128))
        for name, r in (("off", off), ("on", on)):
            x = r[key]
            res = np.linalg.norm(C @ x - b) / np.linalg.norm(b)
            err = np.linalg.norm(x - xref) / np.linalg.norm(xref)
            print(f"{case} {key} top {name}: |b - C x|/|b| = {res:.2e}, |x - x_SuperLU|/|x_SuperLU| = {err:.2e}")
            assert res <= 1e-12
            assert err <= 1e-10
        d = np.linalg.norm(on[key] - off[key]) / np.linalg.norm(off[key])
        print(f"{case} {key}: |x_on - x_off|/|x_off| = {d:.2e}")
        assert d <= 1e-10
    for r in (off, on):
        assert r["repeat_same"] and r["factor_twice_same"] and r["refactor_same_as_fresh"] and r["batch_same"]


def test_top_wider_than_one_staging_pass(tmp_path):
    """S120k: 1203 unknowns in the top, more than the 1024 vector entries a workgroup stages at a time.  The residual bound of a
    solve and the distance between the two forms (no SuperLU at this size: the residual is the check)."""
    from test_topinv_cpu import TOP_LIMIT

    off = _child("S120k", SIGMA, "c", tmp_path / "off.npz", "0")
    on = _child("S120k", SIGMA, "c", tmp_path / "on.npz", None)
    assert _eligible("S120k", SIGMA, TOP_LIMIT) and not _eligible("S120k", SIGMA, 1024)
    assert on["launches"] == off["launches"] - 2
    b = on["b"]
    for key, sig in (("x", SIGMA), ("x_second", complex(*on["sigma_second"]))):
        C = _matrix("S120k", sig, on["perm"])
        for name, r in (("off", off), ("on", on)):
            res = np.linalg.norm(C @ r[key] - b) / np.linalg.norm(b)
            print(f"S120k {key} top {name}: |b - C x|/|b| = {res:.2e}")
            assert res <= 1e-12
        d = np.linalg.norm(on[key] - off[key]) / np.linalg.norm(off[key])
        print(f"S120k {key}: |x_on - x_off|/|x_off| = {d:.2e}")
        assert d <= 1e-10
    for r in (off, on):
        assert r["repeat_same"] and r["factor_twice_same"] and r["refactor_same_as_fresh"] and r["batch_same"]


@pytest.mark.parametrize("case,sigma,knob", [("S5k", SIGMA, "700"), ("C20k", -5.0, None)])
def test_refused_forests_keep_their_launches(tmp_path, case, sigma, knob):
    """S5k under a limit below its 739 top unknowns; a 3D forest, whose root's children do not share a level."""
    off = _child(case, sigma, "c", tmp_path / "off.npz", "0")
    on = _child(case, sigma, "c", tmp_path / "on.npz", knob)
    assert not _eligible(case, sigma, int(knob) if knob else 1 << 30)
    assert on["launches"] == off["launches"] and on["bytes"] == off["bytes"]
    assert np.array_equal(on["x"], off["x"]) and np.array_equal(on["x_second"], off["x_second"])


_BENCH_CHILD = r"""
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/lsa-fw_amd"]
from synthetic import fem
from Solver.eigen import EigenSolver, EigensolverConfig
from Solver.utils import PreconditionerType, iSTType
es = fem.cylinder_case("S30k")
s = EigenSolver(es.A, es.M, EigensolverConfig(num_eig=20, atol=1e-10, ncv=80), check_hermitian=False)
s.solver.set_st_type(iSTType.SINVERT); s.solver.set_st_pc_type(PreconditionerType.LU); s.solver.set_target(fem.SIGMA_RE50)
pairs = s.solve()
st = s.solver.stats
print(json.dumps({"lam": [[p[0].real, p[0].imag] for p in pairs[:20]], "applies": st["op_applies"], "n": len(pairs),
                  "refined": st["refined_solves"], "backward": st["backward_accepted"]}))
"""


def test_bench_configuration_with_and_without_the_merged_top():
    """S30k, 20 pairs, ncv = 80, tol 1e-10: the same operator applies, the eigenvalues to 1e-11 relative, and no inner solve
    refined or accepted on its backward error -- a top that cost the solves their 1e-12 check would add a step to every apply."""
    runs = {}
    for knob in ("0", None):
        env = {k: v for k, v in os.environ.items() if k != "LSA_ND_TOPINV"}
        if knob is not None:
            env["LSA_ND_TOPINV"] = knob
        p = subprocess.run([sys.executable, "-c", _BENCH_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        runs[knob] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        print(knob, {k: v for k, v in runs[knob].items() if k != "lam"})
    a, b = runs["0"], runs[None]
    assert a["n"] >= 20 and b["n"] >= 20
    assert a["applies"] == b["applies"]
    assert a["refined"] == 0 and b["refined"] == 0 and a["backward"] == 0 and b["backward"] == 0
    lam0 = np.array([complex(re, im) for re, im in a["lam"]])
    lam1 = np.array([complex(re, im) for re, im in b["lam"]])
    assert np.max(np.abs(lam1 - lam0) / np.abs(lam0)) <= 1e-11
