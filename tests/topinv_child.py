"""Child process of tests/test_gpu_topinv.py: ``LSA_ND_TOPINV`` is read once per process, so every setting of it runs here.

usage: topinv_child.py ROOT CASE SIGMA_RE SIGMA_IM VECTORS(c|r) OUT.npz   -> one JSON line; the solutions in OUT.npz

The matrix goes in the elimination order with the forest handed back, as ``Solver/utils.py`` does it (only then are the
vectors in elimination order, which the merged top needs)."""

import json
import sys

sys.path[:0] = [sys.argv[1], sys.argv[1] + "/lsa-fw_amd"]
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

import lsa_hip  # noqa: E402
from synthetic import fem  # noqa: E402

case, sigma, vectors, out = sys.argv[2], complex(float(sys.argv[3]), float(sys.argv[4])), sys.argv[5], sys.argv[6]
es = fem.cube_case(case) if case.startswith("C") else fem.cylinder_case(case)


def shifted(sig, perm=None):
    C = sp.csr_matrix((es.A.data - sig * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
    if sig.imag == 0.0:
        C = sp.csr_matrix(C.real)
    if perm is not None:
        C = C[perm][:, perm].tocsr()
    C.sort_indices()
    return C


C0 = shifted(sigma)
zd = C0.diagonal() == 0  # (3D cases: the zero-diagonal unknowns are eliminated after their neighbours, as Solver/utils.py asks)
o = lsa_hip.nd_order(C0, 0, constraint=zd if (zd.any() and C0.nnz > 60 * es.n) else None)
perm = o["perm"]
tree = {"first": o["first"], "size": o["size"], "parent": o["parent"]}
ctx = lsa_hip.Context(0)
rng = np.random.default_rng(17)
b = rng.standard_normal(es.n) + (1j * rng.standard_normal(es.n) if vectors == "c" else 0.0)
step = 0.01 if sigma.imag == 0.0 else 0.01j
sigmas = [sigma, sigma + step, sigma + 2 * step]
mats = [lsa_hip.CsrMatrix.from_scipy(ctx, shifted(s, perm)) for s in sigmas]


def solve(f, rhs):
    dx = lsa_hip.DeviceVector(ctx, es.n, rhs.dtype)
    f.solve(lsa_hip.DeviceVector.from_numpy(ctx, rhs), dx)
    return dx.numpy()


fs = [lsa_hip.NdLu(ctx, m, 0, tree=tree) for m in mats]
info = fs[0].info()
x = solve(fs[0], b)
repeat_same = bool(np.array_equal(solve(fs[0], b), x))
solo = [solve(f, b) for f in fs]
dbs = [lsa_hip.DeviceVector.from_numpy(ctx, b) for _ in fs]
dxs = [lsa_hip.DeviceVector(ctx, es.n, b.dtype) for _ in fs]
lsa_hip.NdLu.solve_batch(fs, dbs, dxs)
batch_same = all(bool(np.array_equal(dx.numpy(), ref)) for dx, ref in zip(dxs, solo))
# the first factorisation again at the second shift, then back at the first: a second factorisation of the same matrix
fs[0].refactor(mats[1])
x_second = solve(fs[0], b)
refactor_same_as_fresh = bool(np.array_equal(x_second, solo[1]))
fs[0].refactor(mats[0])
factor_twice_same = bool(np.array_equal(solve(fs[0], b), x))
np.savez(out, x=x, x_second=x_second, b=b, perm=perm)
print(json.dumps({"launches": info["apply_launches"], "bytes": info["apply_bytes"], "levels": info["levels"], "repeat_same": repeat_same,
                  "batch_same": batch_same, "refactor_same_as_fresh": refactor_same_as_fresh, "factor_twice_same": factor_twice_same,
                  "sigma_second": [sigmas[1].real, sigmas[1].imag]}))
