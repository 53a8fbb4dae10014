"""Child process of tests/test_gpu_sweep_shapes.py: ``LSA_ND_SWEEP_WIDE`` is read once per process, so every setting of it runs here.

usage: sweep_shapes_child.py ROOT CASE OUT.npz   -> one JSON line; every solution in OUT.npz

For each configuration of the case -- (shift, vectors c|r, order tree|idx) -- one factorisation and, on it: a solve and its
repetition, a block of four columns through ``solve_multi`` against the four solo solves, and (first configuration only) a batch of
three shifts against their solo solves.  ``tree``: the matrix in the elimination order with the forest handed back, as
``Solver/utils.py`` does it (vectors in elimination order, the assembled top where the forest has one); ``idx``: the library's own
dissection of the matrix as it comes (vectors addressed through the index lists).  The residuals are taken against the scipy
matrix here; the parent compares the solutions of different settings."""

import json
import sys

sys.path[:0] = [sys.argv[1], sys.argv[1] + "/lsa-fw_amd"]
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

import lsa_hip  # noqa: E402
from synthetic import fem  # noqa: E402

case, out = sys.argv[2], sys.argv[3]
SIGMA = 0.018 + 0.7379601143282424j
cube = case.startswith("C")
es = fem.cube_case(case) if cube else fem.cylinder_case(case)
# complex factors with complex vectors, real factors with complex and with real vectors (the 3D case at the real shift of the 3D tests)
shifts = [(-5.0, "c"), (-5.0, "r")] if cube else [(SIGMA, "c"), (0.05, "c"), (0.05, "r")]
configs = [(s, v, o) for o in ("tree", "idx") for s, v in shifts]
ctx = lsa_hip.Context(0)


def shifted(sig):
    C = sp.csr_matrix((es.A.data - sig * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
    if complex(sig).imag == 0.0:
        C = sp.csr_matrix(C.real)
    C.sort_indices()
    return C


def solve(f, rhs):
    dx = lsa_hip.DeviceVector(ctx, es.n, rhs.dtype)
    f.solve(lsa_hip.DeviceVector.from_numpy(ctx, np.ascontiguousarray(rhs)), dx)
    return dx.numpy()


def residual(C, x, b):
    return float(np.linalg.norm(C @ x - b) / np.linalg.norm(b))


arrays, report = {}, []
for i, (sigma, vectors, order) in enumerate(configs):
    C = shifted(sigma)
    tree = perm = None
    if order == "tree":
        zd = C.diagonal() == 0  # (3D: the zero-diagonal unknowns are eliminated after their neighbours, as Solver/utils.py asks)
        o = lsa_hip.nd_order(C, 0, constraint=zd if (zd.any() and C.nnz > 60 * es.n) else None)
        perm = o["perm"]
        tree = {"first": o["first"], "size": o["size"], "parent": o["parent"]}

    def factor(sig):
        M = shifted(sig)
        if perm is not None:
            M = M[perm][:, perm].tocsr()
            M.sort_indices()
        return M, lsa_hip.NdLu(ctx, lsa_hip.CsrMatrix.from_scipy(ctx, M), 0, tree=tree)

    Cp, f = factor(sigma)
    rng = np.random.default_rng(17 + i)
    B = rng.standard_normal((es.n, 4)) + (1j * rng.standard_normal((es.n, 4)) if vectors == "c" else 0.0)
    B = np.asfortranarray(B)
    cols = np.stack([solve(f, B[:, q]) for q in range(4)], axis=1)
    levels = f.sweep_levels()
    r = {"sigma": [complex(sigma).real, complex(sigma).imag], "vectors": vectors, "order": order, "levels": levels,
         "repeat_same": bool(np.array_equal(solve(f, B[:, 0]), cols[:, 0])),
         "residual": max(residual(Cp, cols[:, q], B[:, q]) for q in range(4))}
    dX = lsa_hip.DeviceVector(ctx, 4 * es.n, B.dtype)
    f.solve_multi(lsa_hip.DeviceVector.from_numpy(ctx, B.reshape(-1, order="F")), dX, 4)
    X4 = dX.numpy().reshape((es.n, 4), order="F")
    r["multi_same"] = bool(np.array_equal(X4, cols))
    arrays[f"{i}_cols"], arrays[f"{i}_multi"] = cols, X4
    if i == 0:
        step = 0.01 if complex(sigma).imag == 0.0 else 0.01j
        others = [factor(sigma + k * step) for k in (1, 2)]
        fs = [f] + [g for _, g in others]
        b = np.ascontiguousarray(B[:, 0])
        solo = [cols[:, 0]] + [solve(g, b) for g in fs[1:]]
        dbs = [lsa_hip.DeviceVector.from_numpy(ctx, b) for _ in fs]
        dxs = [lsa_hip.DeviceVector(ctx, es.n, b.dtype) for _ in fs]
        lsa_hip.NdLu.solve_batch(fs, dbs, dxs)
        batch = [dx.numpy() for dx in dxs]
        r["batch_same"] = all(bool(np.array_equal(a, s)) for a, s in zip(batch, solo))
        r["batch_residual"] = max(residual(M, x, b) for M, x in zip([Cp] + [M for M, _ in others], batch))
        arrays["batch"] = np.stack(batch, axis=1)
        del fs, others
    report.append(r)
    del f
np.savez(out, **arrays)
print(json.dumps({"case": case, "configs": report}))
