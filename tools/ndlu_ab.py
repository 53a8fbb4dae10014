"""SHA-256 digests of the solutions of the nested-dissection LU over its sweep forms, as one JSON object (development aid):
run it on two builds and compare the files -- a refactoring of the sweeps must leave every digest as it was.

Per case (S2k, S5k cylinders; C2k cube) and per order of the matrix (natural: the library's own dissection, vectors addressed
through index lists; ordered: permuted by ``nd_order`` with the forest handed back, which is what takes the merged top), with
complex and with real factors: solve, solve in place, both adjoint solves, the batched solve of three shifts, real factors also
with real vectors.  The knobs that are read once per process run in children: the defaults, ``LSA_ND_TOPINV=0`` (S5k: the
launch per level instead of the merged top) and ``LSA_ND_SWEEP_FEW=0`` (S5k: at these sizes every level would otherwise take
the 8-row tiles; with it the 32-row and, on thin levels, 128-row tiles run).

usage: ndlu_ab.py [OUT.json]          (ndlu_ab.py --child CASE is the per-process part)"""
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
RUNS = (("S2k", {}), ("S5k", {}), ("C2k", {}), ("S5k", {"LSA_ND_TOPINV": "0"}), ("S5k", {"LSA_ND_SWEEP_FEW": "0"}))


def child(case):
    sys.path[:0] = [str(ROOT), str(ROOT / "lsa-fw_amd")]
    import numpy as np
    import scipy.sparse as sp

    import lsa_hip
    from synthetic import fem

    cube = case.startswith("C")
    es = fem.cube_case(case) if cube else fem.cylinder_case(case)
    ctx = lsa_hip.Context(0)
    rng = np.random.default_rng(23)
    bc = rng.standard_normal(es.n) + 1j * rng.standard_normal(es.n)
    out = {}

    def digest(a):
        return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

    def shifted(sig, perm):
        C = sp.csr_matrix((es.A.data - sig * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
        if sig.imag == 0.0:
            C = sp.csr_matrix(C.real)
        if perm is not None:
            C = C[perm][:, perm].tocsr()
        C.sort_indices()
        return C

    for factors, sigma, step in (("complex", (fem.SIGMA_CUBE + 0.5j) if cube else fem.SIGMA_RE50, 0.01j),
                                 ("real", complex(fem.SIGMA_CUBE if cube else 0.05), 0.01)):
        for order in ("natural", "ordered"):
            perm = tree = None
            if order == "ordered":  # as tests/topinv_child.py orders it: the zero-diagonal unknowns of the cube after their neighbours
                C0 = shifted(sigma, None)
                zd = C0.diagonal() == 0
                o = lsa_hip.nd_order(C0, 0, constraint=zd if (zd.any() and C0.nnz > 60 * es.n) else None)
                perm, tree = o["perm"], {"first": o["first"], "size": o["size"], "parent": o["parent"]}
            fs = [lsa_hip.NdLu(ctx, lsa_hip.CsrMatrix.from_scipy(ctx, shifted(sigma + j * step, perm)), 0, tree=tree) for j in range(3)]
            key = f"{case}/{order}/{factors}"
            info = fs[0].info()
            out[key + "/launches,levels"] = [info["apply_launches"], info["levels"]]
            for vectors, b in (("cvec", bc),) + ((("rvec", bc.real.copy()),) if factors == "real" else ()):
                def run(fn, rhs=b, inplace=False):
                    db = lsa_hip.DeviceVector.from_numpy(ctx, rhs)
                    dx = db if inplace else lsa_hip.DeviceVector(ctx, es.n, rhs.dtype)
                    fn(db, dx)
                    return digest(dx.numpy())

                k = f"{key}/{vectors}/"
                out[k + "solve"] = run(fs[0].solve)
                out[k + "solve_inplace"] = run(fs[0].solve, inplace=True)
                out[k + "adjoint_conj0"] = run(lambda db, dx: fs[0].solve_adjoint(db, dx, conj=False))
                out[k + "adjoint_conj1"] = run(lambda db, dx: fs[0].solve_adjoint(db, dx, conj=True))
                out[k + "adjoint_conj1_inplace"] = run(lambda db, dx: fs[0].solve_adjoint(db, dx, conj=True), inplace=True)
                dbs = [lsa_hip.DeviceVector.from_numpy(ctx, b * (1 + j)) for j in range(3)]
                dxs = [lsa_hip.DeviceVector(ctx, es.n, b.dtype) for _ in range(3)]
                lsa_hip.NdLu.solve_batch(fs, dbs, dxs)
                out[k + "batch3"] = [digest(dx.numpy()) for dx in dxs]
                lsa_hip.NdLu.solve_batch(fs, dbs, dbs)
                out[k + "batch3_inplace"] = [digest(dx.numpy()) for dx in dbs]
    print(json.dumps(out))


def main():
    merged = {}
    for case, env in RUNS:
        tag = ",".join(f"{k}={v}" for k, v in env.items()) or "defaults"
        r = subprocess.run([sys.executable, __file__, "--child", case], env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:  # (nothing more is started on the GPU after a failure)
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"ndlu_ab: {case} [{tag}] failed with status {r.returncode}")
        for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
            merged[f"[{tag}] {k}"] = v
    text = json.dumps(merged, indent=1, sort_keys=True)
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
