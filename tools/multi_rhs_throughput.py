"""Block solves on one factorisation of the exact LU: milliseconds per column of ``NdLu.solve_multi`` against the solo solve.

    python tools/multi_rhs_throughput.py [--cases S30k S500k C160k] [--nrhs 1 2 4 8 16 32] [--parent-solo-us US ...]
                                         [--trans {N,T,H}] [--rounds R] [--out profiles/multi_rhs.json]

Per case (2D cylinder cases at the complex shift of the bench, 3D cube cases at their real shift; the matrix in the
elimination order with the forest handed back, as ``Solver/utils.py`` prepares it): the time of one ``lsa_ndlu_solve``
(``time_solve``, 100 back-to-back solves between HIP events), then for every ``nrhs`` the time of one block solve
(``time_solve_multi``) divided by ``nrhs``, with what ``multi_info`` reports and the bytes one sweep reads.  With
``LSA_ND_MULTI_WIDTH=W`` in the environment (read once per process) the library takes passes of at most ``W`` columns: the
recorded ``width_cap``.  Every block solve is checked bit for bit against solo solves of its columns.  ``--parent-solo-us``
(one figure per case) records beside the solo time what ``tools/bench_ndlu.py --case CASE`` of the PARENT commit, built
apart, printed as "solve ... us per apply" on the same box: ``parent_commit_solo_ms`` and the ratio ``solo_vs_parent`` (the
solo path is meant to be that code unchanged; DESIGN section 4b states a box-to-box spread of 4 %).  Appends to ``--out`` when
the file exists (one case per call keeps a call short).

``--trans T`` / ``H`` measures the transposed / adjoint block solve instead (``--out`` then defaults to
``profiles/multi_rhs_adjoint.json``): the solo figure is ``time_solve_multi(..., nrhs=1)`` in that direction (one
``lsa_ndlu_solve_adjoint`` per repetition), every ``nrhs`` runs with ``NdLu.set_multi_transposed(True)``, and the blocks are
checked bit for bit against solo adjoint solves.  The solo figure and every ``nrhs`` are timed ``--rounds`` times in turn and the
medians are recorded (all rounds are kept in the file).  ``--parent-solo-us`` is then the parent commit's
``time_solve_multi(..., nrhs=1, trans=...)`` of the same process order on the same box.

``--sets J`` measures the block solve on a batch of factor sets instead (``--out`` then defaults to ``profiles/multi_batch.json``):
J factorisations of the case at J shifts on one ordering, one block of ``--nrhs`` columns (the first figure given; default 4) per
set.  ``NdLu.time_solve_multi_batch`` on all sets against ``NdLu.time_solve_multi`` looped over the sets, in the same process,
alternating for ``--rounds`` rounds after a warm-up; the medians are recorded as milliseconds per column per set.  Every block is
checked bit for bit against ``solve_multi`` on its set alone.  With ``--trans T`` / ``H`` the transposed form is measured
(``NdLu.time_solve_multi_batch_adjoint`` against ``time_solve_multi(trans=...)`` with the transposed switch on, looped over the sets;
``--out`` then defaults to ``profiles/multi_batch_adjoint.json``).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "lsa-fw_amd")]


def measure_transposed(case: str, counts: list[int], iters: int, trans: str, rounds: int, parent_solo_us: float | None = None) -> dict:
    """The transposed (``trans="T"``) or adjoint (``"H"``) block solve in wide passes against the solo solve of that direction."""
    import statistics

    import numpy as np
    import scipy.sparse as sp

    import lsa_hip
    from synthetic import fem

    cube = case.startswith("C")
    es = fem.cube_case(case) if cube else fem.cylinder_case(case)
    sigma = fem.SIGMA_CUBE if cube else fem.SIGMA_RE50
    C = sp.csr_matrix((es.A.data - sigma * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
    zd = C.diagonal() == 0
    o = lsa_hip.nd_order(C, 0, constraint=zd if (zd.any() and C.nnz > 60 * es.n) else None)
    C = C[o["perm"]][:, o["perm"]].tocsr()
    C.sort_indices()
    opC = (C.conj().T if trans == "H" else C.T).tocsr()
    ctx = lsa_hip.Context(0)
    dC = lsa_hip.CsrMatrix.from_scipy(ctx, C)
    f = lsa_hip.NdLu(ctx, dC, 0, tree={"first": o["first"], "size": o["size"], "parent": o["parent"]})
    info = f.info()
    n, kmax = es.n, max(counts)
    vdt = np.complex128 if np.iscomplexobj(C.data) else np.float64
    rng = np.random.default_rng(0)
    B = rng.standard_normal((n, kmax)) + (1j * rng.standard_normal((n, kmax)) if vdt is np.complex128 else 0.0)
    B = np.asfortranarray(B.astype(vdt))
    db, dx = lsa_hip.DeviceVector.from_numpy(ctx, np.ascontiguousarray(B[:, 0])), lsa_hip.DeviceVector(ctx, n, vdt)
    ref = np.empty((n, min(kmax, 8)), dtype=vdt)  # solo adjoint answers of the first columns: the bit-for-bit check
    for q in range(ref.shape[1]):
        f.solve_adjoint(lsa_hip.DeviceVector.from_numpy(ctx, np.ascontiguousarray(B[:, q])), dx, conj=trans == "H")
        ref[:, q] = dx.numpy()
    f.set_multi_transposed(True)
    blocks = {k: (lsa_hip.DeviceVector.from_numpy(ctx, B[:, :k].reshape(-1, order="F")), lsa_hip.DeviceVector(ctx, n * k, vdt)) for k in counts}
    f.time_solve_multi(db, dx, 1, iters=10, trans=trans)
    for k, (dB, dX) in blocks.items():
        f.time_solve_multi(dB, dX, k, iters=3, trans=trans)
    solo_rounds, multi_rounds = [], {k: [] for k in counts}
    for _ in range(rounds):  # the solo figure and every width in turn, round after round: drift hits all of them alike
        solo_rounds.append(f.time_solve_multi(db, dx, 1, iters=iters, trans=trans))
        for k, (dB, dX) in blocks.items():
            multi_rounds[k].append(f.time_solve_multi(dB, dX, k, iters=max(3, iters // k), trans=trans))
    solo_ms = statistics.median(solo_rounds)
    out = {"case": case, "n": int(n), "trans": trans, "sigma": [complex(sigma).real, complex(sigma).imag], "factor_dtype": np.dtype(vdt).name,
           "factor_bytes_per_sweep": int(info["apply_bytes"]), "rounds": rounds, "solo_ms": solo_ms, "solo_ms_rounds": solo_rounds,
           "width_cap": int(os.environ.get("LSA_ND_MULTI_WIDTH", lsa_hip.NDLU_MULTI_MAX)), "multi": []}
    for k, (dB, dX) in blocks.items():
        ms = statistics.median(multi_rounds[k])
        X = dX.numpy().reshape((n, k), order="F")
        same = bool(np.array_equal(X[:, :ref.shape[1]], ref[:, :k]))
        res = float(np.linalg.norm(B[:, :k] - opC @ X) / np.linalg.norm(B[:, :k]))
        f.time_solve_multi(dB, dX, k, iters=1, trans=trans)  # (what multi_info reports is the last block solve's)
        mi = f.multi_info()
        if k == 1:
            mi["width"] = 1  # (a single column is the solo solve: multi_info still holds the block solve before it)
        out["multi"].append({"nrhs": k, "ms_per_block": ms, "ms_per_column": ms / k, "solo_over_multi_per_column": solo_ms / (ms / k),
                             "ms_per_block_rounds": multi_rounds[k], "bit_identical_to_solo": same, "residual": res, **mi})
        print(f"{case} trans={trans} nrhs={k:2d}: {ms / k * 1e3:9.1f} us per column ({solo_ms / (ms / k):.2f}x the solo {solo_ms * 1e3:.1f} us), "
              f"width {mi['width']}, bits {'same' if same else 'DIFFER'}, residual {res:.1e}", flush=True)
    if parent_solo_us is not None:
        out["parent_commit_solo_ms"] = parent_solo_us / 1e3
        out["solo_vs_parent"] = solo_ms / (parent_solo_us / 1e3)
        print(f"{case} trans={trans}: solo {solo_ms * 1e3:.1f} us, parent commit {parent_solo_us:.1f} us ({out['solo_vs_parent']:.3f})", flush=True)
    return out


def measure_sets(case: str, J: int, nrhs: int, iters: int, rounds: int, trans: str = "N") -> dict:
    """``solve_multi_batch`` (``trans`` T / H: ``solve_multi_batch_adjoint``) on J factor sets against ``solve_multi`` in that direction
    looped over them: ms per column per set."""
    import statistics

    import numpy as np
    import scipy.sparse as sp

    import lsa_hip
    from synthetic import fem

    es = fem.cylinder_case(case)
    shifts = [fem.SIGMA_RE50 + 0.01 * j * (1 + 1j) for j in range(J)]
    C0 = sp.csr_matrix((es.A.data - shifts[0] * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
    zd = C0.diagonal() == 0
    o = lsa_hip.nd_order(C0, 0, constraint=zd if (zd.any() and C0.nnz > 60 * es.n) else None)
    A = sp.csr_matrix(es.A)[o["perm"]][:, o["perm"]].tocsr()
    M = sp.csr_matrix((es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)[o["perm"]][:, o["perm"]].tocsr()
    for m in (A, M):
        m.sort_indices()
    ctx = lsa_hip.Context(0)
    n = es.n
    fs, keep = [], []
    for z in shifts:
        C = sp.csr_matrix((A.data - z * M.data, A.indices, A.indptr), shape=A.shape)
        dC = lsa_hip.CsrMatrix.from_scipy(ctx, C)
        fs.append(lsa_hip.NdLu(ctx, dC, 0, tree={"first": o["first"], "size": o["size"], "parent": o["parent"]}))
        keep.append(dC)
    rng = np.random.default_rng(0)
    B = np.asfortranarray(rng.standard_normal((n, nrhs)) + 1j * rng.standard_normal((n, nrhs)))
    dB = lsa_hip.DeviceVector.from_numpy(ctx, B.reshape(-1, order="F"))
    dXs = [lsa_hip.DeviceVector(ctx, n * nrhs, np.complex128) for _ in range(J)]
    dY = lsa_hip.DeviceVector(ctx, n * nrhs, np.complex128)
    loop_iters = max(3, iters // J)
    if trans == "N":
        lsa_hip.NdLu.solve_multi_batch(fs, [dB] * J, dXs, nrhs)
        batched = lambda: lsa_hip.NdLu.time_solve_multi_batch(fs, [dB] * J, dXs, nrhs, iters=loop_iters)  # noqa: E731
    else:
        for f in fs:
            f.set_multi_transposed(True)  # (the looped side's wide passes; the batch entry does not read the switch)
        lsa_hip.NdLu.solve_multi_batch_adjoint(fs, [dB] * J, dXs, nrhs, conj=trans == "H")
        batched = lambda: lsa_hip.NdLu.time_solve_multi_batch_adjoint(fs, [dB] * J, dXs, nrhs, iters=loop_iters, conj=trans == "H")  # noqa: E731
    same = True
    for f, dX in zip(fs, dXs):
        f.solve_multi(dB, dY, nrhs, trans=trans)
        same = same and bool(np.array_equal(dX.numpy(), dY.numpy()))
    looped = lambda: sum(f.time_solve_multi(dB, dY, nrhs, iters=loop_iters, trans=trans) for f in fs)  # noqa: E731
    looped(), batched()  # warm-up
    loop_rounds, batch_rounds = [], []
    for _ in range(rounds):
        loop_rounds.append(looped())
        batch_rounds.append(batched())
    lm, bm = statistics.median(loop_rounds), statistics.median(batch_rounds)
    per = 1.0 / (J * nrhs)
    out = {"case": case, "n": int(n), "sets": J, "nrhs": nrhs, "trans": trans, "rounds": rounds, "iters": loop_iters, "apply_launches": int(fs[0].info()["apply_launches"]),
           "looped_ms_per_column_per_set": lm * per, "batched_ms_per_column_per_set": bm * per, "looped_over_batched": lm / bm,
           "looped_ms_rounds": loop_rounds, "batched_ms_rounds": batch_rounds, "bit_identical_to_solve_multi": same, "width": fs[0].multi_info()["width"]}
    print(f"{case} sets={J} nrhs={nrhs} trans={trans}: looped solve_multi {lm * per * 1e3:.1f} us, batched {bm * per * 1e3:.1f} us per column per set "
          f"({lm / bm:.2f}x), bits {'same' if same else 'DIFFER'}", flush=True)
    return out


def measure(case: str, counts: list[int], iters: int, parent_solo_us: float | None = None) -> dict:
    import numpy as np
    import scipy.sparse as sp

    import lsa_hip
    from synthetic import fem

    cube = case.startswith("C")
    es = fem.cube_case(case) if cube else fem.cylinder_case(case)
    sigma = fem.SIGMA_CUBE if cube else fem.SIGMA_RE50
    C = sp.csr_matrix((es.A.data - sigma * es.M.data, es.A.indices, es.A.indptr), shape=es.A.shape)
    zd = C.diagonal() == 0
    o = lsa_hip.nd_order(C, 0, constraint=zd if (zd.any() and C.nnz > 60 * es.n) else None)
    C = C[o["perm"]][:, o["perm"]].tocsr()
    C.sort_indices()
    ctx = lsa_hip.Context(0)
    dC = lsa_hip.CsrMatrix.from_scipy(ctx, C)
    t0 = time.time()
    f = lsa_hip.NdLu(ctx, dC, 0, tree={"first": o["first"], "size": o["size"], "parent": o["parent"]})
    info = f.info()
    n, kmax = es.n, max(counts)
    vdt = np.complex128 if np.iscomplexobj(C.data) else np.float64
    rng = np.random.default_rng(0)
    B = rng.standard_normal((n, kmax)) + (1j * rng.standard_normal((n, kmax)) if vdt is np.complex128 else 0.0)
    B = np.asfortranarray(B.astype(vdt))
    db, dx = lsa_hip.DeviceVector.from_numpy(ctx, np.ascontiguousarray(B[:, 0])), lsa_hip.DeviceVector(ctx, n, vdt)
    f.time_solve(db, dx, 10)
    solo_ms = f.time_solve(db, dx, iters)
    out = {"case": case, "n": int(n), "sigma": [complex(sigma).real, complex(sigma).imag], "factor_dtype": np.dtype(vdt).name,
           "create_seconds": round(time.time() - t0, 3), "factor_bytes_per_sweep": int(info["apply_bytes"]), "apply_launches": int(info["apply_launches"]),
           "solo_ms": solo_ms, "solo_GBps": info["apply_bytes"] / solo_ms / 1e6, "width_cap": int(os.environ.get("LSA_ND_MULTI_WIDTH", lsa_hip.NDLU_MULTI_MAX)),
           "multi": []}
    ref = np.empty((n, min(kmax, 8)), dtype=vdt)  # solo answers of the first columns: the bit-for-bit check
    for q in range(ref.shape[1]):
        f.solve(lsa_hip.DeviceVector.from_numpy(ctx, np.ascontiguousarray(B[:, q])), dx)
        ref[:, q] = dx.numpy()
    for k in counts:
        dB = lsa_hip.DeviceVector.from_numpy(ctx, B[:, :k].reshape(-1, order="F"))
        dX = lsa_hip.DeviceVector(ctx, n * k, vdt)
        f.time_solve_multi(dB, dX, k, iters=3)
        ms = f.time_solve_multi(dB, dX, k, iters=max(3, iters // k))
        X = dX.numpy().reshape((n, k), order="F")
        same = bool(np.array_equal(X[:, :ref.shape[1]], ref[:, :k]))
        res = float(np.linalg.norm(B[:, :k] - C @ X) / np.linalg.norm(B[:, :k]))
        mi = f.multi_info()
        out["multi"].append({"nrhs": k, "ms_per_block": ms, "ms_per_column": ms / k, "solo_over_multi_per_column": solo_ms / (ms / k),
                             "bit_identical_to_solo": same, "residual": res, **mi})
        print(f"{case} nrhs={k:2d}: {ms / k * 1e3:9.1f} us per column ({solo_ms / (ms / k):.2f}x the solo {solo_ms * 1e3:.1f} us), width {mi['width']}, "
              f"extra {mi['extra_bytes'] / 1e6:.1f} MB, bits {'same' if same else 'DIFFER'}, residual {res:.1e}", flush=True)
        del dB, dX
    solo_after = f.time_solve(db, dx, iters)
    out["solo_ms_after"] = solo_after
    if parent_solo_us is not None:
        out["parent_commit_solo_ms"] = parent_solo_us / 1e3
        out["solo_vs_parent"] = solo_ms / (parent_solo_us / 1e3)
        print(f"{case}: solo {solo_ms * 1e3:.1f} us, after the block solves {solo_after * 1e3:.1f} us, parent commit {parent_solo_us:.1f} us "
              f"({out['solo_vs_parent']:.3f})", flush=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["S30k", "S500k", "C160k"])
    ap.add_argument("--nrhs", nargs="+", type=int, default=[1, 2, 4, 8, 16, 32])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--parent-solo-us", nargs="+", type=float, default=None, help="per case: the parent commit's bench_ndlu.py figure on this box")
    ap.add_argument("--trans", choices=["N", "T", "H"], default="N", help="N: C^-1 (the default); T / H: the transposed / adjoint block solve in wide passes")
    ap.add_argument("--rounds", type=int, default=3, help="--trans T / H: rounds of (solo, every nrhs) whose medians are recorded")
    ap.add_argument("--sets", type=int, default=0, help="J > 0: the block solve on J factor sets (solve_multi_batch) against solve_multi looped over them")
    ap.add_argument("--out", default=None, help="default: profiles/multi_rhs.json, or profiles/multi_rhs_adjoint.json with --trans T / H, or profiles/multi_batch.json (multi_batch_adjoint.json) with --sets")
    args = ap.parse_args()
    name = ("multi_batch.json" if args.trans == "N" else "multi_batch_adjoint.json") if args.sets else "multi_rhs.json" if args.trans == "N" else "multi_rhs_adjoint.json"
    path = Path(args.out) if args.out else ROOT / "profiles" / name
    doc = json.loads(path.read_text()) if path.exists() else {"tool": "tools/multi_rhs_throughput.py", "runs": []}
    if args.parent_solo_us is not None and len(args.parent_solo_us) != len(args.cases):
        ap.error("--parent-solo-us needs one figure per case")
    for i, case in enumerate(args.cases):
        parent = None if args.parent_solo_us is None else args.parent_solo_us[i]
        if args.sets:
            doc["runs"].append(measure_sets(case, args.sets, 4 if len(args.nrhs) > 1 else args.nrhs[0], args.iters, args.rounds, args.trans))
        elif args.trans == "N":
            doc["runs"].append(measure(case, args.nrhs, args.iters, parent))
        else:
            doc["runs"].append(measure_transposed(case, args.nrhs, args.iters, args.trans, args.rounds, parent))
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
