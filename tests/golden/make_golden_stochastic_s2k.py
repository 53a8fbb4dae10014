"""Writes tests/golden/stochastic_s2k.json: the leading eigenvalues of the dense stochastic-forcing quadrature operators of S2k
(n = 1953, Re = 50) on the band [0, 1.5] with 8 Gauss-Legendre nodes, for both kinds, from numpy's dense eigenvalue solver
(tests/stochastic_reference.py: dense_operator).  About 20 s per kind; run from the repository root:

    python tests/golden/make_golden_stochastic_s2k.py
"""

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "lsa-fw_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import stochastic_reference as ref  # noqa: E402

KEEP = 8
NODES = 8


def main() -> None:
    A, M = ref.case("S2k")
    om, w = ref.gauss_band(*ref.BAND, NODES)
    out = {"case": "S2k", "n": int(A.shape[0]), "band": list(ref.BAND), "nodes": NODES, "omegas": om.tolist(), "weights": w.tolist()}
    for kind in ("eofs", "optimals"):
        ev = np.linalg.eigvals(ref.dense_operator(A, M, om, w, kind=kind))
        order = np.argsort(-ev.real)
        out[kind] = ev.real[order][:KEEP].tolist()
        out[kind + "_max_imag"] = float(np.abs(ev.imag[order][:KEEP]).max())
        out[kind + "_trace"] = float(ev.real.sum())
    (Path(__file__).resolve().parent / "stochastic_s2k.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
