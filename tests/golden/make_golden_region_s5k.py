"""Writes tests/golden/region_s5k.json: the region of the S5k case of tests/test_gpu_region.py and the dense eigenvalues around it.

    python tests/golden/make_golden_region_s5k.py [--spectrum spectrum.npy]

The dense spectrum (``scipy.linalg.eig`` of the S5k pencil, n = 4851: minutes on a CPU, which is why the test reads a fixture;
``--spectrum`` reuses a saved one) without non-finite values and the Dirichlet rows' ``lambda = 1``.  The region is a circle about
CENTRE = -0.08 + 0.45j (the S5k spectrum has nothing within 0.09 of the bench shift; a scan of centres on a 0.01 grid with 6 or more
eigenvalues inside gave this one the widest eigenvalue-free margin about its contour among those with more than ten inside) with
``subspace`` L = 40 columns (five 8-column product passes, ten 4-column solve passes): the radius is 0.45 x
the distance of the (L+1)-th nearest eigenvalue, so that it lies beyond 2 x the radius; then L - count >= 12 is required, and no
eigenvalue within 5 % of the radius of the contour.  The fixture keeps the eigenvalues within 3 radii: all the matching rule reads.
"""

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "lsa-fw_amd"), str(ROOT / "tests")]

L = 40
CENTRE = -0.08 + 0.45j


def main() -> None:
    import scipy.linalg as sla
    from synthetic import fem

    ap = argparse.ArgumentParser()
    ap.add_argument("--spectrum", type=Path)
    args = ap.parse_args()
    if args.spectrum is not None:
        lam = np.load(args.spectrum)
    else:
        es = fem.cylinder_case("S5k")
        lam = sla.eig(es.A.toarray(), es.M.toarray(), right=False)
        lam = lam[np.isfinite(lam)]
        lam = lam[np.abs(lam - 1.0) > 1e-8]
    centre = CENTRE
    d = np.sort(np.abs(lam - centre))
    radius = float(np.round(0.45 * d[L], 4))
    count = int(np.sum(d < radius))
    assert d[L] > 2.0 * radius and L - count >= 12 and count >= 1, (d[L], radius, count)
    assert np.min(np.abs(d - radius)) > 0.05 * radius, "an eigenvalue sits next to the contour"
    near = lam[np.abs(lam - centre) < 3.0 * radius]
    near = near[np.argsort(np.abs(near - centre))]
    out = {"case": "S5k", "n": 4851, "centre": [centre.real, centre.imag], "radius": radius, "nodes": 16, "subspace": L, "count": count,
           "distance_of_subspace_plus_first": float(d[L]), "dense_within_3_radii": [[float(z.real), float(z.imag)] for z in near]}
    path = Path(__file__).resolve().parent / "region_s5k.json"
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(f"radius {radius}, count {count}, (L+1)-th nearest at {d[L]:.6f}, {near.size} eigenvalues within 3 radii -> {path}")


if __name__ == "__main__":
    main()
