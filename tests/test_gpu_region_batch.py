"""GPU tests of the region eigensolver with its nodes solved in lockstep (``lsa_contour_set_batch_nodes``,
``RegionConfig(batch_nodes=True)``) on S2k: every result is, byte for byte, that of the node-by-node default, the verdict
counters included."""

from dataclasses import replace

import pytest

pytestmark = pytest.mark.gpu

KSP_RTOL_TIGHT = 1e-16  # test 7: see test_fall_back_to_the_node_by_node_path

_RESULTS = {}


def _region(name):
    from Solver.region import Ellipse, RegionConfig
    import region_reference as rr

    (centre, rx, ry, nodes, cols), _, _ = rr.REGIONS[name]
    return Ellipse(centre, rx, ry), RegionConfig(nodes=nodes, subspace=cols, atol=rr.ATOL, max_it=rr.MAX_IT)


def _solve(name, batch, ksp_rtol=None, **cfg_changes):
    """One fresh solver per (region, switch, ...), kept for the module; the start block is the CPU test's."""
    from Solver.region import RegionEigenSolver
    import region_reference as rr

    key = (name, batch, ksp_rtol, tuple(sorted(cfg_changes.items())))
    if key not in _RESULTS:
        ell, cfg = _region(name)
        cfg = replace(cfg, keep_factors=True, batch_nodes=batch, **cfg_changes)
        A, M = rr.s2k()
        rs = RegionEigenSolver(A, M, cfg, ksp_rtol=ksp_rtol)
        try:
            _RESULTS[key] = (rs.solve(ell, Y0=rr.start_block(A.shape[0], cfg.subspace)), cfg)
        finally:
            rs.release()
    return _RESULTS[key]


def _assert_same(on, off):
    for f in ("eigenvalues", "eigenvectors", "residuals"):
        assert getattr(on, f).tobytes() == getattr(off, f).tobytes(), f
    assert (on.count, on.complete, on.iterations, on.estimate) == (off.count, off.complete, off.iterations, off.estimate)
    for k in ("block_solves", "refined_solves", "backward_accepted", "max_rel_res"):
        assert on.stats[k] == off.stats[k], (k, on.stats[k], off.stats[k])


@pytest.mark.parametrize("name", ["R1", "R2", "R0"])
def test_batched_nodes_give_the_default_bytes(name):
    """R1 (8 nodes, 12 columns), R2 (16 nodes, 48 columns) and the empty R0 with its confirming second iteration."""
    (on, _), (off, _) = _solve(name, True), _solve(name, False)
    print(name, "on:", {k: on.stats[k] for k in ("batch_nodes", "batched_groups", "batched_columns", "block_solves", "seconds_solve")},
          "off seconds_solve:", off.stats["seconds_solve"])
    _assert_same(on, off)
    assert on.stats["batch_nodes"] is True and off.stats["batch_nodes"] is False
    assert on.stats["batched_columns"] > 0 and off.stats["batched_columns"] == 0 and off.stats["batched_groups"] == 0
    if name == "R0":
        assert on.iterations == 2 and on.count == 0


def test_two_groups_and_a_single_column_remainder():
    """R1's ellipse with 20 nodes and 13 columns: two runs of factor sets (16 + 4) and column passes 4 + 4 + 4 + 1, three of them
    through the block kernel and the last column through the batched solo sweep.  The bytes are those of the default; one iteration
    (``max_it = 1``, where the block has all 13 columns) launches 2 x 3 batched groups."""
    (on, cfg), (off, _) = _solve("R1", True, nodes=20, subspace=13), _solve("R1", False, nodes=20, subspace=13)
    _assert_same(on, off)
    print("iterations", on.iterations, "rank", on.stats["rank"], "groups", on.stats["batched_groups"], "columns", on.stats["batched_columns"])
    assert 0 < on.stats["batched_columns"] <= on.stats["block_solves"]  # (nodes that took the refinement step leave the runs)
    (one, _), (one_off, _) = _solve("R1", True, nodes=20, subspace=13, max_it=1), _solve("R1", False, nodes=20, subspace=13, max_it=1)
    _assert_same(one, one_off)
    assert one.iterations == 1 and one.stats["batched_columns"] == 20 * 13
    assert one.stats["batched_groups"] == 2 * 3


def test_fall_back_to_the_node_by_node_path():
    """R1 with ``ksp_rtol = 1e-16``, which no double-precision solve reaches: the DEFAULT path (switch off) takes its refinement step
    (``refined_solves > 0``), accepts on the backward error and still completes -- the value was chosen on the default path alone (the
    first one tried).  With the switch on the bytes and the four counters are the same; every node is flagged in the first iteration,
    so only that iteration's columns were batched (and solved again node by node)."""
    (off, cfg) = _solve("R1", False, ksp_rtol=KSP_RTOL_TIGHT)
    print("default path at ksp_rtol", KSP_RTOL_TIGHT, {k: off.stats[k] for k in ("refined_solves", "backward_accepted", "block_solves", "max_rel_res")},
          "complete", off.complete, "iterations", off.iterations)
    assert off.stats["refined_solves"] > 0 and off.complete
    (on, _) = _solve("R1", True, ksp_rtol=KSP_RTOL_TIGHT)
    _assert_same(on, off)
    assert on.iterations > 1
    assert on.stats["batched_columns"] == cfg.nodes * cfg.subspace  # the first iteration's; then every node carries the flag


def test_switch_needs_kept_factors(hip_ctx):
    import lsa_hip
    import region_reference as rr

    A, M = rr.s2k()
    dA, dM = lsa_hip.CsrMatrix.from_scipy(hip_ctx, A), lsa_hip.CsrMatrix.from_scipy(hip_ctx, M)
    (centre, rx, ry, nodes, cols), _, _ = rr.REGIONS["R1"]
    cs = lsa_hip.ContourSolver(hip_ctx, dA, dM, nodes, centre, rx, ry, cols, keep_factors=False)
    with pytest.raises(ValueError, match="keep_factors = 0"):  # (LSA_ERR_ARG is the binding's ValueError)
        cs.set_batch_nodes(True)
    assert cs.batch_info() == {"enabled": False, "groups": 0, "batched_columns": 0, "serial_columns": 0}
    with pytest.raises(ValueError, match="keep_factors = 0"):
        lsa_hip.ContourSolver(hip_ctx, dA, dM, nodes, centre, rx, ry, cols, keep_factors=False, batch_nodes=True)
