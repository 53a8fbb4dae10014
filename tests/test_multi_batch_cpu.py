"""CPU tests of the front ends of the block solve on a batch of factor sets and of the region solver's ``batch_nodes`` switch: the
argument errors raised before the library is touched, the configuration checks, and the memory rule."""

from types import SimpleNamespace

import pytest


def test_solve_multi_batch_argument_errors_need_no_context():
    """``J`` outside 1..16, list lengths that differ, ``trans`` other than ``"N"``: ``ValueError`` before anything of the library (or
    of the factorisations: they are ``None`` here) is touched."""
    import lsa_hip

    with pytest.raises(ValueError, match="between 1 and 16"):
        lsa_hip.NdLu.solve_multi_batch([], [], [], 4)
    with pytest.raises(ValueError, match="between 1 and 16"):
        lsa_hip.NdLu.solve_multi_batch([None] * 17, [None] * 17, [None] * 17, 4)
    with pytest.raises(ValueError, match="as many blocks"):
        lsa_hip.NdLu.solve_multi_batch([None] * 3, [None] * 2, [None] * 3, 4)
    with pytest.raises(ValueError, match="as many blocks"):
        lsa_hip.NdLu.solve_multi_batch([None] * 3, [None] * 3, [None] * 4, 4)
    for trans in ("T", "H", "n", 0):
        with pytest.raises(ValueError, match="transposed form .* is not built"):
            lsa_hip.NdLu.solve_multi_batch([None] * 3, [None] * 3, [None] * 3, 4, trans=trans)


def test_region_config_checks_batch_nodes():
    from Solver.region import RegionConfig, _check_config

    cfg = RegionConfig()
    assert cfg.batch_nodes is False and cfg.keep_factors is None and (cfg.nodes, cfg.subspace, cfg.atol, cfg.max_it) == (16, 48, 1e-10, 20)
    _check_config(cfg)
    _check_config(RegionConfig(batch_nodes=True))
    _check_config(RegionConfig(batch_nodes=True, keep_factors=True))
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="batch_nodes"):
            _check_config(RegionConfig(batch_nodes=bad))
    with pytest.raises(ValueError, match="keep_factors = False"):
        _check_config(RegionConfig(batch_nodes=True, keep_factors=False))


class _StubContext:
    """What ``_keep_factors`` asks of a context: the bytes of one prepared factor set and the free device memory."""

    def __init__(self, lu_bytes, free_bytes):
        self._lu, self._free = lu_bytes, free_bytes

    def prepared_lu_bytes(self):
        return self._lu

    def mem_info(self):
        return self._free, 2 * self._free


def test_memory_rule_counts_the_blocks_of_all_nodes():
    """``keep_factors=None``: kept when ``nodes`` factor sets and the blocks fit 0.8 of the free memory -- six blocks by default,
    ``6 + nodes`` under ``batch_nodes``.  Free memory between the two needs keeps the factors only with the switch off."""
    from Solver.region import RegionConfig, RegionEigenSolver

    n, nodes, cols, lu = 1000, 16, 48, 10_000_000
    block = 16 * n * cols
    need_off, need_on = nodes * lu + 6 * block, nodes * lu + (6 + nodes) * block
    keep = lambda cfg, free: RegionEigenSolver._keep_factors(SimpleNamespace(_cfg=cfg, _n=n), _StubContext(lu, free))  # noqa: E731
    off, on = RegionConfig(nodes=nodes, subspace=cols), RegionConfig(nodes=nodes, subspace=cols, batch_nodes=True)
    between = (need_off + need_on) / 2 / 0.8
    assert keep(off, between) is True and keep(on, between) is False
    assert keep(on, need_on / 0.8 + 1) is True and keep(on, need_on / 0.8 - 1e3) is False
    assert keep(off, need_off / 0.8 + 1) is True and keep(off, need_off / 0.8 - 1e3) is False
    assert keep(RegionConfig(nodes=nodes, subspace=cols, keep_factors=True, batch_nodes=True), 0) is True  # (an explicit choice is not sized)
