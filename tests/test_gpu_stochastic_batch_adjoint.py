"""GPU suite: the stochastic-forcing step with its adjoint solves through the batched transposed sweeps and their check products
through the batched transposed SpMV (``batch_adjoint=True``, ``lsa_stochastic_set_batch_adjoint``), on S2k: the results of the default,
byte for byte."""

import json
from pathlib import Path

import numpy as np
import pytest

import helpers  # noqa: F401
import stochastic_reference as ref

pytestmark = pytest.mark.gpu
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "stochastic_s2k.json").read_text())

_SOLVED = {}


def solved(kind="eofs", nodes=8, ncv=12, num_modes=2, atol=1e-8, batch_forward=False, batch_adjoint=False, refine=False):
    """One front-end solve per configuration and process: S2k, band [0, 1.5]."""
    key = (kind, nodes, ncv, num_modes, atol, batch_forward, batch_adjoint, refine)
    if key not in _SOLVED:
        from Solver.stochastic import StochasticConfig, StochasticForcingSolver

        A, M = ref.case("S2k")
        sf = StochasticForcingSolver(A, M, StochasticConfig(num_modes=num_modes, ncv=ncv, atol=atol, nodes=nodes), batch_forward=batch_forward,
                                     batch_adjoint=batch_adjoint)
        sf._force_refinement = refine
        _SOLVED[key] = sf.solve(band=ref.BAND, kind=kind)
        sf.release()
    return _SOLVED[key]


@pytest.mark.parametrize("nodes,kind,batch_forward", [(3, "eofs", False), (16, "eofs", True), (17, "eofs", True), (3, "optimals", True)])
def test_batched_adjoint_solves_give_the_same_bits(nodes, kind, batch_forward):
    """``batch_adjoint=True`` against the default: variances, modes, spectrum and estimates byte for byte alike.  3 nodes are a partial
    group, 16 fill one, 17 make two groups of which one is a single node (it runs through the solo entry); the optimals' adjoint solves
    are the second ones of a step, with a column of the weighted block per node.  No solve of S2k misses ``ksp_rtol``, so no step is
    done again and every step queues one grouped call per group of more than one node: one per apply for all four cases."""
    one = solved(kind, nodes=nodes, batch_forward=batch_forward)
    two = solved(kind, nodes=nodes, batch_forward=batch_forward, batch_adjoint=True)
    print(f"{kind}, {nodes} nodes: default {one.stats}; batched adjoint {two.stats}")
    assert two.stats["batch_adjoint"] and not one.stats["batch_adjoint"]
    assert len(one.variances) == 2
    for name in ("variances", "modes", "spectrum", "estimates"):
        assert getattr(one, name).tobytes() == getattr(two, name).tobytes(), name
    assert one.stats["applies"] == two.stats["applies"]
    assert one.stats["refinements"] == two.stats["refinements"] == 0
    assert two.stats["adjoint_batches"] > 0
    assert two.stats["adjoint_batches"] == two.stats["applies"]
    assert one.stats["adjoint_batches"] == 0
    assert two.stats["forward_batches"] == one.stats["forward_batches"] == (one.stats["applies"] if batch_forward else 0)


def test_forced_refinement_runs_every_node_alone():
    """Every solve with the refinement step (the configuration of ``test_gpu_stochastic.py::test_forced_refinement``: 8 nodes, four
    modes, ncv = 24, atol = 1e-10, whose bound against the dense eigenvalues this asserts too): no node enters a group, and the counts
    show 8 refined adjoint solves per step."""
    res = solved("eofs", nodes=8, ncv=24, num_modes=4, atol=1e-10, batch_adjoint=True, refine=True)
    dense = np.array(GOLDEN["eofs"][:4])
    st = res.stats
    err = np.abs(res.variances - dense).max() / dense[0] if len(res.variances) == 4 else np.inf
    print(f"forced refinement, batch_adjoint: |theta - dense|_max / theta_1 = {err:.2e}; stats {st}")
    assert st["batch_adjoint"]
    assert st["adjoint_batches"] == 0
    assert st["refined_adjoint"] == 8 * st["applies"]
    assert err <= 1e-10
