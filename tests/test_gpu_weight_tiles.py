"""GPU: every weights kernel launch_weights can pick (k_weights.hip), at the edges of its range of
K -- the wave kernel's last K, the second 64-rollout block with one row, both sides of each
threshold between two weights_rows<BLOCK, TCW, EPT> instantiations, and ragged last blocks in the
tiles that hold 8 and 32 rows per lane -- bit for bit against the CPU oracle.

chain5 at N = 39 has J N = 195 flat columns: the last column tile is ragged at every tile width
(195 = 24 * 8 + 3 = 48 * 4 + 3 = 97 * 2 + 1).  stick1 at N = 11 has 11 columns: fewer than 8 tiles,
so the XCD tile map runs with q8 = 0.  Each case asserts the instantiation the engine reports
(STOMP_DEBUG_LEAN_PRINT), so a retuning of the thresholds cannot leave one untested; tests/
GROUPS_AND_TILES.md holds the K -> instantiation table.
"""
import numpy as np
import pytest

from oracle import pyoracle as po
from stomp_motion_planner_icra2011_amd import engine as eng
from tests import model_zoo as mz
from tests.test_gpu_model_space import model_line
from tests.test_gpu_parity import _compare_iteration

pytestmark = pytest.mark.gpu

# K -> the kernel of launch_weights (a lone engine, the fused mode)
WEIGHTS = {64: "wave", 65: "rows<256,4,4>", 256: "rows<256,4,4>", 257: "rows<512,4,4>", 512: "rows<512,4,4>",
           513: "rows<512,4,8>", 1000: "rows<512,4,8>", 1024: "rows<512,4,8>", 1025: "rows<256,4,32>",
           1983: "rows<256,4,32>", 2048: "rows<256,4,32>", 2049: "rows<256,2,32>"}
PROBLEMS = dict(chain5=lambda K, **kw: mz.chain5(K=K, Kr=0, waypoints=40, **kw),
                stick1=lambda K, **kw: mz.stick1(K=K, Kr=0, waypoints=12, **kw))


def run_case(monkeypatch, capfd, name, K, **kw):
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    p = PROBLEMS[name](K, **kw)
    assert p.J * p.N == (195 if name == "chain5" else 11)
    o, e = po.Oracle(p, threads=8), eng.Engine(p)
    line = model_line(capfd)
    assert line.endswith(f", weights {WEIGHTS[K]}"), line
    for it in range(1, 3):
        _compare_iteration(o, e, it)
    # the weights are not degenerate: the probabilities of a column differ
    assert np.ptp(e.rollouts("probabilities")[:, 0, p.N // 2]) > 0
    e.close()


@pytest.mark.parametrize("K", sorted(WEIGHTS))
@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_weights_kernels_at_k_edges_bitwise(monkeypatch, capfd, name, K):
    run_case(monkeypatch, capfd, name, K)


@pytest.mark.parametrize("K", [65, 1000, 1983])
@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_weights_kernels_cumulative_costs_bitwise(monkeypatch, capfd, name, K):
    # use_cumulative_costs: the tiles load the suffix sums k_cumulative made (the a.cum path)
    run_case(monkeypatch, capfd, name, K, use_cumulative_costs=True)
