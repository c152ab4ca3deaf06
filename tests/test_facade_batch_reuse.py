"""GPU: StompOptimizer::optimizeBatch of the C++ facade with reused rollouts -- three optimizers
of the reference's own kind of configuration (K = 20, K_r = 10) on one shared stream, optimized as
one engine group (stomp_group_optimize), each against the CPU oracle's optimize() of its problem,
bit for bit.  The driver is tests/facade_batch_driver.cpp as it is."""
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import facade_util as fu
from tests.test_facade_batch import build_batch_driver
from tests.group_util import INT_STATS
from tests.test_gpu_group_reuse import recipe

pytestmark = pytest.mark.gpu


def test_facade_optimize_batch_with_reuse_matches_the_oracles(tmp_path):
    ps = [recipe()[i] for i in (1, 2, 3)]
    assert all(p.params.num_reused_rollouts == 10 for p in ps)
    oracles = [po.Oracle(p, threads=8) for p in ps]
    oresults = [o.optimize() for o in oracles]
    ostops = [int(st.iterations) for st, _ in oresults]
    assert len(set(ostops)) == 3 and max(ostops) == 60, ostops   # the three stop on their own
    dirs = []
    for i, p in enumerate(ps):
        d = tmp_path / f"p{i}"
        d.mkdir()
        fu.write_problem(p, str(d))
        dirs.append(str(d))
    exe = build_batch_driver(str(tmp_path))
    res = str(tmp_path / "out.txt")
    r = subprocess.run([exe, res] + dirs, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    toks = open(res).read().split()
    pos = 0
    for i, (p, o) in enumerate(zip(ps, oracles)):
        ost, ocosts = oresults[i]
        head = toks[pos:pos + 9]
        pos += 9
        it, ntq = int(head[0]), int(head[8])
        print("optimizer", i, "iterations", it, "oracle", ost.iterations)
        assert [int(x) for x in head[:5]] == [int(getattr(ost, k)) for k in INT_STATS], i
        assert float(head[5]) == ost.best_cost, i
        success_duration, collision_duration = float(head[6]), float(head[7])
        assert (success_duration > 0) == (ost.success_iteration >= 0) and 0 <= success_duration < 60
        assert (collision_duration > 0) == (ost.collision_success_iteration >= 0) and 0 <= collision_duration < 60
        vals = np.array([float(x) for x in toks[pos:pos + it + ntq + p.J * p.N]])
        pos += it + ntq + p.J * p.N
        np.testing.assert_array_equal(vals[:it], ocosts, err_msg=f"optimizer {i} costs")
        assert ntq == p.N
        np.testing.assert_array_equal(vals[it:it + ntq], o.best_torques(), err_msg=f"optimizer {i} torques")
        np.testing.assert_array_equal(vals[it + ntq:].reshape(p.J, p.N), o.best_trajectory(),
                                      err_msg=f"optimizer {i} best trajectory")
    assert pos == len(toks)
