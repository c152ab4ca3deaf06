"""GPU: StompOptimizer::serveBatch of the C++ facade -- three optimizers on one shared stream serve a
queue of seven requests as slots (stomp_group_serve).  Every request's slot and start step equal
serve_schedule on the oracle's iteration counts; its statistics, cost history and best trajectory
equal the CPU oracle's optimize() of the request, bit for bit; every optimizer ends as after
retarget(the last request it planned) + optimize(), torques included.  The driver itself checks that
a refused queue changes nothing and that no result carries torques (tests/facade_serve_driver.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from stomp_motion_planner_icra2011_amd import engine as eng
from oracle import pyoracle as po
from tests import facade_util as fu
from tests.group_util import INT_STATS, shelf_problems

pytestmark = pytest.mark.gpu


def build_serve_driver(directory):
    """facade_util.build_driver's compile line for tests/facade_serve_driver.cpp."""
    from stomp_motion_planner_icra2011_amd import _build
    lib = _build.build_facade()
    exe = os.path.join(directory, "facade_serve_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(fu.ROOT, "include"),
                           os.path.join(fu.ROOT, "tests", "facade_serve_driver.cpp"), "-o", exe, lib, _build.LIB,
                           "-Wl,-rpath," + fu.PKG])
    return exe


def test_facade_serve_batch_matches_the_oracles(tmp_path):
    P, n = 3, 7
    # the queue of tests/test_gpu_serve.py, K_r = 10: requests 1 and 8 stop early
    every = shelf_problems(14, 20, 10, grid=64, rng_seed=11, max_iterations=40, max_iterations_after_collision_free=2)
    ps = every[:P]
    qs = [every[i] for i in (0, 1, 2, 8, 4, 1, 11)]
    oracles = [po.Oracle(q, threads=8) for q in qs]
    oresults = [o.optimize() for o in oracles]
    its = [int(st.iterations) for st, _ in oresults]
    assert len(set(its)) >= 3, its
    want_slot, want_start, _ = eng.serve_schedule(P, its)
    dirs = []
    for i, p in enumerate(ps + qs):
        d = tmp_path / f"p{i}"
        d.mkdir()
        fu.write_problem(p, str(d))
        dirs.append(str(d))
    exe = build_serve_driver(str(tmp_path))
    res = str(tmp_path / "out.txt")
    r = subprocess.run([exe, res, str(P), str(n)] + dirs, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr)
    toks = open(res).read().split()
    pos = 0
    J, N = ps[0].J, ps[0].N
    last = {}
    for i, o in enumerate(oracles):
        ost, ocosts = oresults[i]
        head = toks[pos:pos + 8]
        pos += 8
        slot, start, it = int(head[0]), int(head[1]), int(head[2])
        print("request", i, "slot", slot, "start step", start, "iterations", it, "oracle", ost.iterations)
        assert (slot, start) == (want_slot[i], want_start[i]), i
        assert [int(x) for x in head[2:7]] == [int(getattr(ost, k)) for k in INT_STATS], i
        assert float(head[7]) == ost.best_cost, i
        vals = np.array([float(x) for x in toks[pos:pos + it + J * N]])
        pos += it + J * N
        np.testing.assert_array_equal(vals[:it], ocosts, err_msg=f"request {i} costs")
        np.testing.assert_array_equal(vals[it:].reshape(J, N), o.best_trajectory(), err_msg=f"request {i} best")
        last[slot] = i
    assert sorted(last) == list(range(P))
    # every optimizer: as after retarget(its last request) + optimize()
    for s in range(P):
        i = last[s]
        ost, ocosts = oresults[i]
        head = toks[pos:pos + 9]
        pos += 9
        it, ntq = int(head[0]), int(head[8])
        assert [int(x) for x in head[:5]] == [int(getattr(ost, k)) for k in INT_STATS], s
        assert float(head[5]) == ost.best_cost and ntq == N, s
        vals = np.array([float(x) for x in toks[pos:pos + it + ntq + J + J * N]])
        pos += it + ntq + J + J * N
        np.testing.assert_array_equal(vals[:it], ocosts, err_msg=f"optimizer {s} costs")
        np.testing.assert_array_equal(vals[it:it + ntq], oracles[i].best_torques(), err_msg=f"optimizer {s} torques")
        np.testing.assert_array_equal(vals[it + ntq:it + ntq + J], qs[i].start, err_msg=f"optimizer {s} start")
        np.testing.assert_array_equal(vals[it + ntq + J:].reshape(J, N), oracles[i].best_trajectory(),
                                      err_msg=f"optimizer {s} trajectory")
    assert pos == len(toks)
