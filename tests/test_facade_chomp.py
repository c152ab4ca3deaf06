"""GPU: the C++ facade's StompOptimizer::optimize() with StompParameters::use_chomp -- the reference's
CHOMP mode (stomp_optimizer.cpp:289-299) over stomp_chomp_*.  On the shelf fixture its statistics,
cost history, best trajectory and last cost equal the loop of tests/chomp_ref.c bit for bit, and an
optimizer with use_hamiltonian_monte_carlo fails with the STOMP_E_UNSUPPORTED message in lastError()
(tests/facade_chomp_driver.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from tests import chomp_util as cu
from tests import facade_util as fu

pytestmark = pytest.mark.gpu


def build_chomp_driver(directory):
    """facade_util.build_driver's compile line for tests/facade_chomp_driver.cpp."""
    from stomp_motion_planner_icra2011_amd import _build
    lib = _build.build_facade()
    exe = os.path.join(directory, "facade_chomp_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(fu.ROOT, "include"),
                           os.path.join(fu.ROOT, "tests", "facade_chomp_driver.cpp"), "-o", exe, lib, _build.LIB,
                           "-Wl,-rpath," + fu.PKG])
    return exe


def test_facade_optimize_with_use_chomp_matches_the_reference_loop(tmp_path):
    # the loop's starts of test_gpu_chomp.py come free late; from theta_0 the descent is free at
    # iteration 3 and stops after 5 (a streak of 2), with a later improvement
    p = cu.shelf(grid_n=32, N=33, max_iterations=12, cf=2, smoothness_cost_weight=0.1)
    prm = cu.ChompParams(learning_rate=0.05, use_pseudo_inverse=True, joint_update_limits=(0.05, 0.04, 0.05, 0.03, 0.05, 0.05, 0.02))
    r = cu.ChompRef(p, prm)
    r.reset(None)
    st, costs, best = r.optimize()
    print(cu.stats_tuple(st), costs)
    assert 1 < st.iterations < p.params.max_iterations and st.success
    fu.write_problem(p, str(tmp_path))
    with open(tmp_path / "chomp.txt", "w") as f:
        f.write(" ".join(map(repr, [prm.learning_rate, prm.smoothness_cost_weight, int(prm.use_pseudo_inverse),
                                    prm.pseudo_inverse_ridge_factor, *map(float, prm.limits(p.J))])) + "\n")
    exe = build_chomp_driver(str(tmp_path))
    res = str(tmp_path / "out.txt")
    run = subprocess.run([exe, res, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr)
    lines = open(res).read().splitlines()
    head = lines[0].split()
    got = tuple(int(x) for x in head[:5]) + (float(head[5]),)
    assert got == cu.stats_tuple(st), (got, cu.stats_tuple(st))
    assert float(head[6]) == r.get("cost") and int(head[7]) == int(r.get("collision_free"))
    n = st.iterations
    np.testing.assert_array_equal(np.array([float(x) for x in lines[1:1 + n]]), costs)
    traj = np.array([float(x) for x in lines[1 + n:1 + n + p.J * p.N]]).reshape(p.J, p.N)
    np.testing.assert_array_equal(traj, best)
    assert len(lines) == 2 + n + p.J * p.N
    assert "use_hamiltonian_monte_carlo is not supported" in lines[-1]
