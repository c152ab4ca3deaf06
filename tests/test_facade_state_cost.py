"""GPU: the C++ facade's StompOptimizer::getStateCosts -- the reference's GetStateCost.srv shape
(link segments and robot states in; per-link costs, validity, in_collision and the least clearance
out) over stomp_engine_query_states.  On the shelf fixture its responses equal the Python binding's
arrays for the same states, bit for bit, and those equal the CPU oracle's
(tests/state_query_util.py); the driver itself checks that refused calls leave the output alone
(tests/facade_state_cost_driver.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from stomp_motion_planner_icra2011_amd import engine as eng
from tests import facade_util as fu
from tests import state_query_util as squ

pytestmark = pytest.mark.gpu


def build_state_cost_driver(directory):
    """facade_util.build_driver's compile line for tests/facade_state_cost_driver.cpp."""
    from stomp_motion_planner_icra2011_amd import _build
    lib = _build.build_facade()
    exe = os.path.join(directory, "facade_state_cost_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(fu.ROOT, "include"),
                           os.path.join(fu.ROOT, "tests", "facade_state_cost_driver.cpp"), "-o", exe, lib, _build.LIB,
                           "-Wl,-rpath," + fu.PKG])
    return exe


def test_facade_state_costs_match_the_binding(tmp_path):
    p, q, links, ref, c = squ.case("pr2")
    squ.assert_census("pr2", c)
    fu.write_problem(p, str(tmp_path))
    with open(tmp_path / "states.txt", "w") as f:
        f.write(f"{len(q)} {p.J}\n" + "\n".join(" ".join(map(repr, map(float, row))) for row in q) + "\n")
    with open(tmp_path / "links.txt", "w") as f:
        f.write(f"{len(links)}\n" + " ".join(map(str, links)) + "\n")
    exe = build_state_cost_driver(str(tmp_path))
    res = str(tmp_path / "out.txt")
    r = subprocess.run([exe, res, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    toks = open(res).read().split()
    M, L = len(q), len(links)
    assert len(toks) == M * (4 + L)
    rows = np.array(toks, dtype=object).reshape(M, 4 + L)
    valid = rows[:, 0].astype(int).astype(bool)
    in_collision = rows[:, 1].astype(int).astype(bool)
    min_sphere = rows[:, 2].astype(int)
    min_clearance = np.array([float(x) for x in rows[:, 3]])
    costs = np.array([[float(x) for x in row[4:]] for row in rows])
    e = eng.Engine(p)
    got = e.query_states(q, links=links)
    np.testing.assert_array_equal(costs, got.link_costs)
    np.testing.assert_array_equal(valid, ~got.limits_violated)
    np.testing.assert_array_equal(in_collision, got.in_collision)
    np.testing.assert_array_equal(min_sphere, got.min_sphere)
    np.testing.assert_array_equal(min_clearance, got.min_clearance)
    np.testing.assert_array_equal(costs, ref.link_costs)          # and the oracle's
    np.testing.assert_array_equal(in_collision, ref.in_collision)
    assert valid.any() and not valid.all() and in_collision.any() and not in_collision.all()
    e.close()
