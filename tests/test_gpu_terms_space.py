"""GPU parity of the state-cost terms kernel (k_terms.hip) beyond the PR2 fixture: the HIP engine
against the CPU oracle, bit for bit, on torque chains of every shape the Newton-Euler sweep
branches on, on crafted constraint rows that take each branch of KDL GetQuaternion and of bullet
getRPY, at the N where launch_terms changes its instantiation and its LDS opt-in, at the LDS limit
where creation refuses, and in every engine mode whose trajectories the kernel reads.

tests/STATE_TERMS.md lists what each test reaches; tests/test_terms_space.py holds the oracle to the
numpy restatements on the same problems.  Every comparison is assert_array_equal; each test asserts
on its inputs (model_zoo.census, the crafted census on the oracle) and on the engine's own account
of its launches (STOMP_DEBUG_LEAN_PRINT) before it compares anything.
"""
import numpy as np
import pytest

from oracle import pyoracle as po
from stomp_motion_planner_icra2011_amd import engine as eng
from tests import model_zoo as mz
from tests.test_gpu_model_space import model_line, pair
from tests.test_gpu_parity import _compare_iteration
from tests.test_terms_space import assert_crafted_census, crafted_census_all

pytestmark = pytest.mark.gpu

TERMS = list(mz.TERMS_ZOO)


def terms_line(err):
    """The engine's own account of the launch launch_terms takes (STOMP_DEBUG_LEAN_PRINT)."""
    lines = [l for l in err.splitlines() if l.startswith("stomp: terms ")]
    assert lines, err
    return lines[-1]


def assert_terms_rows_equal(o, e, rows, member=1):
    """stomp_engine_eval on all rows at once against the oracle's execute, row by row, with the
    constraints_satisfied flags."""
    costs, cf, traj = e.execute(rows, iteration_member=member)
    ecs = e.last_constraints_satisfied
    sat = []
    for r in range(len(rows)):
        oc, ocf, otr = o.execute(rows[r], iteration_member=member)
        np.testing.assert_array_equal(traj[r], otr, err_msg=f"row {r}")
        np.testing.assert_array_equal(costs[r], oc, err_msg=f"row {r}")
        assert bool(cf[r]) == ocf and bool(ecs[r]) == o.last_constraints_satisfied, r
        sat.append(o.last_constraints_satisfied)
    return sat


def compare_iterations(o, e, count):
    for it in range(1, count + 1):
        _compare_iteration(o, e, it)
        assert e.last_constraints_satisfied == o.last_constraints_satisfied, it


def assert_terms_census(p, rows):
    c = mz.census(p, rows)
    assert c["rows_limited"] >= 1 and c["collision"] >= 1 and c["hinge"] >= 1, c


# ---------------------------------------------------------------------------- chain shapes

@pytest.mark.parametrize("name", TERMS + ["hand9"])
def test_terms_robots_bitwise(monkeypatch, capfd, name):
    # torque and constraints on every chain shape (tests/test_terms_space.py asserts the shapes):
    # execute rows, then two iterations at K = 12, K_r = 5 (the second reuses)
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    p = mz.hand9_constrained() if name == "hand9" else mz.TERMS_ZOO[name]()
    o, e = pair(p)
    line = terms_line(capfd.readouterr().err)
    if name == "hand9":
        # no torque chain: Q and the one row of costs, (3 * 9 + 1) * 39 * 8 bytes
        assert "nchain 0 noc 2 torque 0 stats 0, k_terms<128>, LDS 8736 B, opt-in 0" in line, line
    else:
        rows_lds = mz.TERMS_LDS_ROWS[name]
        assert f"nchain {(rows_lds - 3 * p.J) // 6} noc {len(p.orientation_constraints)} torque 1 stats 1," in line, line
        assert f"k_terms<128>, LDS {rows_lds * p.N * 8} B, opt-in 0" in line, line
    rows = mz.execute_rows(p, o.theta(), rows=4, seed=7)
    assert_terms_census(p, rows)
    assert_terms_rows_equal(o, e, rows)
    # the terms are in the costs: the same row without them costs less
    if name == "hand9":
        plain = po.Oracle(mz.hand9())
    else:
        plain = po.Oracle(mz.TERMS_ZOO[name](torque=0.0, constrained=False))
    assert np.all(e.execute(rows[0], 1)[0] > plain.execute(rows[0], 1)[0])
    compare_iterations(o, e, 2)


# ---------------------------------------------------------------------------- crafted constraint rows

@pytest.fixture(scope="module")
def crafted():
    cases = crafted_census_all()
    assert_crafted_census(cases)      # on the oracle alone, before any engine is created
    return cases


@pytest.mark.parametrize("case", list(mz.CRAFTED_CASES))
def test_crafted_constraint_rows_bitwise(crafted, case):
    p, rows, census, sat = crafted[case]
    o, e = pair(p)
    assert assert_terms_rows_equal(o, e, rows) == sat
    if case == "satisfied":
        assert sat == [True, False, False, False]
    compare_iterations(o, e, 2)


# ---------------------------------------------------------------------------- N and LDS edges
# launch_terms: k_terms<128> for N <= 128, k_terms<256> above; dynamic LDS (3 J + 6 nchain) N 8 bytes,
# through the opt-in above 64 KiB; creation refuses above 160 KiB.

N_EDGES = {9: 10, 128: 129, 129: 130, 255: 256, 256: 257}      # N -> waypoints


@pytest.mark.parametrize("N", sorted(N_EDGES))
def test_n_edges_bitwise(monkeypatch, capfd, N):
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    p = mz.TERMS_ZOO["chain5"](waypoints=N_EDGES[N], K=12, Kr=5)
    assert p.N == N and len(p.orientation_constraints) == 1
    o, e = pair(p)
    line = terms_line(capfd.readouterr().err)
    lds = 51 * N * 8
    assert f"J 5 N {N} nchain 6 noc 1 torque 1 stats 1, k_terms<{128 if N <= 128 else 256}>, LDS {lds} B, " \
           f"opt-in {int(lds > 65536)}" in line, line
    assert (lds > 65536) == (N >= 255)
    rows = mz.execute_rows(p, o.theta())
    assert_terms_census(p, rows)
    assert_terms_rows_equal(o, e, rows)
    assert_terms_rows_equal(o, e, rows[:1], member=0)
    compare_iterations(o, e, 2)


def test_opt_in_with_the_small_instantiation_bitwise(monkeypatch, capfd):
    # fork12 at N = 128: k_terms<128> with 120 * 128 * 8 = 122 880 B of dynamic LDS
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    p = mz.TERMS_ZOO["fork12_pedestal"](waypoints=129)
    o, e = pair(p)
    line = terms_line(capfd.readouterr().err)
    assert "J 12 N 128 nchain 14 noc 3 torque 1 stats 1, k_terms<128>, LDS 122880 B, opt-in 1" in line, line
    rows = mz.execute_rows(p, o.theta(), rows=4, seed=7)
    assert_terms_census(p, rows)
    assert_terms_rows_equal(o, e, rows)
    compare_iterations(o, e, 2)


def test_lds_limit_bitwise_and_refusal(monkeypatch, capfd):
    # chain17: 153 doubles per waypoint.  N = 133 is the last that fits (162 792 B <= 160 KiB),
    # N = 134 (164 016 B) is refused at creation, and the next engine of the process works
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    assert 153 * 133 * 8 == 162792 <= 160 * 1024 < 164016 == 153 * 134 * 8
    with pytest.raises(RuntimeError) as ei:
        eng.Engine(mz.TERMS_ZOO["chain17"](waypoints=135))
    assert "error -3" in str(ei.value) and "state-terms kernel needs 164016 B of LDS" in str(ei.value), str(ei.value)
    capfd.readouterr()
    p = mz.TERMS_ZOO["chain17"](waypoints=134)
    assert p.N == 133
    o, e = pair(p)
    line = terms_line(capfd.readouterr().err)
    assert "J 17 N 133 nchain 17 noc 1 torque 1 stats 1, k_terms<256>, LDS 162792 B, opt-in 1" in line, line
    rows = mz.execute_rows(p, o.theta(), rows=3, seed=7)
    assert_terms_census(p, rows)
    assert_terms_rows_equal(o, e, rows)
    compare_iterations(o, e, 2)


@pytest.mark.parametrize("name", TERMS)
def test_best_torques_with_the_term_off_bitwise(name):
    # STOMPStatistics.torques: the torque chain is evaluated on the best trajectory also when the
    # torque term is off (k_terms with the constraints off, on one row)
    p = mz.TERMS_ZOO[name](torque=0.0, max_iterations=4, max_iterations_after_collision_free=4)
    o, e = pair(p)
    ost, ocosts = o.optimize()
    est, ecosts = e.optimize()
    assert est.iterations == ost.iterations == 4
    np.testing.assert_array_equal(ecosts, ocosts)
    np.testing.assert_array_equal(e.best_trajectory(), o.best_trajectory())
    tq = o.best_torques()
    assert np.all(tq > 0.0)
    np.testing.assert_array_equal(e.best_torques(), tq)


def test_best_torques_say_when_the_statistics_kernel_does_not_fit():
    # term and constraints off at N = 134: creation succeeds (no k_terms launch in an iteration), the
    # statistics cannot run, and the error says why
    p = mz.TERMS_ZOO["chain17"](torque=0.0, constrained=False, waypoints=135)
    assert p.N == 134
    o, e = pair(p)
    with pytest.raises(RuntimeError) as ei:
        e.best_torques()
    assert "error -3" in str(ei.value), str(ei.value)
    assert "torque statistics kernel needs 164016 B of LDS" in str(ei.value), str(ei.value)
    assert "inertias not given" not in str(ei.value)
    assert np.all(o.best_torques() >= 0.0)      # the oracle has the chain
    _compare_iteration(o, e, 1)                 # and the engine goes on working


# ---------------------------------------------------------------------------- engine modes
# k_terms reads the joint-limited trajectories each rollout body writes (traj_out)

MODES = {   # mode -> (builder arguments, environment, body of the launch, oracle threads, iterations)
    "split": (dict(K=12, Kr=5), {}, "launch of 13 rollouts: split,", 1, 3),
    "phased": (dict(K=12, Kr=5), {"STOMP_DEBUG_SPLIT_MAX": "1"}, "launch of 13 rollouts: phased,", 1, 3),
    "wide": (dict(K=12, Kr=5, waypoints=256), {"STOMP_DEBUG_SPLIT_MAX": "1"}, "launch of 13 rollouts: wide,", 1, 2),
    "slot_loop": (dict(K=260, Kr=0), {}, "launch of 261 rollouts: slot loop,", 8, 2),
    "lean_slot_loop": (dict(K=260, Kr=0), {"STOMP_DEBUG_LEAN": "1"}, "launch of 261 rollouts: lean slot loop,", 8, 2),
    "cumulative": (dict(K=12, Kr=5, use_cumulative_costs=True), {}, "launch of 13 rollouts: split,", 1, 3),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_engine_modes_with_terms_bitwise(monkeypatch, capfd, mode):
    kw, env, body, threads, iterations = MODES[mode]
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = mz.TERMS_ZOO["chain5"](**kw)
    assert p.params.torque_cost_weight > 0 and len(p.orientation_constraints) == 1
    o, e = pair(p, threads=threads)
    err = capfd.readouterr().err
    line = [l for l in err.splitlines() if l.startswith("stomp: model ")][-1]
    assert body in line, line
    if mode == "lean_slot_loop":
        assert "lean 1 " in line, line
    assert "torque 1 " in terms_line(err)
    assert mz.census(p, o.theta()[None])["collision"] >= 1
    compare_iterations(o, e, iterations)


def test_unfused_reuse_with_terms_bitwise(monkeypatch, capfd):
    # J > 16: the reuse step runs first and nothing is pipelined; the second and third iteration reuse
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    p = mz.TERMS_ZOO["chain17"](K=12, Kr=5)
    o, e = pair(p)
    assert "pregen 0 fused_noise 0" in model_line(capfd)
    compare_iterations(o, e, 3)
    assert len(o.reuse_log()) >= 2


def test_eval_with_more_rows_than_rollouts_bitwise():
    K = 12
    p = mz.TERMS_ZOO["chain5"](K=K, Kr=5)
    o, e = pair(p)
    rows = mz.execute_rows(p, o.theta(), rows=K + 3, seed=11)
    assert_terms_census(p, rows)
    sat = assert_terms_rows_equal(o, e, rows)
    assert len(sat) == K + 3
    compare_iterations(o, e, 2)         # the iterations after the wide eval are undisturbed
    assert_terms_rows_equal(o, e, rows)


def test_group_refuses_engines_with_constraints():
    # constraint-only engines (no torque term) at K_r = 0 are still engines with state-cost terms
    ps = [mz.TERMS_ZOO["chain5"](torque=0.0, K=20, Kr=0, robot_seed=105 + i) for i in range(2)]
    assert all(len(p.orientation_constraints) == 1 and p.params.torque_cost_weight == 0.0 for p in ps)
    s = eng.Stream()
    es = [eng.Engine(p, stream=s.ptr) for p in ps]
    with pytest.raises(RuntimeError) as ei:
        eng.EngineGroup(es)
    assert "error -3" in str(ei.value) and "state-cost terms" in str(ei.value), str(ei.value)
    for p, e in zip(ps, es):
        compare_iterations(po.Oracle(p), e, 2)
