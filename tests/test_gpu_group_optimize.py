"""GPU: stomp_group_optimize -- StompOptimizer::optimize for a whole engine group, each problem
stopping on its own (its collision-free streak or its own max_iterations) while the group runs in
lockstep through the grouped launches.  Every engine must end exactly where the CPU oracle's
optimize() of its problem ends and where its own stomp_engine_optimize leaves it, bit for bit, with
and without the compaction that takes stopped engines out of the launches.

The PR2 recipe is tests/group_util.py's `shelf_problems` with default_rng(11): its 16 problems stop
at well-spread iterations (each test asserts the spread it needs on the oracle's own counts)."""
import functools

import numpy as np
import pytest

from stomp_motion_planner_icra2011_amd import engine as eng
from tests import model_zoo as mz
from tests.group_util import (FIELDS, Group, assert_group, assert_results_equal, assert_spread, assert_states_equal,
                              assert_twin, continue_against_oracle, iterations, optimize_oracles, shelf_problems,
                              twins_of, variants)

pytestmark = pytest.mark.gpu

# what a K_r = 0 engine is compared on with its twin, and with its oracle after each further iteration
# (at K_r = 0 the oracle holds no extra rollout's params / noise / control rows)
TWIN_ROWS = FIELDS + ("best", "x_state")
ITER_ROWS = FIELDS + ("control",)


@functools.lru_cache(maxsize=None)
def recipe(K, max_it, P=16):
    """The 16 PR2 shelf problems (shared between the tests, never written)."""
    return tuple(shelf_problems(P, K, 0, rng_seed=11, max_iterations=max_it, max_iterations_after_collision_free=2))


@functools.lru_cache(maxsize=None)
def pr2(K, max_it, idx):
    """(problems, oracles after optimize, snapshots) of the recipe's problems `idx`.  The
    snapshots are the shared reference and are never written (copies, read-only); the oracle objects
    are used by the one test that continues them with further iterations."""
    ps = [recipe(K, max_it)[i] for i in idx]
    oracles, snaps = optimize_oracles(ps)
    return ps, oracles, snaps


ALL16 = tuple(range(16))


def test_spread_by_collisions():
    # 16 problems, K = 20, max_iterations = 60: stops spread over the run and engines that run it out
    ps, oracles, snaps = pr2(20, 60, ALL16)
    assert_spread(snaps, 60)
    g = Group(ps)
    results = g.group.optimize()
    assert_group(g, results, snaps)
    # four engines against twins that ran their own stomp_engine_optimize: the earliest and the
    # latest early stop, one that ran out its iterations, and engine 0
    its = iterations(snaps)
    early = [i for i in range(16) if its[i] < 60]
    picks = sorted({0, min(early, key=lambda i: its[i]), max(early, key=lambda i: its[i]), its.index(60)})
    picks += [i for i in range(16) if i not in picks][: 4 - len(picks)]
    for i in picks:
        twin = eng.Engine(ps[i])
        assert_twin(g.engines[i], results[i], twin, twin.optimize(), f"engine {i} against its twin", TWIN_ROWS)
        twin.close()
    for i, (o, e) in enumerate(zip(oracles, g.engines)):
        continue_against_oracle(o, e, its[i] + 1, 2, ITER_ROWS)
    g.close()


def test_four_column_tiles_k129():
    # K = 129: the four-column weights tiles, 6 x 130 rollout workgroups (more than the compute units)
    idx = (0, 1, 2, 8, 11, 14)
    ps, _, snaps = pr2(129, 40, idx)
    assert_spread(snaps, 40)
    g = Group(ps)
    assert_group(g, g.group.optimize(), snaps)
    g.close()


@pytest.mark.parametrize("robot", ["chain5", "fork12"])
def test_per_engine_caps(robot):
    caps = (1, 7, 8, 9, 20)
    ps = variants(mz.ZOO[robot], 5, K=20, Kr=0, max_iterations_after_collision_free=1000)
    for p, c in zip(ps, caps):
        p.params.max_iterations = c
    _, snaps = optimize_oracles(ps)
    assert tuple(iterations(snaps)) == caps, iterations(snaps)
    g = Group(ps)
    results = g.group.optimize(costs_stride=20)
    assert_group(g, results, snaps)
    g.close()


def test_everyone_stops_early():
    idx = (1, 8, 11, 14)
    ps, _, snaps = pr2(20, 200, idx)
    its = iterations(snaps)
    assert all(n < 20 for n in its), its
    g = Group(ps)
    g.engines[0].set_timing(True)
    results = g.group.optimize()
    launches = g.engines[0].timing("rollout_cost")[1]
    chunk = eng.EngineGroup.optimize_chunk()
    print("rollout launches", launches, "stops", its, "chunk", chunk)
    assert chunk >= 1 and launches <= max(its) + 2 * chunk + 2, (launches, its, chunk)
    assert_group(g, results, snaps)
    g.close()


LIFECYCLE = (1, 2, 8, 11)


def test_lifecycle_run_then_optimize():
    ps = [recipe(20, 60)[i] for i in LIFECYCLE]
    g, twins = Group(ps), twins_of(ps)
    g.group.run(1, 3)
    gres = g.group.optimize()
    for t in twins:
        t.run(1, 3)
    tres = [t.optimize() for t in twins]
    assert_results_equal(gres, tres, "run then optimize")
    assert_states_equal(g, twins, "run then optimize", TWIN_ROWS)
    g.close()


def test_lifecycle_optimize_then_run():
    ps = [recipe(20, 60)[i] for i in LIFECYCLE]
    g, twins = Group(ps), twins_of(ps)
    gres = g.group.optimize()
    g.group.run(61, 2)
    g.group.synchronize()
    tres = [t.optimize() for t in twins]
    for t in twins:
        t.run(61, 2)
        t.synchronize()
    assert_results_equal(gres, tres, "optimize then run")
    assert_states_equal(g, twins, "optimize then run", TWIN_ROWS)
    g.close()


def test_lifecycle_optimize_twice():
    ps = [recipe(20, 60)[i] for i in LIFECYCLE]
    g, twins = Group(ps), twins_of(ps)
    g1, g2 = g.group.optimize(), g.group.optimize()
    t1 = [t.optimize() for t in twins]
    t2 = [t.optimize() for t in twins]
    assert_results_equal(g1, t1, "first optimize")
    assert_results_equal(g2, t2, "second optimize")
    assert_states_equal(g, twins, "optimize twice", TWIN_ROWS)
    g.close()


@pytest.mark.parametrize("compact", ["0", "1"])
def test_compaction_on_and_off(monkeypatch, compact):
    # the switch is read when the group is created
    monkeypatch.setenv("STOMP_DEBUG_GROUP_COMPACT", compact)
    ps, _, snaps = pr2(20, 60, ALL16)
    assert_spread(snaps, 60)
    g = Group(ps)
    results = g.group.optimize()
    assert_group(g, results, snaps)
    g.close()


def test_refusals():
    idx = (1, 8, 14)
    ps, _, snaps = pr2(20, 60, idx)
    g = Group(ps)
    before = [e.theta() for e in g.engines]
    with pytest.raises(RuntimeError) as ei:
        g.group.optimize(costs_stride=59)
    assert "error -1" in str(ei.value), str(ei.value)
    for e, th in zip(g.engines, before):
        np.testing.assert_array_equal(e.theta(), th)
    assert_group(g, g.group.optimize(), snaps)
    g.close()
