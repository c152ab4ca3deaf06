"""GPU: stomp_group_serve -- a queue of requests served by a group's engines as slots, a slot that
stops taking the next waiting request.  Every request's results are compared with assert_array_equal
against the CPU oracle's optimize() of the planning slot's problem with the request's start, goal and
seed; the slots and start steps against serve_schedule (the host-only decision procedure) on the
oracle's iteration counts; every used engine afterwards against a twin that did retarget(last
request of the slot) + optimize() on its own.  tests/SERVE.md lists the cases.

Without the feature EngineGroup has no serve and every case fails."""
import dataclasses
import functools

import numpy as np
import pytest

from stomp_motion_planner_icra2011_amd import engine as eng
from oracle import pyoracle as po
from tests import model_zoo as mz
from tests import rank_util as ru
from tests.group_util import (FULL, INT_STATS, NO_REUSE_ORACLE_SKIPS, ROWS, Group, advance, assert_group, assert_same,
                              continue_against_oracle, iterations, optimize_oracles, shelf_problems, snapshot, state)

pytestmark = pytest.mark.gpu

SLOTS = 4
MAX_IT = 40
SHORT = dict(max_iterations=8, max_iterations_after_collision_free=2)
# the oracle's iteration counts of the two queues, checked on the CPU when the cases were written
EXPECTED_ITERATIONS = {0: [30, 8, 40, 40, 40, 40, 40, 40, 12, 40, 40, 13, 37, 40],
                       10: [22, 10, 40, 40, 26, 40, 40, 40, 7, 30, 10, 12, 12, 40]}


def request_arrays(qs):
    return [q.start for q in qs], [q.goal for q in qs], [q.seed for q in qs]


def on_slot(p, q):
    """the problem slot p plans for request q: its own model and parameters, q's start, goal and seed"""
    return dataclasses.replace(p, start=q.start.copy(), goal=q.goal.copy(), seed=q.seed)


def assert_request(res, snap, tag):
    slot, start, st, costs, best = res
    print(tag, "slot", slot, "start step", start, "iterations", st.iterations, "oracle", snap["stats"][0])
    assert tuple(int(getattr(st, k)) for k in INT_STATS) == snap["stats"], tag
    assert st.best_cost == snap["best_cost"], tag
    np.testing.assert_array_equal(costs, snap["costs"], err_msg=tag)
    np.testing.assert_array_equal(best, snap["best"], err_msg=tag)


def assert_schedule(results, its, slots, tag):
    want_slot, want_start, _ = eng.serve_schedule(slots, its)
    assert [r[0] for r in results] == want_slot, tag
    assert [r[1] for r in results] == want_start, tag


def assert_results_same(a, b, tag):
    assert len(a) == len(b), tag
    for r, (x, y) in enumerate(zip(a, b)):
        assert x[:2] == y[:2], (tag, r)
        for k in INT_STATS + ("best_cost",):
            assert getattr(x[2], k) == getattr(y[2], k), (tag, r, k)
        np.testing.assert_array_equal(x[3], y[3], err_msg=f"{tag}: request {r} costs")
        np.testing.assert_array_equal(x[4], y[4], err_msg=f"{tag}: request {r} best")


@functools.lru_cache(maxsize=None)
def queue(Kr):
    """(the 14 problems, their oracle snapshots): computed once, never written"""
    ps = shelf_problems(14, 20, Kr, grid=64, rng_seed=11, max_iterations=MAX_IT, max_iterations_after_collision_free=2)
    return ps, optimize_oracles(ps)[1]


@functools.lru_cache(maxsize=None)
def served(Kr):
    """the queue served once by four slots built from its first four problems: (group, results, info);
    the group stays open for the end-state case"""
    ps, _ = queue(Kr)
    g = Group(ps[:SLOTS])
    results = g.group.serve(*request_arrays(ps))
    return g, results, g.group.serve_info()


# ------------------------------------------------------------------------------------------------
# 1. the queue against the oracle

@pytest.mark.parametrize("Kr", [0, 10])
def test_queue_against_the_oracle(Kr):
    ps, snaps = queue(Kr)
    its = iterations(snaps)
    # on the oracle alone: the stops are spread
    assert len({n for n in its if n < MAX_IT}) >= 4 and MAX_IT in its, its
    assert its == EXPECTED_ITERATIONS[Kr], its
    _, results, info = served(Kr)
    for r, (res, snap) in enumerate(zip(results, snaps)):
        assert_request(res, snap, f"K_r {Kr}, request {r}")
    assert_schedule(results, its, SLOTS, f"K_r {Kr}")
    print("info", info)
    chunk = eng.EngineGroup.optimize_chunk()
    assert info["turnovers"] == 10 and info["mixed_steps"] > 0 and info["largest_idle_gap"] <= 3 * chunk, info
    assert info["occupied_slot_steps"] == sum(its) and info["steps"] == eng.serve_schedule(SLOTS, its)[2], info


# ------------------------------------------------------------------------------------------------
# 2. the end state

@pytest.mark.parametrize("Kr", [0, 10])
def test_end_state(Kr):
    ps, snaps = queue(Kr)
    g, results, _ = served(Kr)
    last = {}
    for r, res in enumerate(results):
        last[res[0]] = r
    assert sorted(last) == list(range(SLOTS))
    for s, e in enumerate(g.engines):
        q = on_slot(ps[s], ps[last[s]])
        assert e.problem.seed == q.seed
        np.testing.assert_array_equal(e.problem.start, q.start)
        twin = eng.Engine(ps[s])
        twin.retarget(q.start, q.goal, q.seed)
        twin.optimize()
        assert_same(state(e, FULL), state(twin, FULL), f"K_r {Kr}, slot {s} against its twin")
        twin.close()
    # one slot goes on iterating on its own, against its oracle
    s = 1
    o = po.Oracle(on_slot(ps[s], ps[last[s]]), threads=8)
    assert snapshot(o)["stats"] == snaps[last[s]]["stats"]
    rows = ROWS if Kr > 0 else tuple(k for k in ROWS if k not in NO_REUSE_ORACLE_SKIPS)
    continue_against_oracle(o, g.engines[s], snaps[last[s]]["stats"][0] + 1, 2, rows)
    # and the group plans a batch afterwards
    g.group.retarget(*request_arrays(ps[:SLOTS]))
    assert_group(g, g.group.optimize(), snaps[:SLOTS])


# ------------------------------------------------------------------------------------------------
# 3. fewer requests than slots

def test_fewer_requests_than_slots():
    ps, snaps = queue(10)
    g = Group(ps[:SLOTS])
    g.group.run(1, 2)
    g.group.synchronize()
    before = [state(e, FULL) for e in g.engines]
    results = g.group.serve(*request_arrays(ps[4:6]))
    for r, res in enumerate(results):
        assert_request(res, snaps[4 + r], f"request {r}")
    assert [(r[0], r[1]) for r in results] == [(0, 1), (1, 1)]
    assert g.group.serve_info()["turnovers"] == 0
    for s in (2, 3):
        assert g.engines[s].problem is ps[s]
        assert_same(state(g.engines[s], FULL), before[s], f"slot {s} untouched")
        o = po.Oracle(ps[s], threads=8)
        advance([o], 1, 2)
        continue_against_oracle(o, g.engines[s], 3, 1)
    g.close()


# ------------------------------------------------------------------------------------------------
# 4. per-slot parameters: max_iterations 5 + i, so cap flushes mix with turnovers

def moved(p, k, span=0.3):
    rng = np.random.default_rng(900 + k)
    f = np.array([not (j.has_limits and j.min == j.max) for j in p.robot.joints], np.float64)
    return dataclasses.replace(p, start=p.start + f * rng.uniform(-span, span, p.J),
                               goal=p.goal + f * rng.uniform(-span, span, p.J), seed=p.seed + 1000 + k)


def serve_against_slot_oracles(g, ps, qs, tag):
    """serve qs on the group of ps; every result against the oracle of the planning slot's own problem,
    the schedule against serve_schedule on the oracle's iteration counts"""
    results = g.group.serve(*request_arrays(qs))
    its = []
    for r, res in enumerate(results):
        snap = snapshot(po.Oracle(on_slot(ps[res[0]], qs[r]), threads=8))
        assert_request(res, snap, f"{tag}, request {r}")
        its.append(snap["stats"][0])
    assert_schedule(results, its, len(ps), tag)
    return results, its


@pytest.mark.parametrize("Kr", [5, 0])
def test_per_slot_parameters(Kr):
    p = mz.chain5(Kr=Kr, **SHORT)
    ps = [dataclasses.replace(moved(p, 20 + i), params=dataclasses.replace(p.params, max_iterations=5 + i))
          for i in range(4)]
    qs = [moved(p, 40 + r) for r in range(9)]
    g = Group(ps)
    results, its = serve_against_slot_oracles(g, ps, qs, f"zoo K_r {Kr}")
    caps = [ps[res[0]].params.max_iterations for res in results]
    assert any(n == c for n, c in zip(its, caps)), (its, caps)     # a request ended by its slot's own cap
    assert g.group.serve_info()["turnovers"] == 5
    g.close()


# ------------------------------------------------------------------------------------------------
# 5. state-cost terms and cumulative costs, mixed in one group

def test_with_state_terms_and_cumulative_costs():
    p = mz.TERMS_ZOO["chain5"](use_cumulative_costs=True, **SHORT)
    assert p.params.torque_cost_weight > 1e-9 and p.orientation_constraints and p.params.num_reused_rollouts == 5
    ps = [moved(p, 50 + i) for i in range(3)]
    # slot 1 without terms, slot 2 without cumulative costs
    ps[1] = dataclasses.replace(ps[1], orientation_constraints=[],
                                params=dataclasses.replace(p.params, torque_cost_weight=0.0))
    ps[2] = dataclasses.replace(ps[2], params=dataclasses.replace(p.params, use_cumulative_costs=False))
    qs = [moved(p, 60 + r) for r in range(7)]
    g = Group(ps, state_terms=True, cumulative_costs=True)
    serve_against_slot_oracles(g, ps, qs, "terms and cumulative costs")
    g.close()


# ------------------------------------------------------------------------------------------------
# 6. compaction on and off

def test_compaction_on_and_off():
    ps, snaps = queue(10)
    out = []
    for compact in (False, True):
        g = Group(ps[:SLOTS], compact=compact)
        results = g.group.serve(*request_arrays(ps))
        info = g.group.serve_info()
        for r, (res, snap) in enumerate(zip(results, snaps)):
            assert_request(res, snap, f"compact {compact}, request {r}")
        out.append((results, [info[k] for k in eng.EngineGroup.SERVE_INFO[:5]], [state(e, FULL) for e in g.engines]))
        g.close()
    assert_results_same(out[0][0], out[1][0], "compaction off / on")
    assert out[0][1] == out[1][1]
    for s, (a, b) in enumerate(zip(out[0][2], out[1][2])):
        assert_same(a, b, f"slot {s}, compaction off / on")


# ------------------------------------------------------------------------------------------------
# 7. lifecycle

def test_optimize_then_serve_twice_and_a_request_twice():
    ps, snaps = queue(10)
    g = Group(ps[:SLOTS])
    assert_group(g, g.group.optimize(), snaps[:SLOTS])
    # requests 1 and 8 stop early; request 1 is in the queue twice
    order = [0, 1, 2, 3, 8, 1, 4]
    qs = [ps[r] for r in order]
    first = g.group.serve(*request_arrays(qs))
    second = g.group.serve(*request_arrays(qs))
    assert_results_same(first, second, "the same queue twice")
    for k, r in enumerate(order):
        assert_request(first[k], snaps[r], f"queue entry {k} (request {r})")
    assert first[1][0] != first[5][0] or first[1][1] != first[5][1]
    assert g.group.serve_info()["allocations"] == 0       # the second call found every buffer large enough
    g.close()


# ------------------------------------------------------------------------------------------------
# 8. refusals

def test_refusals_leave_every_engine_untouched(monkeypatch):
    ps, _ = queue(10)
    g = Group(ps[:SLOTS])
    g.group.run(1, 1)
    g.group.synchronize()
    before = [state(e, FULL) for e in g.engines]
    starts, goals, seeds = request_arrays(ps)
    bad = [s.copy() for s in goals]
    bad[9][3] = np.nan
    with pytest.raises(RuntimeError) as ei:
        g.group.serve(starts, bad, seeds)
    assert "error -1" in str(ei.value) and "request 9" in str(ei.value) and "not finite" in str(ei.value), str(ei.value)
    with pytest.raises(RuntimeError) as ei:
        g.group.serve(starts, goals, seeds, costs_stride=MAX_IT - 1)
    assert "error -1" in str(ei.value) and "costs_stride" in str(ei.value), str(ei.value)
    for s, e in enumerate(g.engines):
        assert e.problem is ps[s]
        assert_same(state(e, FULL), before[s], f"slot {s} after the refusals")
    g.close()
    # sharded engines never reach a serve call: a group does not take them, by retarget's rule
    p = mz.chain5(K=128, Kr=0)
    ranks = ru.make_ranks(p, 2, None, monkeypatch)
    with pytest.raises(RuntimeError) as ei:
        eng.EngineGroup(ranks[:1])
    assert "error -3" in str(ei.value), str(ei.value)
    ru.close_all(ranks)
