"""GPU: engine groups whose engines carry state-cost terms -- the torque term and / or orientation
path constraints (stomp_optimizer.cpp:1107-1151) -- created with stomp_group_create_with
(state_terms = 1): stomp_group_run, stomp_group_synchronize and stomp_group_optimize with one
k_terms_group launch after every grouped rollout launch and every grouped noiseless flush.

Every engine of a group must end exactly where a twin engine making the same calls alone ends (its
own k_terms launches) and where the CPU oracle of its problem is, bit for bit: theta, the last
trajectory, probabilities, state costs, noise, params, control costs and the extra rollout's rows;
after optimize also the statistics, the cost history, the best trajectory and best_torques.  Every
comparison is assert_array_equal.  tests/GROUP_TERMS.md lists what each test reaches.

Without stomp_group_create_with the tests of the groups fail at creation: the symbol is missing,
and stomp_group_create refuses every engine with terms (error -3)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from stomp_motion_planner_icra2011_amd import engine as eng
from stomp_motion_planner_icra2011_amd import problem as pb
from oracle import pyoracle as po
from tests import model_zoo as mz
from tests import group_util as gu
from tests.group_util import (CHUNKS, FULL, Group, advance, assert_result, assert_results_equal, assert_same,
                              assert_states_equal, close_all, distinct, iterations, optimize_oracles, oracle_skips, state,
                              twins_of, variants)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def TermsGroup(ps, compact=None):
    """Engines of `ps` on one stream and their group, created with state_terms = 1."""
    return Group(ps, state_terms=True, compact=compact)


def terms_group_line(err):
    """The group's own account of the launch launch_terms_group takes (STOMP_DEBUG_LEAN_PRINT)."""
    lines = [l for l in err.splitlines() if l.startswith("stomp: group terms ")]
    assert lines, err
    return lines[-1]


def run_in_chunks(ps, chunks=CHUNKS, threads=1):
    gu.run_in_chunks(ps, chunks, threads, TermsGroup, oracle_skips).close()


def terms_robot(name):
    return mz.hand9_constrained if name == "hand9" else mz.TERMS_ZOO[name]


# ------------------------------------------------------------------------------------------------
# 1. runs in chunks over the chain shapes

@pytest.mark.parametrize("Kr", [0, 5])
@pytest.mark.parametrize("name", ["stick1_pedestal", "chain5", "hand9", "fork12_base"])
def test_run_matches_single_engines_and_oracles(name, Kr):
    # stick1_pedestal: J = 1, a fixed first chain segment; chain5: torque and the upright constraint;
    # hand9: constraints only, no chain (the one-row F of terms_lds_bytes); fork12_base: J = 12, 41 KB
    ps = variants(terms_robot(name), 3, K=12, Kr=Kr)
    assert (ps[0].params.num_rollouts, ps[0].params.num_reused_rollouts) == (12, Kr)
    assert ps[0].orientation_constraints or ps[0].params.torque_cost_weight > 0
    run_in_chunks(ps)


# ------------------------------------------------------------------------------------------------
# 2. a mixed group: torque and constraint, constraint only, torque only, neither

def mixed4(K=12, Kr=5):
    kw = dict(K=K, Kr=Kr, max_iterations=12, max_iterations_after_collision_free=2)
    make = mz.TERMS_ZOO["chain5"]
    return distinct([make(torque=0.001, **kw), make(torque=0.0, **kw), make(torque=0.001, constrained=False, **kw),
                     make(torque=0.0, constrained=False, **kw)])


def test_mixed_group_each_engine_its_own_terms(monkeypatch, capfd):
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    ps = mixed4()
    # one group shape, four terms models
    assert len({(p.J, p.N, p.params.num_rollouts, p.params.num_reused_rollouts, len(p.spheres),
                 len(p.robot.segments)) for p in ps}) == 1
    assert [(p.params.torque_cost_weight > 1e-9, len(p.orientation_constraints)) for p in ps] == \
        [(True, 1), (False, 1), (True, 0), (False, 0)]
    g = TermsGroup(ps)
    err = capfd.readouterr().err
    # each engine's own account of its terms (the line build_terms prints): the fourth has none
    terms = [l for l in err.splitlines() if l.startswith("stomp: terms ")]
    assert len(terms) == 4, err
    for line, want in zip(terms, ("noc 1 torque 1 ", "noc 1 torque 0 ", "noc 0 torque 1 ", "noc 0 torque 0 ")):
        assert want in line, line
    assert "k_terms_group<128>, LDS 15912 B, opt-in 0, engines with terms 3 of 4" in terms_group_line(err), err
    assert 51 * 39 * 8 == 15912
    twins = twins_of(ps)
    twins[3].set_timing(True)
    oracles = [po.Oracle(p) for p in ps]
    for first, count in CHUNKS:
        g.group.run(first, count)
        g.group.synchronize()
        advance(oracles, first, count)
        for i, (ge, te, o) in enumerate(zip(g.engines, twins, oracles)):
            te.run(first, count)
            te.synchronize()
            a = state(ge)
            assert_same(a, state(te), f"after ({first}, {count}): engine {i} against its own run,")
            assert_same(a, state(o), f"after ({first}, {count}): engine {i} against its oracle,")
    # the twin of the engine without terms never saw a terms launch
    assert twins[3].timing("state_terms")[1] == 0
    gres = g.group.optimize()
    tres = [t.optimize() for t in twins]
    assert_results_equal(gres, tres, "mixed optimize")
    assert_states_equal(g, twins, "mixed optimize")
    close_all(g, twins)


# ------------------------------------------------------------------------------------------------
# 3. / 4. N edges and the LDS opt-in of the group kernel's own instantiations

@pytest.mark.parametrize("waypoints", [10, 129, 130])
def test_n_edges(monkeypatch, capfd, waypoints):
    # N = 9: six of the seven taps of the first rows are padding; N = 128: the last k_terms_group<128>;
    # N = 129: the first k_terms_group<256>
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    ps = variants(mz.TERMS_ZOO["chain5"], 2, waypoints=waypoints)
    N = waypoints - 1
    assert ps[0].N == N and (ps[0].params.num_rollouts, ps[0].params.num_reused_rollouts) == (12, 5)
    g = TermsGroup(ps)
    line = terms_group_line(capfd.readouterr().err)
    assert f"k_terms_group<{128 if N <= 128 else 256}>, LDS {51 * N * 8} B, opt-in 0, engines with terms 2 of 2" in line, line
    g.close()
    run_in_chunks(ps, [(1, 2)])


def test_lds_opt_in_on_the_group_kernel(monkeypatch, capfd):
    # fork12_pedestal at N = 128: 120 doubles per waypoint, 122 880 B through the opt-in made on
    # k_terms_group<128> itself (this process may never have launched k_terms<128>)
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    ps = variants(mz.TERMS_ZOO["fork12_pedestal"], 2, waypoints=129)
    assert ps[0].N == 128 and mz.TERMS_LDS_ROWS["fork12_pedestal"] * 128 * 8 == 122880
    g = TermsGroup(ps)
    line = terms_group_line(capfd.readouterr().err)
    assert "k_terms_group<128>, LDS 122880 B, opt-in 1, engines with terms 2 of 2" in line, line
    oracles = [po.Oracle(p) for p in ps]
    g.group.run(1, 2)
    g.group.synchronize()
    advance(oracles, 1, 2)
    for i, (e, o) in enumerate(zip(g.engines, oracles)):
        assert_same(state(e), state(o), f"engine {i} against its oracle,")
    twins = twins_of(ps)
    for i, (e, t) in enumerate(zip(g.engines, twins)):
        t.run(1, 2)
        t.synchronize()
        assert_same(state(e), state(t), f"engine {i} against its own run,")
        t.close()
    g.close()


# ------------------------------------------------------------------------------------------------
# 5. engines created with the lean rollout layout

def test_group_on_lean_engines_with_terms(monkeypatch, capfd):
    monkeypatch.setenv("STOMP_DEBUG_LEAN", "1")
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    ps = variants(mz.TERMS_ZOO["chain5"], 2, K=260, Kr=0)
    g = TermsGroup(ps)
    err = capfd.readouterr().err
    models = [l for l in err.splitlines() if l.startswith("stomp: model ")]
    assert len(models) == 2 and all("lean 1 " in l and "lean slot loop" in l for l in models), err
    assert "engines with terms 2 of 2" in terms_group_line(err)
    oracles = [po.Oracle(p, threads=8) for p in ps]
    g.group.run(1, 2)
    g.group.synchronize()
    advance(oracles, 1, 2)
    for i, (e, o) in enumerate(zip(g.engines, oracles)):
        assert_same(state(e), state(o), f"engine {i} against its oracle,", oracle_skips(ps[i]))
    # a member's own run (the lean kernel and its own k_terms) continues the same iterations
    g.engines[1].run(3, 1)
    g.engines[1].synchronize()
    advance(oracles[1:], 3, 1)
    assert_same(state(g.engines[1]), state(oracles[1]), "engine 1 after its own run,", oracle_skips(ps[1]))
    g.close()


# ------------------------------------------------------------------------------------------------
# 6. stomp_group_optimize with a stop rule that depends on the constraints
# The 16 PR2 shelf problems of tests/test_gpu_group_reuse.py's recipe (default_rng(11), +-0.15 rad)
# with the reference's upright constraint on the gripper at the tolerances UPRIGHT_TOL; odd problems
# carry the torque term too (a mixed group).  GROUP_TERMS.md records the oracle's stop iterations.

# roll / pitch / yaw (yaw free, as in test/test_omp.cpp:76-91).  On these shelf problems the gripper is
# 2.0 .. 2.5 rad of roll away from upright: at 0.2 rad no trajectory ever satisfies the constraint (no
# problem stops before max_iterations), from 2.5 rad every one does; at 2.3 rad some problems' noiseless
# trajectories satisfy it and others' do not
UPRIGHT_TOL = (2.3, 2.3, 10.0)
LOOSE_TOL = (2.45, 2.45, 10.0)      # the same costs (no weight is zeroed below pi): only the gate differs
WIDE_TOL = (3.2, 3.2, 10.0)         # every tolerance >= pi: always satisfied, every weight zeroed


def upright(tol):
    return pb.OrientationConstraint("r_gripper_tool_frame", (0.0, 0.0, 0.0, 1.0), header_frame=True,
                                    absolute_roll_tolerance=tol[0], absolute_pitch_tolerance=tol[1],
                                    absolute_yaw_tolerance=tol[2], weight=1.0)


@functools.lru_cache(maxsize=None)
def recipe(tol=UPRIGHT_TOL, K=20, Kr=10, max_it=60, P=16):
    base = pb.make_problem(grid_n=64, num_rollouts=K, num_reused_rollouts=Kr)
    d = np.random.default_rng(11).uniform(-0.15, 0.15, (P, 2, base.J))
    return tuple(pb.make_problem(grid_n=64, num_rollouts=K, num_reused_rollouts=Kr, seed=base.seed + 1 + i,
                                 start=list(base.start + d[i, 0]), goal=list(base.goal + d[i, 1]),
                                 max_iterations=max_it, max_iterations_after_collision_free=2,
                                 orientation_constraints=[upright(tol)],
                                 torque_cost_weight=0.001 if i % 2 else 0.0) for i in range(P))


@functools.lru_cache(maxsize=None)
def pr2(idx, tol=UPRIGHT_TOL):
    """(problems, oracles after optimize, snapshots) of the recipe's problems `idx`; the snapshots are
    read-only and shared between the tests."""
    ps = [recipe(tol)[i] for i in idx]
    oracles, snaps = optimize_oracles(ps)
    for o, s in zip(oracles, snaps):
        s["torques"] = o.best_torques()
        s["torques"].setflags(write=False)
    return ps, oracles, snaps


ALL16 = tuple(range(16))


def assert_recipe(snaps, wide_snaps, loose_snaps):
    """On the oracles alone: (i) at least three distinct stop iterations, (ii) a stop before
    max_iterations, (iii) a problem whose stop moves when every tolerance is widened to >= pi; and,
    stricter, one whose stop moves at LOOSE_TOL, where the costs of every trajectory are the same and
    only constraints_satisfied differs."""
    its, wide, loose = iterations(snaps), iterations(wide_snaps), iterations(loose_snaps)
    print("stop iterations", its, "with tolerances >= pi", wide, "at", LOOSE_TOL, loose)
    assert len(set(its)) >= 3, its
    assert min(its) < 60, its
    assert any(a != b for a, b in zip(its, wide)), (its, wide)
    gated = [i for i in range(len(its)) if its[i] != loose[i]]
    assert gated, (its, loose)
    for i in gated:     # the same iterations up to the earlier stop
        n = min(its[i], loose[i])
        np.testing.assert_array_equal(snaps[i]["costs"][:n], loose_snaps[i]["costs"][:n])


def assert_terms_group(g, results, snaps):
    assert len(results) == len(snaps)
    for i, (e, res, snap) in enumerate(zip(g.engines, results, snaps)):
        assert_result(e, res, snap, f"engine {i}")
        np.testing.assert_array_equal(e.best_torques(), snap["torques"], err_msg=f"engine {i} best_torques")


def test_optimize_stop_rule_depends_on_the_constraints():
    ps, oracles, snaps = pr2(ALL16)
    _, _, wide_snaps = pr2(ALL16, WIDE_TOL)
    _, _, loose_snaps = pr2(ALL16, LOOSE_TOL)
    assert_recipe(snaps, wide_snaps, loose_snaps)        # before any engine is created
    g = TermsGroup(ps)
    results = g.group.optimize()
    assert_terms_group(g, results, snaps)
    # four engines against twins that ran their own stomp_engine_optimize: the earliest and the
    # latest early stop, one of the latest of all, and engine 0
    its = iterations(snaps)
    early = [i for i in range(16) if its[i] < 60]
    picks = sorted({0, min(early, key=lambda i: its[i]), max(early, key=lambda i: its[i]), its.index(max(its))})
    picks += [i for i in range(16) if i not in picks][: 4 - len(picks)]
    for i in picks:
        twin = eng.Engine(ps[i])
        tres = twin.optimize()
        assert_results_equal([results[i]], [tres], f"engine {i} against its twin")
        assert_same(state(g.engines[i], FULL), state(twin, FULL), f"engine {i} against its twin")
        np.testing.assert_array_equal(g.engines[i].best_torques(), twin.best_torques())
        twin.close()
    # the engines go on from where the loop left them (the restored reuse state shows here)
    for i in picks:
        o, e = oracles[i], g.engines[i]
        for it in (its[i] + 1, its[i] + 2):
            assert e.iterate(it) == o.iterate(it), (i, it)
            assert e.last_constraints_satisfied == o.last_constraints_satisfied, (i, it)
        assert_same(state(e), state(o), f"engine {i} two iterations on,")
    g.close()


# ------------------------------------------------------------------------------------------------
# 7. more optimize cases

@pytest.mark.parametrize("compact", [False, True])
def test_compaction_through_the_options(monkeypatch, compact):
    # the options decide, not the environment (set to the opposite)
    monkeypatch.setenv("STOMP_DEBUG_GROUP_COMPACT", "0" if compact else "1")
    ps, _, snaps = pr2(ALL16)
    g = TermsGroup(ps, compact=compact)
    g.engines[0].set_timing(True)
    results = g.group.optimize()
    print("compact", compact, "rollout launches", g.engines[0].timing("rollout_cost")[1], "terms launches",
          g.engines[0].timing("state_terms")[1])
    assert_terms_group(g, results, snaps)
    g.close()


def test_per_engine_caps():
    # engines whose own max_iterations ends them: their grouped flush and its terms launch run while
    # the others still iterate; never reusing, one reuse, and both sides of the chunk of 8
    caps = (1, 2, 7, 8, 9, 20)
    ps = variants(mz.TERMS_ZOO["chain5"], len(caps), max_iterations_after_collision_free=1000)
    assert (ps[0].params.num_rollouts, ps[0].params.num_reused_rollouts) == (12, 5)
    for p, c in zip(ps, caps):
        p.params.max_iterations = c
    oracles, snaps = optimize_oracles(ps)
    assert tuple(iterations(snaps)) == caps, iterations(snaps)
    g = TermsGroup(ps)
    results = g.group.optimize(costs_stride=20)
    for i, (e, res, snap, o) in enumerate(zip(g.engines, results, snaps, oracles)):
        assert_result(e, res, snap, f"engine {i}")
        assert_same(state(e), state(o), f"engine {i} against its oracle,")
        np.testing.assert_array_equal(e.best_torques(), o.best_torques(), err_msg=f"engine {i} best_torques")
    g.close()


def test_torque_only_optimize_with_best_torques():
    ps = variants(mz.TERMS_ZOO["chain5"], 3, constrained=False, max_iterations=12, max_iterations_after_collision_free=3)
    assert all(not p.orientation_constraints and p.params.torque_cost_weight == 0.001 for p in ps)
    oracles, snaps = optimize_oracles(ps)
    g, twins = TermsGroup(ps), twins_of(ps)
    results = g.group.optimize()
    tres = [t.optimize() for t in twins]
    assert_results_equal(results, tres, "torque only")
    for i, (e, t, o, res, snap) in enumerate(zip(g.engines, twins, oracles, results, snaps)):
        assert_result(e, res, snap, f"engine {i}")
        tq = o.best_torques()
        assert np.all(tq > 0.0)
        np.testing.assert_array_equal(e.best_torques(), tq, err_msg=f"engine {i} best_torques")
        np.testing.assert_array_equal(t.best_torques(), tq, err_msg=f"twin {i} best_torques")
        assert_same(state(e, FULL), state(t, FULL), f"engine {i} against its twin")
        t.close()
    g.close()


# ------------------------------------------------------------------------------------------------
# 8. launch count

def test_one_terms_launch_per_grouped_launch_not_one_per_engine():
    ps = variants(mz.TERMS_ZOO["chain5"], 4)
    g = TermsGroup(ps)
    g.engines[0].set_timing(True)
    g.group.run(1, 5)
    g.group.synchronize()
    terms, cost = g.engines[0].timing("state_terms")[1], g.engines[0].timing("rollout_cost")[1]
    print("terms launches", terms, "rollout launches", cost)
    # run(1, 5): five grouped rollout launches (the noiseless rollouts of 1 .. 4 ride in 2 .. 5), one
    # terms launch after each; synchronize: one grouped flush (iteration 5's) and its terms launch
    assert cost == 5
    assert terms == 5 + 1
    oracles = [po.Oracle(p) for p in ps]
    advance(oracles, 1, 5)
    for i, (e, o) in enumerate(zip(g.engines, oracles)):
        assert_same(state(e), state(o), f"engine {i}")
    g.close()


# ------------------------------------------------------------------------------------------------
# 9. lifecycle

def lifecycle_problems():
    return variants(mz.TERMS_ZOO["chain5"], 3, max_iterations=10, max_iterations_after_collision_free=2)


def test_lifecycle_a_members_own_iteration_puts_the_group_out_of_step():
    ps = lifecycle_problems()
    g, twins = TermsGroup(ps), twins_of(ps)
    g.group.run(1, 3)
    for t in twins:
        t.run(1, 3)
    assert g.engines[2].iterate(4) == twins[2].iterate(4)      # its own k_terms
    before = [state(e, FULL) for e in g.engines]
    with pytest.raises(RuntimeError) as ei:
        g.group.run(5, 2)
    assert "error -1" in str(ei.value) and "not at the same iteration state" in str(ei.value), str(ei.value)
    for i, (e, b) in enumerate(zip(g.engines, before)):   # no engine touched
        assert_same(state(e, FULL), b, f"engine {i}")
    # the others catch up with their own iterate, then the group runs again
    for i in (0, 1):
        assert g.engines[i].iterate(4) == twins[i].iterate(4)
    g.group.run(5, 2)
    g.group.synchronize()
    oracles = [po.Oracle(p) for p in ps]
    advance(oracles, 1, 6)
    for i, (t, o) in enumerate(zip(twins, oracles)):
        t.run(5, 2)
        t.synchronize()
        assert_same(state(g.engines[i]), state(o), f"engine {i} against its oracle,")
    assert_states_equal(g, twins, "after the group ran again")
    close_all(g, twins)


def test_lifecycle_optimize_then_run_and_optimize_twice():
    ps = lifecycle_problems()
    g, twins = TermsGroup(ps), twins_of(ps)
    g1 = g.group.optimize()
    g.group.run(11, 2)
    g.group.synchronize()
    g2 = g.group.optimize()
    t1 = [t.optimize() for t in twins]
    for t in twins:
        t.run(11, 2)
        t.synchronize()
    t2 = [t.optimize() for t in twins]
    assert_results_equal(g1, t1, "first optimize")
    assert_results_equal(g2, t2, "optimize, run, optimize")
    assert_states_equal(g, twins, "optimize, run, optimize")
    close_all(g, twins)


def test_lifecycle_set_theta_between_runs():
    ps = lifecycle_problems()
    g = TermsGroup(ps)
    oracles = [po.Oracle(p) for p in ps]
    g.group.run(1, 2)
    g.group.synchronize()
    advance(oracles, 1, 2)
    th = oracles[0].theta() + 0.01 * np.random.default_rng(9).standard_normal((ps[0].J, ps[0].N)).cumsum(axis=1)
    g.engines[0].set_theta(th)
    oracles[0].set_theta(th)
    g.group.run(3, 2)
    g.group.synchronize()
    advance(oracles, 3, 2)
    for i, (e, o) in enumerate(zip(g.engines, oracles)):
        assert_same(state(e), state(o), f"engine {i}")
    g.close()


# ------------------------------------------------------------------------------------------------
# 10. refusals with state_terms = 1

def assert_untouched(es, ps):
    for e, p in zip(es, ps):
        o = po.Oracle(p)
        assert e.iterate(1) == o.iterate(1)
        np.testing.assert_array_equal(e.theta(), o.theta())


def test_refuses_cumulative_costs_with_state_terms():
    ps = variants(mz.TERMS_ZOO["chain5"], 2, use_cumulative_costs=True)
    s = eng.Stream()
    es = [eng.Engine(p, stream=s.ptr) for p in ps]
    with pytest.raises(RuntimeError) as ei:
        eng.EngineGroup(es, state_terms=True)
    assert "error -3" in str(ei.value) and "cumulative costs" in str(ei.value), str(ei.value)
    assert_untouched(es, ps)
    for e in es:
        e.close()
    s.close()


def test_refuses_more_than_16_joints_with_state_terms():
    ps = variants(mz.TERMS_ZOO["chain17"], 2)
    assert ps[0].J == 17
    s = eng.Stream()
    es = [eng.Engine(p, stream=s.ptr) for p in ps]
    with pytest.raises(RuntimeError) as ei:
        eng.EngineGroup(es, state_terms=True)
    assert "error -3" in str(ei.value), str(ei.value)
    assert_untouched(es, ps)
    # a valid group with terms on the same stream works
    qs = variants(mz.TERMS_ZOO["chain5"], 2)
    fs = [eng.Engine(q, stream=s.ptr) for q in qs]
    g = eng.EngineGroup(fs, state_terms=True)
    g.run(1, 3)
    g.synchronize()
    oracles = [po.Oracle(q) for q in qs]
    advance(oracles, 1, 3)
    for i, (e, o) in enumerate(zip(fs, oracles)):
        assert_same(state(e), state(o), f"engine {i} of the next group")
    g.close()
    for e in fs + es:
        e.close()
    s.close()


def test_wrong_struct_size_and_null_options_are_invalid():
    ps = variants(mz.TERMS_ZOO["chain5"], 2)
    s = eng.Stream()
    es = [eng.Engine(p, stream=s.ptr) for p in ps]
    l = eng.load_library()
    arr = (C.c_void_p * 2)(*[e.h.value for e in es])
    h = C.c_void_p()
    opt = eng.stomp_group_options(C.sizeof(eng.stomp_group_options) + 4, 1, -1)
    assert l.stomp_group_create_with(arr, 2, C.byref(opt), C.byref(h)) == -1 and not h.value
    assert b"struct_size" in l.stomp_last_error()
    assert l.stomp_group_create_with(arr, 2, None, C.byref(h)) == -1 and not h.value
    # and the plain entry point still refuses these engines with its old message
    with pytest.raises(RuntimeError) as ei:
        eng.EngineGroup(es)
    assert "error -3" in str(ei.value) and "without state-cost terms or cumulative costs" in str(ei.value), str(ei.value)
    g = eng.EngineGroup(es, state_terms=True)
    g.run(1, 1)
    g.synchronize()
    oracles = [po.Oracle(p) for p in ps]
    advance(oracles, 1, 1)
    for i, (e, o) in enumerate(zip(es, oracles)):
        assert_same(state(e), state(o), f"engine {i}")
    g.close()
    for e in es:
        e.close()
    s.close()


# ------------------------------------------------------------------------------------------------
# 11. struct layout (the method of tests/test_abi.py::test_struct_layouts_match_c)

def test_group_options_layout_matches_c(tmp_path):
    name, cls = "stomp_group_options", eng.stomp_group_options
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stomp_engine.h"', "int main(void){",
             f'printf("{name} %zu\\n", sizeof({name}));']
    for field, _ in cls._fields_:
        lines.append(f'printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(l.rsplit(" ", 1) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out[name]) == C.sizeof(cls) == 12
    for field, _ in cls._fields_:
        assert int(out[f"{name}.{field}"]) == getattr(cls, field).offset, field
