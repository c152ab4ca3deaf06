"""GPU: engine groups with cumulative costs (use_cumulative_costs, the reference's default:
computeRolloutCumulativeCosts' suffix sums, policy_improvement.cpp:308-316) -- groups created with
cumulative_costs=True (stomp_group_create_flags) over engines that weight their rollouts by the
cost-to-go.  One launch per iteration (k_cumulative_group) makes the [K][J][N] cumulative rows of
every engine of the group before the grouped weights read them.  Every engine must end exactly
where its own stomp_engine_run / stomp_engine_optimize leaves it and where the CPU oracle of its
problem is, bit for bit; its cumulative rows (Engine.rollouts("cumulative_costs"), the only direct
view of the new kernel's output) must equal a twin engine's and numpy's sequential recomputation
from the engine's own state and control costs.  tests/GROUP_CUMULATIVE.md lists the cases.

Without the feature EngineGroup has no cumulative_costs argument and every group made here is
refused (error -3)."""
import functools

import numpy as np
import pytest

from stomp_motion_planner_icra2011_amd import engine as eng
from oracle import pyoracle as po
from tests import model_zoo as mz
from tests import group_util as gu
from tests.group_util import (CHUNKS, FIELDS, X_ROWS, advance, assert_group, assert_same, assert_spread, assert_twin,
                              iterations, optimize_oracles, oracle_skips, shelf_problems, variants)

pytestmark = pytest.mark.gpu

ROWS = FIELDS + ("control",)


def Group(ps, state_terms=False, compact=None):
    """Engines of `ps` on one stream and their group, created accepting cumulative costs."""
    return gu.Group(ps, state_terms=state_terms, compact=compact, cumulative_costs=True)


def state(x, reuse):
    """theta, the FIELDS rows and the control costs of an engine or an oracle; with K_r > 0 also the
    extra rollout's rows."""
    return gu.state(x, ROWS + X_ROWS if reuse else ROWS)


def numpy_cumulative(e):
    """The two loops of computeRolloutCumulativeCosts in float64 on the engine's own rows: one add
    per element, then the suffix sums t = N - 2 .. 0, sequential in t."""
    st, ct = e.rollouts("state_costs"), e.rollouts("control_costs")
    c = st[:, None, :] + ct
    for t in range(c.shape[2] - 2, -1, -1):
        c[:, :, t] += c[:, :, t + 1]
    return c


def assert_cumulative(e, twin, tag):
    """The engine's cumulative rows against a twin's (None: skipped) and against numpy."""
    cum = e.rollouts("cumulative_costs")
    assert cum.shape == (e.K_loc, e.J, e.N) and np.isfinite(cum).all(), tag
    if twin is not None:
        np.testing.assert_array_equal(cum, twin.rollouts("cumulative_costs"), err_msg=f"{tag} cumulative, twin")
    np.testing.assert_array_equal(cum, numpy_cumulative(e), err_msg=f"{tag} cumulative, numpy")


def cumulative(p):
    return bool(p.params.use_cumulative_costs)


def run_in_chunks(ps, chunks=CHUNKS, threads=1, state_terms=False):
    """gu.run_in_chunks, and the cumulative rows of the engines that have them against the twin's
    and numpy's."""
    def cumulative_rows(p, ge, te, tag):
        if cumulative(p):
            assert_cumulative(ge, te, tag)
    return gu.run_in_chunks(ps, chunks, threads, lambda qs: Group(qs, state_terms=state_terms), oracle_skips,
                            cumulative_rows)


def shelf(P, K, Kr, grid=64, **kw):
    """The PR2 shelf problems of the run tests, with cumulative costs."""
    return shelf_problems(P, K, Kr, grid, use_cumulative_costs=True, **kw)


# ------------------------------------------------------------------------------------------------
# 1. stomp_group_run in chunks

@pytest.mark.parametrize("K,Kr", [(20, 10), (12, 0), (12, 11), (65, 8)])
def test_run_matches_single_engines_and_oracles(K, Kr):
    # J = 7, N = 99: K J = 140, 84, 84, 455 rows in slabs of 32 -- a partial last slab every time
    # (455 = 14 x 32 + 7); K = 65: a second canonical 64-block in the weights
    ps = shelf(3, K, Kr)
    assert all(cumulative(p) for p in ps) and (ps[0].J, ps[0].N) == (7, 99)
    run_in_chunks(ps, threads=8 if K > 20 else 1).close()


# ------------------------------------------------------------------------------------------------
# 2. kernel shapes

@pytest.mark.parametrize("name", ["stick1", "chain5", "hand9", "fork12", "fork13"])
def test_kernel_shapes_over_joints(name):
    # K = 12: K J = 12 (less than one slab), 60, 108, 144, 156 rows
    ps = variants(mz.ZOO[name], 3, use_cumulative_costs=True)
    assert (ps[0].params.num_rollouts, ps[0].params.num_reused_rollouts) == (12, 5)
    assert 12 * ps[0].J == dict(stick1=12, chain5=60, hand9=108, fork12=144, fork13=156)[name]
    run_in_chunks(ps).close()


@pytest.mark.parametrize("waypoints,Kr", [(10, 5), (66, 5), (129, 5), (130, 5), (200, 5), (257, 0)])
def test_kernel_shapes_over_time_steps(monkeypatch, capfd, waypoints, Kr):
    # chain5 at N = 9, 65 (odd: the pitch is N), 128 (even: pitch N + 1; the last N of the 32-row
    # instantiation), 129 (the first of the 16-row one), 199 and the limit 256.  The reused rows'
    # kernel of groups is exercised up to N = 199 by tests/test_gpu_group_reuse.py, so N = 256 runs
    # at K_r = 0
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    ps = variants(mz.chain5, 3, Kr=Kr, waypoints=waypoints, use_cumulative_costs=True)
    N = waypoints - 1
    assert ps[0].N == N and ps[0].params.num_rollouts == 12
    g = run_in_chunks(ps)
    lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("stomp: group cumulative ")]
    rows = 32 if N <= 128 else 16
    assert lines and f"k_cumulative_group<{rows}>, rows per workgroup {rows}, LDS {rows * (N | 1) * 8} B" in lines[0], lines
    g.close()


# ------------------------------------------------------------------------------------------------
# 3. mixed groups, 4. with state terms

def test_mixed_group():
    ps = variants(mz.chain5, 4)
    for i in (0, 2):
        ps[i].params.use_cumulative_costs = True
    assert [cumulative(p) for p in ps] == [True, False, True, False] and ps[0].params.num_reused_rollouts == 5
    g = run_in_chunks(ps)     # engines 1 and 3 against their twins and oracles too
    with pytest.raises(RuntimeError) as ei:
        g.engines[1].rollouts("cumulative_costs")
    assert "error -1" in str(ei.value) and "use_cumulative_costs" in str(ei.value), str(ei.value)
    g.close()


def test_with_state_terms():
    ps = variants(mz.TERMS_ZOO["chain5"], 2, use_cumulative_costs=True)
    assert all(cumulative(p) and p.params.torque_cost_weight > 1e-9 and p.orientation_constraints for p in ps)
    run_in_chunks(ps, chunks=[(1, 3)], threads=8, state_terms=True).close()


# ------------------------------------------------------------------------------------------------
# 5. stomp_group_optimize

def freeze(d):
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def recipe(K=20, Kr=10, mixed=False):
    """tests/test_gpu_group_reuse.py's 16-problem recipe with cumulative costs (mixed: on for the even
    indices only); shared between the tests, never written."""
    ps = shelf_problems(16, K, Kr, rng_seed=11, max_iterations=60, max_iterations_after_collision_free=2,
                        use_cumulative_costs=True)
    for p in ps[1::2] if mixed else ():
        p.params.use_cumulative_costs = False
    return tuple(ps)


@functools.lru_cache(maxsize=None)
def pr2(K, Kr, mixed=False):
    """(problems, oracles after optimize, snapshots, the oracles' rows after optimize) of the recipe.
    Snapshots and rows are the shared reference, never written; the oracle objects are continued by
    one test only."""
    ps = list(recipe(K, Kr, mixed))
    oracles, snaps = optimize_oracles(ps)
    rows = [freeze(state(o, Kr > 0)) for o in oracles]
    return ps, oracles, snaps, rows


def assert_stops_spread(snaps):
    """On the oracle's own counts, before the group runs: at least four distinct stops below 60, an
    engine that runs out its 60 iterations, stops at both parities."""
    assert_spread(snaps, 60)
    its = iterations(snaps)
    assert {n % 2 for n in its} == {0, 1}, its


def rows_defined(Kr, its, i):
    """The rollout rows of engine i after the loop are those of the iteration it stopped at: with
    K_r > 0 always (the rollout launch of the iteration after the stop wrote the other row set);
    with K_r = 0 only for an engine that ran out its iterations (the step after its last is the
    flush alone -- an early stop is decided after the next iteration's rows were generated)."""
    return Kr > 0 or its[i] == 60


def assert_optimized(g, results, snaps, rows, Kr):
    assert_group(g, results, snaps)     # stats, cost history, best / last trajectory, theta
    its = iterations(snaps)
    for i, (p, e) in enumerate(zip(g.ps, g.engines)):
        if not rows_defined(Kr, its, i):
            continue
        assert_same(state(e, Kr > 0), rows[i], f"engine {i} against its oracle,")
        if cumulative(p):
            assert_cumulative(e, None, f"engine {i}")


def continue_against_oracle(o, e, first, count, reuse):
    for it in range(first, first + count):
        oc, ec = o.iterate(it), e.iterate(it)
        assert ec[0] == oc[0] and ec[1] == oc[1], (it, ec, oc)
        assert_same(state(e, reuse), state(o, reuse), f"iteration {it}")
        assert_cumulative(e, None, f"iteration {it}")


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("K,Kr", [(20, 10), (32, 0)])
def test_optimize_stops_spread(K, Kr, compact):
    ps, oracles, snaps, rows = pr2(K, Kr)
    assert_stops_spread(snaps)
    g = Group(ps, compact=compact)
    results = g.group.optimize()
    assert_optimized(g, results, snaps, rows, Kr)
    if compact:
        g.close()
        return
    # four engines against twins that ran their own stomp_engine_optimize: the earliest and the
    # latest early stop, one that ran out its iterations, engine 0
    its = iterations(snaps)
    early = [i for i in range(16) if its[i] < 60]
    first, last = min(early, key=lambda i: its[i]), max(early, key=lambda i: its[i])
    picks = sorted({0, first, last, its.index(60)})
    picks += [i for i in range(16) if i not in picks][: 4 - len(picks)]
    for i in picks:
        twin = eng.Engine(ps[i])
        tres = twin.optimize()
        tag = f"engine {i} against its twin"
        assert_twin(g.engines[i], results[i], twin, tres, tag)
        assert_same(state(g.engines[i], Kr > 0), state(twin, Kr > 0), tag)
        np.testing.assert_array_equal(g.engines[i].rollouts("cumulative_costs"), twin.rollouts("cumulative_costs"),
                                      err_msg=tag + " cumulative")
        twin.close()
    # a wrongly restored reuse state, or cumulative rows of a wrong iteration, show here
    for i in (first, its.index(60)):
        continue_against_oracle(oracles[i], g.engines[i], its[i] + 1, 3, Kr > 0)
    g.close()


def test_optimize_mixed_group_with_compaction():
    ps, _, snaps, rows = pr2(20, 10, mixed=True)
    assert [cumulative(p) for p in ps] == [i % 2 == 0 for i in range(16)]
    assert_stops_spread(snaps)
    g = Group(ps, compact=True)
    assert_optimized(g, g.group.optimize(), snaps, rows, 10)
    g.close()


# ------------------------------------------------------------------------------------------------
# 6. refusals and unchanged paths

def assert_untouched_then_grouped(s, es, ps):
    """After a refused creation: the engines still match their oracles on iterate(1), and a valid
    cumulative group on the same stream works."""
    for e, p in zip(es, ps):
        o = po.Oracle(p)
        assert e.iterate(1) == o.iterate(1)
        np.testing.assert_array_equal(e.theta(), o.theta())
    qs = variants(mz.chain5, 2, use_cumulative_costs=True)
    fs = [eng.Engine(q, stream=s.ptr) for q in qs]
    g = eng.EngineGroup(fs, cumulative_costs=True)
    g.run(1, 3)
    g.synchronize()
    oracles = [po.Oracle(q) for q in qs]
    advance(oracles, 1, 3)
    for i, (e, o) in enumerate(zip(fs, oracles)):
        assert_same(state(e, True), state(o, True), f"engine {i} of the next group")
        assert_cumulative(e, None, f"engine {i} of the next group")
    g.close()
    for e in fs + list(es):
        e.close()


def test_still_refuses_more_than_16_joints():
    ps = variants(mz.chain17, 2, use_cumulative_costs=True)
    s = eng.Stream()
    es = [eng.Engine(p, stream=s.ptr) for p in ps]
    with pytest.raises(RuntimeError) as ei:
        eng.EngineGroup(es, cumulative_costs=True)
    assert "error -3" in str(ei.value), str(ei.value)      # STOMP_E_UNSUPPORTED
    assert_untouched_then_grouped(s, es, ps)
    s.close()


def test_still_refuses_engines_of_two_reuse_counts():
    ps = [mz.chain5(Kr=5, use_cumulative_costs=True), mz.chain5(Kr=4, use_cumulative_costs=True)]
    s = eng.Stream()
    es = [eng.Engine(p, stream=s.ptr) for p in ps]
    with pytest.raises(RuntimeError) as ei:
        eng.EngineGroup(es, cumulative_costs=True)
    assert "error -1" in str(ei.value), str(ei.value)      # STOMP_E_INVALID: one shape
    assert_untouched_then_grouped(s, es, ps)
    s.close()


@pytest.mark.parametrize("state_terms", [False, True])
def test_the_other_entry_points_still_refuse_cumulative_engines(state_terms):
    ps = variants(mz.chain5, 2, use_cumulative_costs=True)
    s = eng.Stream()
    es = [eng.Engine(p, stream=s.ptr) for p in ps]
    with pytest.raises(RuntimeError) as ei:
        eng.EngineGroup(es, state_terms=True) if state_terms else eng.EngineGroup(es)
    assert "error -3" in str(ei.value) and "cumulative costs" in str(ei.value), str(ei.value)
    assert_untouched_then_grouped(s, es, ps)
    s.close()


# ------------------------------------------------------------------------------------------------
# 7. timing

def test_the_cumulative_launch_shares_the_weights_scope():
    ps = shelf(4, 20, 10)
    g = Group(ps)
    g.engines[0].set_timing(True)
    g.group.run(1, 5)
    g.group.synchronize()
    weights, cost = g.engines[0].timing("weights")[1], g.engines[0].timing("rollout_cost")[1]
    print("weights launches", weights, "rollout launches", cost)
    assert weights == 5 and cost == 5     # one per iteration, as the single engine counts
    oracles = [po.Oracle(p) for p in ps]
    advance(oracles, 1, 5)
    for i, (e, o) in enumerate(zip(g.engines, oracles)):
        assert_same(state(e, True), state(o, True), f"engine {i}")
        assert_cumulative(e, None, f"engine {i}")
    g.close()
