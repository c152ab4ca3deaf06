"""GPU: engine groups (stomp_group_run) -- a batch of independent planning problems (BASELINE
cfg5: distinct start / goal / seed, one robot and distance field) advanced by shared launches.
Every engine of a group must end exactly where its own stomp_engine_run leaves it, and where
the CPU oracle of its problem is after the same iterations, bit for bit.  The second half of the
file takes groups beyond that fixture: other K, N, robots, per-engine robots and fields, the bricked
layout, lean engines and the lifecycle of a group (tests/GROUPS_AND_TILES.md)."""
import numpy as np
import pytest

from stomp_motion_planner_icra2011_amd import engine as eng
from stomp_motion_planner_icra2011_amd import problem as pb
from oracle import pyoracle as po
from tests import model_zoo as mz
from tests.group_util import FIELDS, Group, advance, assert_same, shelf_problems, state, variants

pytestmark = pytest.mark.gpu


def problems(P, K=64, grid=64):
    return shelf_problems(P, K, 0, grid)


@pytest.mark.parametrize("P,chunks", [(3, [(1, 4), (5, 3)]), (8, [(1, 6)])])
def test_group_matches_single_engines_and_oracles(P, chunks):
    ps = problems(P)
    s = eng.Stream()
    grp_engines = [eng.Engine(p, stream=s.ptr) for p in ps]
    group = eng.EngineGroup(grp_engines)
    for first, count in chunks:
        group.run(first, count)
    group.synchronize()
    total = sum(c for _, c in chunks)
    for p, ge in zip(ps, grp_engines):
        se = eng.Engine(p)
        for first, count in chunks:
            se.run(first, count)
        se.synchronize()
        o = po.Oracle(p)
        for it in range(1, total + 1):
            o.iterate(it)
        a = state(ge, FIELDS)
        assert_same(a, state(se, FIELDS), "against its own run,")
        np.testing.assert_array_equal(a["theta"], o.theta())
        np.testing.assert_array_equal(a["last"], o.last_trajectory())
        np.testing.assert_array_equal(a["prob"], o.rollouts("probabilities"))
        se.close()
    group.close()
    for e in grp_engines:
        e.close()
    s.close()


def test_group_then_own_calls():
    # an engine's own iterate after group runs continues the same trajectory of iterations
    ps = problems(2)
    s = eng.Stream()
    es = [eng.Engine(p, stream=s.ptr) for p in ps]
    g = eng.EngineGroup(es)
    g.run(1, 3)
    g.synchronize()
    c, cf = es[1].iterate(4)
    o = po.Oracle(ps[1])
    for it in range(1, 4):
        o.iterate(it)
    oc, ocf = o.iterate(4)
    assert c == oc and cf == ocf
    np.testing.assert_array_equal(es[1].theta(), o.theta())
    g.close()


def test_group_refusals():
    ps = problems(2)
    a = eng.Engine(ps[0])
    b = eng.Engine(ps[1])   # own streams: refused
    with pytest.raises(RuntimeError):
        eng.EngineGroup([a, b])
    s = eng.Stream()
    reuse = pb.make_problem(grid_n=64, num_rollouts=64, num_reused_rollouts=8)
    c = eng.Engine(ps[0], stream=s.ptr)
    d = eng.Engine(reuse, stream=s.ptr)
    with pytest.raises(RuntimeError):
        eng.EngineGroup([c, d])


# ------------------------------------------------------------------------------------------------
# Groups beyond the PR2 fixture (tests/GROUPS_AND_TILES.md): every weights tile launch_weights_group
# can pick, update_body's ring over N, the bricked rollout kernel at both block widths, other robots,
# engines with their own robots, fields and parameters, and the lifecycle of a group.

# K -> the kernel of launch_weights_group (a group takes the row tiles at every K)
GROUP_WEIGHTS = {12: "rows<256,8,4>", 20: "rows<256,8,4>", 65: "rows<256,8,4>", 128: "rows<256,8,4>",
                 129: "rows<256,4,4>", 257: "rows<512,4,4>", 513: "rows<512,4,8>", 1025: "rows<256,4,32>"}


def group_line(capfd):
    err = capfd.readouterr().err
    lines = [l for l in err.splitlines() if l.startswith("stomp: group ")]
    assert lines, err
    return lines[-1]


def assert_against_oracles(engines, oracles):
    for i, (e, o) in enumerate(zip(engines, oracles)):
        assert_same(state(e, FIELDS), state(o, FIELDS), f"engine {i}")


def assert_members(ps, engines, chunks, threads=1, oracles=None):
    """Every engine against its own single-engine run of the same chunks and its own oracle after
    the same iterations, every field bit for bit."""
    total = sum(c for _, c in chunks)
    for i, (p, ge) in enumerate(zip(ps, engines)):
        se = eng.Engine(p)
        for first, count in chunks:
            se.run(first, count)
        se.synchronize()
        a = state(ge, FIELDS)
        assert_same(a, state(se, FIELDS), f"engine {i} against its own run,")
        se.close()
        if oracles is None:
            o = po.Oracle(p, threads=threads)
            for it in range(1, total + 1):
                o.iterate(it)
        else:
            o = oracles[i]
        assert_same(a, state(o, FIELDS), f"engine {i} against its oracle,")


def run_group(ps, chunks, threads=1):
    g = Group(ps)
    for first, count in chunks:
        g.group.run(first, count)
    g.group.synchronize()
    assert_members(ps, g.engines, chunks, threads)
    g.close()


@pytest.mark.parametrize("K", [12, 65, 128, 129, 257, 513, 1025])
def test_group_weights_tiles_at_k_edges(monkeypatch, capfd, K):
    # chain5 at N = 39: 195 flat columns, a ragged last tile at eight and at four columns; three
    # engines of K + 1 rollouts: 39 .. 387 workgroups at K <= 128 (both block widths of
    # k_rollout_group around the 256 compute units), slot loops above
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    ps = variants(mz.chain5, 3, K=K, Kr=0, waypoints=40)
    chunks = [(1, 2), (3, 1)]
    g = Group(ps)
    line = group_line(capfd)
    assert line.endswith(f"weights {GROUP_WEIGHTS[K]}") and f"of 3 engines J 5 N 39 K {K} " in line, line
    for first, count in chunks:
        g.group.run(first, count)
    g.group.synchronize()
    assert_members(ps, g.engines, chunks, threads=8)
    g.close()


@pytest.mark.parametrize("waypoints", [10, 41, 65, 66, 129, 256, 257])
def test_group_update_ring_over_n(waypoints):
    # update_body (k_update_group alone runs it): N = 9 .. 256, both sides of a wave, of two and of
    # the full 256 lanes; its ring reads kUpdateBatch rows ahead of N.  chain5 at every N (its
    # rollout workgroup takes 67 KB of LDS at N = 256: creation refuses none)
    ps = variants(mz.chain5, 2, K=20, Kr=0, waypoints=waypoints)
    assert ps[0].N == waypoints - 1
    run_group(ps, [(1, 2), (3, 1)])


@pytest.mark.parametrize("name", ["stick1", "chain5", "hand9", "fork12", "fork13"])
def test_group_of_zoo_robots(name):
    run_group(variants(mz.ZOO[name], 3, K=20, Kr=0), [(1, 2), (3, 1)])


def test_group_refuses_more_than_16_joints():
    ps = variants(mz.chain17, 2, K=20, Kr=0)
    s = eng.Stream()
    es = [eng.Engine(p, stream=s.ptr) for p in ps]
    with pytest.raises(RuntimeError) as ei:
        eng.EngineGroup(es)
    assert "error -3" in str(ei.value), str(ei.value)      # STOMP_E_UNSUPPORTED
    # the engines are untouched, and the next group on the same stream works
    qs = variants(mz.chain5, 2, K=20, Kr=0)
    fs = [eng.Engine(q, stream=s.ptr) for q in qs]
    g = eng.EngineGroup(fs)
    g.run(1, 2)
    g.synchronize()
    assert_members(qs, fs, [(1, 2)])
    o = po.Oracle(ps[0])
    assert es[0].iterate(1) == o.iterate(1)
    np.testing.assert_array_equal(es[0].theta(), o.theta())
    g.close()


def test_group_of_two_robots_of_one_structure():
    # the same tree with other rotations, axes, offsets, radii and limits: J, N, K, S and the LDS
    # size agree, so creation accepts them; each engine plans for its own robot
    a, b = mz.chain5(K=20, Kr=0), mz.chain5(K=20, Kr=0, robot_seed=205)
    c = mz.chain5(K=20, Kr=0, robot_seed=305)
    assert (a.J, a.N, len(a.spheres)) == (b.J, b.N, len(b.spheres)) == (c.J, c.N, len(c.spheres))
    assert a.robot.segments[1].rot != b.robot.segments[1].rot and a.spheres[0].radius != b.spheres[0].radius
    assert not np.array_equal(a.sdf, b.sdf)
    run_group([a, b, c], [(1, 2), (3, 1)])


SCENE_SHAPES = (None, mz.NONCUBIC, mz.NONCUBIC_PERM)


def scenes(K):
    """chain5 in three scenes: fields of different shapes, origins (by whole and by fractions of a
    cell, so no engine's lookups are right in another's grid) and obstacles, and each engine's
    own noise_stddev and obstacle_cost_weight."""
    out = []
    for i, shape in enumerate(SCENE_SHAPES):
        p = mz.chain5(K=K, Kr=0, shape=shape, noise_stddev=(2.0, 1.1, 0.6)[i], obstacle_cost_weight=(2.5, 1.0, 4.0)[i])
        g = p.grid
        origin = tuple(o - d for o, d in zip(g.origin, ((0.0, 0.0, 0.0), (0.07, 0.01, 0.03), (0.013, 0.05, 0.0))[i]))
        p.grid = pb.Grid(g.n, origin, g.resolution, g.max_expansion, shape=g.shape)
        p.boxes = list(p.boxes) + [pb.Box((0.05 + 0.1 * i, -0.55 + 0.05 * i, 0.3 + 0.1 * i), (0.1, 0.08, 0.06 + 0.03 * i))]
        p.sdf = pb.build_sdf(p.grid, p.boxes, [])
        p.seed = p.seed + 11 * i
        out.append(p)
    assert len({q.sdf.shape for q in out}) == 3 and len({q.grid.origin[0] for q in out}) == 3
    return out


@pytest.mark.parametrize("K", [20, 100])
@pytest.mark.parametrize("layout", ["linear", "brick"])
def test_group_of_engines_with_their_own_scenes(monkeypatch, capfd, layout, K):
    # 3 (K + 1) = 63 workgroups (the wide block of k_rollout_group) and 303 (more than the compute
    # units: the narrow one); brick: k_rollout_group<*, BRICK = true>, with padding bricks along
    # the axis of 66 cells
    monkeypatch.setenv("STOMP_SDF_LAYOUT", layout)
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    ps = scenes(K)
    for p in ps:     # every scene matters to its engine: the default trajectory touches obstacles
        c = mz.census(p, po.Oracle(p).theta()[None])
        assert c["collision"] >= 1 and c["hinge"] >= 1, c
    g = Group(ps)
    assert f" brick {int(layout == 'brick')}," in group_line(capfd)
    chunks = [(1, 2), (3, 1)]
    for first, count in chunks:
        g.group.run(first, count)
    g.group.synchronize()
    assert_members(ps, g.engines, chunks, threads=8)
    g.close()


def test_group_on_lean_engines_then_own_lean_run(monkeypatch, capfd):
    # engines created with the LDS-lean slot-loop layout (hand9 has a saved frame: sv_glob is
    # allocated); the group runs its full-layout body on them, then a member's own run (the lean
    # kernel) continues the same iterations
    monkeypatch.setenv("STOMP_DEBUG_LEAN", "1")
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    ps = variants(mz.hand9, 2, K=260, Kr=0)
    g = Group(ps)
    err = capfd.readouterr().err
    models = [l for l in err.splitlines() if l.startswith("stomp: model ")]
    assert len(models) == 2 and all("lean 1 " in l and "lean slot loop" in l for l in models), err
    assert "weights rows<512,4,4>" in [l for l in err.splitlines() if l.startswith("stomp: group ")][-1]
    g.group.run(1, 2)
    g.group.synchronize()
    oracles = [po.Oracle(p, threads=8) for p in ps]
    advance(oracles, 1, 2)
    assert_against_oracles(g.engines, oracles)
    g.engines[1].run(3, 1)
    g.engines[1].synchronize()
    advance(oracles[1:], 3, 1)
    assert_against_oracles(g.engines[1:], oracles[1:])
    g.close()


def test_group_lifecycle_empty_calls_and_growing_runs():
    ps = variants(mz.chain5, 3, K=20, Kr=0)
    g = Group(ps)
    oracles = [po.Oracle(p) for p in ps]
    g.group.synchronize()                   # before any run: nothing staged, nothing pending
    g.group.run(1, 0)                       # count = 0
    g.group.synchronize()
    for e, o in zip(g.engines, oracles):
        np.testing.assert_array_equal(e.theta(), o.theta())
    # the argument buffers of a 2-iteration run, then of a 9-iteration run with no synchronize
    # between them: both regrow while the first run's launches may still read the old ones
    g.group.run(1, 2)
    g.group.run(3, 9)
    g.group.synchronize()
    advance(oracles, 1, 11)
    assert_against_oracles(g.engines, oracles)
    assert_members(ps, g.engines, [(1, 2), (3, 9)], oracles=oracles)
    g.close()


def test_group_after_the_engines_own_runs():
    # every engine advanced by its own run first (the pregen rows of iteration 3 are its own: no
    # pregen_first launch), then a group run from 3
    ps = variants(mz.chain5, 3, K=20, Kr=0)
    g = Group(ps)
    for e in g.engines:
        e.run(1, 2)
    g.group.run(3, 2)
    g.group.synchronize()
    assert_members(ps, g.engines, [(1, 2), (3, 2)])
    g.close()


def test_group_refuses_engines_out_of_step():
    ps = variants(mz.chain5, 3, K=20, Kr=0)
    g = Group(ps)
    oracles = [po.Oracle(p) for p in ps]
    assert g.engines[1].iterate(1) == oracles[1].iterate(1)
    before = [e.theta() for e in g.engines]
    with pytest.raises(RuntimeError) as ei:
        g.group.run(1, 2)
    assert "error -1" in str(ei.value) and "not at the same iteration state" in str(ei.value), str(ei.value)
    for e, th in zip(g.engines, before):
        np.testing.assert_array_equal(e.theta(), th)
    # the others levelled by their own iterate: the group runs from 2
    for i in (0, 2):
        assert g.engines[i].iterate(1) == oracles[i].iterate(1)
    g.group.run(2, 2)
    g.group.synchronize()
    advance(oracles, 2, 2)
    assert_against_oracles(g.engines, oracles)
    g.close()


def test_group_members_own_calls_between_runs():
    # after a synchronize, set_theta on one member (and on its oracle) and an execute on another,
    # then a further group run
    ps = variants(mz.chain5, 3, K=20, Kr=0)
    g = Group(ps)
    oracles = [po.Oracle(p) for p in ps]
    g.group.run(1, 2)
    g.group.synchronize()
    advance(oracles, 1, 2)
    th = oracles[0].theta() + 0.01 * np.random.default_rng(9).standard_normal((ps[0].J, ps[0].N)).cumsum(axis=1)
    g.engines[0].set_theta(th)
    oracles[0].set_theta(th)
    rows = mz.execute_rows(ps[2], oracles[2].theta(), rows=3)
    costs, cf, traj = g.engines[2].execute(rows, iteration_member=1)
    for r in range(len(rows)):
        oc, ocf, otr = oracles[2].execute(rows[r], iteration_member=1)
        np.testing.assert_array_equal(costs[r], oc)
        np.testing.assert_array_equal(traj[r], otr)
        assert bool(cf[r]) == ocf
    g.group.run(3, 2)
    g.group.synchronize()
    advance(oracles, 3, 2)
    assert_against_oracles(g.engines, oracles)
    g.close()
