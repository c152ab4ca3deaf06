"""GPU: stomp_engine_query_gradients (Engine.query_gradients) -- per sphere the field gradient and the
potential's gradient, per link and per state the cost and its joint-space gradient -J^T g, of a
batch of joint states against the engine's current model and field.  Every array is compared with
assert_array_equal against the restatement of tests/gradient_query_util.py (the CPU probes
ChompRef.sphere_positions / field_gradient / jacobian and Oracle.potential, and sequential Python
float loops), and, independently of that restatement, against Engine.query_states and the arrays of a
Chomp.reset on the same engine.  tests/GRADIENT_QUERY.md lists the cases.

Every case first asserts its census on the CPU reference alone (gradient_query_util.assert_census).

Without the feature Engine has no query_gradients: every case fails."""
import dataclasses

import numpy as np
import pytest

from stomp_motion_planner_icra2011_amd import engine as eng
from stomp_motion_planner_icra2011_amd import problem as pb
from tests import gradient_query_util as gqu
from tests import model_zoo as mz
from tests import state_query_util as squ
from tests.group_util import Group
from tests.test_gpu_request_model import attach

pytestmark = pytest.mark.gpu

ALL = gqu.OUTPUTS
ZERO = (0.0, 0.0, 0.0)


def assert_equal(got, ref, names=ALL, tag="", rows=None):
    for k in names:
        a, b = getattr(got, k), getattr(ref, k)
        if rows is not None:
            b = b[:rows]
        assert a is not None, (tag, k)
        assert a.shape == b.shape, (tag, k, a.shape, b.shape)
        np.testing.assert_array_equal(a, b, err_msg=f"{tag} {k}")


def checked_case(name, M=gqu.M_STATES, bias=ZERO):
    p, q, links, ref, c = gqu.case(name, M, bias)
    print(name, "census:", c)
    gqu.assert_census(name, c)
    return p, q, links, ref


# ------------------------------------------------------------------------------------------------
# 1. parity with the restatement

@pytest.mark.parametrize("name,bias", [(n, ZERO) for n in sorted(gqu.MODELS)] + [(n, gqu.BIAS) for n in gqu.BIASED])
def test_parity_with_the_restatement(name, bias):
    p, q, links, ref = checked_case(name, bias=bias)
    assert len(set(links)) < len(links)                                      # a link listed twice
    if bias != ZERO:
        assert (ref.potential_gradients != gqu.case(name)[3].potential_gradients).any()
    e = eng.Engine(p)
    got = e.query_gradients(q, links=links, field_bias=bias, want=ALL)
    assert_equal(got, ref, tag=name)
    M, S, L, J = len(q), len(p.spheres), len(links), p.J
    assert got.field_gradients.shape == (M, S, 3) and got.link_gradients.shape == (M, L, J)
    assert got.state_gradient.shape == (M, J) and got.link_costs.shape == (M, L)
    assert e.query_info()["launches"] == 1
    e.close()


# ------------------------------------------------------------------------------------------------
# 2. sizes and chunks

def test_sizes_across_wave_edges():
    p, q, links, ref = checked_case("hand9", 257)
    e = eng.Engine(p)
    for M in (1, 63, 64, 65, 257):
        got = e.query_gradients(q[:M], links=links, want=ALL)
        assert_equal(got, ref, tag=f"M {M}", rows=M)
        assert e.query_info()["chunks"] == 1
    one = e.query_gradients(q[0], links=links, want=ALL)       # a single state of J values
    assert_equal(one, ref, tag="one state", rows=1)
    e.close()


def test_chunks_do_not_change_the_results(monkeypatch):
    p, q, links, ref = checked_case("hand9", 257)
    M = 2 * 64 + 3
    e = eng.Engine(p)
    whole = e.query_gradients(q[:M], links=links, want=ALL)
    assert e.query_info()["chunks"] == 1
    monkeypatch.setenv("STOMP_DEBUG_QUERY_CHUNK", "64")
    got = e.query_gradients(q[:M], links=links, want=ALL)
    info = e.query_info()
    assert info["chunks"] == 3 and info["chunk_states"] == 64 and info["launches"] == 3, info
    assert_equal(got, whole, tag="chunked")
    assert_equal(got, ref, tag="chunked against the restatement", rows=M)
    e.close()


# ------------------------------------------------------------------------------------------------
# 3. optional outputs

@pytest.mark.parametrize("name", ["fork12", "pr2"])
def test_every_single_output_alone(name):
    p, q, links, ref = checked_case(name)
    e = eng.Engine(p)
    for k in ALL:
        got = e.query_gradients(q, links=links, want=(k,))
        assert [n for n in ALL if getattr(got, n) is not None] == [k]
        np.testing.assert_array_equal(getattr(got, k), getattr(ref, k), err_msg=k)
    default = e.query_gradients(q)                               # the per-state outputs, no links
    assert [n for n in ALL if getattr(default, n) is not None] == ["state_cost", "state_gradient", "in_collision"]
    assert_equal(default, ref, ["state_cost", "state_gradient", "in_collision"])
    e.close()


# ------------------------------------------------------------------------------------------------
# 4. the bricked field

@pytest.mark.parametrize("name", ["wand21", "pr2"])
def test_bricked_field_gives_the_same_arrays(name, monkeypatch):
    p, q, links, ref = checked_case(name)
    monkeypatch.setenv("STOMP_SDF_LAYOUT", "linear")
    lin = eng.Engine(p)
    monkeypatch.setenv("STOMP_SDF_LAYOUT", "brick")
    brk = eng.Engine(p)
    a = lin.query_gradients(q, links=links, want=ALL)
    b = brk.query_gradients(q, links=links, want=ALL)
    assert_equal(b, a, tag="brick against linear")
    assert_equal(b, ref, tag="brick against the restatement")
    lin.close()
    brk.close()


# ------------------------------------------------------------------------------------------------
# 5. against the existing paths, independent of the restatement

@pytest.mark.parametrize("name", ["hand9", "chain5", "pr2"])
def test_costs_and_flag_are_the_state_querys(name):
    p, q, links, ref = checked_case(name)
    e = eng.Engine(p)
    got = e.query_gradients(q, links=links, field_bias=gqu.BIAS, want=("link_costs", "state_cost", "in_collision"))
    old = e.query_states(q, links=links, want=("link_costs", "state_cost", "in_collision"))
    for k in ("link_costs", "state_cost", "in_collision"):           # (the bias does not enter the potential)
        np.testing.assert_array_equal(getattr(got, k), getattr(old, k), err_msg=k)
    e.close()


@pytest.mark.parametrize("name,bias", [("hand9", ZERO), ("pr2", gqu.BIAS)])
def test_per_sphere_arrays_are_those_of_a_chomp_reset(name, bias):
    # two kernels, one arithmetic: N states inside their limits as the free waypoints of one descent
    p = gqu.MODELS[name]()
    pool = squ.make_states(p, 8 * p.N, seed=5)
    inside = np.ones(len(pool), bool)
    for j, jt in enumerate(p.robot.joints):
        if jt.has_limits:
            inside &= (jt.min <= pool[:, j]) & (pool[:, j] <= jt.max)
    q = pool[inside][:p.N]
    assert len(q) == p.N, (len(q), p.N)
    e = eng.Engine(p)
    c = eng.Chomp(e, field_bias=bias)
    c.reset(np.ascontiguousarray(q.T))
    np.testing.assert_array_equal(c.get("trajectory")[0], q.T)      # inside the limits: not clipped
    got = e.query_gradients(q, field_bias=bias, want=("field_gradients", "potential_gradients"))
    assert got.field_gradients.any() and got.potential_gradients.any()
    np.testing.assert_array_equal(got.field_gradients, c.get("field_gradients")[0])
    np.testing.assert_array_equal(got.potential_gradients, c.get("potential_gradients")[0])
    np.testing.assert_array_equal(e.query_states(q, want=("distances",)).distances, c.get("distances")[0])
    c.close()
    e.close()


# ------------------------------------------------------------------------------------------------
# 6. the query follows the engine's model and field

@pytest.mark.parametrize("name", ["hand9", "pr2"])
def test_follows_a_retarget_with_attached_spheres(name):
    p, q, links, ref = checked_case(name)
    new = dataclasses.replace(p, spheres=attach(p))
    S = len(p.spheres)
    want = gqu.reference(new, q, links)
    assert (want.state_gradient != ref.state_gradient).any()         # the edit changes a gradient
    e = eng.Engine(p)
    assert_equal(e.query_gradients(q, links=links, want=ALL), ref, tag="before")
    e.retarget(p.start, p.goal, spheres=new.spheres)
    got = e.query_gradients(q, links=links, want=ALL)
    assert got.field_gradients.shape == (len(q), S + 1, 3)
    twin = eng.Engine(new)
    assert_equal(got, twin.query_gradients(q, links=links, want=ALL), tag="against the twin")
    assert_equal(got, want, tag="against the restatement")
    e.close()
    twin.close()


@pytest.mark.parametrize("layout", ["brick", "linear"])
def test_follows_a_field_rebuilt_in_place(layout, monkeypatch):
    monkeypatch.setenv("STOMP_SDF_LAYOUT", layout)
    shelf, q, links, ref = checked_case("pr2")
    empty = dataclasses.replace(shelf, boxes=[], cylinders=[])
    empty.sdf = pb.build_sdf(empty.grid, [], [])
    old = gqu.reference(empty, q, links)
    assert (old.state_gradient != ref.state_gradient).any()          # the rebuilt field changes a gradient
    buf = eng.DeviceBuffer(2 * shelf.grid.cells)
    eng.sdf_build_device(empty, buf.ptr)
    e = eng.Engine(empty, sdf_device_ptr=buf.ptr)
    assert_equal(e.query_gradients(q, links=links, want=ALL), old, tag="the first field")
    eng.sdf_build_device(shelf, buf.ptr)                             # the scene changed: shelf and pole appear
    e.refresh_field()
    assert_equal(e.query_gradients(q, links=links, want=ALL), ref, tag="the rebuilt field")
    e.close()
    buf.free()


# ------------------------------------------------------------------------------------------------
# 7. the query leaves the engine alone

def engine_state(e):
    return dict(theta=e.theta(), params=e.rollouts("params"), state_costs=e.rollouts("state_costs"),
                last=e.last_trajectory(), best=e.best_trajectory())


@pytest.mark.parametrize("Kr", [0, 5])
def test_leaves_the_engine_alone(Kr):
    p0, q, links, ref = checked_case("hand9")
    p = mz.hand9(K=12, Kr=Kr)
    e, twin = eng.Engine(p), eng.Engine(p)
    e.run(1, 3)
    twin.run(1, 3)
    got = e.query_gradients(q, links=links, want=ALL)            # a noiseless rollout is pending here
    assert_equal(got, ref, tag="between the runs")
    allocs = e.query_info()["allocations"]
    assert allocs >= 1
    e.query_gradients(q, links=links, want=ALL)
    assert e.query_info()["allocations"] == allocs               # the same size again: nothing allocated
    e.run(4, 3)
    twin.run(4, 3)
    e.synchronize()
    twin.synchronize()
    a, b = engine_state(e), engine_state(twin)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert e.model_info() == twin.model_info()
    e.close()
    twin.close()


def test_leaves_a_group_alone():
    p0, q, links, ref = checked_case("hand9")
    ps = [mz.hand9(K=12, Kr=0), dataclasses.replace(mz.hand9(K=12, Kr=0), seed=77)]
    g, g2 = Group(ps), Group(ps)
    for x in (g, g2):
        x.group.run(1, 3)
    got = g.engines[1].query_gradients(q, links=links, want=ALL)   # between two group.run calls
    assert_equal(got, ref, tag="inside a group")
    for x in (g, g2):
        x.group.run(4, 3)
        x.group.synchronize()
    for e, t in zip(g.engines, g2.engines):
        a, b = engine_state(e), engine_state(t)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    g.close()
    g2.close()


@pytest.mark.parametrize("mode", ["gather", "partials"])
def test_a_sharded_engine_answers_and_stays_in_step(mode, monkeypatch):
    # every rank holds the whole model and field: any rank answers, no collective runs, and the
    # ranks' next iteration is the oracle's
    from oracle import pyoracle as po
    from tests import rank_util as ru
    p0, q, links, ref = checked_case("hand9")
    p = mz.hand9(K=128, Kr=0)
    o = po.Oracle(p, threads=ru.THREADS)
    engines = ru.make_ranks(p, 2, mode, monkeypatch)
    try:
        ru.on_threads(engines, lambda r, e: e.iterate(1))
        o.iterate(1)
        for e in engines:                                         # one rank at a time, from this thread
            assert_equal(e.query_gradients(q, links=links, want=ALL), ref, tag=f"rank of {mode}")
        ru.on_threads(engines, lambda r, e: e.iterate(2))
        o.iterate(2)
        for e in engines:
            np.testing.assert_array_equal(e.theta(), o.theta())
    finally:
        ru.close_all(engines)


# ------------------------------------------------------------------------------------------------
# 8. refusals with a device present

def test_refusals_write_nothing():
    p, q, links, ref = checked_case("hand9")
    e = eng.Engine(p)
    e.query_gradients(q, links=links, want=ALL)
    info = e.query_info()
    nseg = len(p.robot.segments)
    bad_nan = q[:9].copy()
    bad_nan[8, p.J - 1] = np.nan
    cases = [("not finite", dict(states=bad_nan, links=links)),
             ("field_bias", dict(states=q[:9], links=links, field_bias=(0.0, np.inf, 0.0))),
             ("names segment", dict(states=q[:9], links=links + [nseg])),
             ("without links", dict(states=q[:9], links=[])),
             ("num_states", dict(states=np.zeros((0, p.J)), links=links))]
    for text, kw in cases:
        with pytest.raises(RuntimeError, match=text) as err:
            e.query_gradients(want=ALL, fill=201, **kw)
        assert "error -1" in str(err.value)
        outs = err.value.outputs
        assert set(outs) == set(ALL)
        for k, a in outs.items():
            assert (a == 201).all(), (text, k)                    # the sentinel everywhere
    with pytest.raises(RuntimeError, match="link_gradients without links"):
        e.query_gradients(q[:9], links=[], want=("link_gradients",), fill=201)
    assert e.query_info() == info                                 # and nothing of the engine
    assert_equal(e.query_gradients(q, links=links, want=ALL), ref, tag="after the refusals")
    e.close()
