"""Seeded call-sequence walks (tests/CALL_WALKS.md): scripts over the public API, the bookkeeping that
keeps them valid, and the pairs that give one script to an engine (or a group, or two ranks) and to
the CPU oracle.  A plain module like group_util.py: it holds no test and no cached oracle.

A script is a list of plain tuples, e.g. ("run", 3, 2) or ("execute", rows_seed, nrows, member).
make_script(mode, seed, length) makes one from numpy.random.default_rng; it uses no GPU and no oracle
and tracks only what keeps the calls valid (the classes Book / GroupBook / RankBook below).  The walk
is biased towards ordered pairs of op kinds that the scripts of the seeds before it have not shown,
so a mode's census (tests/test_call_walks.py) closes in few seeds: make_script(mode, s) therefore
walks the seeds 0 .. s in turn and returns the last script.

The ask modes (third round) add calls that must leave an engine as it was: state queries, gradient
queries and one CHOMP object per pair (class Asks).  The books track the descent's state only; an ask
changes nothing else of a book, and the oracle side of a pair never hears of one.

replay(mode, script, pair) runs a literal script.  A pair compares only what an op returns
(assert_array_equal / ==, no tolerance); state is read by the `observe` ops alone, at the random
points where the walk put them.  Every assertion message carries the mode, the failing op's index
and the script up to that op as a Python literal.
"""
import copy
import ctypes as C
import dataclasses

import numpy as np

from oracle import pyoracle as po
from stomp_motion_planner_icra2011_amd import problem as pb
from tests import chomp_util as cu
from tests import gradient_query_util as gqu
from tests import group_util as gu
from tests import model_zoo as mz
from tests import pi_steps_util as su
from tests import state_query_util as squ

try:   # the CPU tests make scripts and run oracles without the engine library
    from stomp_motion_planner_icra2011_amd import engine as eng
except Exception:   # pragma: no cover
    eng = None

# ---------------------------------------------------------------------------- what observe reads
X_KEYS = ("x_params", "x_noise", "x_control", "x_state")
ROW_KEYS = ("prob", "state", "noise", "params", "control")
ALWAYS = ("theta", "last", "best")          # defined from creation on (tests/RETARGET.md: created())
OBS_ORDER = ALWAYS + ROW_KEYS + X_KEYS + ("cumulative",)
FLUSHING = ("last", "best") + X_KEYS        # reads that evaluate a pending noiseless rollout first


def _get(x, key):
    if key == "theta":
        return x.theta()
    if key == "last":
        return x.last_trajectory()
    if key == "best":
        return x.best_trajectory()
    return x.rollouts(gu.ROW_NAMES[key])


def numpy_cumulative(e):
    """GROUP_CUMULATIVE.md: one add per element, then the suffix sums t = N - 2 .. 0, on the engine's
    own state and control rows."""
    c = e.rollouts("state_costs")[:, None, :] + e.rollouts("control_costs")
    for t in range(c.shape[2] - 2, -1, -1):
        c[:, :, t] += c[:, :, t + 1]
    return c


def moved(p, k, span=0.3):
    """problem p with another start, goal and seed (no offset on a joint whose limits coincide)."""
    rng = np.random.default_rng(4100 + k)
    f = np.array([not (j.has_limits and j.min == j.max) for j in p.robot.joints], np.float64)
    return dataclasses.replace(p, start=p.start + f * rng.uniform(-span, span, p.J),
                               goal=p.goal + f * rng.uniform(-span, span, p.J), seed=p.seed + 2000 + k)


def scene_objects(p, extra):
    """The problem's boxes as collision objects; extra: one more box beside the default trajectory."""
    objs = [pb.SceneObject(pb.SHAPE_BOX, tuple(b.center), (0.0, 0.0, 0.0, 1.0), tuple(b.dims)) for b in p.boxes]
    if extra:
        mid = pb.sphere_positions(p.robot, p.spheres, 0.5 * (p.start + p.goal))[len(p.spheres) // 3]
        objs.append(pb.SceneObject(pb.SHAPE_BOX, tuple(mid + np.array([0.03, -0.02, 0.05])), (0.0, 0.0, 0.0, 1.0),
                                   (0.09, 0.07, 0.11)))
    return objs


def scene_static_layer(p, which):
    """The static layers of the scene modes.  0: the problem's boxes; 1: one more box, near another
    sphere of the default trajectory than scene_objects' extra one."""
    objs = scene_objects(p, False)
    if which:
        at = pb.sphere_positions(p.robot, p.spheres, 0.5 * (p.start + p.goal))[(2 * len(p.spheres)) // 3]
        objs.append(pb.SceneObject(pb.SHAPE_BOX, tuple(at + np.array([-0.04, 0.03, 0.06])), (0.0, 0.0, 0.0, 1.0),
                                   (0.08, 0.1, 0.06)))
    return objs


def scene_dynamic_set(p, variant):
    """The dynamic sets of the scene modes: none; scene_objects' box beside the default trajectory; that
    box moved; a body outside the grid (no mark lands: the static field)."""
    name = DYNAMIC_VARIANTS[variant]
    if name == "none":
        return []
    if name == "outside":
        g = p.grid
        far = np.array(g.origin) + (np.array(g.dims) + 40) * g.resolution
        return [pb.SceneObject(pb.BODY_BOX, tuple(far), dims=(0.2, 0.2, 0.2))]
    box = scene_objects(p, True)[-1]
    if name == "moved_box":
        box = dataclasses.replace(box, position=tuple(np.array(box.position) + np.array([0.05, 0.04, -0.03])))
    return [box]


def has_terms(p):
    return bool(p.orientation_constraints) or p.params.torque_cost_weight > 1e-9


def request_spheres(p, choice):
    """The sphere list of a request on problem p.  attach: one more sphere on the tree's last segment,
    after that segment's own (what attached_collision_points makes of a sphere body of radius 0.05 at
    (0.03, 0, 0.02), as test_gpu_request_model.attach does; built here from pb.Sphere so that the
    CPU tests need no library).  radius_only: every radius and clearance changed, the layout kept."""
    if choice == "base":
        return list(p.spheres)
    if choice == "radius_only":
        cap = p.grid.max_expansion
        return [dataclasses.replace(s, radius=s.radius * 0.8, clearance=min(s.clearance * 1.3, cap - s.radius * 0.8))
                for s in p.spheres]
    assert choice == "attach", choice
    seg, radius = len(p.robot.segments) - 1, 0.05
    clearance = min(0.05, p.grid.max_expansion - radius)
    assert clearance > 0.0
    new = pb.Sphere(seg, radius, clearance, (0.03, 0.0, 0.02))
    return [s for s in p.spheres if s.segment <= seg] + [new] + [s for s in p.spheres if s.segment > seg]


def group_request_spheres(p, choice, m):
    """request_spheres for member m of a group: the same layouts, the attached sphere's values the
    member's own (test_gpu_request_group.requests)"""
    out = request_spheres(p, choice)
    if choice == "attach":
        i = max(i for i, s in enumerate(out) if s.segment == len(p.robot.segments) - 1)
        out[i] = dataclasses.replace(out[i], radius=0.04 + 0.005 * m, pos=(0.03 - 0.01 * m, 0.0, 0.02),
                                     clearance=min(0.05, p.grid.max_expansion - (0.04 + 0.005 * m)))
    return out


def assert_attach_matters(p):
    """On the oracle alone (test_gpu_request_model.assert_edit_matters): the attached sphere changes
    iteration 1's state costs, so a request that silently kept the old spheres cannot pass."""
    a, b = po.Oracle(dataclasses.replace(p, spheres=request_spheres(p, "attach"))), po.Oracle(p)
    a.iterate(1)
    b.iterate(1)
    differ = int(np.sum(np.any(a.rollouts("state_costs") != b.rollouts("state_costs"), axis=1)))
    assert differ >= 1, "the attached sphere changes no state cost of iteration 1"
    for choice in ("radius_only",):
        c = po.Oracle(dataclasses.replace(p, spheres=request_spheres(p, choice)))
        c.iterate(1)
        assert not np.array_equal(c.rollouts("state_costs"), b.rollouts("state_costs")), choice


_MATTERS = set()


def assert_asks_matter(mode, made=None):
    """On the references alone, before any device is touched (once per process and mode): what the
    walk changes under an ask changes what the ask must return, so an ask answered from a stale
    problem, model, field or theta cannot pass."""
    if mode in _MATTERS:
        return
    spec = MODES[mode]
    made = spec["make"]() if made is None else made
    p = made[DESCENT_MEMBER] if spec["kind"] == "group" else made
    if spec.get("scene"):
        p = dataclasses.replace(p, sdf=po.sdf_build_objects(p.grid, scene_static_layer(p, 0))[0])
    prm = spec.get("chomp", _CHOMP_PLAIN)
    links = list(range(len(p.robot.segments)))
    assert mode_info(mode).get("nseg") == len(links), (mode, mode_info(mode), len(links))   # the books draw links from it
    q = squ.make_states(p, 65, 0)

    def first(problem, start=None):
        r = cu.ChompRef(problem, prm)
        r.reset(start)
        return r.snapshot()

    # some drawn query state has a potential and a link gradient that are not zero
    g = gqu.reference(p, q, links)
    assert g.potentials.any() and g.link_gradients.any(), mode
    if spec["kind"] == "ranks":
        _MATTERS.add(mode)
        return
    # the mode's retarget changes the descent's first snapshot (beyond the trajectory itself)
    base = first(p)
    if spec["kind"] == "group":
        t = spec["targets"]()
        moved_p = dataclasses.replace(p, start=t[1].start.copy(), goal=t[1].goal.copy())
    else:
        moved_p = moved(p, 1)
    assert not np.array_equal(first(moved_p)["potentials"], base["potentials"]), mode
    if spec.get("request"):
        # the attached sphere has a query potential and a descent potential of its own
        att = dataclasses.replace(p, spheres=request_spheres(p, "attach"))
        at = max(i for i, s in enumerate(att.spheres) if s.segment == len(p.robot.segments) - 1)
        assert squ.reference(att, q, links).potentials[:, at].any(), mode
        assert first(att)["potentials"][:, at].any(), mode
        rad = dataclasses.replace(p, spheres=request_spheres(p, "radius_only"))
        assert not np.array_equal(first(rad)["potentials"], base["potentials"]), mode
    if spec.get("scene"):
        # every change of the dynamic set that the pair calls a change (none -> box -> moved_box)
        # and of the static layer changes a query distance and a descent's distances
        fields = [po.sdf_build_objects(p.grid, scene_static_layer(p, l) + scene_dynamic_set(p, v))[0]
                  for l, v in ((0, 0), (0, 1), (0, 2), (1, 0))]
        for a, b in ((0, 1), (1, 2), (0, 2), (0, 3)):
            pa, pb_ = dataclasses.replace(p, sdf=fields[a]), dataclasses.replace(p, sdf=fields[b])
            assert not np.array_equal(squ.reference(pa, q, []).distances, squ.reference(pb_, q, []).distances), (mode, a, b)
            assert not np.array_equal(first(pa)["distances"], first(pb_)["distances"]), (mode, a, b)
    if spec["kind"] == "group":
        # a reset from theta after an iteration is not a reset from theta_0
        o = po.Oracle(p, threads=spec.get("threads", 1))
        o.iterate(1)
        after = first(p, o.theta())
        assert not np.array_equal(after["trajectory"], base["trajectory"]) and after["cost"] != base["cost"], mode
    _MATTERS.add(mode)


# ---------------------------------------------------------------------------- modes
def _chain5(K, Kr, max_iterations, **kw):
    return lambda: mz.chain5(K=K, Kr=Kr, max_iterations=max_iterations, max_iterations_after_collision_free=1000, **kw)


def _terms_cum():
    return mz.TERMS_ZOO["chain5"](K=12, Kr=5, use_cumulative_costs=True, max_iterations=4,
                                  max_iterations_after_collision_free=1000)


def _group_plain(K, Kr):
    def make():
        ps = gu.variants(mz.chain5, 4, K=K, Kr=Kr, max_iterations_after_collision_free=1000)
        return [dataclasses.replace(p, params=dataclasses.replace(p.params, max_iterations=3 + (i % 2)))
                for i, p in enumerate(ps)]
    return make


def _group_mixed():
    """Four problems of one shape: terms on 0 and 3, cumulative costs on 1 and 2, max_iterations 4 .. 7."""
    ps = gu.variants(mz.TERMS_ZOO["chain5"], 4, use_cumulative_costs=True, max_iterations_after_collision_free=1000)
    out = []
    for i, p in enumerate(ps):
        prm = dataclasses.replace(p.params, max_iterations=4 + i, use_cumulative_costs=i in (1, 2),
                                  torque_cost_weight=p.params.torque_cost_weight if i in (0, 3) else 0.0)
        out.append(dataclasses.replace(p, params=prm, orientation_constraints=p.orientation_constraints if i in (0, 3) else []))
    return out


def _ranks():
    return mz.chain5(K=128, Kr=0, max_iterations=3, max_iterations_after_collision_free=1000)


def _request(K, Kr, **kw):
    """fork12 with inertias, torque weight 0 and no constraints: the terms launch starts off"""
    return lambda: mz.TERMS_ZOO["fork12_base"](torque=0.0, constrained=False, K=K, Kr=Kr, max_iterations=4,
                                               max_iterations_after_collision_free=1000, **kw)


def _group_request():
    """Three fork12 problems with inertias (no torque term, no constraints), own start / goal / seed and
    max_iterations 3 .. 5, engine 1 with cumulative costs (test_gpu_request_group.base_problems)"""
    p = _request(12, 5)()
    return [dataclasses.replace(moved(p, 60 + i), params=dataclasses.replace(p.params, max_iterations=3 + i,
                                                                             use_cumulative_costs=i == 1)) for i in range(3)]


def _group_shelf():
    """Four copies of the PR2 shelf fixture at the zoo's shape (test_gpu_retarget.shelf(Kr=5)), max_iterations 3 .. 6"""
    return [pb.make_problem(waypoints=40, num_rollouts=12, num_reused_rollouts=5, max_iterations=3 + i,
                            max_iterations_after_collision_free=2) for i in range(4)]


def _shelf_targets():
    """(base, A, B) of test_gpu_retarget.flag_pair: A's padding poses alone collide, B is free"""
    from tests.test_gpu_retarget import flag_pair
    return flag_pair()


# the CHOMP parameters of the ask modes: the reference's defaults with learning_rate 0.05; ask_request
# with the pseudo-inverse and a field bias
_CHOMP_PLAIN = cu.ChompParams(learning_rate=0.05)
_CHOMP_PINV_BIAS = cu.ChompParams(learning_rate=0.05, use_pseudo_inverse=True, field_bias=gqu.BIAS)

# kind: "single" / "group" / "ranks"; make: the problem(s); env: set before creation; expect: pieces
# the engine's own `stomp: model` line (STOMP_DEBUG_LEAN_PRINT) must hold; length: ops per script;
# seeds: scripts per mode, the smallest count at which the census of tests/test_call_walks.py holds
MODES = {
    "reuse_fused": dict(kind="single", make=_chain5(12, 5, 4), env={"STOMP_DEBUG_NO_SPEC": "0", "STOMP_DEBUG_NO_PICK_FUSE": "0"},
                        expect=["J 5 N 39 ", "pregen 1 fused_noise 1 brick 0", "launch of 13 rollouts: split,"]),
    "reuse_no_spec": dict(kind="single", make=_chain5(12, 5, 5), env={"STOMP_DEBUG_NO_SPEC": "1", "STOMP_DEBUG_NO_PICK_FUSE": "0"},
                          expect=["pregen 1 fused_noise 1", "launch of 13 rollouts: split,"]),
    "reuse_no_pick_fuse": dict(kind="single", make=_chain5(12, 5, 3), env={"STOMP_DEBUG_NO_SPEC": "0", "STOMP_DEBUG_NO_PICK_FUSE": "1"},
                               expect=["pregen 1 fused_noise 1", "launch of 13 rollouts: split,"]),
    "pregen": dict(kind="single", make=_chain5(20, 0, 6), env={},
                   expect=["pregen 1 fused_noise 1", "launch of 21 rollouts: "]),
    "unfused": dict(kind="single", make=lambda: mz.chain17(K=12, Kr=5, max_iterations=4, max_iterations_after_collision_free=1000),
                    env={}, expect=["J 17 N 39 ", "pregen 0 fused_noise 0"]),
    "slot_loop": dict(kind="single", make=_chain5(260, 0, 3), env={}, threads=8, length=20, purity=False,
                      expect=["lean 0 ", "launch of 261 rollouts: slot loop,"]),
    "slot_loop_lean": dict(kind="single", make=_chain5(260, 0, 3), env={"STOMP_DEBUG_LEAN": "1"}, threads=8, length=20,
                           purity=False, expect=["lean 1 ", "launch of 261 rollouts: lean slot loop,"]),
    "phased": dict(kind="single", make=_chain5(12, 5, 5), env={"STOMP_DEBUG_SPLIT_MAX": "1"},
                   expect=["launch of 13 rollouts: phased,"]),
    "terms_cum": dict(kind="single", make=_terms_cum, env={}, threads=8, expect=["J 5 N 39 ", "launch of 13 rollouts: "]),
    "device_brick": dict(kind="single", make=_chain5(12, 5, 4, shape=(66, 66, 66)), env={"STOMP_SDF_LAYOUT": "brick"},
                         device_field=True, expect=["brick 1,"]),
    "group_reuse": dict(kind="group", make=_group_plain(12, 5), env={}, expect=["group of 4 engines J 5 N 39 K 12 "]),
    "group_pregen": dict(kind="group", make=_group_plain(20, 0), env={}, expect=["group of 4 engines J 5 N 39 K 20 "]),
    "group_mixed": dict(kind="group", make=_group_mixed, env={}, threads=8, length=30,
                        group=dict(state_terms=True, cumulative_costs=True, compact=False),
                        expect=["group of 4 engines J 5 N 39 K 12 ", "engines with terms 2 of 4",
                                "engines with cumulative costs 2 of 4"]),
    "group_mixed_compact": dict(kind="group", make=_group_mixed, env={}, threads=8, length=30,
                                group=dict(state_terms=True, cumulative_costs=True, compact=True),
                                expect=["group of 4 engines J 5 N 39 K 12 ", "engines with terms 2 of 4",
                                        "engines with cumulative costs 2 of 4"]),
    "ranks_partials": dict(kind="ranks", make=_ranks, env={}, shard="partials", threads=8, length=20,
                           expect=["launch of 65 rollouts: "]),
    "ranks_gather": dict(kind="ranks", make=_ranks, env={}, shard="gather", threads=8, length=20,
                         expect=["launch of 65 rollouts: "]),
    # ---- modes added after the 16 above were frozen (IDENTS): new op kinds belong to these alone
    "request_reuse": dict(kind="single", make=_request(12, 5), env={}, request=True, threads=8,
                          expect=["J 12 N 39 ", "launch of 13 rollouts: "]),
    "request_pregen_cum": dict(kind="single", make=_request(20, 0, use_cumulative_costs=True), env={}, request=True,
                               threads=8, expect=["J 12 N 39 ", "launch of 21 rollouts: "]),
    "scene_linear": dict(kind="single", make=_chain5(12, 5, 4, shape=(66, 66, 66)), env={"STOMP_SDF_LAYOUT": "linear"},
                         scene=True, expect=["brick 0,"]),
    "scene_brick": dict(kind="single", make=_chain5(12, 5, 4, shape=(66, 66, 66)), env={"STOMP_SDF_LAYOUT": "brick"},
                        scene=True, expect=["brick 1,"]),
    "group_request": dict(kind="group", make=_group_request, env={}, request=True, threads=8, length=30,
                          group=dict(state_terms=True, cumulative_costs=True),
                          expect=["group of 3 engines J 12 N 39 K 12 ", "engines with terms 0 of 3",
                                  "engines with cumulative costs 1 of 3"]),
    "group_serve_reuse": dict(kind="group", make=_group_plain(12, 5), env={}, serve=True,
                              expect=["group of 4 engines J 5 N 39 K 12 "]),
    "group_serve_pregen": dict(kind="group", make=_group_plain(20, 0), env={}, serve=True,
                               expect=["group of 4 engines J 5 N 39 K 20 "]),
    "group_serve_shelf": dict(kind="group", make=_group_shelf, env={}, serve=True, targets=_shelf_targets, threads=8,
                              length=30, info=dict(P=4, Kr=5, cums=[False] * 4, max_its=[3, 4, 5, 6]),
                              expect=["group of 4 engines J 7 N 39 K 12 "]),
    # ---- the third round: state queries, gradient queries and CHOMP descents among the calls above
    "ask_reuse": dict(kind="single", make=_chain5(12, 5, 4), env={"STOMP_DEBUG_NO_SPEC": "0", "STOMP_DEBUG_NO_PICK_FUSE": "0"},
                      ask=True, chomp=_CHOMP_PLAIN,
                      expect=["J 5 N 39 ", "pregen 1 fused_noise 1 brick 0", "launch of 13 rollouts: split,"]),
    "ask_pregen": dict(kind="single", make=_chain5(20, 0, 6), env={}, ask=True, chomp=_CHOMP_PLAIN,
                       expect=["pregen 1 fused_noise 1", "launch of 21 rollouts: "]),
    "ask_request": dict(kind="single", make=_request(12, 5), env={}, request=True, threads=8, ask=True,
                        chomp=_CHOMP_PINV_BIAS, expect=["J 12 N 39 ", "launch of 13 rollouts: "]),
    "ask_scene_linear": dict(kind="single", make=_chain5(12, 5, 4, shape=(66, 66, 66)), env={"STOMP_SDF_LAYOUT": "linear"},
                             scene=True, ask=True, chomp=_CHOMP_PLAIN, expect=["brick 0,"]),
    "ask_scene_brick": dict(kind="single", make=_chain5(12, 5, 4, shape=(66, 66, 66)), env={"STOMP_SDF_LAYOUT": "brick"},
                            scene=True, ask=True, chomp=_CHOMP_PLAIN, expect=["brick 1,"]),
    "ask_group": dict(kind="group", make=_group_shelf, env={}, serve=True, targets=_shelf_targets, threads=8, length=30,
                      ask=True, chomp=_CHOMP_PLAIN,
                      info=dict(P=4, Kr=5, cums=[False] * 4, max_its=[3, 4, 5, 6], nseg=17),
                      expect=["group of 4 engines J 7 N 39 K 12 "]),
    "ask_ranks": dict(kind="ranks", make=_ranks, env={}, shard="partials", threads=8, length=20, ask=True,
                      expect=["launch of 65 rollouts: "]),
}
# make_script seeds its generator with a mode's ident.  The first 16 are the modes' indices in
# sorted order at the time the walks were written, frozen: a new mode must not move an old script.
IDENTS = {
    "device_brick": 0, "group_mixed": 1, "group_mixed_compact": 2, "group_pregen": 3, "group_reuse": 4, "phased": 5,
    "pregen": 6, "ranks_gather": 7, "ranks_partials": 8, "reuse_fused": 9, "reuse_no_pick_fuse": 10, "reuse_no_spec": 11,
    "slot_loop": 12, "slot_loop_lean": 13, "terms_cum": 14, "unfused": 15,
    "request_reuse": 16, "request_pregen_cum": 17, "scene_linear": 18, "scene_brick": 19, "group_request": 20,
    "group_serve_reuse": 21, "group_serve_pregen": 22,
    "group_serve_shelf": 23,
    "ask_reuse": 24, "ask_pregen": 25, "ask_request": 26, "ask_scene_linear": 27, "ask_scene_brick": 28, "ask_group": 29,
    "ask_ranks": 30,
}
DEFAULT_LENGTH = 40
# scripts per mode: see tests/CALL_WALKS.md for how they were found (test_call_walks.py asserts that
# the census holds at these counts and fails one seed earlier)
SEEDS = {
    "reuse_fused": 12, "reuse_no_spec": 14, "reuse_no_pick_fuse": 12, "pregen": 13, "unfused": 13, "slot_loop": 28,
    "slot_loop_lean": 25, "phased": 18, "terms_cum": 15, "device_brick": 16, "group_reuse": 5, "group_pregen": 4,
    "group_mixed": 18, "group_mixed_compact": 8, "ranks_partials": 4, "ranks_gather": 4,
    "request_reuse": 16, "request_pregen_cum": 25, "scene_linear": 20, "scene_brick": 16, "group_request": 20,
    "group_serve_reuse": 12, "group_serve_pregen": 21,
    "group_serve_shelf": 22,
    "ask_reuse": 24, "ask_pregen": 44, "ask_request": 38, "ask_scene_linear": 34, "ask_scene_brick": 64, "ask_group": 31,
    "ask_ranks": 8,
}


def length_of(mode):
    return MODES[mode].get("length", DEFAULT_LENGTH)


# ---------------------------------------------------------------------------- single-engine bookkeeping
FUSED = ("iterate", "run", "optimize")
STEP = ("pi_get_rollouts", "pi_set_rollout_costs", "pi_improve_policy", "pi_add_extra_rollout", "pi_reset")
NEUTRAL = ("observe", "execute", "set_timing", "refuse")     # ops that change no state the model has
SINGLE_KINDS = FUSED + ("synchronize", "observe", "set_theta", "execute") + STEP + ("retarget", "set_timing", "refuse")
REFUSALS = ("nan_goal", "extra_num0", "null_sigma")
# the request modes: retarget_request(k, keep_seed, spheres, constraints) and two more refusals
REQUEST_REFUSALS = REFUSALS + ("unordered_spheres", "bad_segment")
SPHERE_CHOICES = ("keep", "attach", "base", "radius_only")
CONSTRAINT_CHOICES = ("keep", 0, 1, 2)
# the scene modes: the field belongs to a scene of two layers on the engine's stream
SCENE_KINDS = ("scene_dynamic", "scene_static")
DYNAMIC_VARIANTS = ("none", "box", "moved_box", "outside")
# the ask modes: calls that must leave the engine as it was -- the two queries and a CHOMP descent
ASK_QUERIES = ("query_states", "query_gradients")
DESCENT_KINDS = ("chomp_reset", "chomp_step", "chomp_get", "chomp_optimize", "chomp_refused")
ASK_KINDS = ASK_QUERIES + DESCENT_KINDS
GROUP_ASK_QUERIES = ("m_query_states", "m_query_gradients")
ASKS = ASK_KINDS + GROUP_ASK_QUERIES
CHOMP_REFUSALS = ("no_reset", "stale_target", "stale_model", "needs_fresh_reset")
QUERY_M = (1, 63, 64, 65, 130)          # one state, a wave's edges, two waves and a partial one
QS_OUTPUTS = ("positions", "distances", "potentials", "sphere_collides", "link_costs", "state_cost", "min_clearance",
              "min_sphere", "in_collision", "limits_violated")
GQ_OUTPUTS = gqu.OUTPUTS
CHOMP_NAMES = tuple(cu.NAMES)
DESCENT_MEMBER = 1                      # the group member whose engine the ask_group mode's descent borrows

# The descent's state in a book: none (no reset yet) / fresh / stepped / optimized / stale_silent /
# stale_target / stale_model.  A staling op leaves `none` as it is (the "no reset" refusal comes
# first in check_live) and never lowers a stale state: the model's reason wins over the target's, and
# both over stale_silent -- a field read in place that a scene op rewrote, which the library cannot
# notice: no descent op but chomp_reset is drawn then, and no refusal, since none would come.
_STALE_RANK = {"stale_silent": 1, "stale_target": 2, "stale_model": 3}
_REFUSAL_OF = {"none": "no_reset", "stale_target": "stale_target", "stale_model": "stale_model",
               "stepped": "needs_fresh_reset", "optimized": "needs_fresh_reset"}


def descent_allows(state, kind):
    if kind == "chomp_step":
        return state in ("fresh", "stepped")
    if kind == "chomp_get":
        return state in ("fresh", "stepped", "optimized")
    if kind == "chomp_optimize":
        return state == "fresh"
    if kind == "chomp_refused":
        return state in _REFUSAL_OF
    return True


def descent_staled(state, reason):
    new = "stale_" + reason
    return state if state == "none" or _STALE_RANK.get(state, 0) >= _STALE_RANK[new] else new


def descent_after(state, op):
    kind = op[0]
    assert descent_allows(state, kind), (op, state)
    if kind == "chomp_reset":
        assert 1 <= op[1] <= 3, op
        return "fresh"
    if kind == "chomp_step":
        assert 1 <= op[1] <= 3, op
        return "stepped"
    if kind == "chomp_optimize":
        return "optimized"
    if kind == "chomp_get":
        assert 1 <= len(op[1]) and set(op[1]) <= set(CHOMP_NAMES), op
    if kind == "chomp_refused":
        assert op[1] == _REFUSAL_OF[state], (op, state)
    return state


def _check_query(op, nseg):
    """a query op's arguments (after a group's member index): seed, M, links, want[, biased]"""
    kind, (seed, M, links, want) = op[0], op[1:5]
    names = QS_OUTPUTS if kind.endswith("query_states") else GQ_OUTPUTS
    assert M in QUERY_M and all(0 <= g < nseg for g in links) and len(set(links)) == len(links), op
    assert want and set(want) <= set(names), op
    assert links or not (set(want) & {"link_costs", "link_gradients"}), op


def _ask_op(kind, state, nseg, rng):
    """an ask of `kind` (a query without its member or rank) from seeds, small ints and names"""
    if kind in ASK_QUERIES:
        M = QUERY_M[int(rng.integers(len(QUERY_M)))]
        links = tuple(g for g in range(nseg) if rng.random() < 0.4) if rng.random() < 0.8 else ()
        names = QS_OUTPUTS if kind == "query_states" else GQ_OUTPUTS
        ok = [n for n in names if links or n not in ("link_costs", "link_gradients")]
        want = tuple(n for n in ok if rng.random() < 0.4) or (ok[int(rng.integers(len(ok)))],)
        op = (kind, int(rng.integers(1 << 20)), M, links, want)
        return op + (bool(rng.random() < 0.5),) if kind == "query_gradients" else op
    if kind == "chomp_reset":
        return ("chomp_reset", int(rng.integers(1, 4)), None if rng.random() < 0.5 else int(rng.integers(1 << 20)))
    if kind == "chomp_step":
        return ("chomp_step", int(rng.integers(1, 4)))
    if kind == "chomp_get":
        pick = sorted(rng.permutation(len(CHOMP_NAMES))[: int(rng.integers(1, 5))].tolist())
        return ("chomp_get", tuple(CHOMP_NAMES[i] for i in pick))
    if kind == "chomp_refused":
        return ("chomp_refused", _REFUSAL_OF[state])
    assert kind == "chomp_optimize", kind
    return (kind,)


class Book:
    """What the generator knows of one engine: the next iteration number, the step round's phase
    (closed -> pi_get_rollouts -> got -> pi_set_rollout_costs -> costed -> pi_improve_policy -> closed),
    whether a setRolloutCosts has been called since creation / retarget, whether a noiseless rollout
    may be pending, and which fields both sides define (`valid`).

    Orders excluded (tests/CALL_WALKS.md): between pi_get_rollouts and pi_improve_policy no fused
    iteration, no second pi_get_rollouts and no pi_add_extra_rollout; pi_improve_policy only after a
    pi_set_rollout_costs of the same round; pi_add_extra_rollout only after the first
    pi_set_rollout_costs; refresh_field only with no noiseless rollout pending."""

    def __init__(self, problem_info):
        self.Kr, self.cum, self.device = problem_info["Kr"], problem_info["cum"], problem_info.get("device", False)
        self.max_it = problem_info["max_it"]
        self.request, self.scene = problem_info.get("request", False), problem_info.get("scene", False)
        self.ask, self.nseg, self.brick = problem_info.get("ask", False), problem_info.get("nseg", 0), problem_info.get("brick", False)
        self.kinds = (SINGLE_KINDS + (("refresh_field",) if self.device else ()) + (("retarget_request",) if self.request else ())
                      + (SCENE_KINDS if self.scene else ()) + (ASK_KINDS if self.ask else ()))
        self.descent = "none"       # (outside reset(): a retarget makes a descent stale, it does not forget it)
        self.refusals = REQUEST_REFUSALS if self.request else REFUSALS
        self.reset()

    def reset(self):
        self.next_it, self.phase, self.costed_once, self.pending = 1, "closed", False, False
        self.valid = set(ALWAYS)
        self.extra_box = False

    def allowed(self, kind):
        closed = self.phase == "closed"
        if kind in DESCENT_KINDS:
            return self.ask and descent_allows(self.descent, kind)
        if kind in FUSED or kind == "pi_get_rollouts":
            return closed
        if kind == "pi_add_extra_rollout":
            return closed and self.costed_once
        if kind == "pi_set_rollout_costs":
            return self.phase in ("got", "costed")
        if kind == "pi_improve_policy":
            return self.phase == "costed"
        if kind == "refresh_field":
            return self.device and not self.pending
        if kind == "scene_check":
            return self.scene
        if kind in SCENE_KINDS:     # (refresh_field's rule: the pending noiseless rollout would read the new field)
            return self.scene and not self.pending
        return kind in self.kinds

    def _iterated(self):
        self.valid |= set(ROW_KEYS) | {"x_state"}
        if self.Kr > 0:
            self.valid |= set(X_KEYS)
        else:   # the oracle's iteration writes the extra rollout's rows, the engine's only with reuse
            self.valid -= set(gu.NO_REUSE_ORACLE_SKIPS)
        if self.cum:
            self.valid.add("cumulative")

    def apply(self, op):
        kind = op[0]
        assert self.allowed(kind), (kind, self.phase)
        if kind == "iterate":
            assert op[1] >= 1
            self.next_it, self.pending = op[1] + 1, False
            self._iterated()
        elif kind == "run":
            assert op[1] >= 1 and 1 <= op[2] <= 4
            self.next_it, self.pending = op[1] + op[2], True
            self._iterated()
        elif kind == "optimize":
            self.next_it, self.pending = self.max_it + 1, False
            self._iterated()
        elif kind in ("synchronize", "set_theta"):
            self.pending = False
        elif kind == "observe":
            assert op[1] and set(op[1]) <= self.valid, (op, sorted(self.valid))
            if set(op[1]) & set(FLUSHING):
                self.pending = False
        elif kind == "pi_get_rollouts":
            assert op[1] >= 1
            self.next_it, self.pending, self.phase = op[1] + 1, False, "got"
            self.valid -= {"state", "control", "prob", "cumulative"}
            self.valid |= {"params", "noise"}
        elif kind == "pi_set_rollout_costs":
            assert op[1] in (1, 2)
            self.phase, self.costed_once = "costed", True
            self.valid |= {"state", "control"}
        elif kind == "pi_improve_policy":
            self.phase = "closed"
            self.valid.add("prob")
            if self.cum:
                self.valid.add("cumulative")
        elif kind == "pi_add_extra_rollout":
            self.pending = False
            self.valid |= set(X_KEYS)
        elif kind in ("retarget", "retarget_request"):
            if kind == "retarget_request":
                assert op[3] in SPHERE_CHOICES and op[4] in CONSTRAINT_CHOICES, op
            box = self.extra_box
            self.reset()
            self.extra_box = box
        elif kind == "refresh_field":
            assert op[1] != self.extra_box, "one more or one fewer box"
            self.extra_box = op[1]
        elif kind == "refuse":
            assert op[1] in self.refusals
        elif kind == "scene_dynamic":
            assert op[1] in range(len(DYNAMIC_VARIANTS)), op
        elif kind == "scene_static":
            assert op[1] in (0, 1), op
        elif kind == "scene_check":     # (final_observe's: not in the alphabet)
            assert self.scene
        elif kind in ASK_QUERIES:       # the asks change nothing above: that is the claim under test
            assert self.ask
            _check_query(op, self.nseg)
        elif kind in DESCENT_KINDS:
            self.descent = descent_after(self.descent, op)
        else:
            assert kind in ("execute", "set_timing", "pi_reset"), kind
        # what makes a descent stale
        if kind in ("retarget", "refresh_field"):
            self.descent = descent_staled(self.descent, "target")
        elif kind == "retarget_request":     # a replaced list changes the model, radius_only included
            self.descent = descent_staled(self.descent, "target" if (op[3], op[4]) == ("keep", "keep") else "model")
        elif kind in SCENE_KINDS:            # the bricked copy follows by a refresh call; a field read in place by none
            self.descent = descent_staled(self.descent, "target" if self.brick else "silent")

    def final_observe(self):
        return ("observe", tuple(k for k in OBS_ORDER if k in self.valid))

    def final_ops(self):
        live = self.ask and descent_allows(self.descent, "chomp_get")
        return ([self.final_observe()] + ([("scene_check",)] if self.scene else [])
                + ([("chomp_get", ("trajectory", "final_increments", "cost"))] if live else []))


def _single_op(book, kind, rng):
    if kind in ASK_KINDS:
        return _ask_op(kind, book.descent, book.nseg, rng)
    if kind == "iterate":
        r = rng.random()
        nxt = book.next_it
        it = nxt if r < 0.7 else (max(nxt - 1, 1) if r < 0.8 else (nxt + int(rng.integers(1, 3)) if r < 0.9 else max(nxt - 2, 1)))
        return ("iterate", it)
    if kind == "run":
        first = book.next_it if rng.random() < 0.8 else max(book.next_it + int(rng.integers(-1, 2)), 1)
        return ("run", first, int(rng.integers(1, 5)))
    if kind == "observe":
        valid = [k for k in OBS_ORDER if k in book.valid]
        pick = [k for k in valid if rng.random() < 0.4] or [valid[int(rng.integers(len(valid)))]]
        return ("observe", tuple(pick))
    if kind == "set_theta":
        return ("set_theta", int(rng.integers(1 << 20)))
    if kind == "execute":
        return ("execute", int(rng.integers(1 << 20)), int(rng.integers(1, 4)), int(rng.integers(0, 3)))
    if kind == "pi_get_rollouts":
        return ("pi_get_rollouts", book.next_it if rng.random() < 0.8 else max(book.next_it - 1, 1))
    if kind == "pi_set_rollout_costs":
        return ("pi_set_rollout_costs", int(rng.integers(1, 3)))
    if kind == "pi_add_extra_rollout":
        return ("pi_add_extra_rollout", None if rng.random() < 0.5 else int(rng.integers(1 << 20)))
    if kind == "retarget":
        return ("retarget", int(rng.integers(1, 50)), bool(rng.random() < 0.3))
    if kind == "refresh_field":
        return ("refresh_field", not book.extra_box)
    if kind == "set_timing":
        return ("set_timing", bool(rng.random() < 0.5))
    if kind == "refuse":
        return ("refuse", book.refusals[int(rng.integers(len(book.refusals)))])
    if kind == "scene_dynamic":
        return ("scene_dynamic", int(rng.integers(len(DYNAMIC_VARIANTS))))
    if kind == "scene_static":
        return ("scene_static", int(rng.integers(2)))
    if kind == "retarget_request":
        return ("retarget_request", int(rng.integers(1, 50)), bool(rng.random() < 0.3),
                SPHERE_CHOICES[int(rng.integers(4))], CONSTRAINT_CHOICES[int(rng.integers(4))])
    return (kind,)


# ---------------------------------------------------------------------------- group bookkeeping
GROUP_REQUEST_KINDS = ("g_retarget_requests", "m_retarget_request", "g_refused_model")


def _layout(choice):
    """the sphere layout a request's choice gives: radius_only keeps the base list's"""
    return "attach" if choice == "attach" else "base"

GROUP_KINDS = ("g_run", "g_run_refused", "g_synchronize", "g_optimize", "g_retarget", "observe", "m_set_theta",
               "m_execute", "m_retarget", "m_iterate")


class GroupBook:
    """What the generator knows of a group of P engines: per member the fields stomp_group_run
    compares before it accepts a run (a pending noiseless rollout's member, the iteration whose rows
    were made ahead, and with reuse the two generateRollouts flags), the fields both sides define,
    and the next iteration number.  The group is in lockstep when the members' tuples agree."""

    def __init__(self, info):
        self.P, self.Kr, self.cums, self.max_its = info["P"], info["Kr"], info["cums"], info["max_its"]
        self.serve = info.get("serve", False)
        self.request = info.get("request", False)
        self.ask, self.nseg = info.get("ask", False), info.get("nseg", 0)
        self.kinds = (GROUP_KINDS + (("g_serve",) if self.serve else ()) + (GROUP_REQUEST_KINDS if self.request else ())
                      + (GROUP_ASK_QUERIES + DESCENT_KINDS if self.ask else ()))
        self.descent = "none"       # of the descent on member DESCENT_MEMBER's engine
        # the request mode: members that replaced a list of their model on their own since the last
        # g_retarget_requests (the group's copies of the models are behind them), and every
        # member's sphere layout (the engines a group plans are of one shape)
        self.stale, self.layout = set(), ["base"] * info["P"]
        self.split = False    # a g_serve of fewer requests than slots left the members in different states
        self.sig = [(-1, -1, False) for _ in range(self.P)]     # (pending member, pre_it, reused_next = extra_added)
        self.valid = [set(ALWAYS) for _ in range(self.P)]
        self.next_it = 1
        self.lead = None      # (member, it): a member's own iterate the others have not followed yet
        self.refused = False  # the refused group.run of this excursion was made

    def lockstep(self):
        return all(s == self.sig[0] for s in self.sig)

    def _behind(self):
        """members that have not made the leader's iterate yet"""
        return [m for m in range(self.P) if self.sig[m] != self.sig[self.lead[0]]] if self.lead else []

    def allowed(self, kind):
        if kind in DESCENT_KINDS:
            return self.ask and descent_allows(self.descent, kind)
        if kind == "g_refused_model":
            return self.request and bool(self.stale)
        if self.stale and kind in ("g_run", "g_run_refused", "g_synchronize", "g_optimize", "g_retarget", "g_serve"):
            return False      # refused until a g_retarget_requests (g_refused_model asserts it)
        if kind == "m_retarget_request":
            return self.request and self.lead is None      # (as m_retarget)
        if kind == "g_run":
            return self.lockstep()
        if kind == "g_run_refused":
            return (self.lead is not None or self.split) and not self.lockstep() and not self.refused
        if kind == "g_optimize":
            return self.lockstep()
        if kind == "m_iterate":
            # one member leaves lockstep; until the others have followed, only they may iterate
            return self.lockstep() or (self.lead is not None and bool(self._behind()))
        if kind == "m_retarget":
            return self.lead is None      # (inside an excursion the followers are told by their tuples)
        return kind in self.kinds

    def _iterated(self, m):
        self.valid[m] |= set(ROW_KEYS) | set(X_KEYS)
        if self.cums[m]:
            self.valid[m].add("cumulative")

    def apply(self, op):
        kind = op[0]
        assert self.allowed(kind), (op, self.sig)
        reuse = self.Kr > 0
        if kind == "g_run":
            first, count = op[1], op[2]
            assert first >= 1 and 1 <= count <= 4
            for m in range(self.P):
                self.sig[m] = (first + count - 2, first + count, reuse)
                self._iterated(m)
            self.next_it, self.lead = first + count, None
        elif kind == "g_run_refused":
            self.refused = True
        elif kind == "g_synchronize":
            self.sig = [(-1,) + s[1:] for s in self.sig]
        elif kind == "g_optimize":
            for m in range(self.P):
                self.sig[m] = (-1, -1, reuse)
                self._iterated(m)
            self.next_it, self.lead = max(self.max_its) + 1, None
        elif kind == "g_serve":
            # slots 0 .. min(n, P) - 1 are as after g_optimize; the others keep their state
            n = op[2]
            assert self.serve and n >= 1, op      # (the generator draws 1 .. 2P + 2; a literal script may queue more)
            for m in range(min(n, self.P)):
                self.sig[m] = (-1, -1, reuse)
                self._iterated(m)
            self.lead, self.refused = None, False
            if self.lockstep():
                self.next_it = max(self.max_its) + 1
        elif kind in ("g_retarget", "g_retarget_requests"):
            if kind == "g_retarget_requests":
                assert len(op[3]) == self.P and all(s in SPHERE_CHOICES and c in CONSTRAINT_CHOICES for s, c in op[3]), op
                self.layout = [self.layout[m] if s == "keep" else _layout(s) for m, (s, _) in enumerate(op[3])]
                assert len(set(self.layout)) == 1, (op, self.layout)
                self.stale = set()
            self.sig = [(-1, -1, False) for _ in range(self.P)]
            self.valid = [set(ALWAYS) for _ in range(self.P)]
            self.next_it, self.lead = 1, None
        elif kind == "observe":
            members = range(self.P) if op[1] < 0 else [op[1]]
            for m in members:
                assert op[2] and set(op[2]) <= self.valid[m], (op, sorted(self.valid[m]))
                if set(op[2]) & set(FLUSHING):
                    self.sig[m] = (-1,) + self.sig[m][1:]
        elif kind == "m_set_theta":
            self.sig[op[1]] = (-1,) + self.sig[op[1]][1:]
        elif kind in ("m_retarget", "m_retarget_request"):
            if kind == "m_retarget_request":
                assert op[4] in SPHERE_CHOICES and op[5] in CONSTRAINT_CHOICES, op
                if (op[4], op[5]) != ("keep", "keep"):      # (both lists kept: the plain path, no model change)
                    self.stale.add(op[1])
                if op[4] != "keep":
                    self.layout[op[1]] = _layout(op[4])
            self.sig[op[1]] = (-1, -1, False)
            self.valid[op[1]] = set(ALWAYS)
        elif kind == "m_iterate":
            m, it = op[1], op[2]
            if self.lead is None or self.lockstep():
                self.lead, self.refused = (m, it), False
            else:
                assert m in self._behind() and it == self.lead[1], (op, self.lead)
            self.sig[m] = (-1, it + 1, reuse)
            self._iterated(m)
            if self.lockstep():
                self.next_it, self.lead = it + 1, None
        elif kind in GROUP_ASK_QUERIES:
            assert self.ask and 0 <= op[1] < self.P, op
            _check_query(op[:1] + op[2:], self.nseg)
        elif kind in DESCENT_KINDS:
            self.descent = descent_after(self.descent, op)
        else:
            assert kind in ("m_execute", "g_refused_model"), kind
        # what makes the descent stale: a retarget of its member, a serve whose turnovers reach its slot
        if (kind in ("g_retarget", "g_retarget_requests") or (kind in ("m_retarget", "m_retarget_request") and op[1] == DESCENT_MEMBER)
                or (kind == "g_serve" and min(op[2], self.P) > DESCENT_MEMBER)):
            self.descent = descent_staled(self.descent, "target")
        if self.lead is not None and self.lockstep():
            self.lead = None
        if kind == "g_serve" or self.lockstep():
            self.split = not self.lockstep()

    def final_ops(self):
        ops = [("g_refused_model",) if self.stale else ("g_synchronize",)]
        for m in range(self.P):
            ops.append(("observe", m, tuple(k for k in OBS_ORDER if k in self.valid[m])))
        if self.ask and descent_allows(self.descent, "chomp_get"):
            ops.append(("chomp_get", ("trajectory", "final_increments", "cost")))
        return ops


def _group_op(book, kind, rng):
    P = book.P
    m = int(rng.integers(P))
    if kind in GROUP_ASK_QUERIES:
        op = _ask_op(kind[2:], book.descent, book.nseg, rng)
        return (kind, m) + op[1:]
    if kind in DESCENT_KINDS:
        return _ask_op(kind, book.descent, book.nseg, rng)
    if kind in ("g_run", "g_run_refused"):
        first = book.next_it if rng.random() < 0.8 else max(book.next_it + int(rng.integers(-1, 2)), 1)
        return (kind, first, int(rng.integers(1, 5)))
    if kind == "g_retarget":
        return ("g_retarget", int(rng.integers(1, 50)), bool(rng.random() < 0.3))
    if kind == "g_serve":
        return ("g_serve", int(rng.integers(1 << 20)), int(rng.integers(1, 2 * P + 3)))
    if kind == "g_retarget_requests":
        # one layout for the group: a member may keep its list only if it has that layout already
        attach = bool(rng.random() < 0.5)
        choices = []
        for i in range(P):
            opts = ["attach"] if attach else ["base", "radius_only"]
            if book.layout[i] == ("attach" if attach else "base"):
                opts.append("keep")
            choices.append((opts[int(rng.integers(len(opts)))], CONSTRAINT_CHOICES[int(rng.integers(4))]))
        return ("g_retarget_requests", int(rng.integers(1, 50)), bool(rng.random() < 0.3), tuple(choices))
    if kind == "m_retarget_request":
        return ("m_retarget_request", m, int(rng.integers(1, 50)), bool(rng.random() < 0.3),
                SPHERE_CHOICES[int(rng.integers(4))], CONSTRAINT_CHOICES[int(rng.integers(4))])
    if kind == "observe":
        who = -1 if rng.random() < 0.3 else m
        common = set.intersection(*book.valid) if who < 0 else book.valid[who]
        valid = [k for k in OBS_ORDER if k in common]
        pick = [k for k in valid if rng.random() < 0.4] or [valid[int(rng.integers(len(valid)))]]
        return ("observe", who, tuple(pick))
    if kind == "m_set_theta":
        return ("m_set_theta", m, int(rng.integers(1 << 20)))
    if kind == "m_execute":
        return ("m_execute", m, int(rng.integers(1 << 20)), int(rng.integers(1, 4)), int(rng.integers(0, 3)))
    if kind == "m_retarget":
        return ("m_retarget", m, int(rng.integers(1, 50)), bool(rng.random() < 0.3))
    if kind == "m_iterate":
        if book.lead is not None and not book.lockstep():
            behind = book._behind()
            return ("m_iterate", behind[int(rng.integers(len(behind)))], book.lead[1])
        return ("m_iterate", m, book.next_it)
    return (kind,)


# ---------------------------------------------------------------------------- rank bookkeeping
RANK_KINDS = ("iterate", "run", "synchronize", "observe", "set_theta", "execute", "optimize", "refuse")
RANK_REFUSALS = ("pi_get_rollouts", "pi_set_rollout_costs", "pi_improve_policy", "pi_add_extra_rollout", "pi_reset",
                 "retarget")


class RankBook(Book):
    """Two ranks of one problem: the calls ranks accept; the step API and retarget only refused."""

    def __init__(self, info):
        super().__init__(info)
        self.kinds = RANK_KINDS + (ASK_QUERIES if self.ask else ())
        self.refusals = RANK_REFUSALS + (("chomp_create",) if self.ask else ())

    def allowed(self, kind):
        return kind in self.kinds

    def apply(self, op):
        if op[0] == "refuse":
            assert op[1] in self.refusals
        elif op[0] in ASK_QUERIES:      # the last argument: the rank that answers
            assert self.ask and op[-1] in (0, 1), op
            _check_query(op[:-1], self.nseg)
        else:
            super().apply(op)


def _rank_op(book, kind, rng):
    if kind == "refuse":
        return ("refuse", book.refusals[int(rng.integers(len(book.refusals)))])
    if kind in ASK_QUERIES:
        return _ask_op(kind, "none", book.nseg, rng) + (int(rng.integers(2)),)
    return _single_op(book, kind, rng)


# ---------------------------------------------------------------------------- generation
_INFO = {}


def mode_info(mode):
    """What the bookkeeping needs of a mode's problems (built once: generation reads them only)."""
    if mode not in _INFO:
        spec = MODES[mode]
        if "info" in spec:      # (a mode whose problems are slow to build says what its book needs)
            _INFO[mode] = dict(spec["info"], serve=spec.get("serve", False), ask=spec.get("ask", False))
            return _INFO[mode]
        made = spec["make"]()
        if spec["kind"] == "group":
            _INFO[mode] = dict(serve=spec.get("serve", False), request=spec.get("request", False), P=len(made), Kr=made[0].params.num_reused_rollouts,
                               cums=[bool(p.params.use_cumulative_costs) for p in made],
                               max_its=[p.params.max_iterations for p in made])
        else:
            _INFO[mode] = dict(Kr=made.params.num_reused_rollouts, cum=bool(made.params.use_cumulative_costs),
                               max_it=made.params.max_iterations, device=spec.get("device_field", False),
                               request=spec.get("request", False), scene=spec.get("scene", False),
                               ask=spec.get("ask", False), nseg=len(made.robot.segments),
                               brick=spec["env"].get("STOMP_SDF_LAYOUT") == "brick")
    return _INFO[mode]


def new_book(mode):
    kind = MODES[mode]["kind"]
    return {"single": Book, "group": GroupBook, "ranks": RankBook}[kind](mode_info(mode))


def kinds_of(mode):
    return new_book(mode).kinds


def _walk(mode, rng, length, seen):
    book = new_book(mode)
    make_op = {"single": _single_op, "group": _group_op, "ranks": _rank_op}[MODES[mode]["kind"]]
    script, prev = [], None
    for _ in range(length):
        kinds = [k for k in book.kinds if book.allowed(k)]
        ops, w = [], []
        for k in kinds:
            # a candidate op of every kind the bookkeeping allows; its weight: 1, a hundred more for
            # a pair of kinds no script of this mode has shown yet, and five more for every such
            # pair that could follow it
            op = make_op(book, k, rng)
            after = copy.deepcopy(book)
            after.apply(op)
            ahead = sum(1 for k2 in after.kinds if after.allowed(k2) and (k, k2) not in seen)
            ops.append(op)
            w.append(1.0 + (100.0 if prev is not None and (prev, k) not in seen else 0.0) + 5.0 * ahead)
        w = np.array(w)
        op = ops[int(rng.choice(len(ops), p=w / w.sum()))]
        book.apply(op)
        if prev is not None:
            seen.add((prev, op[0]))
        script.append(op)
        prev = op[0]
    return script


_SCRIPTS = {}


def make_script(mode, seed, length=None):
    """The script of (mode, seed): the walks of the seeds 0 .. seed in turn, each steered away from
    the pairs of op kinds the ones before it showed (kept per process; the result depends on the
    arguments alone)."""
    length = length_of(mode) if length is None else length
    ident = IDENTS[mode]
    if (mode, length) not in _SCRIPTS:
        # an ask mode's walks are steered to the pairs its census counts: those with an ask.  Pairs
        # of two old kinds are the old modes' business and count as shown from the start.
        old = [k for k in kinds_of(mode) if k not in ASKS] if MODES[mode].get("ask") else []
        _SCRIPTS[(mode, length)] = ([], {(a, b) for a in old for b in old})
    made, seen = _SCRIPTS[(mode, length)]
    while len(made) <= seed:
        made.append(_walk(mode, np.random.default_rng([ident, len(made), length]), length, seen))
    return list(made[seed])


def final_ops(mode, script):
    """The full observe of everything both sides define after the script (groups and ranks: after a
    synchronize)."""
    book = new_book(mode)
    for op in script:
        book.apply(op)
    if MODES[mode]["kind"] == "group":
        return book.final_ops()
    if MODES[mode]["kind"] == "ranks":
        return [("synchronize",), book.final_observe()]
    return book.final_ops()


# Ordered pairs of kinds that no valid script holds, with the rule that excludes them.  The census
# asserts that exactly these are missing.
def impossible_pairs(mode):
    kind = MODES[mode]["kind"]
    out = {}
    if kind == "single":
        kinds = kinds_of(mode)
        opens = ("pi_get_rollouts", "pi_set_rollout_costs")     # leave a step round open
        closes = FUSED + ("pi_improve_policy", "pi_add_extra_rollout", "retarget")   # leave it closed
        if "retarget_request" in kinds:      # the book treats it as retarget
            closes += ("retarget_request",)
            out[("retarget_request", "pi_add_extra_rollout")] = "a fresh PolicyImprovement has no control cost weight yet"
        for a in opens:
            for b in FUSED + ("pi_get_rollouts", "pi_add_extra_rollout"):
                out[(a, b)] = "between pi_get_rollouts and pi_improve_policy the oracle's rows hold no control costs yet"
        out[("pi_get_rollouts", "pi_improve_policy")] = "pi_improve_policy needs the round's pi_set_rollout_costs"
        for a in closes:
            out[(a, "pi_set_rollout_costs")] = "pi_set_rollout_costs needs a pi_get_rollouts since the last fused iteration"
            out[(a, "pi_improve_policy")] = "pi_improve_policy needs the round's pi_set_rollout_costs"
        out[("retarget", "pi_add_extra_rollout")] = "a fresh PolicyImprovement has no control cost weight yet"
        if "refresh_field" in kinds:
            out[("run", "refresh_field")] = "the pending noiseless rollout would read the new field"
        for b in SCENE_KINDS:
            if b in kinds:
                out[("run", b)] = "the pending noiseless rollout would read the new field"
    elif kind == "group":
        for b in ("g_run", "g_optimize"):
            out[("g_run_refused", b)] = "the group is out of lockstep until every member has followed the leader"
        for a in ("g_run", "g_optimize", "g_retarget"):
            out[(a, "g_run_refused")] = "a refused run needs a member ahead of the others"
        out[("g_run_refused", "g_run_refused")] = "one refused run per excursion"
        for pair in (("g_run_refused", "m_retarget"), ("m_retarget", "g_run_refused")):
            out[pair] = "no member retargets while the others still follow a member's own iterate"
        if "g_refused_model" in kinds_of(mode):
            level = ("g_run", "g_synchronize", "g_optimize", "g_retarget", "g_retarget_requests")
            for a in level:
                out[(a, "g_refused_model")] = "the call was accepted: no member's model is ahead of the group's copy"
            for b in ("g_run", "g_run_refused", "g_synchronize", "g_optimize", "g_retarget"):
                out[("g_refused_model", b)] = "a member's model stays ahead of the group's copy until g_retarget_requests"
            out[("g_run_refused", "g_refused_model")] = "a run refused for the iteration state was not refused for a model"
            out[("g_retarget_requests", "g_run_refused")] = "a refused run needs a member ahead of the others"
            for pair in (("g_run_refused", "m_retarget_request"), ("m_retarget_request", "g_run_refused")):
                out[pair] = "no member retargets while the others still follow a member's own iterate"
        if "g_serve" in kinds_of(mode):
            # a g_serve of fewer requests than slots leaves members in different states with no
            # leader to follow: a refused run may follow it, and a member's retarget may stand on
            # either side of that refused run.  g_serve itself is accepted in every state, and
            # every kind can follow one (n >= P levels the group, n < P may split it): no new pair
            del out[("g_run_refused", "m_retarget")], out[("m_retarget", "g_run_refused")]
    if "chomp_reset" in kinds_of(mode):
        # ops after which the descent is stale whatever their arguments (a member's own retarget
        # and a serve stale it only when they reach its member)
        staling = {"single": ("retarget", "retarget_request") + SCENE_KINDS, "group": ("g_retarget",)}[kind]
        for a in staling:
            if a in kinds_of(mode):
                for b in ("chomp_step", "chomp_get", "chomp_optimize"):
                    out[(a, b)] = "the descent is stale: only chomp_refused and chomp_reset may follow"
        out[("chomp_reset", "chomp_refused")] = "a fresh descent refuses nothing"
        out[("chomp_refused", "chomp_optimize")] = "no refusal leaves a fresh descent"
        for a in ("chomp_step", "chomp_optimize"):
            out[(a, "chomp_optimize")] = "the loop starts from a fresh reset (chomp_refused asserts the refusal)"
        out[("chomp_optimize", "chomp_step")] = ("tests/chomp_ref.c restates one descent, and its cr_step knows no stopped "
                                                 "descent: stepping behind a loop has no reference")
    return out


# ---------------------------------------------------------------------------- pairs
def _expect_refusal(fn, code, word):
    try:
        fn()
    except RuntimeError as ex:
        assert f"error {code}" in str(ex) and word in str(ex), str(ex)
        return
    raise AssertionError(f"the call was accepted; expected error {code} ({word})")


def _assert_stats(a, b, tag):
    """(stomp_stats, costs) of an optimize against another's: integer statistics, best_cost, history."""
    for k in gu.INT_STATS:
        assert int(getattr(a[0], k)) == int(getattr(b[0], k)), (tag, k, getattr(a[0], k), getattr(b[0], k))
    assert a[0].best_cost == b[0].best_cost, (tag, a[0].best_cost, b[0].best_cost)
    np.testing.assert_array_equal(a[1], b[1], err_msg=f"{tag} cost history")


def _execute_rows(p, theta, op_seed, nrows):
    return mz.execute_rows(p, theta, rows=nrows, seed=op_seed)


def _oracle_execute(o, rows, member):
    out = [o.execute(r, member) + (o.last_constraints_satisfied,) for r in rows]
    return (np.stack([r[0] for r in out]), np.array([r[1] for r in out]), np.stack([r[2] for r in out]),
            np.array([r[3] for r in out]))


def _assert_execute(e, want, rows, member, terms, tag):
    c, cf, tr = e.execute(rows, member)
    np.testing.assert_array_equal(c, want[0], err_msg=f"{tag} costs")
    np.testing.assert_array_equal(cf, want[1], err_msg=f"{tag} collision flags")
    np.testing.assert_array_equal(tr, want[2], err_msg=f"{tag} trajectories")
    if terms:
        np.testing.assert_array_equal(e.last_constraints_satisfied, want[3], err_msg=f"{tag} constraints flags")


def _subset(res, ref, want, tag):
    for k in want:
        a, b = getattr(res, k), getattr(ref, k)
        assert a is not None and a.shape == b.shape, (tag, k, None if a is None else a.shape, b.shape)
        np.testing.assert_array_equal(a, b, err_msg=f"{tag} {k}")


class Asks:
    """The asks of a pair: state queries, gradient queries and one CHOMP object that lives through
    the walk.  Each takes the engine asked, that engine's current problem with its current field, and
    (a reset from theta) its oracle; the oracle side of the pair never hears of an ask.  With no
    engine (the CPU tests) an ask does nothing."""
    chomp_params = _CHOMP_PLAIN
    ch = None

    def ask_query_states(self, e, p, seed, M, links, want, tag=""):
        if e is None:
            return
        q = squ.make_states(p, M, seed)
        res = e.query_states(q, links=list(links) or None, want=want)
        _subset(res, squ.reference(p, q, list(links)), want, f"{tag}query_states")
        for k in QS_OUTPUTS:      # and nothing that was not asked for
            assert k in want or getattr(res, k) is None, k

    def ask_query_gradients(self, e, p, seed, M, links, want, biased, tag=""):
        if e is None:
            return
        q = squ.make_states(p, M, seed)
        bias = gqu.BIAS if biased else (0.0, 0.0, 0.0)
        res = e.query_gradients(q, links=list(links) or None, field_bias=bias, want=want)
        _subset(res, gqu.reference(p, q, list(links), bias), want, f"{tag}query_gradients")
        for k in GQ_OUTPUTS:
            assert k in want or getattr(res, k) is None, k

    def _chomp(self, e):
        if self.ch is None:
            prm = self.chomp_params
            self.ch = eng.Chomp(e, learning_rate=prm.learning_rate, smoothness_cost_weight=prm.smoothness_cost_weight,
                                use_pseudo_inverse=prm.use_pseudo_inverse,
                                pseudo_inverse_ridge_factor=prm.pseudo_inverse_ridge_factor, field_bias=prm.field_bias,
                                joint_update_limits=prm.limits(e.J))
            self.ch_sizes, self.refs = [], []
        assert self.ch.engine is e
        return self.ch

    def close_chomp(self):
        if self.ch is not None:
            self.ch.close()
            self.ch = None

    def ask_chomp_reset(self, e, p, o, B, source):
        if e is None:
            return
        ch = self._chomp(e)
        # the reference: a new ChompRef of the current problem and field per descent; a reset from
        # theta starts at the ORACLE's theta, which is what "as they are on its stream" must equal
        starts = [o.theta() if source is None else cu.noisy_start(p, source + b) for b in range(B)]
        self.refs = []
        for t in starts:
            r = cu.ChompRef(p, self.chomp_params)
            r.reset(t)
            self.refs.append(r)
        before = ch.info()["allocations"]
        if source is None:
            ch.reset(None, num_trajectories=B)
        else:
            ch.reset(np.stack(starts))
        # the capacity rule: the slabs grow with B and S alone (J, N, the segments and max_iterations
        # stay), so a reset that an earlier one covers in both allocates nothing
        S = len(p.spheres)
        assert e.S == S, (e.S, S)
        if any(B <= b and S <= s for b, s in self.ch_sizes):
            assert ch.info()["allocations"] == before, (B, S, self.ch_sizes, before, ch.info())
        self.ch_sizes.append((B, S))
        assert ch.info()["B"] == B and ch.info()["iterations"] == 0

    def ask_chomp_step(self, e, count):
        if e is None:
            return
        self.ch.step(count)      # enqueued: nothing waits
        for r in self.refs:
            r.step(count)

    def ask_chomp_get(self, e, names):
        if e is None:
            return
        for name in names:
            got = self.ch.get(name)
            assert len(got) == len(self.refs), (name, got.shape, len(self.refs))
            for b, r in enumerate(self.refs):
                ref = r.get(name)
                assert got[b].shape == np.shape(ref), (name, got[b].shape, np.shape(ref))
                np.testing.assert_array_equal(got[b], ref, err_msg=f"chomp_get descent {b} {name}")

    def ask_chomp_optimize(self, e):
        if e is None:
            return
        out = self.ch.optimize()
        assert len(out) == len(self.refs)
        for b, ((st, costs, best), r) in enumerate(zip(out, self.refs)):
            rst, rcosts, rbest = r.optimize()
            assert cu.stats_tuple(st) == cu.stats_tuple(rst), (b, cu.stats_tuple(st), cu.stats_tuple(rst))
            np.testing.assert_array_equal(costs, rcosts, err_msg=f"chomp_optimize descent {b} cost history")
            np.testing.assert_array_equal(best, rbest, err_msg=f"chomp_optimize descent {b} best trajectory")

    def ask_chomp_refused(self, e, why):
        if e is None:
            return
        ch = self._chomp(e)
        word = {"no_reset": "no reset", "stale_target": "retargeted or its field refreshed", "stale_model": "model changed",
                "needs_fresh_reset": "fresh reset"}[why]
        if why == "needs_fresh_reset":
            _expect_refusal(ch.optimize, -1, word)
            return
        for call in (lambda: ch.step(1), ch.optimize, lambda: ch.get("cost")):
            _expect_refusal(call, -1, word)
        # and get wrote nothing
        out = np.full(max(ch.B, 1) * e.J * e.N, -7.25)
        l = eng.load_library()
        assert l.stomp_chomp_get(ch.h, b"trajectory", eng._dp(out)) == -1 and word.encode() in l.stomp_chomp_last_error(ch.h)
        assert (out == -7.25).all()


class Pair(Asks):
    """One engine (None: the oracle alone, for the CPU tests) and its oracle."""

    def __init__(self, problem, engine=None, threads=1, field=None, scene=None, stream=None, brick=False):
        self.p0 = self.p = problem
        self.e, self.threads, self.field = engine, threads, field
        # a scene mode: the field is the scene's, on the stream it shares with the engine
        self.scene, self.stream, self.brick = scene, stream, brick
        self.layer, self.dynamic, self.fields = 0, 0, {}
        self.cur_sdf = np.array(problem.sdf, np.uint16)
        self.o = self._oracle(problem)
        self.it, self.K_gen = 1, problem.params.num_rollouts

    def _oracle(self, p):
        # a field of its own: Oracle.refresh_field writes the array it was created on
        return po.Oracle(dataclasses.replace(p, sdf=self.cur_sdf.copy()), threads=self.threads)

    def close(self):
        self.close_chomp()      # it borrows the engine
        if self.e is not None:
            self.e.close()
        if self.scene is not None:
            self.scene.close()
        if self.field is not None:
            self.field.free()
        if self.stream is not None:
            self.stream.close()

    # -------------------------------------------------------------- ops
    def op_iterate(self, it):
        self.it = it
        ro = self.o.iterate(it)
        if self.e is not None:
            re_ = self.e.iterate(it)
            assert re_ == ro, (re_, ro)
            if has_terms(self.p):
                assert self.e.last_constraints_satisfied == bool(self.o.last_constraints_satisfied)

    def op_run(self, first, count):
        for it in range(first, first + count):
            self.o.iterate(it)
        self.it = first + count - 1
        if self.e is not None:
            self.e.run(first, count)

    def op_synchronize(self):
        if self.e is not None:
            self.e.synchronize()

    def op_observe(self, keys):
        for k in keys:
            if k == "cumulative":
                if self.e is not None:
                    cum = self.e.rollouts("cumulative_costs")
                    np.testing.assert_array_equal(cum, numpy_cumulative(self.e), err_msg="cumulative_costs against numpy")
                continue
            want = _get(self.o, k)
            if self.e is not None:
                np.testing.assert_array_equal(_get(self.e, k), want, err_msg=k)

    def op_set_theta(self, seed):
        th = su.walk(np.random.default_rng(seed), self.o.theta(), 0.01)
        self.o.set_theta(th)
        if self.e is not None:
            self.e.set_theta(th)

    def op_execute(self, seed, nrows, member):
        rows = _execute_rows(self.p, self.o.theta(), seed, nrows)
        want = _oracle_execute(self.o, rows, member)
        if self.e is not None:
            _assert_execute(self.e, want, rows, member, has_terms(self.p), "execute")

    def op_pi_get_rollouts(self, it):
        self.it = it
        sig = su.sigma(self.p, it)
        ro = self.o.pi_get_rollouts(it, sig)
        self.K_gen = len(ro)
        if self.e is not None:
            re_ = self.e.pi_get_rollouts(it, sig)
            assert len(re_) == len(ro), (len(re_), len(ro))
            np.testing.assert_array_equal(re_, ro, err_msg="rollouts")

    def op_pi_set_rollout_costs(self, mult):
        rows = self.o.rollouts("params")[: self.K_gen]
        costs = np.stack([self.o.execute(r, self.it - 1)[0] for r in rows])
        w = mult * self.p.params.smoothness_cost_weight
        to = self.o.pi_set_rollout_costs(costs, w)
        if self.e is not None:
            np.testing.assert_array_equal(self.e.pi_set_rollout_costs(costs, w), to, err_msg="totals")

    def op_pi_improve_policy(self):
        uo = self.o.pi_improve_policy()
        if self.e is not None:
            np.testing.assert_array_equal(self.e.pi_improve_policy(), uo, err_msg="update")

    def op_pi_add_extra_rollout(self, seed):
        th = self.o.theta()
        xp = th if seed is None else su.walk(np.random.default_rng(seed), th)
        xc = self.o.execute(xp, max(self.it - 1, 0))[0]
        self.o.pi_add_extra_rollout(xp, xc)
        if self.e is not None:
            self.e.pi_add_extra_rollout(xp, xc)

    def op_pi_reset(self):
        self.o.pi_reset()
        if self.e is not None:
            self.e.pi_reset()

    def op_optimize(self):
        ro = self.o.optimize()
        self.it = self.p.params.max_iterations
        if self.e is not None:
            _assert_stats(self.e.optimize(), ro, "optimize")

    def op_retarget(self, k, keep_seed):
        # (a plain retarget keeps the model a request gave the engine)
        q = dataclasses.replace(moved(self.p0, k), spheres=list(self.p.spheres),
                                orientation_constraints=list(self.p.orientation_constraints))
        if keep_seed:
            q = dataclasses.replace(q, seed=self.p.seed)
        if self.e is not None:
            self.e.retarget(q.start, q.goal, None if keep_seed else q.seed)
            assert self.e.problem.seed == q.seed
        self.p = q
        self.o = self._oracle(q)
        self.it, self.K_gen = 1, q.params.num_rollouts

    def op_retarget_request(self, k, keep_seed, spheres, constraints):
        q = moved(self.p0, k)
        if keep_seed:
            q = dataclasses.replace(q, seed=self.p.seed)
        sph = None if spheres == "keep" else request_spheres(self.p0, spheres)
        oc = None if constraints == "keep" else mz.fork12_constraints()[:constraints]
        q = dataclasses.replace(q, spheres=list(self.p.spheres if sph is None else sph),
                                orientation_constraints=list(self.p.orientation_constraints if oc is None else oc))
        e = self.e
        if e is not None:
            seed = None if keep_seed else q.seed
            if sph is None and oc is None:
                # both lists kept: the plain path, through the request's entry point
                s, g = np.ascontiguousarray(q.start, np.float64), np.ascontiguousarray(q.goal, np.float64)
                req, _ = e._request(s, g, int(q.seed), None, None)
                assert req.num_spheres == -1 and req.num_orientation_constraints == -1
                rc = eng.load_library().stomp_engine_retarget_request(e.h, C.byref(req))
                assert rc == 0, (rc, eng.load_library().stomp_last_error())
                e._follow(s, g, int(q.seed))
            else:
                e.retarget(q.start, q.goal, seed, spheres=sph, orientation_constraints=oc)
            info = e.model_info()
            assert e.problem.seed == q.seed and e.S == len(q.spheres) == info["S"], (e.S, len(q.spheres), info)
            assert info["orientation_constraints"] == len(q.orientation_constraints), info
            assert info["terms_on"] == int(has_terms(q)), info
        self.p = q
        self.o = self._oracle(q)
        self.it, self.K_gen = 1, q.params.num_rollouts

    def op_refresh_field(self, extra):
        objs = scene_objects(self.p0, extra)
        grid = self.p0.grid
        if self.e is not None:
            eng.sdf_build_objects_device(grid, objs, self.field.ptr)
            new = self.field.to_numpy(np.uint16, tuple(grid.dims))
            self.e.refresh_field()
        else:
            new = po.sdf_build_objects(grid, objs)[0]
        assert not np.array_equal(new, self.cur_sdf), "the scene must change"
        self.cur_sdf = new.copy()
        self.o.refresh_field(new)

    def scene_field(self, layer, dynamic):
        """the oracle's full build of a static layer and a dynamic set (kept: a walk returns to them)"""
        if (layer, dynamic) not in self.fields:
            objs = scene_static_layer(self.p0, layer) + scene_dynamic_set(self.p0, dynamic)
            self.fields[(layer, dynamic)] = po.sdf_build_objects(self.p0.grid, objs)[0]
        return self.fields[(layer, dynamic)]

    def _scene_changed(self, layer, dynamic):
        # whether the field changes is known from the inputs: no mark of `none` and `outside` lands
        empty = ("none", "outside")
        same = layer == self.layer and (dynamic == self.dynamic or
                                        (DYNAMIC_VARIANTS[dynamic] in empty and DYNAMIC_VARIANTS[self.dynamic] in empty))
        new = self.scene_field(layer, dynamic)
        assert np.array_equal(new, self.cur_sdf) == same, "the scene must change" if not same else "the scene must stay"
        self.layer, self.dynamic = layer, dynamic
        if self.e is not None and self.brick:
            self.e.refresh_field()      # the header's contract: the bricked copy follows the caller's buffer
        self.cur_sdf = new.copy()
        self.o.refresh_field(new.copy())

    def op_scene_dynamic(self, variant):
        if self.e is not None:
            self.scene.set_dynamic(scene_dynamic_set(self.p0, variant))      # enqueued: nothing waits
        self._scene_changed(self.layer, variant)

    def op_scene_static(self, which):
        if self.e is not None:
            self.scene.set_static(scene_static_layer(self.p0, which))        # drops the dynamic set
        self._scene_changed(which, 0)

    def op_scene_check(self):
        if self.e is not None:
            info = self.scene.info()        # waits for the scene's stream
            assert info["stray"] == 0, info
            np.testing.assert_array_equal(self.field.to_numpy(np.uint16, tuple(self.p0.grid.dims)), self.cur_sdf,
                                          err_msg="the scene's buffer against the oracle's field")

    def op_set_timing(self, on):
        if self.e is not None:
            self.e.set_timing(on)

    def op_refuse(self, what):
        e = self.e
        if e is None:
            return
        l = eng.load_library()
        if what == "nan_goal":
            before = e.problem
            goal = np.array(self.p.goal, np.float64)
            goal[self.p.J // 2] = np.nan
            _expect_refusal(lambda: e.retarget(self.p.start, goal), -1, "not finite")
            assert e.problem is before
        elif what in ("unordered_spheres", "bad_segment"):
            # a refused request: nothing of the engine is written, and the staging it shares with
            # the plain retarget stays usable by the next accepted call of either kind
            before, info = e.problem, e.model_info()
            bad = list(request_spheres(self.p0, "attach"))
            if what == "unordered_spheres":
                bad = bad[::-1]
                assert [s.segment for s in bad] != sorted(s.segment for s in bad)
                _expect_refusal(lambda: e.retarget(self.p.start, self.p.goal, spheres=bad), -3, "ordered by segment")
            else:
                bad[3] = dataclasses.replace(bad[3], segment=len(self.p.robot.segments))
                _expect_refusal(lambda: e.retarget(self.p.start, self.p.goal, spheres=bad), -1, "bad segment")
            assert e.problem is before and e.model_info() == info
        elif what == "extra_num0":
            th = np.ascontiguousarray(self.o.theta())
            assert l.stomp_pi_add_extra_rollouts(e.h, 0, eng._dp(th), eng._dp(np.zeros(self.p.N))) == -1
            assert b"one extra rollout" in l.stomp_engine_last_error(e.h)
        else:
            n = C.c_int32(-7)
            out = np.zeros((e.K, e.J, e.N))
            assert l.stomp_pi_get_rollouts(e.h, self.it + 1, None, eng._dp(out), C.byref(n)) == -1
            assert b"null noise_stddev" in l.stomp_engine_last_error(e.h) and n.value == -7 and not out.any()

    # -------------------------------------------------------------- asks
    def _asked(self):
        """the engine's current problem with its current field: after every retarget, request,
        refresh_field and scene op so far"""
        return dataclasses.replace(self.p, sdf=self.cur_sdf)

    def op_query_states(self, seed, M, links, want):
        self.ask_query_states(self.e, self._asked(), seed, M, links, want)

    def op_query_gradients(self, seed, M, links, want, biased):
        self.ask_query_gradients(self.e, self._asked(), seed, M, links, want, biased)

    def op_chomp_reset(self, B, source):
        self.ask_chomp_reset(self.e, self._asked(), self.o, B, source)

    def op_chomp_step(self, count):
        self.ask_chomp_step(self.e, count)

    def op_chomp_get(self, names):
        self.ask_chomp_get(self.e, names)

    def op_chomp_optimize(self):
        self.ask_chomp_optimize(self.e)

    def op_chomp_refused(self, why):
        self.ask_chomp_refused(self.e, why)

    def apply(self, op):
        getattr(self, "op_" + op[0])(*op[1:])

    def full_state(self):
        """Everything the oracle holds (the CPU purity test compares two oracles on it)."""
        st = {k: _get(self.o, k) for k in ALWAYS + ROW_KEYS + X_KEYS}
        st["reuse_log"] = self.o.reuse_log()
        return st


class GroupPair(Asks):
    """A group on one stream, twins that make the equivalent single-engine calls, and the oracles.
    The asks go to the group's engines alone: the twins and the oracles never hear of them."""

    def __init__(self, problems, threads=1, targets=None, **group_kw):
        self.ps0 = list(problems)
        self.ps = list(problems)
        self.threads = threads
        self.targets = targets      # problems whose start / goal every retarget and request draws from (None: moved())
        self.served = None          # the last g_serve's (requests, results)
        self.stale = set()          # members that replaced a list of their model on their own
        self.g = gu.Group(self.ps, **group_kw)
        self.twins = gu.twins_of(self.ps)
        self.os = [po.Oracle(p, threads=threads) for p in self.ps]

    def close(self):
        self.close_chomp()      # it borrows member DESCENT_MEMBER's engine
        gu.close_all(self.g, self.twins)

    def _refused_run(self, first, count):
        try:
            self.g.group.run(first, count)
        except RuntimeError as ex:
            assert "error -1" in str(ex) and "same iteration state" in str(ex), str(ex)
            return
        raise AssertionError("group.run was accepted with one member ahead of the others")

    def op_g_run(self, first, count):
        self.g.group.run(first, count)
        gu.advance(self.os, first, count)
        for t in self.twins:
            t.run(first, count)

    def op_g_run_refused(self, first, count):
        self._refused_run(first, count)

    def op_g_synchronize(self):
        self.g.group.synchronize()
        for t in self.twins:
            t.synchronize()

    def op_g_optimize(self):
        res = self.g.group.optimize()
        for i, (r, t, o) in enumerate(zip(res, self.twins, self.os)):
            _assert_stats(r, o.optimize(), f"engine {i} against its oracle,")
            _assert_stats(r, t.optimize(), f"engine {i} against its twin,")

    def _moved(self, m, k, keep_seed):
        if self.targets:
            t = self.targets[(k + m) % len(self.targets)]
            q = dataclasses.replace(self.ps0[m], start=t.start.copy(), goal=t.goal.copy(), seed=t.seed + 2000 + k + 50 * m)
        else:
            q = moved(self.ps0[m], k + 50 * m)
        # (a plain retarget keeps the model a request gave the engine)
        q = dataclasses.replace(q, spheres=list(self.ps[m].spheres), orientation_constraints=list(self.ps[m].orientation_constraints))
        return dataclasses.replace(q, seed=self.ps[m].seed) if keep_seed else q

    def _queue(self, seed, n, which):
        """n requests as (start, goal, seed), drawn from the op's seed (which: the targets' indices given)"""
        rng = np.random.default_rng(seed)
        out = []
        for r in range(n):
            if self.targets:
                t = self.targets[int(rng.integers(len(self.targets))) if which is None else which[r]]
                out.append((t.start.copy(), t.goal.copy(), int(t.seed + rng.integers(1, 1 << 16))))
            else:
                q = moved(self.ps0[r % len(self.ps0)], int(rng.integers(1, 1000)))
                out.append((q.start, q.goal, int(q.seed)))
        return out

    def _lists(self, m, spheres, constraints):
        """(sphere list, constraint list) of a request's choices for member m; None: kept"""
        sph = None if spheres == "keep" else group_request_spheres(self.ps0[m], spheres, m)
        oc = None if constraints == "keep" else mz.fork12_constraints()[:constraints]
        return sph, oc

    def _requested(self, m, k, keep_seed, sph, oc):
        q = self._moved(m, k, keep_seed)
        return dataclasses.replace(q, spheres=list(q.spheres if sph is None else sph),
                                   orientation_constraints=list(q.orientation_constraints if oc is None else oc))

    def _assert_model(self, m, q):
        for x, tag in ((self.g.engines[m], "engine"), (self.twins[m], "twin")):
            info = x.model_info()
            assert x.problem.seed == q.seed and x.S == len(q.spheres) == info["S"], (tag, m, info)
            assert info["orientation_constraints"] == len(q.orientation_constraints), (tag, m, info)
            assert info["terms_on"] == int(has_terms(q)), (tag, m, info)

    def op_g_retarget_requests(self, k, keep_seed, choices):
        P = len(self.ps)
        lists = [self._lists(m, *choices[m]) for m in range(P)]
        qs = [self._requested(m, k, keep_seed, *lists[m]) for m in range(P)]
        # (lists of None entries, never None itself: every request through stomp_group_retarget_requests)
        self.g.group.retarget([q.start for q in qs], [q.goal for q in qs], None if keep_seed else [q.seed for q in qs],
                              spheres=[l[0] for l in lists], orientation_constraints=[l[1] for l in lists])
        for m, q in enumerate(qs):
            self.twins[m].retarget(q.start, q.goal, q.seed, spheres=lists[m][0], orientation_constraints=lists[m][1])
            self._assert_model(m, q)
            self.os[m] = po.Oracle(q, threads=self.threads)
        self.ps = qs
        self.stale = set()

    def op_m_retarget_request(self, m, k, keep_seed, spheres, constraints):
        sph, oc = self._lists(m, spheres, constraints)
        q = self._requested(m, k, keep_seed, sph, oc)
        for x in (self.g.engines[m], self.twins[m]):
            x.retarget(q.start, q.goal, None if keep_seed else q.seed, spheres=sph, orientation_constraints=oc)
        self._assert_model(m, q)
        self.os[m] = po.Oracle(q, threads=self.threads)
        self.ps[m] = q
        if sph is not None or oc is not None:
            self.stale.add(m)

    def op_g_refused_model(self):
        assert self.stale
        first = min(self.stale)
        ps = self.ps
        calls = [lambda: self.g.group.run(1, 1), self.g.group.synchronize, self.g.group.optimize,
                 lambda: self.g.group.retarget([p.start for p in ps], [p.goal for p in ps])]
        for call in calls:
            _expect_refusal(call, -1, f"engine {first} of the group")
        for m, p in enumerate(ps):      # (the refused plain retarget followed nothing)
            assert self.g.engines[m].problem.seed == p.seed

    def op_g_serve(self, seed, n, which=None):
        P = len(self.ps)
        assert which is None or len(which) == n
        reqs = self._queue(seed, n, which)
        results = self.g.group.serve([r[0] for r in reqs], [r[1] for r in reqs], [r[2] for r in reqs])
        assert len(results) == n
        its, last = [], {}
        for r, (res, (start, goal, sd)) in enumerate(zip(results, reqs)):
            slot = res[0]
            assert 0 <= slot < P, (r, slot)
            # the planning slot's problem: its own model and parameters, the request's start, goal and seed
            q = dataclasses.replace(self.ps0[slot], start=start.copy(), goal=goal.copy(), seed=sd)
            o = po.Oracle(q, threads=self.threads)
            _assert_stats((res[2], res[3]), o.optimize(), f"request {r} on slot {slot} against its oracle,")
            np.testing.assert_array_equal(res[4], o.best_trajectory(), err_msg=f"request {r} on slot {slot}: best trajectory")
            its.append(int(res[2].iterations))
            last[slot] = (q, o)
        want_slot, want_start, _ = eng.serve_schedule(P, its)
        assert [res[0] for res in results] == want_slot, ([res[0] for res in results], want_slot, its)
        assert [res[1] for res in results] == want_start, ([res[1] for res in results], want_start, its)
        assert sorted(last) == list(range(min(n, P))), sorted(last)
        for slot, (q, o) in last.items():
            assert self.g.engines[slot].problem.seed == q.seed
            self.twins[slot].retarget(q.start, q.goal, q.seed)
            self.twins[slot].optimize()
            self.os[slot], self.ps[slot] = o, q
        self.served = (reqs, results)

    def op_g_retarget(self, k, keep_seed):
        qs = [self._moved(m, k, keep_seed) for m in range(len(self.ps))]
        self.g.group.retarget([q.start for q in qs], [q.goal for q in qs], None if keep_seed else [q.seed for q in qs])
        for m, q in enumerate(qs):
            assert self.g.engines[m].problem.seed == q.seed
            self.twins[m].retarget(q.start, q.goal, q.seed)
            self.os[m] = po.Oracle(q, threads=self.threads)
        self.ps = qs

    def op_observe(self, who, keys):
        for m in (range(len(self.ps)) if who < 0 else [who]):
            ge, te, o, p = self.g.engines[m], self.twins[m], self.os[m], self.ps[m]
            for k in keys:
                if k == "cumulative":
                    cum = ge.rollouts("cumulative_costs")
                    np.testing.assert_array_equal(cum, numpy_cumulative(ge), err_msg=f"engine {m} cumulative_costs, numpy")
                    np.testing.assert_array_equal(cum, te.rollouts("cumulative_costs"), err_msg=f"engine {m} cumulative_costs, twin")
                    continue
                got = _get(ge, k)
                np.testing.assert_array_equal(got, _get(te, k), err_msg=f"engine {m} {k} against its twin")
                if k not in gu.oracle_skips(p):
                    np.testing.assert_array_equal(got, _get(o, k), err_msg=f"engine {m} {k} against its oracle")

    def op_m_set_theta(self, m, seed):
        th = su.walk(np.random.default_rng(seed), self.os[m].theta(), 0.01)
        for x in (self.os[m], self.g.engines[m], self.twins[m]):
            x.set_theta(th)

    def op_m_execute(self, m, seed, nrows, member):
        p = self.ps[m]
        rows = _execute_rows(p, self.os[m].theta(), seed, nrows)
        want = _oracle_execute(self.os[m], rows, member)
        _assert_execute(self.g.engines[m], want, rows, member, has_terms(p), f"engine {m} execute")
        _assert_execute(self.twins[m], want, rows, member, has_terms(p), f"twin {m} execute")

    def op_m_retarget(self, m, k, keep_seed):
        q = self._moved(m, k, keep_seed)
        for x in (self.g.engines[m], self.twins[m]):
            x.retarget(q.start, q.goal, None if keep_seed else q.seed)
            assert x.problem.seed == q.seed
        self.os[m] = po.Oracle(q, threads=self.threads)
        self.ps[m] = q

    def op_m_iterate(self, m, it):
        ro = self.os[m].iterate(it)
        assert self.g.engines[m].iterate(it) == ro, f"engine {m}"
        assert self.twins[m].iterate(it) == ro, f"twin {m}"

    # -------------------------------------------------------------- asks
    def op_m_query_states(self, m, seed, M, links, want):
        self.ask_query_states(self.g.engines[m], self.ps[m], seed, M, links, want, f"engine {m} ")

    def op_m_query_gradients(self, m, seed, M, links, want, biased):
        self.ask_query_gradients(self.g.engines[m], self.ps[m], seed, M, links, want, biased, f"engine {m} ")

    def op_chomp_reset(self, B, source):
        m = DESCENT_MEMBER
        self.ask_chomp_reset(self.g.engines[m], self.ps[m], self.os[m], B, source)

    def op_chomp_step(self, count):
        self.ask_chomp_step(self.g.engines[DESCENT_MEMBER], count)

    def op_chomp_get(self, names):
        self.ask_chomp_get(self.g.engines[DESCENT_MEMBER], names)

    def op_chomp_optimize(self):
        self.ask_chomp_optimize(self.g.engines[DESCENT_MEMBER])

    def op_chomp_refused(self, why):
        self.ask_chomp_refused(self.g.engines[DESCENT_MEMBER], why)

    def apply(self, op):
        getattr(self, "op_" + op[0])(*op[1:])


class RankPair(Asks):
    """Two in-process ranks of one problem (tests/rank_util.py) beside one oracle of the whole K.
    Every rank makes every call on a thread of its own and asserts nothing there: what the calls
    returned is compared after the threads joined."""

    def __init__(self, problem, ranks, threads=8):
        from tests import rank_util as ru
        self.ru = ru
        self.p, self.ranks = problem, ranks
        self.o = po.Oracle(problem, threads=threads)
        self.K_loc = problem.params.num_rollouts // len(ranks)
        self.it = 1

    def close(self):
        self.ru.close_all(self.ranks)

    def _all(self, fn):
        return self.ru.on_threads(self.ranks, lambda r, e: fn(e))

    def op_iterate(self, it):
        self.it = it
        ro = self.o.iterate(it)
        for r, got in enumerate(self._all(lambda e: e.iterate(it))):
            assert got == ro, (r, got, ro)

    def op_run(self, first, count):
        for it in range(first, first + count):
            self.o.iterate(it)
        self.it = first + count - 1
        self._all(lambda e: e.run(first, count))

    def op_synchronize(self):
        self._all(lambda e: e.synchronize())

    def op_observe(self, keys):
        got = self._all(lambda e: {k: _get(e, k) for k in keys})
        for k in keys:
            want = _get(self.o, k)
            for r, rec in enumerate(got):
                w = want[r * self.K_loc:(r + 1) * self.K_loc] if k in ROW_KEYS else want
                np.testing.assert_array_equal(rec[k], w, err_msg=f"rank {r} {k}")

    def op_set_theta(self, seed):
        th = su.walk(np.random.default_rng(seed), self.o.theta(), 0.01)
        self.o.set_theta(th)
        self._all(lambda e: e.set_theta(th))

    def op_execute(self, seed, nrows, member):
        rows = _execute_rows(self.p, self.o.theta(), seed, nrows)
        want = _oracle_execute(self.o, rows, member)
        for r, (c, cf, tr) in enumerate(self._all(lambda e: e.execute(rows, member))):
            np.testing.assert_array_equal(c, want[0], err_msg=f"rank {r} execute costs")
            np.testing.assert_array_equal(cf, want[1], err_msg=f"rank {r} execute collision flags")
            np.testing.assert_array_equal(tr, want[2], err_msg=f"rank {r} execute trajectories")

    def op_optimize(self):
        ro = self.o.optimize()
        self.it = self.p.params.max_iterations
        for r, got in enumerate(self._all(lambda e: e.optimize())):
            _assert_stats(got, ro, f"rank {r} optimize")

    def op_refuse(self, what):
        p, th, sig = self.p, self.o.theta(), su.sigma(self.p, 1)
        calls = dict(pi_get_rollouts=lambda e: e.pi_get_rollouts(self.it + 1, sig),
                     pi_set_rollout_costs=lambda e: e.pi_set_rollout_costs(np.zeros((e.K, e.N)), 1.0),
                     pi_improve_policy=lambda e: e.pi_improve_policy(),
                     pi_add_extra_rollout=lambda e: e.pi_add_extra_rollout(th, np.zeros(p.N)),
                     pi_reset=lambda e: e.pi_reset(),
                     retarget=lambda e: e.retarget(p.start, p.goal, p.seed + 1))
        for e in self.ranks:   # refused on the host before anything is posted: no thread needed
            if what == "chomp_create":
                _expect_refusal(lambda: eng.Chomp(e), -3, "sharded")
                continue
            _expect_refusal(lambda: calls[what](e), -3, "single-rank")
            assert e.problem is p

    # one rank answers at a time, from the main thread, between the collective calls: every rank
    # holds the whole model and field, and no collective runs
    def op_query_states(self, seed, M, links, want, rank):
        self.ask_query_states(self.ranks[rank], self.p, seed, M, links, want, f"rank {rank} ")

    def op_query_gradients(self, seed, M, links, want, biased, rank):
        self.ask_query_gradients(self.ranks[rank], self.p, seed, M, links, want, biased, f"rank {rank} ")

    def apply(self, op):
        getattr(self, "op_" + op[0])(*op[1:])


# ---------------------------------------------------------------------------- replay
def replay(mode, script, pair, seed=None, start=0):
    """Runs the literal script on the pair.  A failure names the mode, the seed, the op's index and
    the script up to that op, ready to paste into a regression test."""
    for i, op in enumerate(script):
        try:
            pair.apply(op)
        except AssertionError as ex:
            raise AssertionError(f"walk {mode} seed {seed}: op {start + i} {op!r} failed\nscript = {script[: i + 1]!r}\n{ex}") from None
        except Exception as ex:
            raise AssertionError(f"walk {mode} seed {seed}: op {start + i} {op!r} raised {type(ex).__name__}: {ex}\n"
                                 f"script = {script[: i + 1]!r}") from ex
