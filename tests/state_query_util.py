"""TEST INFRASTRUCTURE of the state-query tests (tests/STATE_QUERY.md): the models, the fixed-seed
state recipe, the oracle's reference arrays with the reductions written out as sequential float64
loops, and the census of what a state set reaches.  CPU only; nothing here touches a device."""
import functools

import numpy as np

from stomp_motion_planner_icra2011_amd import problem as pb
from oracle import pyoracle as po
from tests import model_zoo as mz

M_STATES = 130          # two wave edges (64, 128) and a partial wave
SEED = 11

MODELS = dict(
    stick1=mz.stick1,                       # J = 1, nsaves = 0
    hand9=mz.hand9,                         # a branch above the last joint: nsaves = 1
    fork12=mz.fork12,                       # saved frames after the last joint, sincos_pre = 1
    fork24=mz.fork24,                       # two nested forks: nsaves = 2
    chain17=mz.chain17,                     # J > 16
    wand21=lambda: mz.wand((2, 1)),         # 40 x 52 x 66 grid, the sphere at the grid's high z face
    pr2=lambda: pb.make_problem(grid_n=64, num_rollouts=16, num_reused_rollouts=0))   # the shelf fixture
# the conditions that hold only for some models (tests/STATE_QUERY.md has the counts)
HAS_FREE_STATES = ("hand9", "chain17", "three_saves", "wand21")
HAS_BOTH_LIMIT_KINDS = ("hand9", "chain17", "three_saves", "stick1")


def make_states(p, M=M_STATES, seed=SEED):
    """start + t (goal - start) + N(0, 0.25) with t ~ U(-0.15, 1.15); every 7th state U(-3, 3) per joint"""
    rng = np.random.default_rng(seed)
    start, goal = np.asarray(p.start, np.float64), np.asarray(p.goal, np.float64)
    t = rng.uniform(-0.15, 1.15, M)
    q = start[None, :] + t[:, None] * (goal - start)[None, :] + rng.normal(0.0, 0.25, (M, p.J))
    wild = rng.uniform(-3.0, 3.0, (M, p.J))
    q[::7] = wild[::7]
    return np.ascontiguousarray(q)


def all_links(p):
    """every segment of the tree (segments without spheres included), then one segment again"""
    return list(range(len(p.robot.segments))) + [p.spheres[0].segment]


class Reference:
    pass


def reference(p, q, links, oracle=None):
    """stomp_state_query's outputs for states q from the oracle's probes; the reductions are the
    contract's sequential float64 loops in ascending sphere order from 0.0"""
    o = oracle or po.Oracle(p)
    M, S, L = len(q), len(p.spheres), len(links)
    r = Reference()
    r.positions = np.stack([o.sphere_positions(x) for x in q]) if M else np.zeros((0, S, 3))
    r.distances = np.zeros((M, S))
    r.potentials = np.zeros((M, S))
    r.sphere_collides = np.zeros((M, S), bool)
    for m in range(M):
        for s in range(S):
            x = r.positions[m, s]
            r.distances[m, s] = o.sdf_distance(float(x[0]), float(x[1]), float(x[2]))
            r.potentials[m, s], r.sphere_collides[m, s] = o.potential(s, x)
    seg = [sp.segment for sp in p.spheres]
    radius = [np.float64(sp.radius) for sp in p.spheres]
    r.state_cost = np.zeros(M)
    r.link_costs = np.zeros((M, L))
    r.min_clearance = np.full(M, np.inf)
    r.min_sphere = np.full(M, -1, np.int32)
    for m in range(M):
        c = np.float64(0.0)
        for s in range(S):
            c = c + r.potentials[m, s]
        r.state_cost[m] = c
        for l, g in enumerate(links):
            c = np.float64(0.0)
            for s in range(S):
                if seg[s] == g:
                    c = c + r.potentials[m, s]
            r.link_costs[m, l] = c
        for s in range(S):
            cl = r.distances[m, s] - radius[s]
            if cl < r.min_clearance[m]:
                r.min_clearance[m], r.min_sphere[m] = cl, s
    r.in_collision = r.sphere_collides.any(axis=1)
    r.limits_violated = np.zeros(M, bool)
    for j, jt in enumerate(p.robot.joints):
        if jt.has_limits:
            r.limits_violated |= ~((jt.min <= q[:, j]) & (q[:, j] <= jt.max))
    return r


def census(p, q, r):
    """what the state set reaches, from the reference arrays and the cell rule alone"""
    g = p.grid
    radius = np.array([s.radius for s in p.spheres])
    clear = np.array([s.clearance for s in p.spheres])
    d = r.distances - radius[None, :]
    f = pb.c_round((r.positions - np.array(g.origin)) * (1.0 / g.resolution))
    inb = np.all((f >= 1) & (f < np.array(g.dims, np.float64) - 1), axis=-1)
    return dict(zero=int(np.sum(d >= clear[None, :])), hinge=int(np.sum((d >= 0.0) & (d < clear[None, :]))),
                penetrating=int(np.sum(d < 0.0)), outside=int(np.sum(~inb)),
                colliding_states=int(np.sum(r.in_collision)), free_states=int(np.sum(~r.in_collision)),
                violating_states=int(np.sum(r.limits_violated)), within_states=int(np.sum(~r.limits_violated)))


def assert_census(name, c):
    """the conditions every case asserts on the oracle alone before any device call"""
    assert c["zero"] >= 1 and c["hinge"] >= 1 and c["penetrating"] >= 1, (name, c)
    assert c["outside"] >= 1 and c["colliding_states"] >= 1, (name, c)
    if name in HAS_FREE_STATES:
        assert c["free_states"] >= 1, (name, c)
    if name in HAS_BOTH_LIMIT_KINDS:
        assert c["violating_states"] >= 1 and c["within_states"] >= 1, (name, c)


@functools.lru_cache(maxsize=None)
def case(name, M=M_STATES):
    """(problem, states, links, reference, census) of a model, made once and shared (read-only)"""
    p = MODELS[name]() if name in MODELS else getattr(mz, name)()
    q = make_states(p, M)
    links = all_links(p)
    r = reference(p, q, links)
    for a in vars(r).values():
        a.setflags(write=False)
    q.setflags(write=False)
    return p, q, links, r, census(p, q, r)
