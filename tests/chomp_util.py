"""TEST INFRASTRUCTURE of the CHOMP tests (tests/CHOMP.md): the ctypes binding of tests/chomp_ref.c
(compiled with the unchanged oracle into build/libchomp_ref.so), the problems and start poses the
CPU and GPU cases share, and the reference's arrays per case.  CPU only; nothing here touches a device."""
import ctypes as C
import dataclasses
import functools
import os
import subprocess

import numpy as np

from stomp_motion_planner_icra2011_amd import problem as pb
from oracle import pyoracle as po
from tests import model_zoo as mz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "chomp_ref.c")
_LIB = os.path.join(ROOT, "build", "libchomp_ref.so")
# the oracle's own flags (oracle/Makefile)
_CFLAGS = ["-O2", "-msse2", "-mno-fma", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-std=gnu11", "-Wall",
           "-Wno-unused-function"]

# every name of stomp_chomp_get, with its shape per descent from (J, N, S)
NAMES = dict(
    trajectory=lambda J, N, S: (J, N), smoothness_increments=lambda J, N, S: (J, N),
    collision_increments=lambda J, N, S: (J, N), final_increments=lambda J, N, S: (J, N),
    scales=lambda J, N, S: (J,), sphere_positions=lambda J, N, S: (N + 12, S, 3),
    distances=lambda J, N, S: (N, S), field_gradients=lambda J, N, S: (N, S, 3),
    potentials=lambda J, N, S: (N, S), potential_gradients=lambda J, N, S: (N, S, 3),
    velocities=lambda J, N, S: (N, S, 3), accelerations=lambda J, N, S: (N, S, 3),
    vel_mags=lambda J, N, S: (N, S), joint_origins=lambda J, N, S: (N, J, 3),
    joint_axes=lambda J, N, S: (N, J, 3), costs=lambda J, N, S: (N,), cost=lambda J, N, S: (),
    collision_free=lambda J, N, S: ())


class cr_params(C.Structure):
    _fields_ = [("learning_rate", C.c_double), ("smoothness_cost_weight", C.c_double),
                ("use_pseudo_inverse", C.c_int), ("pseudo_inverse_ridge_factor", C.c_double),
                ("field_bias", C.c_double * 3), ("joint_update_limits", C.POINTER(C.c_double))]


@dataclasses.dataclass(frozen=True)
class ChompParams:
    """stomp_chomp_params without the pointers; the defaults are the reference's
    (stomp_parameters.cpp, stomp_robot_model.cpp)"""
    learning_rate: float = 0.01
    smoothness_cost_weight: float = 0.1
    use_pseudo_inverse: bool = False
    pseudo_inverse_ridge_factor: float = 1e-4
    field_bias: tuple = (0.0, 0.0, 0.0)
    joint_update_limits: tuple = ()      # () = 0.05 for every joint (stomp_robot_model.cpp:78)

    def limits(self, J):
        return np.array(self.joint_update_limits if len(self.joint_update_limits) else [0.05] * J, np.float64)


_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [_SRC] + [os.path.join(ROOT, "oracle", f) for f in ("stomp_oracle.c", "stomp_oracle.h", "dmath.h")]
        if not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
            os.makedirs(os.path.dirname(_LIB), exist_ok=True)
            tmp = _LIB + ".%d.tmp" % os.getpid()
            subprocess.check_call(["gcc"] + _CFLAGS + ["-shared", "-Wl,-Bsymbolic", "-o", tmp, _SRC, "-lm"])
            os.replace(tmp, _LIB)
        l = C.CDLL(_LIB)
        P, dp = C.c_void_p, C.POINTER(C.c_double)
        l.cr_create.restype = P
        l.cr_create.argtypes = [C.POINTER(po.so_config), C.POINTER(cr_params)]
        l.cr_destroy.argtypes = [P]
        l.cr_reset.argtypes = [P, dp]
        l.cr_step.argtypes = [P, C.c_int]
        l.cr_optimize.argtypes = [P, C.POINTER(po.so_stats), dp, dp]
        l.cr_get.restype = C.c_longlong
        l.cr_get.argtypes = [P, C.c_char_p, dp]
        l.cr_counts.argtypes = [P, C.POINTER(C.c_longlong)]
        l.cr_field_gradient.restype = C.c_double
        l.cr_field_gradient.argtypes = [P, C.c_double, C.c_double, C.c_double, dp]
        l.cr_jacobian.argtypes = [P, dp, C.c_int, dp]
        l.cr_sphere_positions.argtypes = [P, dp, dp]
        l.cr_theta.argtypes = [P, dp]
        l.cr_pad_collision.argtypes = [P]
        l.so_last_error.restype = C.c_char_p
        _lib = l
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class ChompRef:
    """One descent on tests/chomp_ref.c (the problem's start, goal, model and field)."""

    def __init__(self, problem, params=ChompParams()):
        self.problem, self.params = problem, params
        self.J, self.N, self.S = problem.J, problem.N, len(problem.spheres)
        self._oracle = po.Oracle(problem)       # keeps the configuration's buffers alive
        self._upd = params.limits(self.J)
        prm = cr_params(params.learning_rate, params.smoothness_cost_weight, int(params.use_pseudo_inverse),
                        params.pseudo_inverse_ridge_factor, (C.c_double * 3)(*params.field_bias), _dp(self._upd))
        self.h = lib().cr_create(C.byref(self._oracle._cfg), C.byref(prm))
        if not self.h:
            raise RuntimeError("cr_create: " + lib().so_last_error().decode())

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            lib().cr_destroy(h)
            self.h = None

    def reset(self, trajectory=None):
        t = None if trajectory is None else np.ascontiguousarray(trajectory, np.float64).reshape(self.J, self.N)
        assert lib().cr_reset(self.h, None if t is None else _dp(t)) == 0

    def step(self, count=1):
        lib().cr_step(self.h, count)

    def optimize(self):
        """(so_stats, costs[:iterations], best trajectory) of the loop, from the state reset left"""
        st = po.so_stats()
        costs = np.zeros(max(self.problem.params.max_iterations, 1))
        best = np.zeros((self.J, self.N))
        lib().cr_optimize(self.h, C.byref(st), _dp(costs), _dp(best))
        return st, costs[:st.iterations].copy(), best

    def get(self, name):
        shape = NAMES[name](self.J, self.N, self.S)
        out = np.zeros(shape if shape else (1,))
        n = lib().cr_get(self.h, name.encode(), _dp(out))
        if n != out.size:
            raise KeyError(name)
        return out if shape else out[0]

    def snapshot(self):
        return {n: self.get(n) for n in NAMES}

    def counts(self):
        out = (C.c_longlong * 3)()
        lib().cr_counts(self.h, out)
        return dict(breaks=out[0], skips=out[1], clamped=out[2])

    def field_gradient(self, x, y, z):
        g = np.zeros(3)
        d = lib().cr_field_gradient(self.h, float(x), float(y), float(z), _dp(g))
        return d, g

    def jacobian(self, q, sphere):
        """3 x J; changes free waypoint 0 of the descent: reset afterwards"""
        out = np.zeros((3, self.J))
        qq = np.ascontiguousarray(q, np.float64)
        assert lib().cr_jacobian(self.h, _dp(qq), sphere, _dp(out)) == 0
        return out

    def sphere_positions(self, q):
        out = np.zeros((self.S, 3))
        qq = np.ascontiguousarray(q, np.float64)
        lib().cr_sphere_positions(self.h, _dp(qq), _dp(out))
        return out

    def theta(self):
        out = np.zeros((self.J, self.N))
        lib().cr_theta(self.h, _dp(out))
        return out


# ---------------------------------------------------------------- the problems of the cases

def with_params(p, **kw):
    return dataclasses.replace(p, params=dataclasses.replace(p.params, **kw))


def with_spheres(p, S):
    """the problem with its sphere list cut or repeated to S spheres (the order by segment is kept)"""
    sp = list(p.spheres)
    if S == 1:
        return dataclasses.replace(p, spheres=[sp[-1]])      # the tip: the sphere that meets the scene
    if S <= len(sp):
        keep = sorted(np.linspace(0, len(sp) - 1, S).round().astype(int).tolist())
        out = [sp[i] for i in keep]
    else:
        out = sorted(sp + [sp[i % len(sp)] for i in range(S - len(sp))], key=lambda s: s.segment)
    return dataclasses.replace(p, spheres=out)


def with_waypoints(p, N):
    """the problem with N free waypoints; below N = 19 the discretization grows so that the
    trajectory's duration does not truncate to zero (getDuration() returns int)"""
    disc = 0.05 if N >= 19 else 0.1
    q = with_params(p, trajectory_discretization=disc, trajectory_duration=(N + 1.25) * disc)
    assert q.N == N, (q.N, N)
    return q


def shelf(grid_n=32, N=33, dof=7, max_iterations=6, cf=3, **kw):
    """the PR2-like shelf fixture (tests/golden/setup_pr2like7.npz is its set-up at the bench shape)"""
    p = pb.make_problem(dof=dof, waypoints=100, grid_n=grid_n, num_rollouts=4, num_reused_rollouts=0)
    return with_waypoints(with_params(p, max_iterations=max_iterations, max_iterations_after_collision_free=cf, **kw), N)


def noisy_start(p, seed, scale=0.15):
    """an initial trajectory: the straight line start..goal plus a smooth fixed-seed bump per joint"""
    rng = np.random.default_rng(seed)
    t = (np.arange(p.N) + 1.0) / (p.N + 1.0)
    line = np.asarray(p.start)[:, None] + (np.asarray(p.goal) - np.asarray(p.start))[:, None] * t[None, :]
    amp = rng.normal(0.0, scale, (p.J, 1))
    return np.ascontiguousarray(line + amp * np.sin(np.pi * t)[None, :])


def stats_tuple(st):
    return (st.iterations, st.success, st.success_iteration, st.collision_success_iteration,
            st.last_improvement_iteration, st.best_cost)


def first_colliding(col_dist, radius):
    """per waypoint the index of the first colliding sphere (distance <= radius), -1: none"""
    hit = col_dist <= radius[None, :]
    return np.where(hit.any(axis=1), hit.argmax(axis=1), -1)


def crafted_field(p, trajectory, picks):
    """the problem with a field made of single occupied cells (so_sdf_from_occupancy): for each
    (waypoint, sphere) of picks the cell inside that sphere, at that waypoint of the trajectory's
    reset state, that is farthest outside every other sphere of the waypoint -- so that the picked
    sphere collides there and, where the geometry allows, alone"""
    r = ChompRef(p)
    r.reset(trajectory)
    pos = r.get("sphere_positions")[6:6 + p.N]
    g = p.grid
    origin, res = np.array(g.origin), g.resolution
    radius = np.array([s.radius for s in p.spheres])
    occ = np.zeros(g.dims, np.uint8)
    cells = pb.c_round((pos - origin) * (1.0 / res)).astype(int)     # each centre's cell, [N][S][3]
    for t, s in picks:
        i0 = cells[t, s]
        k = int(np.floor(radius[s] / res))
        best, best_margin = None, -np.inf
        for d in np.ndindex(2 * k + 1, 2 * k + 1, 2 * k + 1):
            i = i0 + np.array(d) - k
            if np.any(i < 1) or np.any(i > np.array(g.dims) - 2):
                continue
            if np.linalg.norm(i - i0) * res > radius[s]:          # the picked sphere reads this distance
                continue
            others = np.delete(np.linalg.norm(cells[t] - i[None, :], axis=1) * res - radius, s)
            margin = others.min() if len(others) else np.inf
            if margin > best_margin:
                best, best_margin = i, margin
        assert best is not None, (t, s)
        occ[tuple(best)] = 1
    return dataclasses.replace(p, sdf=po.sdf_from_occupancy(occ, res, g.max_expansion))


@dataclasses.dataclass
class Case:
    problem: object
    params: ChompParams
    trajectories: np.ndarray        # [B][J][N]
    layout: str = "plain"           # the engine's field layout: read in place, or "brick" (STOMP_SDF_LAYOUT)


def _trajs(p, seeds, scale=0.15):
    r = ChompRef(p)
    return np.stack([r.theta() if s is None else noisy_start(p, s, scale) for s in seeds])


def _case_pr2(**kw):
    p = shelf(**kw)
    return p, _trajs(p, (None, 3))


def make_case(name):
    """the cases of tests/test_gpu_chomp.py (tests/CHOMP.md lists what each is for)"""
    P = ChompParams
    if name == "pr2":                      # J = 7 chain, N = 33, S = 49, field read in place at 32^3
        p, t = _case_pr2(grid_n=32, N=33)
        return Case(p, P(), t)
    if name == "pr2_pinv_bias":            # the pseudo-inverse and a field bias
        p, t = _case_pr2(grid_n=32, N=33)
        return Case(p, P(use_pseudo_inverse=True, field_bias=(0.3, -0.2, 0.1)), t)
    if name == "pr2_n5":                   # every stencil reaches both paddings
        p, t = _case_pr2(grid_n=32, N=5)
        return Case(p, P(), t)
    if name == "pr2_n65_s65":              # N and S cross a wave; bricked copy at 64^3
        p = with_spheres(shelf(grid_n=64, N=65), 65)
        return Case(p, P(), _trajs(p, (None, 5)), "brick")
    if name == "pr2_s1":                   # one sphere; bricked copy at 66^3 (padding bricks)
        p = with_spheres(shelf(grid_n=66, N=33), 1)
        return Case(p, P(learning_rate=0.05), _trajs(p, (None, 7)), "brick")
    if name == "pr2_14":                   # J = 14, two arms
        p = shelf(grid_n=32, N=33, dof=14)
        return Case(p, P(use_pseudo_inverse=True), _trajs(p, (None,)))
    if name == "hand9":                    # a branched tree with fixed segments: zero Jacobian columns
        p = with_waypoints(with_params(mz.hand9(K=4, Kr=0), max_iterations=6, max_iterations_after_collision_free=3), 33)
        return Case(p, P(learning_rate=0.05), _trajs(p, (None, 9)))
    if name == "chain5":                   # a joint that drives no segment; limits (0.4, 0.4) that clamp every step
        p = with_waypoints(with_params(mz.chain5(K=4, Kr=0), max_iterations=6, max_iterations_after_collision_free=3), 33)
        return Case(p, P(learning_rate=0.05, use_pseudo_inverse=True), _trajs(p, (None, 11), 0.3))
    if name == "crafted":                  # the break after the first, a middle and the last sphere
        p = with_spheres(shelf(grid_n=64, N=33), 17)
        t = _trajs(p, (13,))
        # (sphere 0, at the shoulder, hardly moves: its cell keeps it colliding over the first waypoints,
        # so the other two picks lie behind them)
        p = crafted_field(p, t[0], [(5, 0), (25, 8), (30, 16)])
        return Case(p, P(learning_rate=0.02), t)
    raise KeyError(name)


CASES = ("pr2", "pr2_pinv_bias", "pr2_n5", "pr2_n65_s65", "pr2_s1", "pr2_14", "hand9", "chain5", "crafted")
STEPS = 3


@functools.lru_cache(maxsize=None)
def case(name):
    """(Case, per descent the reference's snapshots after reset and after each of STEPS steps, per
    descent the counts and the census of the reset state), made once and shared (read-only)"""
    c = make_case(name)
    p = c.problem
    radius = np.array([s.radius for s in p.spheres])
    snaps, info = [], []
    for traj in c.trajectories:
        r = ChompRef(p, c.params)
        r.reset(traj)
        ss = [r.snapshot()]
        firsts = [first_colliding(ss[0]["distances"], radius)]
        for _ in range(STEPS):
            r.step(1)
            ss.append(r.snapshot())
            firsts.append(first_colliding(ss[-1]["distances"], radius))
        g = p.grid
        f = pb.c_round((ss[0]["sphere_positions"][6:6 + p.N] - np.array(g.origin)) * (1.0 / g.resolution))
        outside = int(np.sum(~np.all((f >= 1) & (f < np.array(g.dims, np.float64) - 1), axis=-1)))
        scales = np.stack([s["scales"] for s in ss[1:]])
        info.append(dict(r.counts(), firsts=sorted(set(np.concatenate(firsts[:-1]).tolist())), outside=outside,
                         scaled=int(np.sum(scales < 1.0)), unscaled=int(np.sum(scales == 1.0))))
        for s in ss:
            for a in s.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        snaps.append(ss)
    c.trajectories.setflags(write=False)
    return c, snaps, info


def loop_trajectories(p):
    """three starts on the shelf (N = 33) that the loop leaves at different iterations with
    learning_rate 0.05 and a collision-free streak of 2: a streak from iteration 0 (stops after 2), one
    that comes free at iteration 5 (stops after 7, inside the first chunk of 8) and one that is never
    free twice in a row (runs to max_iterations 12, into the second chunk); chosen on the CPU reference"""
    return np.stack([noisy_start(p, 23, 0.6), noisy_start(p, 35, 0.6), noisy_start(p, 22, 0.6)])


def assert_census(name, c, info):
    """what a case is known to exercise, asserted on the reference alone (CPU and GPU tests)"""
    if name != "chain5":       # (chain5's first sphere collides at every waypoint: the fold ends before any skip)
        assert all(i["skips"] >= 1 for i in info), info
    if name != "pr2_n5":
        assert all(i["breaks"] >= 1 for i in info), info
    else:
        assert info[0]["breaks"] >= 1, info
    if name in ("hand9", "chain5"):
        assert all(i["outside"] >= 1 for i in info), info            # spheres off the grid
    if name in ("pr2", "pr2_pinv_bias"):                             # a scale below 1 on some joints, not on all
        assert any(i["scaled"] >= 1 and i["unscaled"] >= 1 for i in info), info
    if name == "chain5":
        assert all(i["clamped"] >= 1 for i in info), info            # limit passes that changed the trajectory
    if name == "crafted":
        S = len(c.problem.spheres)
        f = info[0]["firsts"]
        assert 0 in f and S - 1 in f and any(0 < x < S - 1 for x in f), f   # the break first, in the middle, last
