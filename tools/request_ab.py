"""A/B of putting a live batch of planning problems onto requests that also carry collision points and
path constraints: one stomp_group_retarget_requests against destroying and recreating the engines
and their group (the only path before it), beside a plain stomp_group_retarget that keeps the model.

The batch is tools/retarget_ab.py's: P problems of K rollouts with K_r reused, 100 waypoints, on one
shared device-built field, distinct start / goal / seed, max_iterations = 200 and
max_iterations_after_collision_free = 2.  Two sets of requests alternate; each request of a set
attaches one body to the gripper (a sphere of the set's own radius and place, through
attached_collision_points) and sets one orientation constraint (the reference's upright constraint,
with the set's own tolerances).  Per repeat, host wall-clock time ending in a synchronize:

    n  one stomp_group_retarget_requests of the live group onto the requests (the new call)
    r  one stomp_group_retarget of the live group onto the same starts, goals and seeds, model kept
    a  destroy the P engines and their group, create P engines and a group for the requests

The plans after n and after a must agree on every statistic, cost history and best trajectory.

    python tools/request_ab.py [--out FILE] [--problems 16 64] [--rollouts 20] [--reused 10] [--grid 256]
                               [--repeats 5]
"""
import argparse
import dataclasses
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stomp_motion_planner_icra2011_amd import engine as eng   # noqa: E402
from stomp_motion_planner_icra2011_amd import problem as pb   # noqa: E402

INT_STATS = ("iterations", "success", "success_iteration", "collision_success_iteration",
             "last_improvement_iteration")


def measure(P, args, sdf, stream, base, kw):
    tool = base.robot.index("r_gripper_tool_frame")
    sets = []
    for s, rng_seed in enumerate((1234, 4321)):
        offsets = np.random.default_rng(rng_seed).uniform(-0.15, 0.15, (P, 2, base.J))
        body = pb.SceneObject(pb.BODY_SPHERE, (0.03 + 0.02 * s, 0.0, 0.02), (0.0, 0.0, 0.0, 1.0), (0.05 + 0.01 * s, 0.0, 0.0))
        spheres = eng.attached_collision_points(base.spheres, [(tool, body)], 0.05)
        con = dataclasses.replace(pb.upright_constraint(), absolute_roll_tolerance=0.2 + 0.1 * s)
        sets.append([dataclasses.replace(
            pb.make_problem(seed=base.seed + 1 + i + 1000 * s, start=list(base.start + offsets[i, 0]),
                            goal=list(base.goal + offsets[i, 1]), max_iterations=args.max_iterations,
                            max_iterations_after_collision_free=2, **kw),
            spheres=spheres, orientation_constraints=[con]) for i in range(P)])

    def create(ps):
        engines = [eng.Engine(p, device=0, sdf_device_ptr=sdf.ptr, stream=stream.ptr) for p in ps]
        group = eng.EngineGroup(engines, state_terms=True)
        group.synchronize()
        return engines, group

    def destroy(engines, group):
        group.close()
        for e in engines:
            e.close()

    def request(group, ps):     # waits for the stream
        group.retarget([p.start for p in ps], [p.goal for p in ps], [p.seed for p in ps],
                       spheres=[p.spheres for p in ps], orientation_constraints=[p.orientation_constraints for p in ps])

    def retarget(group, ps):
        group.retarget([p.start for p in ps], [p.goal for p in ps], [p.seed for p in ps])

    def plan(engines, group):
        res = group.optimize()
        return ([tuple(int(getattr(st, k)) for k in INT_STATS) + (float(st.best_cost),) for st, _ in res],
                [np.array(c) for _, c in res], [e.best_trajectory() for e in engines])

    engines, group = create(sets[1])
    t = dict(n=[], r=[], a=[])
    for rep in range(args.repeats + 1):   # the first is a warm-up
        ps, other = sets[rep % 2], sets[(rep + 1) % 2]
        t0 = time.perf_counter()
        destroy(engines, group)
        engines, group = create(ps)
        ta = time.perf_counter() - t0
        ra = plan(engines, group)
        request(group, other)              # away, so that n re-models a batch that planned something else
        plan(engines, group)
        t0 = time.perf_counter()
        request(group, ps)
        tn = time.perf_counter() - t0
        rn = plan(engines, group)
        assert ra[0] == rn[0], "statistics differ between the recreated and the re-modelled batch"
        for x, y in zip(ra[1] + ra[2], rn[1] + rn[2]):
            np.testing.assert_array_equal(x, y)
        t0 = time.perf_counter()
        retarget(group, ps)
        tr = time.perf_counter() - t0
        if rep:
            for k, v in zip(("n", "r", "a"), (tn, tr, ta)):
                t[k].append(v * 1e3)
    allocs = [e.model_info()["request_allocations"] for e in engines]
    destroy(engines, group)
    lines = [f"request_ab: {P} requests, K = {args.rollouts}, K_r = {args.reused}, {args.grid}^3, one attached body and "
             f"one orientation constraint per request, {args.repeats} repeats after one warm-up, host wall clock"]
    names = dict(n="n: stomp_group_retarget_requests", r="r: stomp_group_retarget (model kept)",
                 a="a: destroy and recreate the engines and the group")
    med = {}
    for k in ("n", "r", "a"):
        v = sorted(t[k])
        med[k] = v[len(v) // 2]
        lines.append(f"{names[k]:52s} median {med[k]:9.3f} ms  min {v[0]:9.3f}  max {v[-1]:9.3f}")
    lines.append("statistics, cost histories and best trajectories identical after n and after a in every repeat")
    lines.append(f"per request: n {med['n'] / P * 1e3:.1f} us, r {med['r'] / P * 1e3:.1f} us, a {med['a'] / P * 1e3:.1f} us; "
                 f"allocations inside the calls per engine since its creation: {sorted(set(allocs))}")
    lines.append(f"n / a = {med['n'] / med['a']:.4f} ({med['a'] / med['n']:.1f}x); n / r = {med['n'] / med['r']:.2f}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--problems", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--rollouts", type=int, default=20)
    ap.add_argument("--reused", type=int, default=10)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-iterations", type=int, default=200)
    args = ap.parse_args()
    kw = dict(dof=7, waypoints=100, grid_n=args.grid, num_rollouts=args.rollouts, num_reused_rollouts=args.reused,
              build_grid=False)
    base = pb.make_problem(**kw)
    sdf = eng.DeviceBuffer(2 * args.grid ** 3, device=0)
    eng.sdf_build_device(base, sdf.ptr)
    stream = eng.Stream(0)
    text = ""
    for P in args.problems:
        text += measure(P, args, sdf, stream, base, kw)
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    stream.close()


if __name__ == "__main__":
    main()
