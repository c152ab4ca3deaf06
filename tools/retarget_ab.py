"""A/B of putting a live batch of planning problems onto new requests: destroying and recreating
the engines and their group against one stomp_group_retarget, beside the time the plan itself takes.

The batch is profiles/ab/group_reuse.txt's: P problems of K rollouts with K_r reused, 100 waypoints,
on one shared device-built field, distinct start / goal / seed, max_iterations = 200 and
max_iterations_after_collision_free = 2.  Two sets of requests alternate.  Per repeat, host
wall-clock time ending in a synchronize (creation is host work: device events would not see it):

    a  destroy the P engines and their group, create P engines and a group for the new requests
    b  one stomp_group_retarget of the live group onto the same requests
    c  stomp_group_optimize of that batch (timed after a and after b)

The plans after a and after b must agree on every statistic, cost history and best trajectory.

    python tools/retarget_ab.py [--out FILE] [--problems 64] [--rollouts 20] [--reused 10] [--grid 256]
                                [--repeats 5] [--append]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stomp_motion_planner_icra2011_amd import engine as eng   # noqa: E402
from stomp_motion_planner_icra2011_amd import problem as pb   # noqa: E402

INT_STATS = ("iterations", "success", "success_iteration", "collision_success_iteration",
             "last_improvement_iteration")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--rollouts", type=int, default=20)
    ap.add_argument("--reused", type=int, default=10)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-iterations", type=int, default=200)
    args = ap.parse_args()
    P = args.problems
    kw = dict(dof=7, waypoints=100, grid_n=args.grid, num_rollouts=args.rollouts, num_reused_rollouts=args.reused,
              build_grid=False)
    base = pb.make_problem(**kw)
    sdf = eng.DeviceBuffer(2 * args.grid ** 3, device=0)
    eng.sdf_build_device(base, sdf.ptr)
    stream = eng.Stream(0)
    # two sets of P requests (set 0 is group_optimize_ab's batch)
    sets = []
    for s, rng_seed in enumerate((1234, 4321)):
        offsets = np.random.default_rng(rng_seed).uniform(-0.15, 0.15, (P, 2, base.J))
        sets.append([pb.make_problem(seed=base.seed + 1 + i + 1000 * s, start=list(base.start + offsets[i, 0]),
                                     goal=list(base.goal + offsets[i, 1]), max_iterations=args.max_iterations,
                                     max_iterations_after_collision_free=2, **kw) for i in range(P)])

    def create(ps):
        engines = [eng.Engine(p, device=0, sdf_device_ptr=sdf.ptr, stream=stream.ptr) for p in ps]
        group = eng.EngineGroup(engines)
        group.synchronize()
        return engines, group

    def destroy(engines, group):
        group.close()
        for e in engines:
            e.close()

    def retarget(group, ps):
        group.retarget([p.start for p in ps], [p.goal for p in ps], [p.seed for p in ps])   # waits for the stream

    def plan(engines, group):
        t0 = time.perf_counter()
        res = group.optimize()
        dt = time.perf_counter() - t0
        return dt, ([tuple(int(getattr(st, k)) for k in INT_STATS) + (float(st.best_cost),) for st, _ in res],
                    [np.array(c) for _, c in res], [e.best_trajectory() for e in engines])

    engines, group = create(sets[1])
    t = dict(a=[], b=[], ca=[], cb=[])
    stops = None
    for rep in range(args.repeats + 1):   # the first is a warm-up
        ps, other = sets[rep % 2], sets[(rep + 1) % 2]
        t0 = time.perf_counter()
        destroy(engines, group)
        engines, group = create(ps)
        ta = time.perf_counter() - t0
        tca, ra = plan(engines, group)
        retarget(group, other)             # away, so that b retargets a batch that planned something else
        plan(engines, group)
        t0 = time.perf_counter()
        retarget(group, ps)
        tb = time.perf_counter() - t0
        tcb, rb = plan(engines, group)
        assert ra[0] == rb[0], "statistics differ between the recreated and the retargeted batch"
        for x, y in zip(ra[1] + ra[2], rb[1] + rb[2]):
            np.testing.assert_array_equal(x, y)
        if rep:
            for k, v in zip(("a", "b", "ca", "cb"), (ta, tb, tca, tcb)):
                t[k].append(v * 1e3)
        if rep % 2 == 0:
            stops = sorted(s[0] for s in ra[0])
    med = {}
    lines = [f"retarget_ab: {P} problems, K = {args.rollouts}, K_r = {args.reused}, {args.grid}^3, max_iterations = "
             f"{args.max_iterations}, max_iterations_after_collision_free = 2, {args.repeats} repeats after one warm-up, "
             "host wall clock"]
    names = dict(a="a: destroy and recreate the engines and the group", b="b: stomp_group_retarget",
                 ca="c: stomp_group_optimize after a", cb="c: stomp_group_optimize after b")
    for k in ("a", "b", "ca", "cb"):
        v = sorted(t[k])
        med[k] = v[len(v) // 2]
        lines.append(f"{names[k]:52s} median {med[k]:9.3f} ms  min {v[0]:9.3f}  max {v[-1]:9.3f}")
    c = 0.5 * (med["ca"] + med["cb"])
    lines.append("statistics, cost histories and best trajectories identical after a and after b in every repeat")
    lines.append(f"stop iterations of set 0 (sorted): {stops}")
    lines.append(f"per problem: a {med['a'] / P * 1e3:.1f} us, b {med['b'] / P * 1e3:.1f} us")
    lines.append(f"b / a = {med['b'] / med['a']:.4f} ({med['a'] / med['b']:.1f}x); per request (b + c) / (a + c) = "
                 f"{(med['b'] + c) / (med['a'] + c):.3f} ({(med['a'] + c) / (med['b'] + c):.2f}x)")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)
    destroy(engines, group)
    stream.close()


if __name__ == "__main__":
    main()
