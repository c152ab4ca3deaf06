"""A/B of optimizing a batch of planning problems: one stomp_engine_optimize per problem against
stomp_group_optimize of the whole batch, without and with the compaction that takes stopped
problems out of the group's launches.

The batch is bench.py's cfg5: 64 problems of K = 128 rollouts at 256^3 on one shared device-built
field, distinct start / goal / seed, with max_iterations = 200 and
max_iterations_after_collision_free = 2.  Every way optimizes the same engines from the same
initial trajectories, five repeats each; the three must agree on every statistic and best
trajectory.

--reused K_r gives every problem K_r reused rollouts (0: none, cfg5); every repeat then starts from
a reset generateRollouts state too, so that all of them optimize the same thing.

--upright gives every problem the reference's upright path constraint on the gripper
(problem.upright_constraint; --upright-tolerance R replaces its 0.2 rad of roll and pitch), and
--torque-weight W the torque term; the groups are then created with state_terms (and their compaction
chosen through the options).  --ways picks the ways to run (a library without
stomp_group_create_with, or one that refuses terms in groups, runs `--ways a` alone).

--cumulative sets use_cumulative_costs (the reference's default) on every problem; the groups are
then created accepting cumulative costs (stomp_group_create_flags), with or without the terms above.
A library from before groups took cumulative costs runs `--ways a` alone.

    python tools/group_optimize_ab.py [--out FILE] [--problems 64] [--repeats 5] [--reused 0]
                                      [--upright] [--upright-tolerance 0.2] [--torque-weight 0] [--cumulative]
                                      [--ways abc]
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
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--rollouts", type=int, default=128)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-iterations", type=int, default=200)
    ap.add_argument("--reused", type=int, default=0, help="num_reused_rollouts of every problem")
    ap.add_argument("--upright", action="store_true", help="the reference's upright constraint on every problem")
    ap.add_argument("--upright-tolerance", type=float, default=None, help="roll / pitch tolerance (rad) in its place")
    ap.add_argument("--torque-weight", type=float, default=0.0, help="torque_cost_weight of every problem")
    ap.add_argument("--cumulative", action="store_true", help="use_cumulative_costs on every problem")
    ap.add_argument("--ways", default="abc", help="which of a, b, c to run")
    args = ap.parse_args()
    P = args.problems
    terms = args.upright or args.torque_weight > 1e-9
    extra = {}
    if args.upright:
        oc = pb.upright_constraint()
        if args.upright_tolerance is not None:
            oc.absolute_roll_tolerance = oc.absolute_pitch_tolerance = args.upright_tolerance
        extra["orientation_constraints"] = [oc]
    if args.torque_weight:
        extra["torque_cost_weight"] = args.torque_weight
    if args.cumulative:
        extra["use_cumulative_costs"] = True
    base = pb.make_problem(dof=7, waypoints=100, grid_n=args.grid, num_rollouts=args.rollouts,
                           num_reused_rollouts=args.reused, build_grid=False)
    sdf = eng.DeviceBuffer(2 * args.grid ** 3, device=0)
    eng.sdf_build_device(base, sdf.ptr)
    offsets = np.random.default_rng(1234).uniform(-0.15, 0.15, (P, 2, base.J))
    stream = eng.Stream(0)
    engines = []
    for i in range(P):
        p = pb.make_problem(dof=7, waypoints=100, grid_n=args.grid, num_rollouts=args.rollouts,
                            num_reused_rollouts=args.reused, build_grid=False, seed=base.seed + 1 + i,
                            start=list(base.start + offsets[i, 0]),
                            goal=list(base.goal + offsets[i, 1]), max_iterations=args.max_iterations,
                            max_iterations_after_collision_free=2, **extra)
        engines.append(eng.Engine(p, device=0, sdf_device_ptr=sdf.ptr, stream=stream.ptr))
    group_all = group_compact = None
    if args.cumulative:
        if "b" in args.ways:
            group_all = eng.EngineGroup(engines, state_terms=terms, compact=False, cumulative_costs=True)
        if "c" in args.ways:
            group_compact = eng.EngineGroup(engines, state_terms=terms, compact=True, cumulative_costs=True)
    elif terms:
        if "b" in args.ways:
            group_all = eng.EngineGroup(engines, state_terms=True, compact=False)
        if "c" in args.ways:
            group_compact = eng.EngineGroup(engines, state_terms=True, compact=True)
    else:
        # the switch is read when a group is created
        if "b" in args.ways:
            os.environ["STOMP_DEBUG_GROUP_COMPACT"] = "0"
            group_all = eng.EngineGroup(engines)
        if "c" in args.ways:
            os.environ["STOMP_DEBUG_GROUP_COMPACT"] = "1"
            group_compact = eng.EngineGroup(engines)
    theta0 = [e.theta() for e in engines]

    def reset():
        for e, th in zip(engines, theta0):
            e.set_theta(th)
        for e in engines:
            e.synchronize()
            if args.reused:
                e.pi_reset()   # the first iteration generates every rollout again

    ways = [("a: one stomp_engine_optimize per problem", lambda: [e.optimize() for e in engines]),
            ("b: stomp_group_optimize, compaction off", group_all.optimize if group_all else None),
            ("c: stomp_group_optimize, compaction on", group_compact.optimize if group_compact else None)]
    ways = [(name, run) for name, run in ways if name[0] in args.ways]
    reused = f", K_r = {args.reused}" if args.reused else ""
    if args.upright:
        tol = 0.2 if args.upright_tolerance is None else args.upright_tolerance
        reused += f", upright constraint (roll / pitch within {tol:g} rad)"
    if args.torque_weight:
        reused += f", torque_cost_weight = {args.torque_weight:g}"
    if args.cumulative:
        reused += ", cumulative costs"
    lines = [f"group_optimize_ab: {P} problems, K = {args.rollouts}{reused}, {args.grid}^3, max_iterations = "
             f"{args.max_iterations}, max_iterations_after_collision_free = 2, {args.repeats} repeats after one warm-up"]
    reference = None
    medians = {}
    for name, run in ways:
        times = []
        for rep in range(args.repeats + 1):   # the first is a warm-up
            reset()
            t0 = time.perf_counter()
            res = run()
            dt = time.perf_counter() - t0
            if rep:
                times.append(dt * 1e3)
            got = ([tuple(int(getattr(st, k)) for k in INT_STATS) + (float(st.best_cost),) for st, _ in res],
                   [np.array(c) for _, c in res], [e.best_trajectory() for e in engines])
            if reference is None:
                reference = got
            else:
                assert got[0] == reference[0], f"{name}: statistics differ"
                for a, b in zip(got[1] + got[2], reference[1] + reference[2]):
                    np.testing.assert_array_equal(a, b, err_msg=name)
        times.sort()
        medians[name[0]] = times[len(times) // 2]
        lines.append(f"{name:48s} median {times[len(times) // 2]:9.2f} ms  min {times[0]:9.2f}  max {times[-1]:9.2f}")
    stops = sorted(s[0] for s in reference[0])
    total = sum(stops)
    lines.append(f"statistics, cost histories and best trajectories identical across {', '.join(args.ways)} and all "
                 "repeats")
    lines.append(f"stop iterations (sorted): {stops}")
    lines.append(f"problems that stop before max_iterations: {sum(1 for n in stops if n < args.max_iterations)} of {P}")
    lines.append(f"problem-iterations run: {total} of {P * args.max_iterations} "
                 f"(lockstep without compaction: {P} x {max(stops)} = {P * max(stops)})")
    if all(w in medians for w in "abc"):
        lines.append(f"speed-up of c over a: {medians['a'] / medians['c']:.2f}x, of c over b: "
                     f"{medians['b'] / medians['c']:.2f}x")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    for g in (group_all, group_compact):
        if g:
            g.close()
    for e in engines:
        e.close()
    stream.close()


if __name__ == "__main__":
    main()
