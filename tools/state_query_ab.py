"""Measures the state query (stomp_engine_query_states) on the cfg2 shape -- the 7-DOF PR2-like arm,
100 waypoints, a 256^3 field built on the device -- for M in {64, 4096, 65536} states:

  (a) Engine.query_states: host wall clock of the call (it ends in a stream wait) and the device time
      of its launches (stomp_engine_query_time: events around each chunk's launches), for all
      outputs and for the two flags only (in_collision, limits_violated);
  (b) what the engine offered before for the collision flag: stomp_engine_eval of M constant
      trajectories (every waypoint the state) with iteration_member = 1, host wall clock.

Every shape is warmed up once, then timed `--repeats` times; the minimum and the median are printed.
The flags of (a) and (b) are compared on the states inside their joint limits (eval clips the
others).  One JSON line per measurement; profiles/ab/state_query.txt keeps an MI355X run's output.

usage: python tools/state_query_ab.py [--repeats 5] [--sizes 64,4096,65536] [--eval-max 4096]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_states(p, M, seed=11):
    rng = np.random.default_rng(seed)
    t = rng.uniform(-0.15, 1.15, M)
    q = p.start[None, :] + t[:, None] * (p.goal - p.start)[None, :] + rng.normal(0.0, 0.25, (M, p.J))
    return np.ascontiguousarray(q)


def timed(fn, repeats):
    fn()                                   # warm: code objects, staging at this size
    wall = []
    extra = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        extra.append(r)
    return wall, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="64,4096,65536")
    ap.add_argument("--eval-max", type=int, default=65536, help="largest M the eval arm is run at")
    ap.add_argument("--eval-batch", type=int, default=2048, help="trajectories per stomp_engine_eval call")
    ap.add_argument("--grid", type=int, default=256)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    from stomp_motion_planner_icra2011_amd import engine as eng
    from stomp_motion_planner_icra2011_amd import problem as pb

    p = pb.make_problem(dof=7, waypoints=100, grid_n=args.grid, num_rollouts=512, num_reused_rollouts=0,
                        build_grid=False)
    sdf = eng.DeviceBuffer(2 * args.grid ** 3)
    eng.sdf_build_device(p, sdf.ptr)
    e = eng.Engine(p, sdf_device_ptr=sdf.ptr)
    S, nseg = e.model_info()["S"], len(p.robot.segments)
    links = list(range(nseg))
    everything = tuple(eng.Engine.QUERY_OUTPUTS)
    flags = ("in_collision", "limits_violated")
    print(json.dumps(dict(shape="cfg2", J=p.J, N=p.N, S=S, links=len(links), grid=args.grid,
                          library=eng.load_library().stomp_engine_source_hash().decode())))
    for M in [int(x) for x in args.sizes.split(",")]:
        q = make_states(p, M)
        for arm, want, lk in (("query_all_outputs", everything, links), ("query_flags_only", flags, None)):
            def run():
                e.query_states(q, links=lk, want=want)
                return e.query_info()
            wall, infos = timed(run, args.repeats)
            kern = [i["kernel_ms"] for i in infos]
            print(json.dumps(dict(arm=arm, M=M, wall_ms_min=round(min(wall), 4), wall_ms_median=round(statistics.median(wall), 4),
                                  kernel_ms_min=round(min(kern), 4), kernel_ms_median=round(statistics.median(kern), 4),
                                  chunks=infos[-1]["chunks"], launches=infos[-1]["launches"],
                                  chunk_states=infos[-1]["chunk_states"])), flush=True)
        got = e.query_states(q, want=flags)
        if M > args.eval_max:
            print(json.dumps(dict(arm="eval_constant_trajectories", M=M, skipped="above --eval-max")), flush=True)
            continue

        def run_eval():
            cf = np.zeros(M, bool)
            for m0 in range(0, M, args.eval_batch):
                rows = np.repeat(q[m0:m0 + args.eval_batch][:, :, None], p.N, axis=2)
                cf[m0:m0 + len(rows)] = e.execute(rows, iteration_member=1)[1]
            return cf
        wall, cfs = timed(run_eval, max(1, min(args.repeats, 3)))
        inside = ~got.limits_violated
        agree = bool(np.array_equal(cfs[-1][inside], ~got.in_collision[inside]))
        print(json.dumps(dict(arm="eval_constant_trajectories", M=M, wall_ms_min=round(min(wall), 3),
                              wall_ms_median=round(statistics.median(wall), 3), eval_batch=args.eval_batch,
                              flags_agree_inside_limits=agree, states_inside_limits=int(inside.sum()),
                              colliding=int(got.in_collision.sum()))), flush=True)
    e.close()


if __name__ == "__main__":
    main()
