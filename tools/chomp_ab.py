"""Measures CHOMP mode (stomp_chomp_*) on the cfg2 shape -- the 7-DOF PR2-like arm, 100 waypoints
(N = 99 free), S = 49 spheres, a 256^3 field built on the device -- for B in {1, 16, 256} descents:

  (a) device time per iteration: events on the engine's stream around step(`--steps`) after a
      warm-up step call, divided by the steps (five launches per iteration);
  (b) host wall clock of a whole optimize() (`--iterations` iterations, no descent stops early: the
      collision-free streak is set above them), reset not included;
  (c) the same two quantities for tests/chomp_ref.c on one core, the only CPU implementation there
      is to compare with: one descent (B descents on one core take B times as long).

Every measurement is warmed up once, then taken `--repeats` times; the minimum and the median are
printed.  The costs of descent 0 after the timed optimize are compared with the reference's, bit for
bit.  One JSON line per measurement; profiles/ab/chomp.txt keeps an MI355X run's output.

usage: python tools/chomp_ab.py [--repeats 5] [--sizes 1,16,256] [--steps 20] [--iterations 40]
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


def stats(xs):
    return dict(min=round(min(xs), 4), median=round(statistics.median(xs), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--grid", type=int, default=256)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    from stomp_motion_planner_icra2011_amd import engine as eng
    from stomp_motion_planner_icra2011_amd import problem as pb
    from tests import chomp_util as cu

    p = pb.make_problem(dof=7, waypoints=100, grid_n=args.grid, num_rollouts=16, num_reused_rollouts=0,
                        build_grid=False)
    p = cu.with_params(p, max_iterations=args.iterations, max_iterations_after_collision_free=args.iterations + 1)
    sdf = eng.DeviceBuffer(2 * args.grid ** 3)
    eng.sdf_build_device(p, sdf.ptr)
    stream = torch.cuda.Stream()
    e = eng.Engine(p, sdf_device_ptr=sdf.ptr, stream=stream.cuda_stream)
    print(json.dumps(dict(shape="cfg2", J=p.J, N=p.N, S=len(p.spheres), grid=args.grid, steps=args.steps,
                          iterations=args.iterations, command=" ".join(["python", "tools/chomp_ab.py"] + sys.argv[1:]),
                          library=eng.load_library().stomp_engine_source_hash().decode())), flush=True)
    prm = cu.ChompParams()
    sizes = [int(x) for x in args.sizes.split(",")]
    trajs = np.stack([cu.noisy_start(p, 100 + b, 0.3) for b in range(max(sizes))])
    ch = eng.Chomp(e)
    dev_costs = None
    for B in sizes:
        t = trajs[:B]
        per_it, wall = [], []
        for rep in range(args.repeats + 1):          # the first repeat warms up
            ch.reset(t)
            ch.step(2)
            ch.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            ch.step(args.steps)
            b.record(stream)
            ch.synchronize()
            if rep:
                per_it.append(a.elapsed_time(b) / args.steps)
            ch.reset(t)
            t0 = time.perf_counter()
            out = ch.optimize()
            if rep:
                wall.append((time.perf_counter() - t0) * 1e3)
        assert all(o[0].iterations == args.iterations for o in out)
        if dev_costs is None:
            dev_costs = out[0][1]
        info = ch.info()
        print(json.dumps(dict(arm="device", B=B, iteration_ms=stats(per_it), optimize_wall_ms=stats(wall),
                              iteration_us_per_descent=round(1e3 * min(per_it) / B, 3), launches=info["launches"],
                              lds=[info[k] for k in ("lds_fk", "lds_gradient", "lds_update")])), flush=True)
    ch.close()
    # the reference on one core, on the same field (read back from the device)
    p.sdf = sdf.to_numpy(np.uint16, (args.grid,) * 3)
    r = cu.ChompRef(p, prm)
    per_it, wall = [], []
    for rep in range(args.repeats + 1):
        r.reset(trajs[0])
        r.step(2)
        t0 = time.perf_counter()
        r.step(args.steps)
        if rep:
            per_it.append((time.perf_counter() - t0) * 1e3 / args.steps)
        r.reset(trajs[0])
        t0 = time.perf_counter()
        st, costs, _ = r.optimize()
        if rep:
            wall.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(arm="chomp_ref_one_core", B=1, iteration_ms=stats(per_it), optimize_wall_ms=stats(wall),
                          costs_equal_device=bool(np.array_equal(costs, dev_costs)))), flush=True)
    e.close()


if __name__ == "__main__":
    main()
