"""A/B of planning a queue of requests longer than the group: consecutive batches of P (retarget,
then optimize: a batch ends with its slowest problem) against stomp_group_serve, where a slot
whose request has stopped takes the next waiting request.

Queues of 256 requests at P = 16 and P = 64, at K = 20 / K_r = 10 on 128^3 and at bench.py's cfg5
K = 128 on 64^3 (the shapes DESIGN.md 7 has batch figures for), max_iterations = 200,
max_iterations_after_collision_free = 2; distinct start / goal / seed per request on one shared
device-built field.  Everything runs in one process, the variants alternating, one warm-up and
five repeats each; times are host wall clock ending in the call's stream wait.  The variants must
agree bit for bit on every request's statistics, cost history and best trajectory in every repeat.

    a0 / a1  batches of P: group.retarget + group.optimize per batch, compaction off / on
    b0 / b1  group.serve over the whole queue, compaction off / on

Reported: requests per second; slot occupancy -- serve: info[1] / (info[0] P), batches: the
iterations summed over the sum of (the batch's longest x P); serve's launches per step; and the
overhead guard: a queue of exactly P requests, where no turnover happens, served against retarget +
optimize.

    python tools/serve_ab.py [--out profiles/ab/serve.txt] [--requests 256] [--repeats 5] [--quick]
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


def record(st, costs, best):
    return (tuple(int(getattr(st, k)) for k in INT_STATS) + (float(st.best_cost),), np.array(costs), np.array(best))


def assert_same(a, b, tag):
    assert len(a) == len(b), tag
    for r, (x, y) in enumerate(zip(a, b)):
        assert x[0] == y[0], f"{tag}: request {r} statistics differ: {x[0]} {y[0]}"
        np.testing.assert_array_equal(x[1], y[1], err_msg=f"{tag}: request {r} costs")
        np.testing.assert_array_equal(x[2], y[2], err_msg=f"{tag}: request {r} best trajectory")


def spread(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def run_config(P, n, K, Kr, grid, max_it, repeats, lines):
    base = pb.make_problem(dof=7, waypoints=100, grid_n=grid, num_rollouts=K, num_reused_rollouts=Kr, build_grid=False)
    sdf = eng.DeviceBuffer(2 * grid ** 3, device=0)
    eng.sdf_build_device(base, sdf.ptr)
    d = np.random.default_rng(1234).uniform(-0.15, 0.15, (n, 2, base.J))
    starts = np.array([base.start + d[r, 0] for r in range(n)])
    goals = np.array([base.goal + d[r, 1] for r in range(n)])
    seeds = [base.seed + 1 + r for r in range(n)]
    stream = eng.Stream(0)
    engines = []
    for i in range(P):
        p = pb.make_problem(dof=7, waypoints=100, grid_n=grid, num_rollouts=K, num_reused_rollouts=Kr, build_grid=False,
                            seed=seeds[i], start=list(starts[i]), goal=list(goals[i]), max_iterations=max_it,
                            max_iterations_after_collision_free=2)
        engines.append(eng.Engine(p, device=0, sdf_device_ptr=sdf.ptr, stream=stream.ptr))
    groups = {c: eng.EngineGroup(engines, compact=bool(c)) for c in (0, 1)}

    def batches(g, count):
        out = []
        for b in range(0, count, P):
            m = min(P, count - b)
            # a last batch shorter than the group repeats its last request on the slots left over
            idx = list(range(b, b + m)) + [b + m - 1] * (P - m)
            g.retarget(starts[idx], goals[idx], [seeds[i] for i in idx])
            res = g.optimize()
            out += [record(res[k][0], res[k][1], engines[k].best_trajectory()) for k in range(m)]
        return out

    def serve(g, count):
        res = g.serve(starts[:count], goals[:count], seeds[:count])
        return [record(r[2], r[3], r[4]) for r in res], g.serve_info()

    variants = [("a0: batches of P, compaction off", lambda c: (batches(groups[0], c), None)),
                ("a1: batches of P, compaction on", lambda c: (batches(groups[1], c), None)),
                ("b0: serve, compaction off", lambda c: serve(groups[0], c)),
                ("b1: serve, compaction on", lambda c: serve(groups[1], c))]
    lines.append(f"serve_ab: {n} requests on P = {P} slots, K = {K}, K_r = {Kr}, {grid}^3, max_iterations = {max_it}, "
                 f"max_iterations_after_collision_free = 2, {repeats} repeats after one warm-up, alternating")
    for count, what in ((n, "queue"), (P, "overhead guard: a queue of exactly P requests, no turnover")):
        times = {name: [] for name, _ in variants}
        reference, info = None, None
        for rep in range(repeats + 1):   # the first is a warm-up
            for name, run in variants:
                t0 = time.perf_counter()
                got, inf = run(count)
                dt = time.perf_counter() - t0
                if rep:
                    times[name].append(dt * 1e3)
                if reference is None:
                    reference = got
                else:
                    assert_same(got, reference, f"{name}, repeat {rep}")
                if inf is not None:
                    assert info is None or [inf[k] for k in eng.EngineGroup.SERVE_INFO[:5]] == \
                        [info[k] for k in eng.EngineGroup.SERVE_INFO[:5]], (inf, info)
                    info = inf if name.startswith("b1") or info is None else info
        its = [r[0][0] for r in reference]
        if count != n:
            lines.append(what)
        for name, _ in variants:
            med, lo, hi = spread(times[name])
            lines.append(f"  {name:36s} median {med:9.2f} ms  min {lo:9.2f}  max {hi:9.2f}   "
                         f"{count / med * 1e3:8.1f} requests/s")
        lines.append(f"  outputs identical across a0, a1, b0, b1 in every repeat ({count} requests: statistics, cost "
                     "histories, best trajectories)")
        if count == n:
            longest = [max(its[b:b + P]) for b in range(0, n, P)]
            lines.append(f"  iterations: {sum(its)} in all, {sum(1 for k in its if k < max_it)} of {n} requests stop before "
                         f"{max_it}; min {min(its)}, median {sorted(its)[n // 2]}")
            lines.append(f"  slot occupancy: batches {sum(its) / (sum(longest) * P):.3f} (sum of the batches' longest: "
                         f"{sum(longest)} steps), serve {info['occupied_slot_steps'] / (info['steps'] * P):.3f} "
                         f"({info['steps']} steps)")
            lines.append(f"  serve: {info['turnovers']} turnovers, {info['mixed_steps']} steps with slots at different "
                         f"iterations, largest idle gap {info['largest_idle_gap']} steps, {info['launches']} launches = "
                         f"{info['launches'] / info['steps']:.2f} per step, {info['result_bytes']} result bytes on the device")
            a, b = spread(times[variants[1][0]])[0], spread(times[variants[3][0]])[0]
            a0, b0 = spread(times[variants[0][0]])[0], spread(times[variants[2][0]])[0]
            lines.append(f"  serve over batches: compaction on {a / b:.2f}x, off {a0 / b0:.2f}x")
        else:
            for off, on in ((0, 2), (1, 3)):
                ma, la, ha = spread(times[variants[off][0]])
                mb, lb, hb = spread(times[variants[on][0]])
                lines.append(f"  {variants[on][0][:2]} - {variants[off][0][:2]}: {mb - ma:+.2f} ms of {ma:.2f} ms "
                             f"(spread of the repeats: {ha - la:.2f} ms and {hb - lb:.2f} ms)")
    for g in groups.values():
        g.close()
    for e in engines:
        e.close()
    stream.close()
    sdf.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-iterations", type=int, default=200)
    ap.add_argument("--quick", action="store_true", help="one small configuration (a smoke run of the tool)")
    args = ap.parse_args()
    configs = [(16, 20, 10, 128), (64, 20, 10, 128), (16, 128, 0, 64), (64, 128, 0, 64)]
    if args.quick:
        configs = [(4, 20, 10, 64)]
    lines = []
    for P, K, Kr, grid in configs:
        done = len(lines)
        run_config(P, args.requests, K, Kr, grid, args.max_iterations, args.repeats, lines)
        sys.stdout.write("\n".join(lines[done:]) + "\n")   # each configuration as it finishes
        sys.stdout.flush()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
