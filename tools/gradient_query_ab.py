"""Measures the gradient query (stomp_engine_query_gradients) on the cfg2 shape -- the 7-DOF PR2-like
arm, 100 waypoints, S = 49, 17 links, a 256^3 field built on the device -- for M in {64, 4096, 65536}:

  (a) Engine.query_gradients: host wall clock of the call (it ends in a stream wait) and the device
      time of its launches (stomp_engine_query_time), for link_gradients + in_collision only and for
      all outputs;
  (b) the route the engine offered before: the states packed as the free waypoints of ceil(M / N)
      descents of one Chomp.reset, get() of potential_gradients, joint_origins, joint_axes and
      sphere_positions, and the J^T products and per-link sums in numpy.  Host wall clock.

Every shape is warmed up once, then timed `--repeats` times; the minimum and the median are printed.
The link gradients of (b) are compared with (a)'s on the states inside their joint limits: reset's
handleJointLimits pass moves a state outside its limits and, through the smoothing projection, the
waypoints around it, so for the comparison route (b) is run once more on those states alone, where
get("trajectory") returns every state as it was given (checked).  numpy sums in another order, so the
comparison is to 1e-12 relative to the largest entry.
One JSON line per measurement; profiles/ab/gradient_query.txt keeps an MI355X run's output.

usage: python tools/gradient_query_ab.py [--repeats 5] [--sizes 64,4096,65536] [--chomp-max 65536]
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
    wall, extra = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        extra.append(r)
    return wall, extra


def path_table(p):
    """on[s][k]: joint k is on the path from the root to sphere s's segment; seg[s]"""
    segs = p.robot.segments
    on = np.zeros((len(p.spheres), p.J))
    for s, sp in enumerate(p.spheres):
        g = sp.segment
        while g >= 0:
            if segs[g].q_index >= 0:
                on[s, segs[g].q_index] = 1.0
            g = segs[g].parent
    return on, np.array([sp.segment for sp in p.spheres])


def chomp_route(e, c, p, q, links, on, seg, block=64):
    """link gradients [M][L][J] by the parent's route"""
    return chomp_route_rows(e, c, p, q, links, on, seg, block)[0]


def chomp_route_rows(e, c, p, q, links, on, seg, block=64, kept=False):
    """... and, with kept, which states reset left as they were"""
    M, N, J = len(q), p.N, p.J
    B = (M + N - 1) // N
    rows = np.empty((B * N, J))
    rows[:M] = q
    rows[M:] = q[-1]
    c.reset(np.ascontiguousarray(rows.reshape(B, N, J).transpose(0, 2, 1)))
    pg = c.get("potential_gradients").reshape(B * N, -1, 3)
    org = c.get("joint_origins").reshape(B * N, J, 3)
    ax = c.get("joint_axes").reshape(B * N, J, 3)
    pos = c.get("sphere_positions")[:, 6:6 + N].reshape(B * N, -1, 3)
    member = np.stack([(seg == g).astype(np.float64) for g in links])          # [L][S]
    out = np.empty((M, len(links), J))
    for m0 in range(0, M, block * N):
        sl = slice(m0, min(M, m0 + block * N))
        d = pos[sl][:, :, None, :] - org[sl][:, None, :, :]                     # [m][S][J][3]
        col = np.cross(ax[sl][:, None, :, :], d) * on[None, :, :, None]
        term = np.einsum("msjr,msr->msj", col, pg[sl])
        out[sl] = -np.einsum("ls,msj->mlj", member, term)
    same = None
    if kept:
        traj = c.get("trajectory").transpose(0, 2, 1).reshape(B * N, J)[:M]
        same = (traj == q).all(axis=1)
    return out, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="64,4096,65536")
    ap.add_argument("--chomp-max", type=int, default=65536, help="largest M the Chomp.reset arm is run at")
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
    c = eng.Chomp(e)
    S, nseg = e.model_info()["S"], len(p.robot.segments)
    links = list(range(nseg))
    on, seg = path_table(p)
    everything = tuple(eng.Engine.GRADIENT_OUTPUTS)
    lean = ("link_gradients", "in_collision")
    print(json.dumps(dict(shape="cfg2", J=p.J, N=p.N, S=S, links=len(links), grid=args.grid,
                          library=eng.load_library().stomp_engine_source_hash().decode())))
    for M in [int(x) for x in args.sizes.split(",")]:
        q = make_states(p, M)
        for arm, want in (("link_gradients_and_flag", lean), ("all_outputs", everything)):
            def run():
                e.query_gradients(q, links=links, want=want)
                return e.query_info()
            wall, infos = timed(run, args.repeats)
            kern = [i["kernel_ms"] for i in infos]
            print(json.dumps(dict(arm=arm, M=M, wall_ms_min=round(min(wall), 4),
                                  wall_ms_median=round(statistics.median(wall), 4),
                                  kernel_ms_min=round(min(kern), 4), kernel_ms_median=round(statistics.median(kern), 4),
                                  chunks=infos[-1]["chunks"], launches=infos[-1]["launches"],
                                  chunk_states=infos[-1]["chunk_states"])), flush=True)
        if M > args.chomp_max:
            print(json.dumps(dict(arm="chomp_reset_and_numpy", M=M, skipped="above --chomp-max")), flush=True)
            continue
        got = e.query_gradients(q, links=links, want=lean).link_gradients
        wall, outs = timed(lambda: chomp_route(e, c, p, q, links, on, seg), max(1, min(args.repeats, 3 if M > 4096 else 5)))
        inside = ~e.query_states(q, want=("limits_violated",)).limits_violated
        alone, same = chomp_route_rows(e, c, p, q[inside], links, on, seg, kept=True)
        scale = max(float(np.abs(got[inside]).max()), 1e-300)
        err = float(np.abs(alone - got[inside]).max()) / scale
        print(json.dumps(dict(arm="chomp_reset_and_numpy", M=M, descents=(M + p.N - 1) // p.N,
                              wall_ms_min=round(min(wall), 3), wall_ms_median=round(statistics.median(wall), 3),
                              states_inside_limits=int(inside.sum()), left_unchanged_by_reset=int(same.sum()),
                              max_rel_difference=err, agree_inside_limits=bool(err <= 1e-12))), flush=True)
    c.close()
    e.close()


if __name__ == "__main__":
    main()
