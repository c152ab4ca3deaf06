#!/usr/bin/env python3
"""A/B of the per-request field update: one full build against the scene layers.

  a: stomp_sdf_build_objects of static + dynamic inputs, what a caller does without a scene
  b: stomp_scene_set_dynamic over a static layer built once, two dynamic sets in turn so that
     every call also restores the other set's window

Static: the shelf scene (problem.shelf_objects).  Dynamic (i): ten robot-body boxes and cylinders
posed along an arm from a seeded start state, and 1000 collision-map points within 0.5 m of them.
Dynamic (ii): 1000 points scattered over the whole grid, the degenerate window.  Host wall clock
to the end of a stream synchronize (a: the call's own; b: stomp_scene_info), medians of
`--repeats` after one warm-up; the two fields are compared byte for byte in every repeat.

    python tools/scene_ab.py --out profiles/ab/scene_layers.txt
"""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stomp_motion_planner_icra2011_amd import _build                # noqa: E402
from stomp_motion_planner_icra2011_amd import engine as eng         # noqa: E402
from stomp_motion_planner_icra2011_amd import problem as pb         # noqa: E402


def arm_bodies(seed):
    """ten bodies along a chain from a seeded start state: boxes and cylinders in turn, link
    lengths 0.10-0.18 m, each link turned a little against the one before"""
    rng = np.random.default_rng(seed)
    pos = np.array([0.0, -0.2, 0.6]) + rng.uniform(-0.1, 0.1, 3)
    rpy = rng.uniform(-0.5, 0.5, 3)
    out = []
    for k in range(10):
        rpy = rpy + rng.uniform(-0.5, 0.5, 3)
        step = rng.uniform(0.10, 0.18)
        d = np.array([math.cos(rpy[2]) * math.cos(rpy[1]), math.sin(rpy[2]) * math.cos(rpy[1]), -math.sin(rpy[1])])
        pos = pos + step * d
        q = pb.quaternion_from_rpy(*rpy)
        if k % 2 == 0:
            out.append(pb.SceneObject(pb.BODY_BOX, tuple(pos), q, (step, 0.08, 0.10)))
        else:
            out.append(pb.SceneObject(pb.BODY_CYLINDER, tuple(pos), q, (0.05, step, 0.0)))
    centres = np.array([o.position for o in out])
    v = rng.normal(size=(1000, 3))
    v *= (0.5 * rng.uniform(0.0, 1.0, 1000) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    pts = centres[rng.integers(0, len(centres), 1000)] + v
    return out, pts


def scattered(grid, seed):
    rng = np.random.default_rng(seed)
    lo = np.array(grid.origin)
    return [], lo + rng.uniform(0.0, 1.0, (1000, 3)) * (np.array(grid.dims) - 1) * grid.resolution


def stats(v):
    return f"median {np.median(v) * 1e3:9.3f} ms  min {min(v) * 1e3:9.3f}  max {max(v) * 1e3:9.3f}"


def run(n, name, sets, repeats, out):
    grid = pb.default_grid(n)
    static = pb.shelf_objects()
    full, layered = eng.DeviceBuffer(2 * grid.cells), eng.DeviceBuffer(2 * grid.cells)
    scene = eng.Scene(grid, layered.ptr)
    scene.set_static(static)
    ta, tb, same, share = [], [], True, []
    for r in range(-1, repeats):          # r = -1: the warm-up
        for objs, pts in sets:
            t0 = time.perf_counter()
            eng.sdf_build_objects_device(grid, static + objs, full.ptr, pts)
            t1 = time.perf_counter()
            scene.set_dynamic(objs, pts)
            info = scene.info()
            t2 = time.perf_counter()
            same = same and info["stray"] == 0 and np.array_equal(full.to_numpy(np.uint16, grid.dims),
                                                                  layered.to_numpy(np.uint16, grid.dims))
            if r >= 0:
                ta.append(t1 - t0)
                tb.append(t2 - t1)
                share.append(info["cells"] / grid.cells)
    allocations = scene.info()["allocations"]
    scene.close()
    full.free()
    layered.free()
    a, b = float(np.median(ta)), float(np.median(tb))
    lines = [
        f"scene_ab: {n}^3, cap {grid.max_dist_int}, static: shelf scene, dynamic: {name}, two sets in turn, "
        f"{repeats} repeats after one warm-up, host wall clock",
        f"a: stomp_sdf_build_objects (static + dynamic)  {stats(ta)}",
        f"b: stomp_scene_set_dynamic                     {stats(tb)}",
        f"b / a = {b / a:.3f} ({a / b:.2f}x){'' if b < a else '  -- b is NOT faster here'}; window share of the grid "
        f"{min(share):.3f}..{max(share):.3f}; allocations in set_dynamic (info[9]) {allocations}",
        "fields identical byte for byte in every repeat, no stray mark" if same else "FIELDS DIFFER",
    ]
    for l in lines:
        print(l)
        out.write(l + "\n")
    out.flush()
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="profiles/ab/scene_layers.txt")
    args = ap.parse_args()
    ok = True
    with open(args.out, "a") as out:
        out.write(f"source hash {_build.embedded_hash(_build.LIB)}\n")
        for n in args.grids:
            grid = pb.default_grid(n)
            ok = run(n, "(i) ten robot bodies + 1000 points within 0.5 m", [arm_bodies(1), arm_bodies(2)],
                     args.repeats, out) and ok
            ok = run(n, "(ii) 1000 points scattered over the grid", [scattered(grid, 3), scattered(grid, 4)],
                     args.repeats, out) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
