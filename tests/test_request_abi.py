"""CPU: the boundary of stomp_engine_retarget_request / stomp_group_retarget_requests /
stomp_engine_model_info / stomp_attached_collision_points (include/stomp_engine.h).  The ctypes
mirrors of stomp_request and stomp_attached_body have the compiler's layout, the header still
compiles as C99 and C++11, the library exports the symbols, the NULL and struct_size refusals are
made before any engine or device is touched (so they run on a machine without a GPU), and
stomp_attached_collision_points -- host code only -- is compared bit for bit with a NumPy
restatement of generateAttachedObjectCollisionPoints + populatePlanningGroupCollisionPoints.
tests/REQUEST_MODEL.md lists the cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from stomp_motion_planner_icra2011_amd import engine as eng
from stomp_motion_planner_icra2011_amd import problem as pb
from tests import model_zoo as mz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stomp_engine_retarget_request", "stomp_group_retarget_requests", "stomp_engine_model_info",
         "stomp_attached_collision_points")


def test_struct_layouts_match_c(tmp_path):
    structs = {"stomp_request": eng.stomp_request, "stomp_attached_body": eng.stomp_attached_body,
               "stomp_shape": eng.stomp_shape}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stomp_engine.h"', "int main(void){"]
    for name, cls in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(l.rsplit(" ", 1) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, cls in structs.items():
        assert int(out[name]) == C.sizeof(cls), name
        for field, _ in cls._fields_:
            assert int(out[f"{name}.{field}"]) == getattr(cls, field).offset, f"{name}.{field}"


def test_header_compiles_as_c_and_cpp_and_keeps_its_version(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "stomp_engine.h"\n'
                   'int main(void){stomp_request r; stomp_attached_body b; r.struct_size = (int32_t)sizeof r;\n'
                   'b.segment = 0; return STOMP_ENGINE_ABI_VERSION - 4 + b.segment + (r.struct_size > 0 ? 0 : 1);}\n')
    for compiler, flag in (("gcc", "-std=c99"), ("g++", "-std=c++11")):
        exe = tmp_path / ("h_" + compiler)
        subprocess.check_call([compiler, flag, "-x", "c" if compiler == "gcc" else "c++", "-Wall", "-Werror",
                               "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
        assert subprocess.call([str(exe)]) == 0          # STOMP_ENGINE_ABI_VERSION stays 4


def test_header_declares_and_library_exports_the_symbols():
    with open(os.path.join(ROOT, "include", "stomp_engine.h")) as f:
        text = f.read()
    lib = eng.load_library()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", text, re.M), name
        assert hasattr(lib, name) and name in eng.EXPORTED, name
    assert re.search(r"stomp_engine_retarget_request\(stomp_engine\* e, const stomp_request\* r\)", text)
    assert re.search(r"stomp_group_retarget_requests\(stomp_group\* g, const stomp_request\* requests", text)
    assert re.search(r"stomp_engine_model_info\(stomp_engine\* e, int64_t info\[12\]\)", text)


def test_null_and_struct_size_are_refused_before_any_engine_is_touched():
    lib = eng.load_library()
    v = (C.c_double * 4)(0.1, 0.2, 0.3, 0.4)
    dp = C.POINTER(C.c_double)
    # a handle that is not null and never dereferenced: every call must return at its argument checks
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)
    good = eng.stomp_request(C.sizeof(eng.stomp_request), v, v, 1, -1, None, -1, None)

    def call(f, *args):
        rc = f(*args)
        return rc, lib.stomp_last_error().decode()

    rc, msg = call(lib.stomp_engine_retarget_request, None, C.byref(good))
    assert rc == -1 and "null engine" in msg, (rc, msg)
    rc, msg = call(lib.stomp_engine_retarget_request, fake, None)
    assert rc == -1 and "null request" in msg, (rc, msg)
    rc, msg = call(lib.stomp_group_retarget_requests, None, C.byref(good))
    assert rc == -1 and "null group" in msg, (rc, msg)
    rc, msg = call(lib.stomp_group_retarget_requests, fake, None)
    assert rc == -1 and "null requests" in msg, (rc, msg)
    for size in (0, C.sizeof(eng.stomp_request) - 8, C.sizeof(eng.stomp_request) + 8):
        bad = eng.stomp_request(size, v, v, 1, 0, None, 0, None)
        rc, msg = call(lib.stomp_engine_retarget_request, fake, C.byref(bad))
        assert rc == -1 and "struct_size" in msg, (size, rc, msg)
    for s, g in ((C.cast(None, dp), v), (v, C.cast(None, dp))):
        bad = eng.stomp_request(C.sizeof(eng.stomp_request), s, g, 1, 0, None, 0, None)
        rc, msg = call(lib.stomp_engine_retarget_request, fake, C.byref(bad))
        assert rc == -1 and "null start or goal" in msg, (rc, msg)
    info = (C.c_int64 * 12)()
    rc, msg = call(lib.stomp_engine_model_info, None, info)
    assert rc == -1 and "null" in msg, (rc, msg)
    rc, msg = call(lib.stomp_engine_model_info, fake, None)
    assert rc == -1 and "null" in msg, (rc, msg)


# ------------------------------------------------------------------------------------------------
# stomp_attached_collision_points against NumPy

def basis(q):
    """btMatrix3x3::setRotation, one rounding per operation"""
    x, y, z, w = (np.float64(v) for v in q)
    d = x * x + y * y + z * z + w * w
    s = np.float64(2.0) / d
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz = w * xs, w * ys, w * zs
    xx, xy, xz = x * xs, x * ys, x * zs
    yy, yz, zz = y * ys, y * zs, z * zs
    return np.array([[1.0 - (yy + zz), xy - wz, xz + wy], [xy + wz, 1.0 - (xx + zz), yz - wx],
                     [xz - wy, yz + wx, 1.0 - (xx + yy)]])


def bounding_sphere(o):
    """bodies::*::computeBoundingSphere of a problem.SceneObject robot body: (centre, radius)"""
    d = [np.float64(v) for v in o.dims] + [np.float64(0.0)] * 3
    centre = np.array(o.position, np.float64)
    if o.type == pb.BODY_SPHERE:
        return centre, d[0]
    if o.type == pb.BODY_BOX:
        a, b, c = d[0] / 2.0, d[1] / 2.0, d[2] / 2.0
        return centre, np.sqrt(a * a + b * b + c * c)
    if o.type == pb.BODY_CYLINDER:
        h = d[1] / 2.0
        return centre, np.sqrt(d[0] * d[0] + h * h)
    assert o.type == pb.BODY_MESH
    V = np.asarray(o.vertices, np.float64)
    bc = (V.min(axis=0) + V.max(axis=0)) / 2.0
    r2 = np.float64(0.0)
    for v in V:
        dx, dy, dz = v - bc
        r2 = max(r2, dx * dx + dy * dy + dz * dz)
    B = basis(o.orientation)
    centre = np.array([B[a, 0] * bc[0] + B[a, 1] * bc[1] + B[a, 2] * bc[2] + np.float64(o.position[a]) for a in range(3)])
    return centre, np.sqrt(r2) + d[0]


def numpy_attached(spheres, bodies, clearance):
    out = [(s.segment, s.radius, s.clearance, tuple(s.pos)) for s in spheres]
    for seg, o in bodies:
        c, r = bounding_sphere(o)
        new = (seg, float(r), float(clearance), tuple(float(v) for v in c))
        same = [k for k, s in enumerate(out) if s[0] == seg]
        later = [k for k, s in enumerate(out) if s[0] > seg]
        at = same[-1] + 1 if same else (later[0] if later else len(out))
        out.insert(at, new)
    return out


def as_tuples(spheres):
    return [(s.segment, s.radius, s.clearance, tuple(s.pos)) for s in spheres]


def mesh_body():
    m = np.load(os.path.join(os.path.dirname(__file__), "golden", "meshes.npz"))
    return pb.mesh_object(m["cabnite_vertices"] * 0.05, position=(0.02, -0.01, 0.03), rpy=(0.3, -0.2, 0.5), padding=0.01)


BODIES = dict(
    sphere=lambda: pb.SceneObject(pb.BODY_SPHERE, (0.03, 0.0, 0.02), (0.0, 0.0, 0.0, 1.0), (0.05, 0.0, 0.0)),
    box=lambda: pb.SceneObject(pb.BODY_BOX, (0.01, 0.02, -0.03), pb.quaternion_from_rpy(0.1, 0.2, 0.3), (0.07, 0.03, 0.11)),
    cylinder=lambda: pb.SceneObject(pb.BODY_CYLINDER, (-0.02, 0.0, 0.05), pb.quaternion_from_rpy(-0.4, 0.0, 1.1),
                                    (0.03, 0.13, 0.0)),
    mesh=mesh_body)


@pytest.mark.parametrize("kind", sorted(BODIES))
def test_one_body_of_each_kind(kind):
    p = mz.chain5()
    body = BODIES[kind]()
    seg = p.robot.index("l3")
    got = eng.attached_collision_points(p.spheres, [(seg, body)], 0.04)
    want = numpy_attached(p.spheres, [(seg, body)], 0.04)
    assert as_tuples(got) == want                       # bit for bit: exact float equality
    new = [s for s in got if s.segment == seg][-1]
    assert new.clearance == 0.04 and new.radius > 0.0
    assert [s.segment for s in got] == sorted(s.segment for s in got)
    if kind == "sphere":
        assert new.radius == 0.05 and tuple(new.pos) == (0.03, 0.0, 0.02)
    if kind == "mesh":                                  # the centre is the posed bounding-box centre, not the position
        assert tuple(new.pos) != tuple(body.position)


def test_placement_order():
    p = mz.chain5()
    l0, l2, l3, tip = (p.robot.index(n) for n in ("l0", "l2", "l3", "tip"))
    assert all(s.segment != tip for s in p.spheres) and all(s.segment != 0 for s in p.spheres)
    bodies = [(l3, BODIES["box"]()), (tip, BODIES["sphere"]()), (l0, BODIES["cylinder"]()), (l3, BODIES["sphere"]()),
              (0, BODIES["box"]()), (l2, BODIES["mesh"]())]
    got = eng.attached_collision_points(p.spheres, bodies, 0.05)
    assert as_tuples(got) == numpy_attached(p.spheres, bodies, 0.05)
    segs = [s.segment for s in got]
    assert segs == sorted(segs) and len(got) == len(p.spheres) + len(bodies)
    # a segment's own spheres first, then its bodies in input order; a segment without spheres (the
    # base: before every sphere; the tip: after them) still lands in order
    on_l3 = [s for s in got if s.segment == l3]
    assert as_tuples(on_l3[:-2]) == as_tuples([s for s in p.spheres if s.segment == l3])
    assert on_l3[-2].radius == bounding_sphere(bodies[0][1])[1] and on_l3[-1].radius == 0.05
    assert got[0].segment == 0 and got[-1].segment == tip
    # no bodies: the base list; no base: the bodies ordered by segment
    assert as_tuples(eng.attached_collision_points(p.spheres, [], 0.05)) == as_tuples(p.spheres)
    only = eng.attached_collision_points([], bodies[:3], 0.05)
    assert [s.segment for s in only] == sorted(b[0] for b in bodies[:3])


def test_capacity_and_argument_refusals():
    lib = eng.load_library()
    p = mz.chain5()
    base = eng.sphere_array(p.spheres)
    shapes = eng.shape_array([BODIES["sphere"](), BODIES["box"]()])
    att = (eng.stomp_attached_body * 2)()
    for i in range(2):
        att[i].segment = 3
        att[i].shape = shapes[i]
    n_base = len(p.spheres)
    out = (eng.stomp_sphere * (n_base + 2))()
    out[0].radius = -7.0
    n = C.c_int32(-1)
    assert lib.stomp_attached_collision_points(base, n_base, att, 2, 0.05, out, n_base + 1, C.byref(n)) == -1
    assert "capacity" in lib.stomp_last_error().decode()
    assert n.value == n_base + 2 and out[0].radius == -7.0        # the size needed; out untouched
    assert lib.stomp_attached_collision_points(base, n_base, att, 2, 0.05, out, n_base + 2, C.byref(n)) == 0
    assert n.value == n_base + 2 and out[0].radius == p.spheres[0].radius
    assert lib.stomp_attached_collision_points(base, n_base, att, 2, 0.05, None, 0, C.byref(n)) == -1
    assert lib.stomp_attached_collision_points(base, n_base, att, 2, 0.05, out, n_base + 2, None) == -1
    assert lib.stomp_attached_collision_points(None, n_base, att, 2, 0.05, out, n_base + 2, C.byref(n)) == -1
    assert lib.stomp_attached_collision_points(base, n_base, None, 2, 0.05, out, n_base + 2, C.byref(n)) == -1
    assert lib.stomp_attached_collision_points(base, -1, att, 2, 0.05, out, n_base + 2, C.byref(n)) == -1
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        assert lib.stomp_attached_collision_points(base, n_base, att, 2, bad, out, n_base + 2, C.byref(n)) == -1
        assert "clearance" in lib.stomp_last_error().decode()
    att[1].shape.type = pb.SHAPE_BOX                             # an environment shape is no attached body
    assert lib.stomp_attached_collision_points(base, n_base, att, 2, 0.05, out, n_base + 2, C.byref(n)) == -1
    assert "no robot body shape" in lib.stomp_last_error().decode()
    att[1].shape.type = pb.BODY_MESH                             # a mesh without vertices
    assert lib.stomp_attached_collision_points(base, n_base, att, 2, 0.05, out, n_base + 2, C.byref(n)) == -1
    assert "vertices" in lib.stomp_last_error().decode()
