"""ctypes binding of the C ABI in include/stomp_engine.h (libstomp_engine.so, built in-tree).

There is no CPU fallback: if the HIP library is missing or cannot be loaded the
constructor raises.  The CPU oracle lives under oracle/ and is test-only.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
from typing import Optional

import numpy as np

from . import _build

_LIB_PATH = _build.LIB
ABI_VERSION = 4


class stomp_segment(C.Structure):
    _fields_ = [("parent", C.c_int32), ("q_index", C.c_int32), ("rot", C.c_double * 9),
                ("trans", C.c_double * 3), ("axis", C.c_double * 3)]


class stomp_sphere(C.Structure):
    _fields_ = [("segment", C.c_int32), ("radius", C.c_double), ("clearance", C.c_double), ("pos", C.c_double * 3)]


class stomp_shape(C.Structure):
    _fields_ = [("type", C.c_int32), ("position", C.c_double * 3), ("orientation", C.c_double * 4),
                ("dims", C.c_double * 3), ("vertices", C.POINTER(C.c_double)), ("num_vertices", C.c_int32)]


class stomp_joint(C.Structure):
    _fields_ = [("has_limits", C.c_int32), ("min", C.c_double), ("max", C.c_double), ("joint_cost", C.c_double)]


class stomp_grid(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("origin", C.c_double * 3),
                ("resolution", C.c_double), ("data", C.c_void_p), ("data_on_device", C.c_int32)]


class stomp_inertia(C.Structure):
    _fields_ = [("mass", C.c_double), ("com", C.c_double * 3), ("inertia", C.c_double * 6)]


class stomp_orientation_constraint(C.Structure):
    _fields_ = [("segment", C.c_int32), ("orientation", C.c_double * 4), ("body_fixed", C.c_int32),
                ("absolute_roll_tolerance", C.c_double), ("absolute_pitch_tolerance", C.c_double),
                ("absolute_yaw_tolerance", C.c_double), ("weight", C.c_double)]


class stomp_request(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("start", C.POINTER(C.c_double)), ("goal", C.POINTER(C.c_double)),
                ("seed", C.c_uint64), ("num_spheres", C.c_int32), ("spheres", C.POINTER(stomp_sphere)),
                ("num_orientation_constraints", C.c_int32),
                ("orientation_constraints", C.POINTER(stomp_orientation_constraint))]


class stomp_state_query(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("num_states", C.c_int32), ("states", C.POINTER(C.c_double)),
                ("num_links", C.c_int32), ("links", C.POINTER(C.c_int32)),
                ("positions", C.POINTER(C.c_double)), ("distances", C.POINTER(C.c_double)),
                ("potentials", C.POINTER(C.c_double)), ("sphere_collides", C.POINTER(C.c_uint8)),
                ("link_costs", C.POINTER(C.c_double)), ("state_cost", C.POINTER(C.c_double)),
                ("min_clearance", C.POINTER(C.c_double)), ("min_sphere", C.POINTER(C.c_int32)),
                ("in_collision", C.POINTER(C.c_uint8)), ("limits_violated", C.POINTER(C.c_uint8))]


class stomp_gradient_query(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("num_states", C.c_int32), ("states", C.POINTER(C.c_double)),
                ("num_links", C.c_int32), ("links", C.POINTER(C.c_int32)), ("field_bias", C.c_double * 3),
                ("field_gradients", C.POINTER(C.c_double)), ("potential_gradients", C.POINTER(C.c_double)),
                ("link_costs", C.POINTER(C.c_double)), ("link_gradients", C.POINTER(C.c_double)),
                ("state_cost", C.POINTER(C.c_double)), ("state_gradient", C.POINTER(C.c_double)),
                ("in_collision", C.POINTER(C.c_uint8))]


class stomp_attached_body(C.Structure):
    _fields_ = [("segment", C.c_int32), ("shape", stomp_shape)]


class stomp_engine_desc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("num_joints", C.c_int32), ("num_time_steps", C.c_int32),
                ("num_rollouts", C.c_int32), ("num_reused_rollouts", C.c_int32), ("num_segments", C.c_int32),
                ("segments", C.POINTER(stomp_segment)), ("num_spheres", C.c_int32),
                ("spheres", C.POINTER(stomp_sphere)), ("joints", C.POINTER(stomp_joint)), ("grid", stomp_grid),
                ("discretization", C.c_double), ("smoothness_costs", C.c_double * 3), ("ridge_factor", C.c_double),
                ("smoothness_cost_weight", C.c_double), ("obstacle_cost_weight", C.c_double),
                ("constraint_cost_weight", C.c_double), ("torque_cost_weight", C.c_double),
                ("noise_stddev", C.POINTER(C.c_double)), ("noise_decay", C.POINTER(C.c_double)),
                ("use_cumulative_costs", C.c_int32), ("start", C.POINTER(C.c_double)),
                ("goal", C.POINTER(C.c_double)), ("seed", C.c_uint64), ("max_iterations", C.c_int32),
                ("max_iterations_after_collision_free", C.c_int32), ("device", C.c_int32), ("stream", C.c_void_p),
                ("rank", C.c_int32), ("world_size", C.c_int32), ("comm_id", C.c_void_p),
                ("inertias", C.POINTER(stomp_inertia)), ("torque_root", C.c_int32), ("torque_tip", C.c_int32),
                ("gravity", C.c_double * 3), ("num_orientation_constraints", C.c_int32),
                ("orientation_constraints", C.POINTER(stomp_orientation_constraint))]


class stomp_iter_out(C.Structure):
    _fields_ = [("cost", C.c_double), ("collision_free", C.c_int32), ("constraints_satisfied", C.c_int32)]


class stomp_stats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("success", C.c_int32), ("success_iteration", C.c_int32),
                ("collision_success_iteration", C.c_int32), ("last_improvement_iteration", C.c_int32),
                ("best_cost", C.c_double), ("success_duration", C.c_double),
                ("collision_success_duration", C.c_double)]


class stomp_serve_result(C.Structure):
    _fields_ = [("slot", C.c_int32), ("start_step", C.c_int32), ("stats", stomp_stats)]


class stomp_chomp_params(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("learning_rate", C.c_double), ("smoothness_cost_weight", C.c_double),
                ("use_pseudo_inverse", C.c_int32), ("pseudo_inverse_ridge_factor", C.c_double),
                ("field_bias", C.c_double * 3), ("joint_update_limits", C.POINTER(C.c_double)),
                ("use_hamiltonian_monte_carlo", C.c_int32)]


# stomp_group_create_flags' accept mask
STOMP_GROUP_ACCEPT_STATE_TERMS = 1
STOMP_GROUP_ACCEPT_CUMULATIVE = 2


class stomp_group_options(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("state_terms", C.c_int32), ("compact", C.c_int32)]


# every symbol include/stomp_engine.h declares (checked by tests/test_abi.py)
EXPORTED = ["stomp_engine_create", "stomp_engine_destroy", "stomp_engine_last_error", "stomp_last_error",
            "stomp_engine_get_theta", "stomp_engine_set_theta", "stomp_engine_iterate", "stomp_engine_run",
            "stomp_engine_synchronize", "stomp_engine_eval", "stomp_engine_optimize",
            "stomp_engine_get_best_trajectory", "stomp_engine_get_last_trajectory", "stomp_engine_get_rollouts",
            "stomp_engine_get_matrix", "stomp_engine_get_pad_positions", "stomp_engine_set_timing",
            "stomp_engine_get_timing", "stomp_engine_local_rollouts", "stomp_sdf_build", "stomp_comm_unique_id",
            "stomp_device_selftest", "stomp_device_normals", "stomp_device_alloc", "stomp_device_free",
            "stomp_device_copy_to_host", "stomp_device_count", "stomp_diff_rules", "stomp_comm_local_id",
            "stomp_engine_get_best_torques", "stomp_pi_get_rollouts", "stomp_pi_set_rollout_costs",
            "stomp_pi_improve_policy", "stomp_pi_add_extra_rollouts", "stomp_pi_reset", "stomp_sdf_build_objects",
            "stomp_stream_create", "stomp_stream_destroy", "stomp_group_create", "stomp_group_run",
            "stomp_group_synchronize", "stomp_group_last_error", "stomp_group_destroy", "stomp_engine_shard_mode",
            "stomp_group_optimize", "stomp_group_optimize_chunk", "stomp_group_create_with",
            "stomp_group_create_flags",
            "stomp_engine_shard_info", "stomp_shard_decide", "stomp_engine_source_hash",
            "stomp_engine_refresh_field", "stomp_device_selftest_trig", "stomp_engine_retarget",
            "stomp_group_retarget", "stomp_scene_create", "stomp_scene_set_static", "stomp_scene_set_dynamic",
            "stomp_scene_window", "stomp_scene_info", "stomp_scene_destroy", "stomp_engine_retarget_request",
            "stomp_engine_model_info", "stomp_group_retarget_requests", "stomp_attached_collision_points",
            "stomp_group_serve", "stomp_group_serve_info", "stomp_serve_schedule", "stomp_engine_query_states",
            "stomp_engine_query_info", "stomp_engine_query_time", "stomp_chomp_create", "stomp_chomp_reset",
            "stomp_chomp_step", "stomp_chomp_synchronize", "stomp_chomp_optimize", "stomp_chomp_get",
            "stomp_chomp_info", "stomp_chomp_last_error", "stomp_chomp_destroy", "stomp_engine_query_gradients"]

_lib = None


def load_library(path: Optional[str] = None):
    """Loads libstomp_engine.so (building it first if absent and hipcc is available)."""
    global _lib
    if _lib is not None:
        return _lib
    explicit = path or os.environ.get("STOMP_ENGINE_LIB")
    path = explicit or _LIB_PATH
    if not os.path.exists(path):
        if os.path.exists(_build.HIPCC):
            _build.build()
        else:
            raise RuntimeError(f"STOMP HIP engine library missing: {path} (run __graft_entry__.build())")
    if not explicit:
        # the product library must be built from this checkout's sources (a variant named by
        # STOMP_ENGINE_LIB is an experiment's build with its own defines)
        built, want = _build.embedded_hash(path), _build.source_hash()
        if built != want:
            raise RuntimeError(f"stale STOMP engine library {path}: built from sources {built}, the checkout's "
                               f"are {want} (run __graft_entry__.build())")
    l = C.CDLL(path)
    l.stomp_engine_source_hash.restype = C.c_char_p
    l.stomp_engine_source_hash.argtypes = []
    P, dp = C.c_void_p, C.POINTER(C.c_double)
    l.stomp_engine_create.argtypes = [C.POINTER(stomp_engine_desc), C.POINTER(C.c_void_p)]
    l.stomp_engine_destroy.argtypes = [P]
    l.stomp_engine_last_error.restype = C.c_char_p
    l.stomp_engine_last_error.argtypes = [P]
    l.stomp_last_error.restype = C.c_char_p
    l.stomp_engine_get_theta.argtypes = [P, dp]
    l.stomp_engine_refresh_field.argtypes = [P]
    if hasattr(l, "stomp_engine_retarget"):   # (a variant library named by STOMP_ENGINE_LIB may predate them)
        l.stomp_engine_retarget.argtypes = [P, dp, dp, C.c_uint64]
        l.stomp_group_retarget.argtypes = [C.c_void_p, dp, dp, C.POINTER(C.c_uint64)]
    if hasattr(l, "stomp_engine_retarget_request"):
        l.stomp_engine_retarget_request.argtypes = [P, C.POINTER(stomp_request)]
        l.stomp_group_retarget_requests.argtypes = [C.c_void_p, C.POINTER(stomp_request)]
        l.stomp_engine_model_info.argtypes = [P, C.POINTER(C.c_int64)]
        l.stomp_attached_collision_points.argtypes = [C.POINTER(stomp_sphere), C.c_int32,
                                                      C.POINTER(stomp_attached_body), C.c_int32, C.c_double,
                                                      C.POINTER(stomp_sphere), C.c_int32, C.POINTER(C.c_int32)]
    l.stomp_engine_set_theta.argtypes = [P, dp]
    l.stomp_engine_iterate.argtypes = [P, C.c_int32, C.POINTER(stomp_iter_out)]
    l.stomp_engine_run.argtypes = [P, C.c_int32, C.c_int32]
    l.stomp_engine_synchronize.argtypes = [P]
    l.stomp_engine_eval.argtypes = [P, dp, C.c_int32, dp, C.POINTER(C.c_uint8), dp, C.c_int32, C.POINTER(C.c_uint8)]
    l.stomp_engine_optimize.argtypes = [P, C.POINTER(stomp_stats), dp]
    l.stomp_engine_get_best_trajectory.argtypes = [P, dp]
    l.stomp_engine_get_best_torques.argtypes = [P, dp]
    l.stomp_pi_get_rollouts.argtypes = [P, C.c_int32, dp, dp, C.POINTER(C.c_int32)]
    l.stomp_pi_set_rollout_costs.argtypes = [P, dp, C.c_double, dp]
    l.stomp_pi_improve_policy.argtypes = [P, dp]
    l.stomp_pi_add_extra_rollouts.argtypes = [P, C.c_int32, dp, dp]
    l.stomp_pi_reset.argtypes = [P]
    l.stomp_engine_get_last_trajectory.argtypes = [P, dp]
    l.stomp_engine_get_rollouts.argtypes = [P, C.c_char_p, dp]
    l.stomp_engine_get_matrix.argtypes = [P, C.c_char_p, C.c_int32, dp]
    l.stomp_engine_get_pad_positions.argtypes = [P, dp]
    l.stomp_engine_set_timing.argtypes = [P, C.c_int32]
    l.stomp_engine_get_timing.argtypes = [P, C.c_char_p, dp, C.POINTER(C.c_int32)]
    l.stomp_engine_local_rollouts.argtypes = [P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    l.stomp_engine_shard_mode.argtypes = [P, C.POINTER(C.c_int32)]
    l.stomp_engine_shard_info.argtypes = [P, dp]
    l.stomp_shard_decide.argtypes = [dp, C.POINTER(C.c_int32)]
    l.stomp_sdf_build.argtypes = [C.c_int32, C.c_int32, C.c_int32, dp, C.c_double, C.c_double, dp, C.c_int32, dp,
                                  C.c_int32, C.c_void_p, C.c_void_p]
    l.stomp_sdf_build_objects.argtypes = [C.c_int32, C.c_int32, C.c_int32, dp, C.c_double, C.c_double,
                                          C.POINTER(stomp_shape), C.c_int32, dp, C.c_int64, C.c_void_p,
                                          C.POINTER(C.c_int64), C.c_void_p]
    l.stomp_scene_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp, C.c_double, C.c_double,
                                     C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    for f in (l.stomp_scene_set_static, l.stomp_scene_set_dynamic):
        f.argtypes = [C.c_void_p, C.POINTER(stomp_shape), C.c_int32, dp, C.c_int64, C.POINTER(C.c_int64)]
    l.stomp_scene_window.argtypes = [C.c_int32, C.c_int32, C.c_int32, dp, C.c_double, C.c_double,
                                     C.POINTER(stomp_shape), C.c_int32, dp, C.c_int64, C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32)]
    l.stomp_scene_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    l.stomp_scene_destroy.argtypes = [C.c_void_p]
    l.stomp_scene_destroy.restype = None
    l.stomp_stream_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
    l.stomp_stream_destroy.argtypes = [C.c_void_p]
    l.stomp_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p)]
    l.stomp_group_create_with.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(stomp_group_options),
                                          C.POINTER(C.c_void_p)]
    if hasattr(l, "stomp_group_create_flags"):   # (a variant library named by STOMP_ENGINE_LIB may predate it)
        l.stomp_group_create_flags.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_uint32, C.c_int32,
                                               C.POINTER(C.c_void_p)]
    l.stomp_group_run.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    l.stomp_group_synchronize.argtypes = [C.c_void_p]
    l.stomp_group_optimize.argtypes = [C.c_void_p, C.POINTER(stomp_stats), dp, C.c_int32]
    l.stomp_group_optimize_chunk.restype = C.c_int32
    l.stomp_group_optimize_chunk.argtypes = []
    if hasattr(l, "stomp_group_serve"):   # (a variant library named by STOMP_ENGINE_LIB may predate them)
        ip = C.POINTER(C.c_int32)
        l.stomp_group_serve.argtypes = [C.c_void_p, dp, dp, C.POINTER(C.c_uint64), C.c_int32,
                                        C.POINTER(stomp_serve_result), dp, dp, C.c_int32]
        l.stomp_group_serve_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        l.stomp_serve_schedule.argtypes = [C.c_int32, C.c_int32, ip, ip, ip, ip]
    if hasattr(l, "stomp_engine_query_states"):   # (a variant library named by STOMP_ENGINE_LIB may predate them)
        l.stomp_engine_query_states.argtypes = [P, C.POINTER(stomp_state_query)]
        l.stomp_engine_query_info.argtypes = [P, C.POINTER(C.c_int64)]
        l.stomp_engine_query_time.argtypes = [P, dp]
    if hasattr(l, "stomp_engine_query_gradients"):
        l.stomp_engine_query_gradients.argtypes = [P, C.POINTER(stomp_gradient_query)]
    if hasattr(l, "stomp_chomp_create"):   # (a variant library named by STOMP_ENGINE_LIB may predate them)
        l.stomp_chomp_create.argtypes = [P, C.POINTER(stomp_chomp_params), C.POINTER(C.c_void_p)]
        l.stomp_chomp_reset.argtypes = [P, C.c_int32, dp]
        l.stomp_chomp_step.argtypes = [P, C.c_int32]
        l.stomp_chomp_synchronize.argtypes = [P]
        l.stomp_chomp_optimize.argtypes = [P, C.POINTER(stomp_stats), dp, C.c_int32, dp]
        l.stomp_chomp_get.argtypes = [P, C.c_char_p, dp]
        l.stomp_chomp_info.argtypes = [P, C.POINTER(C.c_int64)]
        l.stomp_chomp_last_error.restype = C.c_char_p
        l.stomp_chomp_last_error.argtypes = [P]
        l.stomp_chomp_destroy.argtypes = [P]
        l.stomp_chomp_destroy.restype = None
    l.stomp_group_last_error.restype = C.c_char_p
    l.stomp_group_last_error.argtypes = [C.c_void_p]
    l.stomp_group_destroy.argtypes = [C.c_void_p]
    l.stomp_comm_unique_id.argtypes = [C.c_void_p]
    l.stomp_comm_local_id.argtypes = [C.c_int32, C.c_void_p]
    l.stomp_device_alloc.argtypes = [C.c_int32, C.c_uint64, C.POINTER(C.c_void_p)]
    l.stomp_device_free.argtypes = [C.c_void_p]
    l.stomp_device_copy_to_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    l.stomp_device_count.argtypes = [C.POINTER(C.c_int32)]
    l.stomp_diff_rules.argtypes = [dp]
    l.stomp_device_selftest.argtypes = [dp, C.c_int32, dp, dp, dp, dp, dp]
    l.stomp_device_selftest_trig.argtypes = [dp, dp, C.c_int32, dp, dp]
    l.stomp_device_normals.argtypes = [C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp]
    _lib = l
    return l


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _check(rc: int, handle=None):
    if rc != 0:
        l = load_library()
        msg = (l.stomp_engine_last_error(handle) if handle else l.stomp_last_error()).decode()
        raise RuntimeError(f"stomp engine error {rc}: {msg}")


def sdf_build_device(problem, device_tensor_ptr: int, stream: int = 0):
    """Builds problem.grid's distance field directly into a device buffer of nx*ny*nz uint16 squared cell
    distances (stomp_grid's representation; problem.build_sdf is the host twin)."""
    l = load_library()
    g = problem.grid
    boxes = np.array([list(b.center) + list(b.dims) for b in problem.boxes], np.float64).reshape(-1)
    cyl = np.array([list(c.center) + [c.radius, c.length] for c in problem.cylinders], np.float64).reshape(-1)
    origin = np.array(g.origin, np.float64)
    boxes = boxes if boxes.size else np.zeros(1)
    cyl = cyl if cyl.size else np.zeros(1)
    _check(l.stomp_sdf_build(g.nx, g.ny, g.nz, _dp(origin), g.resolution, g.max_expansion, _dp(boxes),
                             len(problem.boxes), _dp(cyl), len(problem.cylinders), C.c_void_p(device_tensor_ptr),
                             C.c_void_p(stream)))


def shape_array(objects):
    """problem.SceneObject list -> stomp_shape[] (ctypes array; length >= 1; it keeps the mesh
    vertex arrays alive as ._keep)."""
    arr = (stomp_shape * max(len(objects), 1))()
    arr._keep = []
    for i, o in enumerate(objects):
        arr[i].type = int(o.type)
        arr[i].position[:] = [float(v) for v in o.position]
        arr[i].orientation[:] = [float(v) for v in o.orientation]
        d = list(o.dims) + [0.0] * (3 - len(o.dims))
        arr[i].dims[:] = [float(v) for v in d[:3]]
        if getattr(o, "vertices", None) is not None:
            v = np.ascontiguousarray(o.vertices, np.float64).reshape(-1, 3)
            arr._keep.append(v)
            arr[i].vertices = _dp(v)
            arr[i].num_vertices = len(v)
    return arr


def sdf_build_objects_device(grid, objects, device_ptr: int, points=None, stream: int = 0) -> int:
    """The reference's distance-field fill (stomp_sdf_build_objects) of problem.Grid `grid` from
    collision objects (problem.SceneObject) and collision-map points (P x 3) into a device buffer
    of nx*ny*nz uint16 squared cell distances.  Returns the number of points that landed in the grid."""
    l = load_library()
    origin = np.array(grid.origin, np.float64)
    pts = np.ascontiguousarray(points if points is not None else np.zeros((0, 3)), np.float64).reshape(-1, 3)
    marked = C.c_int64(0)
    _check(l.stomp_sdf_build_objects(grid.nx, grid.ny, grid.nz, _dp(origin), grid.resolution, grid.max_expansion,
                                     shape_array(objects), len(objects), _dp(pts if pts.size else np.zeros(3)),
                                     len(pts), C.c_void_p(device_ptr), C.byref(marked), C.c_void_p(stream)))
    return marked.value


def _points(points):
    pts = np.ascontiguousarray(points if points is not None else np.zeros((0, 3)), np.float64).reshape(-1, 3)
    return pts, _dp(pts if pts.size else np.zeros(3))


def scene_window(grid, objects, points=None):
    """stomp_scene_window (host only): the window Scene.set_dynamic would use for these inputs on
    problem.Grid `grid`, as inclusive cell bounds (lo, hi), or None when nothing can land in the grid."""
    origin = np.array(grid.origin, np.float64)
    pts, pp = _points(points)
    lo, hi = (C.c_int32 * 3)(), (C.c_int32 * 3)()
    _check(load_library().stomp_scene_window(grid.nx, grid.ny, grid.nz, _dp(origin), grid.resolution,
                                             grid.max_expansion, shape_array(objects), len(objects), pp, len(pts),
                                             lo, hi))
    return None if lo[0] > hi[0] else (tuple(lo), tuple(hi))


class Scene:
    """stomp_scene: the field of sdf_build_objects_device kept in two layers over the device buffer
    `device_ptr` (grid.cells uint16).  set_static builds the layer that stays (shelves, walls);
    set_dynamic replaces the per-request set (the robot's own bodies, the sensor points) and costs
    work over the window around its marks only.  After either the buffer holds, bit for bit,
    sdf_build_objects_device of the static inputs followed by the dynamic ones.  stream: a HIP
    stream (Stream.ptr; None: one the scene owns) -- everything is enqueued there and, unless
    count=True, nothing waits for the device."""

    def __init__(self, grid, device_ptr: int, device: int = 0, stream: Optional[int] = None):
        self._h = None   # set before the call that may raise, so __del__ has nothing to free
        self.grid = grid
        origin = np.array(grid.origin, np.float64)
        h = C.c_void_p()
        _check(load_library().stomp_scene_create(device, grid.nx, grid.ny, grid.nz, _dp(origin), grid.resolution,
                                                 grid.max_expansion, C.c_void_p(device_ptr),
                                                 C.c_void_p(stream) if stream else None, C.byref(h)))
        self._h = h

    def _set(self, fn, objects, points, count):
        pts, pp = _points(points)
        marked = C.c_int64(0)
        _check(fn(self._h, shape_array(objects), len(objects), pp, len(pts), C.byref(marked) if count else None))
        return marked.value if count else None

    def set_static(self, objects, points=None, count: bool = False):
        """The static layer from problem.SceneObject list `objects` and collision-map points (P x 3);
        any dynamic set is dropped.  count=True waits and returns the points that landed in the grid."""
        return self._set(load_library().stomp_scene_set_static, objects, points, count)

    def set_dynamic(self, objects, points=None, count: bool = False):
        """Replaces the dynamic set (empty lists: the static field).  count as in set_static; the
        static and dynamic counts add up to sdf_build_objects_device's of all inputs."""
        return self._set(load_library().stomp_scene_set_dynamic, objects, points, count)

    def info(self) -> dict:
        """stomp_scene_info (waits for the stream): the last call's window (None when empty), its
        cells, the cells restored from the static layer, the stray marks (a check on the window
        bound: always 0) and the allocations set_dynamic has made."""
        v = (C.c_int64 * 10)()
        _check(load_library().stomp_scene_info(self._h, v))
        return dict(window=None if v[0] > v[3] else (tuple(v[0:3]), tuple(v[3:6])), cells=v[6], restored=v[7],
                    stray=v[8], allocations=v[9], raw=list(v))

    def close(self):
        if self._h is not None and self._h.value:
            load_library().stomp_scene_destroy(self._h)
        self._h = None

    def __del__(self):
        self.close()


def sphere_array(spheres):
    """problem.Sphere list -> stomp_sphere[] (ctypes array; length >= 1)."""
    return (stomp_sphere * max(len(spheres), 1))(*[
        stomp_sphere(s.segment, s.radius, s.clearance, (C.c_double * 3)(*s.pos)) for s in spheres])


def constraint_array(robot, constraints):
    """problem.OrientationConstraint list -> stomp_orientation_constraint[] (length >= 1)."""
    return (stomp_orientation_constraint * max(len(constraints), 1))(*[
        stomp_orientation_constraint(robot.index(c.link_name), (C.c_double * 4)(*c.orientation),
                                     0 if c.header_frame else 1, c.absolute_roll_tolerance,
                                     c.absolute_pitch_tolerance, c.absolute_yaw_tolerance, c.weight)
        for c in constraints])


def attached_collision_points(spheres, bodies, clearance: float):
    """stomp_attached_collision_points (host only): the collision points of a robot holding attached
    bodies.  spheres: the robot's own list (problem.Sphere); bodies: (segment, problem.SceneObject)
    pairs, each a STOMP_BODY_* shape posed in its owner segment's frame.  Every body becomes one
    sphere at its bounding sphere's centre with that radius and `clearance`, placed after the last
    sphere of its segment.  Returns the new problem.Sphere list."""
    from .problem import Sphere
    l = load_library()
    base = sphere_array(spheres)
    shapes = shape_array([o for _, o in bodies])
    att = (stomp_attached_body * max(len(bodies), 1))()
    for i, (seg, _) in enumerate(bodies):
        att[i].segment = int(seg)
        att[i].shape = shapes[i]
    cap = len(spheres) + len(bodies)
    out = (stomp_sphere * max(cap, 1))()
    n = C.c_int32(0)
    _check(l.stomp_attached_collision_points(base, len(spheres), att, len(bodies), float(clearance), out, cap,
                                             C.byref(n)))
    return [Sphere(out[i].segment, out[i].radius, out[i].clearance, tuple(out[i].pos)) for i in range(n.value)]


class StateQueryResult:
    """Engine.query_states' arrays, one attribute per output of stomp_state_query (None: not asked for)."""
    positions = distances = potentials = sphere_collides = link_costs = state_cost = None
    min_clearance = min_sphere = in_collision = limits_violated = None


class GradientQueryResult:
    """Engine.query_gradients' arrays, one attribute per output of stomp_gradient_query (None: not asked for)."""
    field_gradients = potential_gradients = link_costs = link_gradients = None
    state_cost = state_gradient = in_collision = None


class Engine:
    """One planning problem on one device: the StompOptimizer / PolicyImprovementLoop pair."""

    def __init__(self, problem, device: int = 0, sdf_device_ptr: Optional[int] = None, stream: Optional[int] = None,
                 rank: int = 0, world_size: int = 1, comm_id: Optional[bytes] = None):
        l = load_library()
        p = problem
        self.problem = p
        self.J, self.N, self.K = p.J, p.N, p.params.num_rollouts
        self.S = len(p.spheres)
        self._segs = (stomp_segment * len(p.robot.segments))(*[
            stomp_segment(s.parent, s.q_index, (C.c_double * 9)(*s.rot), (C.c_double * 3)(*s.trans),
                          (C.c_double * 3)(*s.axis)) for s in p.robot.segments])
        self._sph = sphere_array(p.spheres)
        self._joints = (stomp_joint * self.J)(*[
            stomp_joint(int(j.has_limits), j.min, j.max, j.joint_cost) for j in p.robot.joints])
        pr = p.params
        self._sig = pr.per_joint("noise_stddev", self.J)
        self._dec = pr.per_joint("noise_decay", self.J)
        self._start = np.ascontiguousarray(p.start, np.float64)
        self._goal = np.ascontiguousarray(p.goal, np.float64)
        g = p.grid
        d = stomp_engine_desc()
        d.abi_version = ABI_VERSION
        d.num_joints, d.num_time_steps, d.num_rollouts = self.J, self.N, self.K
        d.num_reused_rollouts = pr.num_reused_rollouts
        d.num_segments = len(p.robot.segments)
        d.segments = self._segs
        d.num_spheres = self.S
        d.spheres = self._sph
        d.joints = self._joints
        if sdf_device_ptr is not None:
            grid_ptr, on_dev = sdf_device_ptr, 1
        else:
            # ABI v4: the field is the integer squared cell distance (PropagationDistanceField's
            # distance_square_), not metres; a float field would truncate to "in collision" silently
            sdf = np.asarray(p.sdf)
            if not np.issubdtype(sdf.dtype, np.integer):
                raise TypeError(f"problem.sdf must hold integer squared cell distances (uint16), got {sdf.dtype}")
            if sdf.size and (int(sdf.min()) < 0 or int(sdf.max()) > 65535):
                raise ValueError("problem.sdf squared cell distances must lie in [0, 65535]")
            if sdf.shape != tuple(g.dims):
                raise ValueError(f"problem.sdf has shape {sdf.shape}, the grid is {tuple(g.dims)}")
            self._sdf = np.ascontiguousarray(sdf, np.uint16)
            grid_ptr, on_dev = self._sdf.ctypes.data, 0
        d.grid = stomp_grid(g.nx, g.ny, g.nz, (C.c_double * 3)(*g.origin), g.resolution, C.c_void_p(grid_ptr), on_dev)
        d.discretization = pr.trajectory_discretization
        d.smoothness_costs = (C.c_double * 3)(pr.smoothness_cost_velocity, pr.smoothness_cost_acceleration,
                                              pr.smoothness_cost_jerk)
        d.ridge_factor = pr.ridge_factor
        d.smoothness_cost_weight = pr.smoothness_cost_weight
        d.obstacle_cost_weight = pr.obstacle_cost_weight
        d.constraint_cost_weight = pr.constraint_cost_weight
        d.torque_cost_weight = pr.torque_cost_weight
        d.noise_stddev = _dp(self._sig)
        d.noise_decay = _dp(self._dec)
        d.use_cumulative_costs = int(pr.use_cumulative_costs)
        d.start = _dp(self._start)
        d.goal = _dp(self._goal)
        d.seed = p.seed
        d.max_iterations = pr.max_iterations
        d.max_iterations_after_collision_free = pr.max_iterations_after_collision_free
        d.device = device
        d.stream = C.c_void_p(stream) if stream else None
        d.rank = rank
        d.world_size = world_size
        self._comm = C.create_string_buffer(comm_id, 128) if comm_id else None
        d.comm_id = C.cast(self._comm, C.c_void_p) if comm_id else None
        nseg = len(p.robot.segments)
        self._inertia = (stomp_inertia * nseg)(*[
            stomp_inertia(s.inertia.mass, (C.c_double * 3)(*s.inertia.com), (C.c_double * 6)(*s.inertia.inertia))
            if s.inertia else stomp_inertia() for s in p.robot.segments])
        d.inertias = self._inertia
        d.torque_root, d.torque_tip = p.torque_segments()
        d.gravity = (C.c_double * 3)(*p.gravity)
        oc = p.orientation_constraints
        self._oc = constraint_array(p.robot, oc)
        d.num_orientation_constraints = len(oc)
        d.orientation_constraints = self._oc
        self._desc = d
        h = C.c_void_p()
        _check(l.stomp_engine_create(C.byref(d), C.byref(h)))
        self.h = h
        first, count = C.c_int32(), C.c_int32()
        l.stomp_engine_local_rollouts(self.h, C.byref(first), C.byref(count))
        self.first, self.K_loc = first.value, count.value
        mode = C.c_int32()
        _check(l.stomp_engine_shard_mode(self.h, C.byref(mode)))
        self.shard_mode = {0: "none", 1: "partials", 2: "gather"}[mode.value]
        info = np.zeros(6)
        _check(l.stomp_engine_shard_info(self.h, _dp(info)))
        # measured at creation when both decompositions were possible (stomp_engine_shard_info), us
        self.shard_info = None if info[1] == 0.0 else dict(
            t_gather=info[1], t_partials=info[2], l_allreduce=info[3], l_allgather_state=info[4],
            l_allgather_partials=info[5])

    def close(self):
        h = getattr(self, "h", None)
        if h:
            load_library().stomp_engine_destroy(h)
            self.h = None

    def __del__(self):
        self.close()

    # ---------------------------------------------------------------- API
    def theta(self) -> np.ndarray:
        out = np.zeros((self.J, self.N))
        _check(load_library().stomp_engine_get_theta(self.h, _dp(out)), self.h)
        return out

    def set_theta(self, theta):
        t = np.ascontiguousarray(theta, np.float64)
        _check(load_library().stomp_engine_set_theta(self.h, _dp(t)), self.h)

    def iterate(self, iteration_number: int):
        o = stomp_iter_out()
        _check(load_library().stomp_engine_iterate(self.h, iteration_number, C.byref(o)), self.h)
        self.last_constraints_satisfied = bool(o.constraints_satisfied)
        return o.cost, bool(o.collision_free)

    def run(self, first_iteration: int, count: int):
        _check(load_library().stomp_engine_run(self.h, first_iteration, count), self.h)

    def synchronize(self):
        _check(load_library().stomp_engine_synchronize(self.h), self.h)

    def refresh_field(self):
        """stomp_engine_refresh_field: the caller rebuilt its device field in place."""
        _check(load_library().stomp_engine_refresh_field(self.h), self.h)

    def retarget(self, start, goal, seed: Optional[int] = None, spheres=None, orientation_constraints=None):
        """stomp_engine_retarget: the live engine onto a new start, goal and seed (None keeps the
        engine's seed).  Afterwards it is the engine Engine(problem') would be for problem' =
        dataclasses.replace(problem, start=..., goal=..., seed=...), which self.problem becomes; the
        iteration state it held is dropped.  A refused call raises and changes nothing.
        spheres (problem.Sphere list) / orientation_constraints (problem.OrientationConstraint list):
        the request's collision points and path constraints too (stomp_engine_retarget_request);
        None keeps the engine's, an empty list means none.  problem' then has them replaced as well,
        and S, pad_positions() and model_info() follow."""
        s = np.ascontiguousarray(start, np.float64).reshape(-1)
        g = np.ascontiguousarray(goal, np.float64).reshape(-1)
        if s.shape != (self.J,) or g.shape != (self.J,):
            raise ValueError(f"start and goal must hold {self.J} values")
        seed = int(self.problem.seed if seed is None else seed)
        if spheres is None and orientation_constraints is None:
            _check(load_library().stomp_engine_retarget(self.h, _dp(s), _dp(g), C.c_uint64(seed)), self.h)
            self._follow(s, g, seed)
            return
        req, keep = self._request(s, g, seed, spheres, orientation_constraints)
        # (a refusal writes nothing of the engine, not even its message: the thread's last error has it)
        _check(load_library().stomp_engine_retarget_request(self.h, C.byref(req)))
        self._follow(s, g, seed, spheres, orientation_constraints, keep)

    def _request(self, s, g, seed, spheres, constraints):
        """a stomp_request and the ctypes arrays it points to (kept by the caller until the call
        returns, and by _follow afterwards: the descriptor copy names them)"""
        sph = None if spheres is None else sphere_array(spheres)
        oc = None if constraints is None else constraint_array(self.problem.robot, constraints)
        req = stomp_request(C.sizeof(stomp_request), _dp(s), _dp(g), seed,
                            -1 if spheres is None else len(spheres), sph,
                            -1 if constraints is None else len(constraints), oc)
        return req, (sph, oc)

    def _follow(self, start, goal, seed, spheres=None, constraints=None, arrays=(None, None)):
        """the Python side of a retarget: the problem attribute and the arrays the descriptor names"""
        # fresh arrays: the old ones may be the caller's problem's own
        self._start, self._goal = np.array(start, np.float64), np.array(goal, np.float64)
        self._desc.start, self._desc.goal, self._desc.seed = _dp(self._start), _dp(self._goal), seed
        changes = dict(start=self._start.copy(), goal=self._goal.copy(), seed=seed)
        if spheres is not None:
            self._sph, self.S = arrays[0], len(spheres)
            self._desc.num_spheres, self._desc.spheres = self.S, self._sph
            changes["spheres"] = list(spheres)
        if constraints is not None:
            self._oc = arrays[1]
            self._desc.num_orientation_constraints, self._desc.orientation_constraints = len(constraints), self._oc
            changes["orientation_constraints"] = list(constraints)
        self.problem = dataclasses.replace(self.problem, **changes)

    MODEL_INFO = ("S", "nops", "nslots", "nsaves", "sph_chunk", "pad_lds", "lean", "sincos_pre",
                  "orientation_constraints", "terms_on", "model_changes", "request_allocations")

    def model_info(self) -> dict:
        """stomp_engine_model_info: the engine's current model (spheres, FK program steps, frame
        slots, saved frames, longest sphere run, the rollout layout's choices, constraints, terms),
        the model changes so far and the allocations made inside retarget calls of either kind (the
        call staging of the first one included; a repeated call allocates nothing)."""
        v = (C.c_int64 * 12)()
        _check(load_library().stomp_engine_model_info(self.h, v), self.h)
        return dict(zip(self.MODEL_INFO, [int(x) for x in v]))

    # stomp_state_query's outputs: name -> (dtype, shape of one state; S spheres, L links)
    QUERY_OUTPUTS = dict(positions=(np.float64, "S3"), distances=(np.float64, "S"), potentials=(np.float64, "S"),
                         sphere_collides=(np.uint8, "S"), link_costs=(np.float64, "L"), state_cost=(np.float64, ""),
                         min_clearance=(np.float64, ""), min_sphere=(np.int32, ""), in_collision=(np.uint8, ""),
                         limits_violated=(np.uint8, ""))
    QUERY_DEFAULT = tuple(k for k in QUERY_OUTPUTS if k != "positions")
    QUERY_INFO = ("chunks", "launches", "allocations", "chunk_states")

    def query_states(self, states, links=None, want=QUERY_DEFAULT, fill=None):
        """stomp_engine_query_states: the M joint states (M x J, or one state of J values) against the
        engine's current model and field.  links: segment indices or link names (resolved through
        problem.robot.segments) whose costs are wanted; want: the names of stomp_state_query's
        outputs to compute (default: all but positions; link_costs only with links).  Returns a
        StateQueryResult whose attributes are numpy arrays (None where not asked for); the flags are
        bool arrays.  fill: a value every output array holds before the call (tests of refusals:
        the arrays of a refused call are attached to the exception as .outputs)."""
        q = np.ascontiguousarray(states, np.float64)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        if q.ndim != 2 or q.shape[1] != self.J:
            raise ValueError(f"states must be M x {self.J}")
        M = q.shape[0]
        names = [s.name for s in self.problem.robot.segments]
        idx = [names.index(v) if isinstance(v, str) else int(v) for v in (links if links is not None else [])]
        L = len(idx)
        lk = np.ascontiguousarray(idx, np.int32)
        unknown = [k for k in want if k not in self.QUERY_OUTPUTS]
        if unknown:
            raise KeyError(f"no such query outputs: {unknown}")
        S = self.S
        dims = {"S3": (S, 3), "S": (S,), "L": (L,), "": ()}
        out = {}
        for k in want:
            if k == "link_costs" and links is None:
                continue
            dt, shp = self.QUERY_OUTPUTS[k]
            out[k] = np.zeros((M,) + dims[shp], dt) if fill is None else np.full((M,) + dims[shp], fill, dt)
        sq = stomp_state_query()
        sq.struct_size = C.sizeof(stomp_state_query)
        sq.num_states = M
        sq.states = _dp(q)
        sq.num_links = L
        sq.links = lk.ctypes.data_as(C.POINTER(C.c_int32)) if L else None
        ctype = {np.float64: C.c_double, np.uint8: C.c_uint8, np.int32: C.c_int32}
        for k, a in out.items():
            setattr(sq, k, a.ctypes.data_as(C.POINTER(ctype[self.QUERY_OUTPUTS[k][0]])))
        # (a refusal writes nothing of the engine, not even its message: the thread's last error has it)
        rc = load_library().stomp_engine_query_states(self.h, C.byref(sq))
        if rc != 0:
            try:
                _check(rc)
            except RuntimeError as err:
                err.outputs = out
                raise
        res = StateQueryResult()
        for k in self.QUERY_OUTPUTS:
            a = out.get(k)
            if a is not None and k in ("sphere_collides", "in_collision", "limits_violated"):
                a = a.astype(bool)
            setattr(res, k, a)
        return res

    # stomp_gradient_query's outputs: name -> (dtype, shape of one state; S spheres, L links, J joints)
    GRADIENT_OUTPUTS = dict(field_gradients=(np.float64, "S3"), potential_gradients=(np.float64, "S3"),
                            link_costs=(np.float64, "L"), link_gradients=(np.float64, "LJ"),
                            state_cost=(np.float64, ""), state_gradient=(np.float64, "J"),
                            in_collision=(np.uint8, ""))
    GRADIENT_DEFAULT = ("link_costs", "link_gradients", "state_cost", "state_gradient", "in_collision")

    def query_gradients(self, states, links=None, field_bias=(0.0, 0.0, 0.0), want=GRADIENT_DEFAULT, fill=None):
        """stomp_engine_query_gradients (srv/GetChompCollisionCost.srv): the M joint states (M x J, or
        one state of J values) against the engine's current model and field.  links: segment indices
        or link names; field_bias: CHOMP's field_bias; want: the names of stomp_gradient_query's
        outputs to compute (default: the per-link and per-state ones; the per-link ones only with
        links).  Returns a GradientQueryResult of numpy arrays (None where not asked for;
        in_collision is a bool array).  fill: as in query_states."""
        q = np.ascontiguousarray(states, np.float64)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        if q.ndim != 2 or q.shape[1] != self.J:
            raise ValueError(f"states must be M x {self.J}")
        M = q.shape[0]
        names = [s.name for s in self.problem.robot.segments]
        idx = [names.index(v) if isinstance(v, str) else int(v) for v in (links if links is not None else [])]
        L = len(idx)
        lk = np.ascontiguousarray(idx, np.int32)
        unknown = [k for k in want if k not in self.GRADIENT_OUTPUTS]
        if unknown:
            raise KeyError(f"no such gradient query outputs: {unknown}")
        S = self.S
        dims = {"S3": (S, 3), "L": (L,), "LJ": (L, self.J), "J": (self.J,), "": ()}
        out = {}
        for k in want:
            if k in ("link_costs", "link_gradients") and links is None:
                continue
            dt, shp = self.GRADIENT_OUTPUTS[k]
            out[k] = np.zeros((M,) + dims[shp], dt) if fill is None else np.full((M,) + dims[shp], fill, dt)
        gq = stomp_gradient_query()
        gq.struct_size = C.sizeof(stomp_gradient_query)
        gq.num_states = M
        gq.states = _dp(q)
        gq.num_links = L
        gq.links = lk.ctypes.data_as(C.POINTER(C.c_int32)) if L else None
        gq.field_bias = (C.c_double * 3)(*[float(v) for v in field_bias])
        for k, a in out.items():
            ct = C.c_uint8 if self.GRADIENT_OUTPUTS[k][0] is np.uint8 else C.c_double
            setattr(gq, k, a.ctypes.data_as(C.POINTER(ct)))
        rc = load_library().stomp_engine_query_gradients(self.h, C.byref(gq))
        if rc != 0:
            try:
                _check(rc)
            except RuntimeError as err:
                err.outputs = out
                raise
        res = GradientQueryResult()
        for k in self.GRADIENT_OUTPUTS:
            a = out.get(k)
            if a is not None and k == "in_collision":
                a = a.astype(bool)
            setattr(res, k, a)
        return res

    def query_info(self) -> dict:
        """stomp_engine_query_info: the last query call's chunks, launches and states per chunk, and
        the allocations made inside query calls so far; kernel_ms: its launches' device time."""
        v = (C.c_int64 * 4)()
        _check(load_library().stomp_engine_query_info(self.h, v), self.h)
        ms = C.c_double()
        _check(load_library().stomp_engine_query_time(self.h, C.byref(ms)), self.h)
        return dict(zip(self.QUERY_INFO, [int(x) for x in v]), kernel_ms=ms.value)

    def execute(self, params, iteration_member: int = 1):
        prm = np.ascontiguousarray(params, np.float64)
        single = prm.ndim == 2
        prm = prm.reshape(-1, self.J, self.N)
        n = prm.shape[0]
        costs = np.zeros((n, self.N))
        cf = np.zeros(n, np.uint8)
        traj = np.zeros((n, self.J, self.N))
        cs = np.zeros(n, np.uint8)
        u8 = C.POINTER(C.c_uint8)
        _check(load_library().stomp_engine_eval(self.h, _dp(prm), n, _dp(costs), cf.ctypes.data_as(u8), _dp(traj),
                                                iteration_member, cs.ctypes.data_as(u8)), self.h)
        self.last_constraints_satisfied = cs.astype(bool)
        if single:
            return costs[0], bool(cf[0]), traj[0]
        return costs, cf.astype(bool), traj

    def optimize(self):
        st = stomp_stats()
        costs = np.zeros(max(self.problem.params.max_iterations, 1))
        _check(load_library().stomp_engine_optimize(self.h, C.byref(st), _dp(costs)), self.h)
        return st, costs[: st.iterations]

    def best_trajectory(self) -> np.ndarray:
        out = np.zeros((self.J, self.N))
        _check(load_library().stomp_engine_get_best_trajectory(self.h, _dp(out)), self.h)
        return out

    def last_trajectory(self) -> np.ndarray:
        out = np.zeros((self.J, self.N))
        _check(load_library().stomp_engine_get_last_trajectory(self.h, _dp(out)), self.h)
        return out

    def best_torques(self) -> np.ndarray:
        out = np.zeros(self.N)
        _check(load_library().stomp_engine_get_best_torques(self.h, _dp(out)), self.h)
        return out

    # ---------------------------------------------------- PolicyImprovement API (stomp_pi_*)
    def pi_get_rollouts(self, iteration: int, noise_stddev) -> np.ndarray:
        sig = np.ascontiguousarray(noise_stddev, np.float64)
        out = np.zeros((self.K, self.J, self.N))
        n = C.c_int32()
        _check(load_library().stomp_pi_get_rollouts(self.h, iteration, _dp(sig), _dp(out), C.byref(n)), self.h)
        return out[: n.value]

    def pi_set_rollout_costs(self, costs, control_cost_weight: float) -> np.ndarray:
        c = np.zeros((self.K, self.N))
        cc = np.asarray(costs, np.float64)
        c[: cc.shape[0]] = cc
        totals = np.zeros(self.K)
        _check(load_library().stomp_pi_set_rollout_costs(self.h, _dp(c), control_cost_weight, _dp(totals)), self.h)
        return totals

    def pi_improve_policy(self) -> np.ndarray:
        out = np.zeros((self.J, self.N))
        _check(load_library().stomp_pi_improve_policy(self.h, _dp(out)), self.h)
        return out

    def pi_add_extra_rollout(self, params, costs):
        p = np.ascontiguousarray(params, np.float64)
        c = np.ascontiguousarray(costs, np.float64)
        _check(load_library().stomp_pi_add_extra_rollouts(self.h, 1, _dp(p), _dp(c)), self.h)

    def pi_reset(self):
        """setNumRollouts with the engine's counts: the next iteration generates every rollout."""
        _check(load_library().stomp_pi_reset(self.h), self.h)

    def rollouts(self, which: str) -> np.ndarray:
        """params, noise, control_costs, probabilities, cumulative_costs (engines with
        use_cumulative_costs: the rows the last weights launch read): K_loc x J x N; state_costs:
        K_loc x N; x_params, x_noise, x_control_costs: J x N; x_state_costs: N."""
        if which.startswith("x_"):
            shape = (self.N,) if which == "x_state_costs" else (self.J, self.N)
        else:
            shape = (self.K_loc, self.N) if which == "state_costs" else (self.K_loc, self.J, self.N)
        out = np.zeros(shape)
        _check(load_library().stomp_engine_get_rollouts(self.h, which.encode(), _dp(out)), self.h)
        return out

    def matrix(self, which: str, joint: int = 0) -> np.ndarray:
        n = self.N + 12 if which in ("D0", "D1", "D2") else self.N
        out = np.zeros((n, n))
        _check(load_library().stomp_engine_get_matrix(self.h, which.encode(), joint, _dp(out)), self.h)
        return out

    def pad_positions(self) -> np.ndarray:
        out = np.zeros((12, self.S, 3))
        _check(load_library().stomp_engine_get_pad_positions(self.h, _dp(out)), self.h)
        return out

    def set_timing(self, enable: bool):
        _check(load_library().stomp_engine_set_timing(self.h, int(enable)), self.h)

    def timing(self, name: str):
        t, n = C.c_double(), C.c_int32()
        _check(load_library().stomp_engine_get_timing(self.h, name.encode(), C.byref(t), C.byref(n)), self.h)
        return t.value, n.value


class Chomp:
    """CHOMP mode on a live engine (stomp_chomp_*): B independent covariant gradient descents between
    the engine's start and goal, on its model, field and cost.  The engine must outlive the object;
    nothing of the engine changes.  The defaults are the reference's (stomp_parameters.cpp:56-72,
    stomp_robot_model.cpp:78)."""

    # per-descent shapes of get()'s arrays from (J, N, S)
    SHAPES = dict(trajectory="JN", smoothness_increments="JN", collision_increments="JN", final_increments="JN",
                  scales="J", sphere_positions="AS3", distances="NS", field_gradients="NS3", potentials="NS",
                  potential_gradients="NS3", velocities="NS3", accelerations="NS3", vel_mags="NS",
                  joint_origins="NJ3", joint_axes="NJ3", costs="N", cost="", collision_free="")
    INFO = ("B", "iterations", "launches", "allocations", "lds_fk", "lds_gradient", "lds_update", "lds_bookkeeping")

    def __init__(self, engine, learning_rate: float = 0.01, smoothness_cost_weight: float = 0.1,
                 use_pseudo_inverse: bool = False, pseudo_inverse_ridge_factor: float = 1e-4,
                 field_bias=(0.0, 0.0, 0.0), joint_update_limits=None, use_hamiltonian_monte_carlo: bool = False):
        self.engine = engine
        self.J, self.N = engine.J, engine.N
        self.B = 0
        lim = np.full(self.J, 0.05) if joint_update_limits is None else np.ascontiguousarray(joint_update_limits,
                                                                                              np.float64)
        if lim.shape != (self.J,):
            raise ValueError(f"joint_update_limits has shape {lim.shape} for {self.J} joints")
        prm = stomp_chomp_params(C.sizeof(stomp_chomp_params), learning_rate, smoothness_cost_weight,
                                 int(use_pseudo_inverse), pseudo_inverse_ridge_factor,
                                 (C.c_double * 3)(*[float(v) for v in field_bias]), _dp(lim),
                                 int(use_hamiltonian_monte_carlo))
        h = C.c_void_p()
        _check(load_library().stomp_chomp_create(engine.h, C.byref(prm), C.byref(h)))
        self.h = h

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(f"stomp engine error {rc}: {load_library().stomp_chomp_last_error(self.h).decode()}")

    def reset(self, trajectories=None, num_trajectories: int = 1):
        """trajectories: [B][J][N] (or [J][N]: one descent); None: num_trajectories descents from the
        engine's policy parameters"""
        if trajectories is None:
            B, ptr = int(num_trajectories), None
        else:
            t = np.ascontiguousarray(trajectories, np.float64).reshape(-1, self.J, self.N)
            B, ptr = len(t), _dp(t)
        self._check(load_library().stomp_chomp_reset(self.h, B, ptr))
        self.B = B

    def step(self, count: int = 1):
        self._check(load_library().stomp_chomp_step(self.h, count))

    def synchronize(self):
        self._check(load_library().stomp_chomp_synchronize(self.h))

    def optimize(self):
        """per descent (stomp_stats, costs[:iterations], best trajectory)"""
        B = max(self.B, 1)
        stride = max(self.engine.problem.params.max_iterations, 1)
        st = (stomp_stats * B)()
        costs = np.zeros((B, stride))
        best = np.zeros((B, self.J, self.N))
        self._check(load_library().stomp_chomp_optimize(self.h, st, _dp(costs), stride, _dp(best)))
        return [(st[b], costs[b, :st[b].iterations].copy(), best[b].copy()) for b in range(self.B)]

    def get(self, name: str) -> np.ndarray:
        if name not in self.SHAPES:
            raise KeyError(name)
        info = self.info()
        dims = dict(J=self.J, N=self.N, A=self.N + 12, S=info["S"])
        shape = (self.B,) + tuple(3 if ch == "3" else dims[ch] for ch in self.SHAPES[name])
        out = np.zeros(shape)
        self._check(load_library().stomp_chomp_get(self.h, name.encode(), _dp(out)))
        return out

    def info(self) -> dict:
        v = (C.c_int64 * 8)()
        self._check(load_library().stomp_chomp_info(self.h, v))
        d = dict(zip(self.INFO, [int(x) for x in v]))
        d["S"] = self.engine.S
        return d

    def close(self):
        if getattr(self, "h", None):
            load_library().stomp_chomp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Stream:
    """A HIP stream of the engine runtime (engines of one group share one)."""

    def __init__(self, device: int = 0):
        self.ptr = None
        p = C.c_void_p()
        _check(load_library().stomp_stream_create(device, C.byref(p)))
        self.ptr = p.value

    def close(self):
        if self.ptr:
            load_library().stomp_stream_destroy(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        self.close()


class EngineGroup:
    """Engines of one shape on one shared stream, advanced in lockstep by shared launches
    (stomp_group_run: three dispatches per iteration for the whole group, four on the iterations
    that reuse rollouts).  One shape: J, N, K, num_reused_rollouts, spheres, model and field layout
    agree; at most 16 joints, no cumulative costs, no state-cost terms, one device per engine, and
    with reused rollouts at most 1023 rollouts.
    state_terms=True (stomp_group_create_with): engines with the torque term and / or orientation
    path constraints are accepted too, each with its own terms (a group may mix engines with the
    torque term, with constraints, with both and with neither); one more launch per grouped rollout
    launch prices the terms of all of them.  compact: None leaves stomp_group_optimize's compaction
    to STOMP_DEBUG_GROUP_COMPACT, False / True turn it off / on.  EngineGroup(engines) alone is
    stomp_group_create.
    cumulative_costs=True (stomp_group_create_flags): engines with use_cumulative_costs are accepted
    too, mixed freely with engines without; one more launch before every grouped weights launch
    makes the cumulative rows of all of them."""

    def __init__(self, engines, state_terms: bool = False, compact: Optional[bool] = None,
                 cumulative_costs: bool = False):
        self._h = None   # set before the call that may raise, so __del__ has nothing to free
        l = load_library()
        self.engines = list(engines)
        arr = (C.c_void_p * len(self.engines))(*[e.h.value for e in self.engines])
        h = C.c_void_p()
        if cumulative_costs:
            accept = STOMP_GROUP_ACCEPT_CUMULATIVE | (STOMP_GROUP_ACCEPT_STATE_TERMS if state_terms else 0)
            rc = l.stomp_group_create_flags(arr, len(self.engines), accept,
                                            -1 if compact is None else (1 if compact else 0), C.byref(h))
        elif state_terms or compact is not None:
            opt = stomp_group_options(C.sizeof(stomp_group_options), 1 if state_terms else 0,
                                      -1 if compact is None else (1 if compact else 0))
            rc = l.stomp_group_create_with(arr, len(self.engines), C.byref(opt), C.byref(h))
        else:
            rc = l.stomp_group_create(arr, len(self.engines), C.byref(h))
        if rc != 0:
            raise RuntimeError(f"stomp group error {rc}: {l.stomp_last_error().decode()}")
        self._h = h

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(f"stomp group error {rc}: {load_library().stomp_group_last_error(self._h).decode()}")

    def run(self, first: int, count: int):
        self._check(load_library().stomp_group_run(self._h, first, count))

    def synchronize(self):
        self._check(load_library().stomp_group_synchronize(self._h))

    @staticmethod
    def optimize_chunk() -> int:
        """Iterations per chunk of optimize() (STOMP_GROUP_OPTIMIZE_CHUNK): the host reads the
        engines' stop flags once per chunk, one chunk behind the one it enqueues."""
        return int(load_library().stomp_group_optimize_chunk())

    def optimize(self, costs_stride: Optional[int] = None):
        """StompOptimizer::optimize for every engine at once (stomp_group_optimize): the engines
        advance in lockstep through the grouped launches and each stops on its own, by its
        collision-free streak or its own max_iterations; the call returns once all have stopped
        (STOMP_DEBUG_GROUP_COMPACT=1 when the group is created: a stopped engine also leaves the
        later launches; same results).  Returns one (stomp_stats, costs[:iterations]) per engine, as Engine.optimize()
        does.  Afterwards every engine is where its own optimize() leaves it (theta, best and last
        trajectory, rollout rows, with reused rollouts also the extra rollout's rows and the row
        set of the iteration it stopped at), not gated, with nothing pending: its own iterate / run and
        group.run(first, count) with any first continue from there.  costs_stride: the row length
        of the cost histories (default: the largest max_iterations; smaller is refused)."""
        n = len(self.engines)
        if costs_stride is None:
            costs_stride = max([e.problem.params.max_iterations for e in self.engines] + [1])
        st = (stomp_stats * n)()
        costs = np.zeros((n, max(costs_stride, 1)))
        self._check(load_library().stomp_group_optimize(self._h, st, _dp(costs), costs_stride))
        return [(st[i], costs[i, : st[i].iterations].copy()) for i in range(n)]

    def retarget(self, starts, goals, seeds=None, spheres=None, orientation_constraints=None):
        """stomp_group_retarget: every engine onto its new start, goal and seed (rows of starts /
        goals, P x J; seeds None keeps every engine's seed) in one launch.  Each engine is then the
        freshly created engine of its new problem, so engines that left optimize() at different
        iterations run in lockstep again; every engine's problem attribute follows.
        spheres / orientation_constraints: per-engine lists of lists (an entry None keeps that
        engine's): stomp_group_retarget_requests, every engine's collision points and path
        constraints replaced in the same launch.  The planned engines must again be of one shape."""
        n = len(self.engines)
        J = self.engines[0].J
        s = np.ascontiguousarray(starts, np.float64).reshape(-1)
        g = np.ascontiguousarray(goals, np.float64).reshape(-1)
        if s.shape != (n * J,) or g.shape != (n * J,):
            raise ValueError(f"starts and goals must be {n} x {J}")
        if seeds is None:
            seeds = [e.problem.seed for e in self.engines]
        sd = np.array([int(v) for v in seeds], np.uint64)
        if sd.shape != (n,):
            raise ValueError(f"seeds must hold {n} values")
        sph = list(spheres) if spheres is not None else [None] * n
        ocs = list(orientation_constraints) if orientation_constraints is not None else [None] * n
        if len(sph) != n or len(ocs) != n:
            raise ValueError(f"spheres and orientation_constraints must hold {n} lists")
        rows = [(s[p * J:(p + 1) * J], g[p * J:(p + 1) * J]) for p in range(n)]   # (views: s and g outlive the call)
        reqs, keep = (stomp_request * n)(), [(None, None)] * n
        if spheres is None and orientation_constraints is None:
            self._check(load_library().stomp_group_retarget(self._h, _dp(s), _dp(g),
                                                            sd.ctypes.data_as(C.POINTER(C.c_uint64))))
        else:
            for p, e in enumerate(self.engines):
                reqs[p], keep[p] = e._request(rows[p][0], rows[p][1], int(sd[p]), sph[p], ocs[p])
            self._check(load_library().stomp_group_retarget_requests(self._h, reqs))
        for p, e in enumerate(self.engines):
            e._follow(rows[p][0], rows[p][1], int(sd[p]), sph[p], ocs[p], keep[p])

    def serve(self, starts, goals, seeds, costs_stride: Optional[int] = None):
        """stomp_group_serve: a queue of n requests (rows of starts / goals, n x J; n seeds) served
        by the group's engines as slots.  Requests are handed out in index order; a slot whose
        request has stopped takes the next waiting one at the next chunk boundary, so no slot idles
        until the slowest problem of a batch ends.  A request is a plain retarget: the model, the
        field and every parameter are the slot's own.  Returns one (slot, start_step, stomp_stats,
        costs[:iterations], best[J][N]) per request, each bit for bit what retarget + optimize() of
        the slot's engine gives; slot and start_step are serve_schedule(P, iterations)'s.
        Afterwards every used engine is where the retarget to the last request it planned and its
        own optimize() leave it, and its problem attribute follows; with n < P the engines n.. are
        untouched."""
        e0 = self.engines[0]
        J, N = e0.J, e0.N
        s = np.ascontiguousarray(starts, np.float64)
        g = np.ascontiguousarray(goals, np.float64)
        sd = np.array([int(v) for v in seeds], np.uint64)
        n = len(sd)
        if n == 0 or s.size != n * J or g.size != n * J:
            raise ValueError("starts and goals must be n x %d for n >= 1 seeds" % J)
        s, g = s.reshape(n, J), g.reshape(n, J)
        if costs_stride is None:
            costs_stride = max([e.problem.params.max_iterations for e in self.engines] + [1])
        res = (stomp_serve_result * n)()
        best = np.zeros((n, J, N))
        costs = np.zeros((n, max(costs_stride, 1)))
        self._check(load_library().stomp_group_serve(self._h, _dp(s), _dp(g), sd.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                     n, res, _dp(best), _dp(costs), costs_stride))
        for r in range(n):   # (in index order: a slot's last request is the one it keeps)
            self.engines[res[r].slot]._follow(s[r], g[r], int(sd[r]))
        return [(int(res[r].slot), int(res[r].start_step), res[r].stats, costs[r, : res[r].stats.iterations].copy(),
                 best[r].copy()) for r in range(n)]

    SERVE_INFO = ("steps", "occupied_slot_steps", "turnovers", "mixed_steps", "largest_idle_gap", "launches",
                  "result_bytes", "allocations")

    def serve_info(self) -> dict:
        """stomp_group_serve_info: the last serve() call's group steps, the requests' iterations
        summed, turnovers, steps in which two live slots ran different iteration numbers, the largest
        idle gap (steps) between a slot's stop and its next request's iteration 1, kernel launches
        enqueued, device bytes held for results and allocations made by the call."""
        info = (C.c_int64 * 8)()
        self._check(load_library().stomp_group_serve_info(self._h, info))
        return dict(zip(self.SERVE_INFO, (int(v) for v in info)))

    def close(self):
        if self._h is not None and self._h.value:
            load_library().stomp_group_destroy(self._h)
        self._h = None

    def __del__(self):
        self.close()


def serve_schedule(num_slots: int, iterations):
    """stomp_serve_schedule, host only: the (slots, start_steps, total_steps) EngineGroup.serve()
    produces for requests that run these numbers of iterations on num_slots slots."""
    it = np.ascontiguousarray(iterations, np.int32).reshape(-1)
    n = len(it)
    slot, start = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    total = C.c_int32()
    ip = C.POINTER(C.c_int32)
    _check(load_library().stomp_serve_schedule(num_slots, n, it.ctypes.data_as(ip), slot.ctypes.data_as(ip),
                                               start.ctypes.data_as(ip), C.byref(total)))
    return [int(v) for v in slot[:n]], [int(v) for v in start[:n]], int(total.value)


class DeviceBuffer:
    """Engine-runtime device allocation (keeps torch's bundled HIP runtime out of the process)."""

    def __init__(self, nbytes: int, device: int = 0):
        self.ptr = None   # set before the call that may raise, so __del__ has nothing to free
        p = C.c_void_p()
        _check(load_library().stomp_device_alloc(device, nbytes, C.byref(p)))
        self.ptr, self.nbytes = p.value, nbytes

    def to_numpy(self, dtype, shape):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        _check(load_library().stomp_device_copy_to_host(out.ctypes.data, C.c_void_p(self.ptr), out.nbytes))
        return out

    def free(self):
        if self.ptr:
            load_library().stomp_device_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        self.free()


def diff_rules() -> np.ndarray:
    """DIFF_RULES as compiled into the engine (host only)."""
    out = np.zeros((3, 7))
    _check(load_library().stomp_diff_rules(_dp(out)))
    return out


def device_count() -> int:
    n = C.c_int32()
    load_library().stomp_device_count(C.byref(n))
    return n.value


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    _check(load_library().stomp_comm_unique_id(buf))
    return buf.raw


def shard_decide(t_gather, t_partials, l_allreduce, l_allgather_state, l_allgather_partials) -> str:
    """The engine's decomposition rule on measured times (us), host only (stomp_shard_decide)."""
    m = np.array([t_gather, t_partials, l_allreduce, l_allgather_state, l_allgather_partials], np.float64)
    mode = C.c_int32()
    _check(load_library().stomp_shard_decide(_dp(m), C.byref(mode)))
    return {1: "partials", 2: "gather"}[mode.value]


def comm_local_id(world_size: int) -> bytes:
    """Id of an in-process exchange group (ranks = engines of this process, one host thread each)."""
    buf = C.create_string_buffer(128)
    _check(load_library().stomp_comm_local_id(world_size, buf))
    return buf.raw


def device_math(x: np.ndarray):
    x = np.ascontiguousarray(x, np.float64)
    n = len(x)
    outs = [np.zeros(n) for _ in range(5)]
    _check(load_library().stomp_device_selftest(_dp(x), n, *[_dp(o) for o in outs]))
    return outs


def device_trig(y: np.ndarray, x: np.ndarray):
    """(atan2(y, x), asin(y)) elementwise by the device's det_atan2 / det_asin."""
    y = np.ascontiguousarray(y, np.float64)
    x = np.ascontiguousarray(x, np.float64)
    assert y.shape == x.shape and y.ndim == 1
    a, s = np.zeros(len(y)), np.zeros(len(y))
    _check(load_library().stomp_device_selftest_trig(_dp(y), _dp(x), len(y), _dp(a), _dp(s)))
    return a, s


def device_normals(seed: int, iteration: int, joint: int, rollout: int, n: int) -> np.ndarray:
    z = np.zeros(n)
    _check(load_library().stomp_device_normals(seed, iteration, joint, rollout, n, _dp(z)))
    return z
