// sdf_lattice.h -- the per-object lattice set-up the distance-field builders share
// (stomp_sdf_build_objects in sdf_build.cpp, the scene layers in scene.cpp): host only.
#pragma once

#include <vector>

#include "stomp_engine.h"
#include "kernels.h"

namespace stomp {

// What the marking kernels need for a list of objects: one job per object, the environment
// objects' per-axis coordinate lists and the meshes' hull planes (4 doubles each).  A mesh job's
// off[0] is its first plane's index in mesh_planes until resolve_mesh_planes names the device copy.
struct LatticeSetup {
    std::vector<double> axes;
    std::vector<double> mesh_planes;
    std::vector<SdfLatticeJob> jobs;
};

// `shapes` into `out` by the reference's rules; 0, or STOMP_E_INVALID with the message set (an
// unknown type, a degenerate mesh, a lattice too large).  Touches no device.
int lattice_setup(const stomp_shape* shapes, int n_shapes, double res, LatticeSetup& out);

// The bounding-sphere rule lattice_setup and stomp_attached_collision_points share: B, the basis
// bodies::Body::setPose makes of the quaternion (x, y, z, w); the centre and radius
// bodies::*::computeBoundingSphere gives a STOMP_BODY_* shape posed with it (false: another type,
// or a mesh without vertices).
void body_basis(const double* q, double* B);
bool body_bounding_sphere(const stomp_shape& sh, const double* B, double* centre, double* radius);

// every mesh job's planes pointed into the device copy of mesh_planes
void resolve_mesh_planes(std::vector<SdfLatticeJob>& jobs, const double* d_planes);

}  // namespace stomp
