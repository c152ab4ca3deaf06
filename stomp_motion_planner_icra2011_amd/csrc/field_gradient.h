// field_gradient.h -- the field gradient and the potential's gradient, shared by CHOMP mode
// (k_chomp.hip) and the gradient query (k_query_grad.hip): one arithmetic, two kernels.
#pragma once

#include "device_fk.h"

namespace stomp {

// the voxel (ix, iy, iz) in the layout of the field (sdf_cell's two index rules)
template <bool BRICK>
__device__ __forceinline__ unsigned voxel_index(const DevModel& m, int ix, int iy, int iz)
{
    if constexpr (BRICK) {
        const unsigned b = (((unsigned)ix >> 2) * (unsigned)m.nby + ((unsigned)iy >> 2)) * (unsigned)m.nbz +
                           ((unsigned)iz >> 2);
        return (b << 6) | (((unsigned)ix & 3u) << 4) | (((unsigned)iy & 3u) << 2) | ((unsigned)iz & 3u);
    } else {
        return ((unsigned)ix * (unsigned)m.ny + (unsigned)iy) * (unsigned)m.nz + (unsigned)iz;
    }
}

// distance_field getDistanceGradient (third party; the definition is in stomp_engine.h and
// DESIGN.md): the distance at the nearest cell and the central differences of sqrt(d2) res over
// its six neighbours; a centre whose cell is outside [1, n - 2] on an axis reads 0 and (0, 0, 0).
// The cell rule is sdf_cell's.  The seven loads go out together; a lane outside reads cell 0.
template <bool BRICK>
__device__ __forceinline__ double field_gradient(const DevModel& m, const double* p, double* g)
{
    const int ix = (int)((p[0] - m.ox) * m.inv_res + 0.5);
    const int iy = (int)((p[1] - m.oy) * m.inv_res + 0.5);
    const int iz = (int)((p[2] - m.oz) * m.inv_res + 0.5);
    const bool ok = ix >= 1 && iy >= 1 && iz >= 1 && ix <= m.nx - 2 && iy <= m.ny - 2 && iz <= m.nz - 2;
    const int cx = ok ? ix : 1, cy = ok ? iy : 1, cz = ok ? iz : 1;   // (a grid has at least 3 cells per axis)
    const unsigned c = m.sdf[voxel_index<BRICK>(m, cx, cy, cz)];
    const unsigned xp = m.sdf[voxel_index<BRICK>(m, cx + 1, cy, cz)], xm = m.sdf[voxel_index<BRICK>(m, cx - 1, cy, cz)];
    const unsigned yp = m.sdf[voxel_index<BRICK>(m, cx, cy + 1, cz)], ym = m.sdf[voxel_index<BRICK>(m, cx, cy - 1, cz)];
    const unsigned zp = m.sdf[voxel_index<BRICK>(m, cx, cy, cz + 1)], zm = m.sdf[voxel_index<BRICK>(m, cx, cy, cz - 1)];
    const double inv_twice = 1.0 / (2.0 * m.res);
    const double gx = (sdf_metres(m, xp) - sdf_metres(m, xm)) * inv_twice;
    const double gy = (sdf_metres(m, yp) - sdf_metres(m, ym)) * inv_twice;
    const double gz = (sdf_metres(m, zp) - sdf_metres(m, zm)) * inv_twice;
    g[0] = ok ? gx : 0.0;
    g[1] = ok ? gy : 0.0;
    g[2] = ok ? gz : 0.0;
    return ok ? sdf_metres(m, c) : 0.0;
}

// getCollisionPointPotentialGradient (stomp_collision_space.h:206-227): the potential of the field
// distance `dist` and its gradient pg from the biased field gradient fgb
__device__ __forceinline__ double potential_gradient(const DevSphere& sp, double dist, const double* fgb, double* pg)
{
    const double d = dist - sp.radius;
    double pot;
    if (d >= sp.clearance) {
        pot = 0.0;
        pg[0] = pg[1] = pg[2] = 0.0;
    } else if (d >= 0.0) {
        const double diff = d - sp.clearance;
        const double gm = diff * sp.inv_clearance;
        pot = 0.5 * gm * diff;
#pragma unroll
        for (int i = 0; i < 3; ++i) pg[i] = gm * fgb[i];
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) pg[i] = fgb[i];
        pot = -d + 0.5 * sp.clearance;
    }
    return pot;
}

// the Jacobian column of a joint with world-frame origin o and axis ax for the sphere at p
// (stomp_collision_point.h:120-136); on: the joint is on the path from the root to the sphere's segment
__device__ __forceinline__ void jacobian_column(bool on, const double* o, const double* ax, const double* p, double* c)
{
    if (!on) {
        c[0] = c[1] = c[2] = 0.0;
        return;
    }
    const double d0 = p[0] - o[0], d1 = p[1] - o[1], d2 = p[2] - o[2];
    c[0] = ax[1] * d2 - ax[2] * d1;
    c[1] = ax[2] * d0 - ax[0] * d2;
    c[2] = ax[0] * d1 - ax[1] * d0;
}

// a joint's world-frame origin and axis from the frame of the segment it drives
// (treefksolverjointposaxis_partial.cpp:129-138 in this build's segment convention): the frame's
// translation, and its rotation times the stored axis
__device__ __forceinline__ void joint_origin_axis(const Frame& f, const DevSegment& sg, double* o, double* ax)
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[i] = f.p[i];
        ax[i] = f.R[3 * i + 0] * sg.axis[0] + f.R[3 * i + 1] * sg.axis[1] + f.R[3 * i + 2] * sg.axis[2];
    }
}

}  // namespace stomp
