// chomp.h -- the CHOMP path's launch arguments (k_chomp.hip, engine_chomp.cpp).
#pragma once

#include "kernels.h"

namespace stomp {

constexpr int kChompBlock = 64;    // one wave per workgroup in every CHOMP kernel
constexpr int kChompMaxN = 256;    // the update kernel holds a joint's row in 4 registers per lane

// StompOptimizer::optimize's bookkeeping of one descent (stomp_optimizer.cpp:301-344), as DevTrack
// without the clock stamps; stop also gates every launch of the descent
struct ChompTrack {
    int stop, cfi, iterations, success, success_iteration, collision_success_iteration, last_improvement_iteration;
    int pad;
    double best;
};

// Every array is [B]... with the descent first; the per-waypoint ones hold the free waypoints only
// (the padding waypoints' sphere centres are the model's pad_pos, their collisions its pad_collision).
struct ChompArgs {
    int B, J, N, Nall, S, nseg;
    int member;                 // StompOptimizer::iteration_ of this pass (0: the padding's collisions count)
    int it;                     // the bookkeeping's iteration index, -1: no bookkeeping (reset, step)
    int max_it, max_it_cf;
    int use_pinv;
    double lr, w_smooth, w_obs, ridge;
    double bias[3];
    double cv[7], ca[7];        // invTime DIFF_RULES[0][k], (invTime invTime) DIFF_RULES[1][k]
    // tables (uploaded at reset)
    const int* sph_seg;         // [S] the sphere's segment
    const unsigned* seg_mask;   // [nseg] joints on the path from the root to the segment, own joint included
    const int* joint_seg;       // [J] the segment joint k drives, -1: none
    const int* hl;              // [J] has_limits
    const double* jlim;         // [J][2] (min, max)
    const double* upd;          // [J] joint_update_limit_
    const double* band;         // [J][Nall][13] scaled quad_cost_full (SetupOutput::Qband)
    // state
    ChompTrack* track;          // [B]
    int* mirror;                // [B] the stop flags, for the host's read-back
    double* traj;               // [B][J][N]
    double *sinc, *cinc, *finc; // [B][J][N]
    double* scales;             // [B][J]
    double* pos;                // [B][N][S][3]
    double *dist, *pot, *vmag;  // [B][N][S]
    double *fgrad, *pgrad, *vel, *acc;   // [B][N][S][3]
    uint8_t* col;               // [B][N][S] point_is_in_collision_
    int* wp_col;                // [B][N] state_is_in_collision_
    double *jorg, *jax;         // [B][N][J][3]
    double* wcost;              // [B][N]
    double* cost;               // [B]
    int* cf;                    // [B]
    double* hist;               // [B][max_it]
    double* best_traj;          // [B][J][N]
};

size_t chomp_fk_lds(const ChompArgs& a);
size_t chomp_grad_lds(const ChompArgs& a);
size_t chomp_update_lds(const ChompArgs& a);
size_t chomp_track_lds(const ChompArgs& a);
// frames, joint origins and axes, sphere centres, the 7 field reads per sphere, distance, gradient,
// potential, potential gradient and the collide flags: one workgroup per (descent, free waypoint)
void launch_chomp_fk(const DevModel& m, const ChompArgs& a, hipStream_t s);
// vel, acc, vel_mag and the waypoint's cost from the centres launch_chomp_fk left
void launch_chomp_vel(const DevModel& m, const ChompArgs& a, hipStream_t s);
// the collision increments of the state the two launches above left
void launch_chomp_grad(const DevModel& m, const ChompArgs& a, hipStream_t s);
// smoothness and final increments, the scale, the add and the joint-limit passes: one workgroup
// per (descent, joint)
void launch_chomp_update(const DevModel& m, const ChompArgs& a, hipStream_t s);
// handleJointLimits alone (reset's pass over the trajectories as given)
void launch_chomp_limits(const DevModel& m, const ChompArgs& a, hipStream_t s);
// the cost total, the collision-free flag and (a.it >= 0) the loop's bookkeeping: one workgroup per descent
void launch_chomp_track(const DevModel& m, const ChompArgs& a, hipStream_t s);

}  // namespace stomp
