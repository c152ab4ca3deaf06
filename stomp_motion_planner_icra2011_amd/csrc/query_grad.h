// query_grad.h -- the gradient query's launch arguments (k_query_grad.hip, engine_query_grad.cpp)
// and the host-only part of the call: what it refuses and the tables it makes of the model
// (query_grad_host.h holds those, so that a host program can run them without a device).
#pragma once

#include "kernels.h"

namespace stomp {

constexpr int kGradQueryBlock = 64;                     // one wave per state
constexpr size_t kGradQueryLdsMax = (size_t)64 << 10;   // dynamic LDS of one workgroup

// One chunk of M states.  Every output may be null (not computed) and is in the caller's shape: a
// workgroup is one state, its lanes store along spheres, (link, joint) pairs or joints, which are
// the fastest dimensions of the caller's arrays.
struct GradQueryArgs {
    int M, L, J, S, nseg;
    double bias[3];
    const double* q;            // [M][J]
    const int* sph_seg;         // [S] the sphere's segment
    const unsigned* seg_mask;   // [nseg] joints on the path from the root to the segment, own joint included
    const int* joint_seg;       // [J] the segment joint k drives, -1: none
    const int* links;           // [L] segment indices
    double* fgrad;              // [M][S][3] without the bias
    double* pgrad;              // [M][S][3]
    double* link_cost;          // [M][L]
    double* link_grad;          // [M][L][J]
    double* cost;               // [M]
    double* grad;               // [M][J]
    uint8_t* in_col;            // [M]
};

size_t grad_query_lds(int J, int S, int nseg);
void launch_query_gradients(const DevModel& m, const GradQueryArgs& a, hipStream_t s);

}  // namespace stomp
