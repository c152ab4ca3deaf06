// query.h -- the state query's launch arguments (k_query.hip, engine_query.cpp).
#pragma once

#include "kernels.h"

namespace stomp {

// One chunk of M states.  Every output may be null (not computed).  The per-sphere and per-link
// outputs are sphere-major / link-major with M as the row length; launch_query_transpose makes the
// caller's state-major arrays of them.
struct QueryArgs {
    int M, L;
    const double* q;            // [J][M] the states, joint-major
    const int* hl;              // [J] has_limits, and [J][2] (min, max): the model image's tables
    const double* jlim;
    const int* seg_link;        // [nseg + 1] links naming segment g: link_idx[seg_link[g] .. seg_link[g + 1])
    const int* link_idx;        // [L]
    double* pos;                // [S][3][M]
    double* dist;               // [S][M]
    double* pot;                // [S][M]
    uint8_t* col;               // [S][M]
    double* link;               // [L][M], zero before the launch (a segment without spheres stays 0.0)
    double* cost;               // [M]
    double* clear;              // [M]
    int* min_s;                 // [M]
    uint8_t* in_col;            // [M]
    uint8_t* lim;               // [M]
};

void launch_query_states(const DevModel& m, const QueryArgs& a, hipStream_t s);
// out [cols][rows] = in [rows][cols] transposed
void launch_query_transpose(const double* in, double* out, int rows, int cols, hipStream_t s);
void launch_query_transpose(const uint8_t* in, uint8_t* out, int rows, int cols, hipStream_t s);

}  // namespace stomp
