// query_grad_host.h -- the host-only part of stomp_engine_query_gradients: what the call refuses
// about its request and the tables it makes of the model.  No device type and no HIP header is
// needed here (the segment and FK-step types are template parameters), so a host program can run
// these functions on their own (tests/gradient_query_host_check.cpp, under the sanitizers).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdio>

#include "stomp_engine.h"

namespace stomp {

// Everything the call refuses about request q for a tree of J joints and nseg segments (q and
// q->states are not null, struct_size is right).  0: accepted; otherwise STOMP_E_INVALID with the
// reason in why[n].  Reads the request's input arrays only.
inline int grad_query_check(const stomp_gradient_query* q, int J, int nseg, char* why, size_t n)
{
    if (q->num_states < 1) {
        std::snprintf(why, n, "gradient query: num_states %d is below 1", q->num_states);
        return STOMP_E_INVALID;
    }
    if (q->num_links < 0) {
        std::snprintf(why, n, "gradient query: num_links %d is negative", q->num_links);
        return STOMP_E_INVALID;
    }
    if (q->num_links >= 1 && !q->links) {
        std::snprintf(why, n, "gradient query: %d links and no link array", q->num_links);
        return STOMP_E_INVALID;
    }
    if ((q->link_costs || q->link_gradients) && q->num_links == 0) {
        std::snprintf(why, n, "gradient query: %s without links", q->link_costs ? "link_costs" : "link_gradients");
        return STOMP_E_INVALID;
    }
    for (int l = 0; l < q->num_links; ++l)
        if (q->links[l] < 0 || q->links[l] >= nseg) {
            std::snprintf(why, n, "gradient query: link %d names segment %d, the tree has %d", l, q->links[l], nseg);
            return STOMP_E_INVALID;
        }
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(q->field_bias[k])) {
            std::snprintf(why, n, "gradient query: field_bias[%d] is not finite", k);
            return STOMP_E_INVALID;
        }
    const size_t count = (size_t)q->num_states * (size_t)J;
    for (size_t i = 0; i < count; ++i)
        if (!std::isfinite(q->states[i])) {
            std::snprintf(why, n, "gradient query: state %zu, joint %zu is not finite", i / J, i % J);
            return STOMP_E_INVALID;
        }
    return 0;
}

// sph_seg[s]: the segment of sphere s, from the FK program (a step with seg < 0 emits more spheres
// of the segment before it)
template <class Op>
void grad_query_sphere_segments(const Op* ops, int nops, int* sph_seg)
{
    int cur = -1;
    for (int i = 0; i < nops; ++i) {
        if (ops[i].seg >= 0) cur = ops[i].seg;
        for (int s = ops[i].sph_begin; s < ops[i].sph_end; ++s) sph_seg[s] = cur;
    }
}

// mask[g]: the joints on the path from the root to segment g, its own joint included (a parent's
// index is below its child's); joint_seg[k]: the first segment joint k drives, -1: none
template <class Seg>
void grad_query_joint_paths(const Seg* segs, int nseg, int J, unsigned* mask, int* joint_seg)
{
    for (int k = 0; k < J; ++k) joint_seg[k] = -1;
    for (int g = 0; g < nseg; ++g) {
        unsigned m = segs[g].parent >= 0 ? mask[segs[g].parent] : 0u;
        if (segs[g].q_index >= 0) {
            m |= 1u << segs[g].q_index;
            if (joint_seg[segs[g].q_index] < 0) joint_seg[segs[g].q_index] = g;
        }
        mask[g] = m;
    }
}

}  // namespace stomp
