// k_query_grad.hip -- the gradient query (stomp_engine_query_gradients): per sphere the field
// gradient and the potential's gradient, per link and per state the collision potential and its
// gradient in joint space, -J^T g, of a batch of joint states against the engine's current model
// and field.  The reference declares the service and never built it
// (srv/GetChompCollisionCost.srv, msg/JointVelocityArray.msg: per link a cost and "the joint
// velocity that will move the link away from collisions").
//
// Mapping: one wave per state, as k_chomp_fk has one per waypoint, and the same arithmetic
// (field_gradient.h): the (sin, cos) of the joints by the lanes, the segment frames by one lane in
// segment order (the chain is sequential) into LDS, the joints' origins and axes by the lanes, then
// a lane per sphere: the centre, the seven field reads together, the potential's cases, and the
// sphere's term J^T pg per joint into LDS.  The folds are ordered sums over the spheres: a lane per
// (link, joint), per joint and per link reads the terms from LDS in ascending sphere order.  Every
// sphere takes part: CHOMP's skip of a potential <= 1e-10 and its break after the first colliding
// sphere are rules of the descent's fold (k_chomp_grad), not of this service.
// The outputs leave in the caller's shape: spheres, (link, joint) pairs and joints are the fastest
// dimensions of the caller's arrays and the dimensions the lanes store along, so nothing is
// transposed afterwards.
// Everything is fp64, one rounding per operation, every sum sequential in ascending index from 0.0.
#include "field_gradient.h"
#include "query_grad.h"

namespace stomp {

namespace {

__host__ __device__ inline int term_stride(int J) { return J | 1; }   // odd: a sphere per lane writes without bank conflicts

// LDS (doubles): the nseg frames [12], (sin, cos) per joint, (origin, axis) per joint [6], the
// potential per sphere, the terms [S][J | 1]; then (ints) the sphere's segment [S]
struct GradLds {
    size_t fr, sc, jo, pot, term, seg, total;
    __host__ __device__ GradLds(int J, int S, int nseg)
    {
        fr = 0;
        sc = fr + (size_t)12 * nseg;
        jo = sc + (size_t)2 * J;
        pot = jo + (size_t)6 * J;
        term = pot + (size_t)S;
        seg = term + (size_t)S * term_stride(J);
        total = seg * sizeof(double) + (size_t)S * sizeof(int);
    }
};

}  // namespace

template <bool BRICK>
__global__ __launch_bounds__(kGradQueryBlock) void k_query_gradients(DevModel m, GradQueryArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int i = blockIdx.x, lane = threadIdx.x;
    const int J = a.J, S = a.S, L = a.L, JP = term_stride(J);
    const GradLds at(J, S, a.nseg);
    Frame* fr = (Frame*)(lds + at.fr);
    double* sc = lds + at.sc;
    double* jo = lds + at.jo;
    double* pot = lds + at.pot;
    double* term = lds + at.term;
    int* seg = (int*)(lds + at.seg);

    for (int j = lane; j < J; j += kGradQueryBlock) det_sincos(a.q[(size_t)i * J + j], &sc[2 * j], &sc[2 * j + 1]);
    for (int s = lane; s < S; s += kGradQueryBlock) seg[s] = a.sph_seg[s];
    __syncthreads();
    if (lane == 0) {   // the tree in segment order (a parent's index is below its child's)
        for (int g = 0; g < a.nseg; ++g) {
            const DevSegment sg = m.segs[g];
            double st = 0.0, ct = 1.0;
            if (sg.q_index >= 0) {
                st = sc[2 * sg.q_index];
                ct = sc[2 * sg.q_index + 1];
            }
            Frame out;
            if (sg.parent >= 0) {
                const Frame par = fr[sg.parent];
                compose(sg, &par, st, ct, out);
            } else {
                compose(sg, nullptr, st, ct, out);
            }
            fr[g] = out;
        }
    }
    __syncthreads();
    const bool folds = a.link_grad || a.grad;
    if (folds) {
        for (int k = lane; k < J; k += kGradQueryBlock) {
            double o[3] = {0.0, 0.0, 0.0}, ax[3] = {0.0, 0.0, 0.0};   // a joint that drives no segment
            const int g = a.joint_seg[k];
            if (g >= 0) {
                const Frame f = fr[g];
                joint_origin_axis(f, m.segs[g], o, ax);
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                jo[6 * k + r] = o[r];
                jo[6 * k + 3 + r] = ax[r];
            }
        }
        __syncthreads();
    }
    int any = 0;
    for (int s = lane; s < S; s += kGradQueryBlock) {
        const DevSphere sp = m.sph[s];
        const int g = seg[s];
        const Frame f = fr[g];
        double p[3], fg[3], pg[3];
        apply(f.R, f.p, sp.pos, p);   // stomp_collision_point.h:138-141
        const double dist = field_gradient<BRICK>(m, p, fg);
        const size_t e = (size_t)i * S + s;
        if (a.fgrad) {
#pragma unroll
            for (int r = 0; r < 3; ++r) a.fgrad[3 * e + r] = fg[r];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) fg[r] += a.bias[r];   // stomp_collision_space.h:202-204
        pot[s] = potential_gradient(sp, dist, fg, pg);
        any |= dist <= sp.radius ? 1 : 0;
        if (a.pgrad) {
#pragma unroll
            for (int r = 0; r < 3; ++r) a.pgrad[3 * e + r] = pg[r];
        }
        if (folds) {
            const unsigned mask = a.seg_mask[g];
            for (int k = 0; k < J; ++k) {
                double c[3];
                jacobian_column((mask >> k) & 1u, jo + 6 * k, jo + 6 * k + 3, p, c);
                double t = 0.0;
#pragma unroll
                for (int r = 0; r < 3; ++r) t += c[r] * pg[r];
                term[(size_t)s * JP + k] = t;
            }
        }
    }
    any = __syncthreads_or(any);
    if (lane == 0 && a.in_col) a.in_col[i] = any ? 1 : 0;
    if (a.link_grad) {   // a lane per (link, joint): the terms of the link's spheres subtracted in ascending order
        for (int x = lane; x < L * J; x += kGradQueryBlock) {
            const int l = x / J, k = x - l * J, g = a.links[l];
            double acc = 0.0;
            for (int s = 0; s < S; ++s)
                if (seg[s] == g) acc -= term[(size_t)s * JP + k];
            a.link_grad[(size_t)i * L * J + x] = acc;
        }
    }
    if (a.grad) {
        for (int k = lane; k < J; k += kGradQueryBlock) {
            double acc = 0.0;
            for (int s = 0; s < S; ++s) acc -= term[(size_t)s * JP + k];
            a.grad[(size_t)i * J + k] = acc;
        }
    }
    if (a.link_cost) {
        for (int l = lane; l < L; l += kGradQueryBlock) {
            const int g = a.links[l];
            double acc = 0.0;
            for (int s = 0; s < S; ++s)
                if (seg[s] == g) acc += pot[s];
            a.link_cost[(size_t)i * L + l] = acc;
        }
    }
    if (a.cost && lane == 0) {
        double acc = 0.0;
        for (int s = 0; s < S; ++s) acc += pot[s];
        a.cost[i] = acc;
    }
}

size_t grad_query_lds(int J, int S, int nseg) { return GradLds(J, S, nseg).total; }

void launch_query_gradients(const DevModel& m, const GradQueryArgs& a, hipStream_t s)
{
    const dim3 grid(a.M);
    const size_t lds = grad_query_lds(a.J, a.S, a.nseg);
    if (m.brick) hipLaunchKernelGGL(k_query_gradients<true>, grid, dim3(kGradQueryBlock), lds, s, m, a);
    else hipLaunchKernelGGL(k_query_gradients<false>, grid, dim3(kGradQueryBlock), lds, s, m, a);
}

}  // namespace stomp
