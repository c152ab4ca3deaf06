// k_chomp.hip -- CHOMP mode (stomp_chomp_*): the reference's covariant gradient descent,
// StompOptimizer::doChompOptimization (stomp_optimizer.cpp:208-247), for a batch of B independent
// descents on the engine's model, field and cost.  All paths below are relative to the reference's
// stomp_motion_planner/.
//
// One iteration is five launches, ordered by the stream (no grid barrier, no flags between
// workgroups):
//   k_chomp_grad    (N, B)  calculateCollisionIncrements (:413-470) from the state the last FK left
//   k_chomp_update  (J, B)  calculateSmoothnessIncrements (:403-411), calculateTotalIncrements
//                           (:472-486), addIncrementsToTrajectory (:488-506), handleJointLimits (:562-616)
//   k_chomp_fk      (N, B)  performForwardKinematics' first loop (:635-680) with the potential and
//                           its gradient (stomp_collision_space.h:193-228)
//   k_chomp_vel     (N, B)  its second loop (:683-698) and the waypoint's cost (:236-244)
//   k_chomp_track   (B)     the cost total (:233-246), the collision-free flag and, in the optimize
//                           loop, the bookkeeping of :301-347
// Every workgroup is one wave (wave64).  Everything is fp64, one rounding per operation
// (-ffp-contract=off), every sum sequential in ascending index from 0.0: lanes hold independent
// elements (spheres, joints, rows), and an ordered sum over them is made by one lane from LDS.
// A descent whose stop flag is up is skipped by every launch: its rows stay as they were.
// tests/chomp_ref.c is the CPU restatement these kernels are compared with bit for bit.
#include <algorithm>

#include "chomp.h"
#include "device_fk.h"
#include "field_gradient.h"
#include "limits_device.h"

namespace stomp {

namespace {

// the centre of sphere s at waypoint i of the whole trajectory (0 .. N + 11) of descent b: the
// padding waypoints' centres do not depend on the descent (the model's pad_pos, [12][S][3])
__device__ __forceinline__ const double* centre_at(const DevModel& m, const ChompArgs& a, int b, int i, int s)
{
    if (i < 6) return m.pad_pos + ((size_t)i * a.S + s) * 3;
    if (i >= 6 + a.N) return m.pad_pos + ((size_t)(i - a.N) * a.S + s) * 3;
    return a.pos + (((size_t)b * a.N + (i - 6)) * a.S + s) * 3;
}

}  // namespace

// LDS: the nseg segment frames, then (sin, cos) per joint
template <bool BRICK>
__global__ __launch_bounds__(kChompBlock) void k_chomp_fk(DevModel m, ChompArgs a)
{
    extern __shared__ double lds[];
    const int t = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    if (a.track[b].stop) return;
    Frame* fr = (Frame*)lds;
    double* sc = lds + (size_t)12 * a.nseg;
    for (int j = lane; j < a.J; j += kChompBlock)
        det_sincos(a.traj[((size_t)b * a.J + j) * a.N + t], &sc[2 * j], &sc[2 * j + 1]);
    __syncthreads();
    // the tree in segment order (a parent's index is below its child's), as the oracle's fk_spheres:
    // one lane, the chain is sequential
    if (lane == 0) {
        for (int s = 0; s < a.nseg; ++s) {
            const DevSegment sg = m.segs[s];
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
            fr[s] = out;
        }
    }
    __syncthreads();
    const size_t w = (size_t)b * a.N + t;
    // joint origin: the translation of the frame of the segment the joint drives (the rotation about
    // the axis leaves it where the parent frame put it); joint axis: that frame's rotation times the
    // stored axis (treefksolverjointposaxis_partial.cpp:129-138 in this build's segment convention)
    for (int k = lane; k < a.J; k += kChompBlock) {
        double o[3] = {0.0, 0.0, 0.0}, ax[3] = {0.0, 0.0, 0.0};
        const int sgi = a.joint_seg[k];
        if (sgi >= 0) {
            const Frame f = fr[sgi];
            joint_origin_axis(f, m.segs[sgi], o, ax);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            a.jorg[(w * a.J + k) * 3 + i] = o[i];
            a.jax[(w * a.J + k) * 3 + i] = ax[i];
        }
    }
    int any = 0;
    for (int s = lane; s < a.S; s += kChompBlock) {
        const DevSphere sp = m.sph[s];
        const Frame f = fr[a.sph_seg[s]];
        double p[3], fg[3], pg[3];
        apply(f.R, f.p, sp.pos, p);   // stomp_collision_point.h:138-141
        const size_t e = w * a.S + s;
        const double dist = field_gradient<BRICK>(m, p, fg);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            a.pos[3 * e + i] = p[i];
            a.fgrad[3 * e + i] = fg[i];
            fg[i] += a.bias[i];       // stomp_collision_space.h:202-204
        }
        const double pot = potential_gradient(sp, dist, fg, pg);   // stomp_collision_space.h:206-227
        const int col = dist <= sp.radius ? 1 : 0;
        any |= col;
        a.dist[e] = dist;
        a.pot[e] = pot;
#pragma unroll
        for (int i = 0; i < 3; ++i) a.pgrad[3 * e + i] = pg[i];
        a.col[e] = (uint8_t)col;
    }
    any = __syncthreads_or(any);
    if (lane == 0) a.wp_col[w] = any ? 1 : 0;
}

// LDS: potential * vel_mag per sphere
__global__ __launch_bounds__(kChompBlock) void k_chomp_vel(DevModel m, ChompArgs a)
{
    extern __shared__ double lds[];
    const int t = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    if (a.track[b].stop) return;
    const size_t w = (size_t)b * a.N + t;
    for (int s = lane; s < a.S; s += kChompBlock) {
        double v[3] = {0.0, 0.0, 0.0}, ac[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const double* p = centre_at(m, a, b, t + 6 + k - 3, s);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                v[i] += a.cv[k] * p[i];
                ac[i] += a.ca[k] * p[i];
            }
        }
        const size_t e = w * a.S + s;
        const double vm = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            a.vel[3 * e + i] = v[i];
            a.acc[3 * e + i] = ac[i];
        }
        a.vmag[e] = vm;
        lds[s] = a.pot[e] * vm;
    }
    __syncthreads();
    if (lane == 0) {   // the reference's prefix sum of prefix sums (:236-244), in sphere order
        double state = 0.0, cum = 0.0;
        for (int s = 0; s < a.S; ++s) {
            cum += lds[s];
            state += cum;
        }
        a.wcost[w] = state * a.w_obs;
    }
}

// the Jacobian column of joint k for the sphere at p (stomp_collision_point.h:120-136)
__device__ __forceinline__ void jac_column(const ChompArgs& a, size_t w, unsigned mask, int k, const double* p,
                                           double* c)
{
    jacobian_column((mask >> k) & 1u, a.jorg + (w * a.J + k) * 3, a.jax + (w * a.J + k) * 3, p, c);
}

// LDS: each sphere's term per joint [S][J], then each sphere's flags [S] (1: it has a term, 2: it collides)
__global__ __launch_bounds__(kChompBlock) void k_chomp_grad(DevModel m, ChompArgs a)
{
    extern __shared__ double lds[];
    const int t = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    if (a.track[b].stop) return;
    const int J = a.J, S = a.S;
    double* term = lds;
    int* flag = (int*)(lds + (size_t)S * J);
    const size_t w = (size_t)b * a.N + t;
    for (int s = lane; s < S; s += kChompBlock) {
        const size_t e = w * S + s;
        const double potential = a.pot[e];
        if (potential <= 1e-10) {   // :430-431
            flag[s] = 0;
            continue;
        }
        flag[s] = 1 | (a.col[e] ? 2 : 0);
        const double vel_mag = a.vmag[e];
        const double vel_mag_sq = vel_mag * vel_mag;
        double nv[3], g[3], p[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            nv[i] = a.vel[3 * e + i] / vel_mag;   // a zero vel_mag divides as IEEE says (:440)
            p[i] = a.pos[3 * e + i];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            double pa = 0.0, pgr = 0.0;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const double P = (r == q ? 1.0 : 0.0) - nv[r] * nv[q];   // :441
                pa += P * a.acc[3 * e + q];
                pgr += P * a.pgrad[3 * e + q];
            }
            const double curv = pa / vel_mag_sq;                          // :442
            g[r] = vel_mag * (pgr - potential * curv);                    // :443
        }
        const unsigned mask = a.seg_mask[a.sph_seg[s]];
        if (a.use_pinv) {
            // calculatePseudoInverse (:466-470): A = J J^T + ridge I, the inverse by cofactors over
            // the determinant, pinv = J^T A^-1, the term pinv g
            double A[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, C[9], inv[9];
            for (int k = 0; k < J; ++k) {
                double c[3];
                jac_column(a, w, mask, k, p, c);
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int q = 0; q < 3; ++q) A[3 * r + q] += c[r] * c[q];
            }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q) A[3 * r + q] = A[3 * r + q] + (r == q ? 1.0 : 0.0) * a.ridge;
            C[0] = A[4] * A[8] - A[5] * A[7];
            C[1] = A[5] * A[6] - A[3] * A[8];
            C[2] = A[3] * A[7] - A[4] * A[6];
            C[3] = A[2] * A[7] - A[1] * A[8];
            C[4] = A[0] * A[8] - A[2] * A[6];
            C[5] = A[1] * A[6] - A[0] * A[7];
            C[6] = A[1] * A[5] - A[2] * A[4];
            C[7] = A[2] * A[3] - A[0] * A[5];
            C[8] = A[0] * A[4] - A[1] * A[3];
            const double det = A[0] * C[0] + A[1] * C[1] + A[2] * C[2];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q) inv[3 * r + q] = C[3 * q + r] / det;
            for (int k = 0; k < J; ++k) {
                double c[3];
                jac_column(a, w, mask, k, p, c);
                double sum = 0.0;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    double pk = 0.0;
#pragma unroll
                    for (int r = 0; r < 3; ++r) pk += c[r] * inv[3 * r + q];
                    sum += pk * g[q];
                }
                term[(size_t)s * J + k] = sum;
            }
        } else {
            for (int k = 0; k < J; ++k) {
                double c[3];
                jac_column(a, w, mask, k, p, c);
                double sum = 0.0;
#pragma unroll
                for (int r = 0; r < 3; ++r) sum += c[r] * g[r];
                term[(size_t)s * J + k] = sum;
            }
        }
    }
    __syncthreads();
    // the row of the waypoint (:451-460): the spheres' terms subtracted in ascending order, up to and
    // including the first colliding sphere
    for (int k = lane; k < J; k += kChompBlock) {
        double row = 0.0;
        for (int s = 0; s < S; ++s) {
            const int f = flag[s];
            if (!f) continue;
            row -= term[(size_t)s * J + k];
            if (f & 2) break;
        }
        a.cinc[((size_t)b * J + k) * a.N + t] = row;
    }
}

// LDS: the joint's whole group trajectory [Nall], the weighted increments [N], the final increments [N]
__global__ __launch_bounds__(kChompBlock) void k_chomp_update(DevModel m, ChompArgs a)
{
    extern __shared__ double lds[];
    const int j = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    if (a.track[b].stop) return;
    const int N = a.N, Nall = a.Nall;
    double* x = lds;
    double* rhs = x + Nall;
    double* fin = rhs + N;
    const size_t rowo = ((size_t)b * a.J + j) * N;
    for (int i = lane; i < Nall; i += kChompBlock)
        x[i] = i < 6 ? m.start[j] : (i >= 6 + N ? m.goal[j] : a.traj[rowo + (i - 6)]);
    __syncthreads();
    // -(quad_cost_full (2 x)) over the free block (stomp_cost.h:80-83): the band's columns in
    // ascending order (outside it the matrix is exactly zero)
    const double* band = a.band + (size_t)j * Nall * 13;
    for (int t = lane; t < N; t += kChompBlock) {
        const int r = t + 6;
        double s = 0.0;
        for (int c = 0; c < 13; ++c) {
            const int col = r - 6 + c;
            if (col < 0 || col >= Nall) continue;
            s += band[(size_t)r * 13 + c] * (2.0 * x[col]);
        }
        const double si = -s;
        a.sinc[rowo + t] = si;
        rhs[t] = a.w_smooth * si + a.w_obs * a.cinc[rowo + t];   // :480-481
    }
    __syncthreads();
    // learning_rate (Qinv rhs) (:476-483): a row per lane, the row's sum sequential; QT is Qinv
    // transposed, so the lanes of a step read consecutive addresses
    const double* QT = m.QT + (size_t)j * N * N;
    for (int r = lane; r < N; r += kChompBlock) {
        double s = 0.0;
        for (int k = 0; k < N; ++k) s += QT[(size_t)k * N + r] * rhs[k];
        const double f = a.lr * s;
        fin[r] = f;
        a.finc[rowo + r] = f;
    }
    __syncthreads();
    // addIncrementsToTrajectory (:491-503); every lane takes the column's max and min itself
    double mx = fin[0], mn = fin[0];
    for (int k = 1; k < N; ++k) {
        const double f = fin[k];
        if (f > mx) mx = f;
        if (f < mn) mn = f;
    }
    double scale = 1.0;
    const double lim = a.upd[j];
    const double max_scale = lim / fabs(mx), min_scale = lim / fabs(mn);
    if (max_scale < scale) scale = max_scale;
    if (min_scale < scale) scale = min_scale;
    if (lane == 0) a.scales[(size_t)b * a.J + j] = scale;
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int t = min(lane + 64 * u, N - 1);
        v[u] = x[6 + t] + scale * fin[t];
    }
    // handleJointLimits (:562-616): at most 11 passes (limits_device.h)
    if (a.hl[j]) {
        const double jmin = a.jlim[2 * j], jmax = a.jlim[2 * j + 1];
        for (int pass = 0; pass < 11; ++pass) {
            const int cm = jl_argmax<4>(v, N, lane, jmin, jmax);
            if (cm < 0) break;
            const double* Qc = QT + (size_t)cm * N;
            double qv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) qv[u] = Qc[min(lane + 64 * u, N - 1)];
            jl_apply<4>(v, N, lane, cm, jmin, jmax, qv, Qc[cm]);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (lane + 64 * u < N) a.traj[rowo + lane + 64 * u] = v[u];
}

// reset's pass over the trajectories as given: handleJointLimits alone (:269)
__global__ __launch_bounds__(kChompBlock) void k_chomp_limits(DevModel m, ChompArgs a)
{
    const int j = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    if (!a.hl[j]) return;
    const int N = a.N;
    const size_t rowo = ((size_t)b * a.J + j) * N;
    const double* QT = m.QT + (size_t)j * N * N;
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = a.traj[rowo + min(lane + 64 * u, N - 1)];
    const double jmin = a.jlim[2 * j], jmax = a.jlim[2 * j + 1];
    for (int pass = 0; pass < 11; ++pass) {
        const int cm = jl_argmax<4>(v, N, lane, jmin, jmax);
        if (cm < 0) break;
        const double* Qc = QT + (size_t)cm * N;
        double qv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) qv[u] = Qc[min(lane + 64 * u, N - 1)];
        jl_apply<4>(v, N, lane, cm, jmin, jmax, qv, Qc[cm]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (lane + 64 * u < N) a.traj[rowo + lane + 64 * u] = v[u];
}

__global__ __launch_bounds__(kChompBlock) void k_chomp_track(DevModel m, ChompArgs a)
{
    __shared__ int copy;
    const int b = blockIdx.x, lane = threadIdx.x;
    ChompTrack* tr = a.track + b;
    if (tr->stop) return;   // uniform: every thread reads the flag before any write
    __syncthreads();
    if (lane == 0) {
        double cost = 0.0;
        int cfree = !(a.member == 0 && m.pad_collision);
        for (int t = 0; t < a.N; ++t) {
            cost += a.wcost[(size_t)b * a.N + t];
            if (a.wp_col[(size_t)b * a.N + t]) cfree = 0;
        }
        a.cost[b] = cost;
        a.cf[b] = cfree;
        copy = 0;
        if (a.it >= 0) {   // stomp_optimizer.cpp:301-347, last_trajectory_constraints_satisfied_ true (:231)
            const int it = a.it;
            tr->cfi = cfree ? tr->cfi + 1 : 0;
            if (cfree && tr->collision_success_iteration == -1) tr->collision_success_iteration = it;
            if (cfree && tr->success_iteration == -1) {
                tr->success_iteration = it;
                tr->success = 1;
            }
            a.hist[(size_t)b * a.max_it + it] = cost;
            if (it == 0 || (cost < tr->best && cfree)) {
                tr->best = cost;
                if (it != 0) tr->last_improvement_iteration = it;
                copy = 1;
            }
            tr->iterations = it + 1;
            const int stop = (tr->cfi >= a.max_it_cf || it + 1 >= a.max_it) ? 1 : 0;
            if (stop) tr->stop = 1;
            a.mirror[b] = stop;
        }
    }
    __syncthreads();
    if (copy) {
        const size_t JN = (size_t)a.J * a.N;
        for (size_t i = lane; i < JN; i += kChompBlock) a.best_traj[b * JN + i] = a.traj[b * JN + i];
    }
}

size_t chomp_fk_lds(const ChompArgs& a) { return sizeof(double) * ((size_t)12 * a.nseg + 2 * a.J); }
size_t chomp_grad_lds(const ChompArgs& a)
{
    const size_t inc = sizeof(double) * (size_t)a.S * a.J + sizeof(int) * (size_t)a.S;
    return std::max(inc, sizeof(double) * (size_t)a.S);
}
size_t chomp_update_lds(const ChompArgs& a) { return sizeof(double) * ((size_t)a.Nall + 2 * a.N); }
size_t chomp_track_lds(const ChompArgs&) { return sizeof(int); }

void launch_chomp_fk(const DevModel& m, const ChompArgs& a, hipStream_t s)
{
    const dim3 grid(a.N, a.B);
    if (m.brick) hipLaunchKernelGGL(k_chomp_fk<true>, grid, dim3(kChompBlock), chomp_fk_lds(a), s, m, a);
    else hipLaunchKernelGGL(k_chomp_fk<false>, grid, dim3(kChompBlock), chomp_fk_lds(a), s, m, a);
}

void launch_chomp_vel(const DevModel& m, const ChompArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_chomp_vel, dim3(a.N, a.B), dim3(kChompBlock), sizeof(double) * (size_t)a.S, s, m, a);
}

void launch_chomp_grad(const DevModel& m, const ChompArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_chomp_grad, dim3(a.N, a.B), dim3(kChompBlock), chomp_grad_lds(a), s, m, a);
}

void launch_chomp_update(const DevModel& m, const ChompArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_chomp_update, dim3(a.J, a.B), dim3(kChompBlock), chomp_update_lds(a), s, m, a);
}

void launch_chomp_limits(const DevModel& m, const ChompArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_chomp_limits, dim3(a.J, a.B), dim3(kChompBlock), 0, s, m, a);
}

void launch_chomp_track(const DevModel& m, const ChompArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_chomp_track, dim3(a.B), dim3(kChompBlock), 0, s, m, a);
}

}  // namespace stomp
