// k_query.hip -- the state query (stomp_engine_query_states): per-sphere clearance and per-link
// costs of a batch of joint states against the engine's current model and field.
//
// The reference declares this capability and never built it (srv/GetStateCost.srv: link names and a
// robot state in, per-link costs out; srv/GetChompCollisionCost.srv: per-link costs and
// in_collision).  What it returns here is what the planner's own cost is made of: the collision
// points' positions (treefksolverjointposaxis_partial.cpp:108-140), the field distance at each
// (stomp_collision_space.h:190), the potential (stomp_collision_space.h:193-228) and the collision
// test, for a robot standing still -- no velocity factor, no joint-limit clipping.
// No gradient: getDistanceGradient's gradient lives in the third-party distance_field package,
// which is not in the reference tree; the reference uses it on the CHOMP path only (out of scope,
// DESIGN.md section 9), and its semantics cannot be pinned from anything the oracle checks.
//
// Mapping: one lane per state (as the rollout kernel has one lane per waypoint), 64-lane
// workgroups.  The FK program, the segment and the sphere tables are wave-uniform; they are read
// from the engine's HBM image through the scalar cache (constant address space, as the lean rollout
// layout reads them): a few KB that every wave of the launch reads alike, no LDS copy, no barrier.
// The running frame and the two saved branch-point frames are per-lane registers.  The arithmetic
// is pad_fk_side_tab's (k_misc.hip), operation for operation.  A run's lookups (up to kQueryBatch
// spheres) go out together; the sums are taken afterwards in ascending sphere order.
// The states come joint-major ([J][M], lanes read consecutive addresses) and the per-sphere outputs
// leave sphere-major ([S][M], lanes store consecutive addresses); k_query_transpose turns them into
// the caller's [M][S] on the device before the copy-out.
#include "device_fk.h"
#include "query.h"

namespace stomp {

namespace {

constexpr int kQueryBlock = 64;
constexpr int kQueryBatch = 8;    // lookups in flight per lane

using CSegment = const __attribute__((address_space(4))) DevSegment;
using COp = const __attribute__((address_space(4))) FkOp;
using CSphere = const __attribute__((address_space(4))) DevSphere;
using CInt = const __attribute__((address_space(4))) int;
using CDouble = const __attribute__((address_space(4))) double;

__device__ __forceinline__ DevSegment load_seg(CSegment* p)
{
    DevSegment r;
    r.parent = p->parent;
    r.q_index = p->q_index;
    r.rot_identity = p->rot_identity;
    r.pad_ = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) r.rot[k] = p->rot[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.trans[k] = p->trans[k];
        r.axis[k] = p->axis[k];
    }
    return r;
}

__device__ __forceinline__ FkOp load_op(COp* p)
{
    FkOp r;
    r.seg = p->seg;
    r.base = p->base;
    r.save = p->save;
    r.sph_begin = p->sph_begin;
    r.sph_end = p->sph_end;
    r.slot = p->slot;
    return r;
}

__device__ __forceinline__ DevSphere load_sph(CSphere* p)
{
    DevSphere r;
    r.slot = p->slot;
    r.zero_lim = p->zero_lim;
    r.col_lim = p->col_lim;
    r.pad_ = 0;
    r.radius = p->radius;
    r.clearance = p->clearance;
    r.inv_clearance = p->inv_clearance;
#pragma unroll
    for (int k = 0; k < 3; ++k) r.pos[k] = p->pos[k];
    return r;
}

}  // namespace

// One lane per state of the chunk.  A lane past the chunk computes state M - 1 again and stores
// nothing, so every branch below is wave-uniform.
template <bool BRICK>
__global__ __launch_bounds__(kQueryBlock) void k_query_states(DevModel m, QueryArgs a)
{
    const int i = blockIdx.x * kQueryBlock + threadIdx.x;
    const bool live = i < a.M;
    const int c = live ? i : a.M - 1;
    const size_t ld = (size_t)a.M;

    if (a.lim) {   // any joint with limits outside [min, max]; the state is not clipped
        CInt* hl = (CInt*)a.hl;
        CDouble* jl = (CDouble*)a.jlim;
        bool bad = false;
        for (int j = 0; j < m.J; ++j) {
            if (!hl[j]) continue;
            const double x = a.q[(size_t)j * ld + c];
            if (!(jl[2 * j] <= x && x <= jl[2 * j + 1])) bad = true;
        }
        if (live) a.lim[i] = bad ? 1 : 0;
    }
    const bool sums = a.dist || a.pot || a.link || a.cost || a.clear || a.min_s;
    const bool looks = sums || a.col || a.in_col;
    if (!looks && !a.pos) return;

    COp* cops = (COp*)m.ops;
    CSegment* cseg = (CSegment*)m.segs;
    CSphere* csph = (CSphere*)m.sph;
    CInt* seg_link = (CInt*)a.seg_link;
    CInt* link_idx = (CInt*)a.link_idx;

    Frame C{}, S0{}, S1{};
    double cost = 0.0, seg_sum = 0.0, clear = __builtin_inf();
    int min_s = -1, cur_seg = -1;
    bool any = false;
    // the finished segment's sum into every listed link that names it
    auto close_segment = [&]() {
        if (!a.link || cur_seg < 0 || !live) return;
        for (int k = seg_link[cur_seg]; k < seg_link[cur_seg + 1]; ++k) a.link[(size_t)link_idx[k] * ld + i] = seg_sum;
    };
    for (int op = 0; op < m.nops; ++op) {
        const FkOp o = load_op(cops + op);
        if (o.seg >= 0) {
            close_segment();
            cur_seg = o.seg;
            seg_sum = 0.0;
            const DevSegment sg = load_seg(cseg + o.seg);
            double st = 0.0, ct = 1.0;
            if (sg.q_index >= 0) det_sincos(a.q[(size_t)sg.q_index * ld + c], &st, &ct);
            fk_op(sg, o.base, o.save, st, ct, C, S0, S1);
        }
        for (int s0 = o.sph_begin; s0 < o.sph_end; s0 += kQueryBatch) {
            unsigned d2[kQueryBatch];
#pragma unroll
            for (int u = 0; u < kQueryBatch; ++u) {
                d2[u] = 0u;
                const int s = s0 + u;
                if (s >= o.sph_end) continue;
                const DevSphere sp = load_sph(csph + s);
                double p[3];
                apply(C.R, C.p, sp.pos, p);
                if (a.pos && live) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) a.pos[(size_t)(3 * s + k) * ld + i] = p[k];
                }
                if (looks) d2[u] = sdf_d2<BRICK>(m, p);
            }
            if (!looks) continue;
#pragma unroll
            for (int u = 0; u < kQueryBatch; ++u) {
                const int s = s0 + u;
                if (s >= o.sph_end) continue;
                const DevSphere sp = load_sph(csph + s);
                const bool col = (int)d2[u] < sp.col_lim;   // distance <= radius
                any = any || col;
                if (a.col && live) a.col[(size_t)s * ld + i] = col ? 1 : 0;
                if (!sums) continue;
                const double dist = sdf_metres(m, d2[u]);
                const double pt = potential(sp, dist);
                cost += pt;
                seg_sum += pt;
                const double cl = dist - sp.radius;
                if (cl < clear) {
                    clear = cl;
                    min_s = s;
                }
                if (live) {
                    if (a.dist) a.dist[(size_t)s * ld + i] = dist;
                    if (a.pot) a.pot[(size_t)s * ld + i] = pt;
                }
            }
        }
    }
    close_segment();
    if (!live) return;
    if (a.cost) a.cost[i] = cost;
    if (a.clear) a.clear[i] = clear;
    if (a.min_s) a.min_s[i] = min_s;
    if (a.in_col) a.in_col[i] = any ? 1 : 0;
}

// out[c][r] = in[r][c] for in [rows][cols]: 32 x 32 tiles through LDS (one padding column, so the
// column reads do not share a bank), loads and stores both along consecutive addresses
template <class T>
__global__ __launch_bounds__(256) void k_query_transpose(const T* __restrict__ in, T* __restrict__ out, int rows, int cols)
{
    __shared__ T tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int k = ty; k < 32; k += 8) {
        const int r = r0 + k, c = c0 + tx;
        if (r < rows && c < cols) tile[k][tx] = in[(size_t)r * cols + c];
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k, r = r0 + tx;
        if (r < rows && c < cols) out[(size_t)c * rows + r] = tile[tx][k];
    }
}

void launch_query_states(const DevModel& m, const QueryArgs& a, hipStream_t s)
{
    const dim3 grid((a.M + kQueryBlock - 1) / kQueryBlock);
    if (m.brick) hipLaunchKernelGGL(k_query_states<true>, grid, dim3(kQueryBlock), 0, s, m, a);
    else hipLaunchKernelGGL(k_query_states<false>, grid, dim3(kQueryBlock), 0, s, m, a);
}

void launch_query_transpose(const double* in, double* out, int rows, int cols, hipStream_t s)
{
    if (rows <= 0 || cols <= 0) return;
    hipLaunchKernelGGL(k_query_transpose<double>, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0, s, in, out,
                       rows, cols);
}

void launch_query_transpose(const uint8_t* in, uint8_t* out, int rows, int cols, hipStream_t s)
{
    if (rows <= 0 || cols <= 0) return;
    hipLaunchKernelGGL(k_query_transpose<uint8_t>, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0, s, in, out,
                       rows, cols);
}

}  // namespace stomp
