// engine_create.cpp -- stomp_engine_create: the descriptor's validation and the stages that build
// an engine from it, in the order their device work is enqueued (each returns a status code; the
// engine under construction is released by its owner when one fails).
#include "engine_internal.h"

#include <algorithm>
#include <cstdlib>

using namespace stomp;

namespace {

// The hinge potential's zero case and the collision test of StompCollisionSpace::
// getCollisionPointPotentialGradient (stomp_collision_space.h:193-228) as thresholds on a voxel's
// squared cell distance d2, whose distance is sqrt((double)d2) * res (the field's sqrt_table_):
//   potential == 0  <=>  d2 >= zero_lim      in collision  <=>  d2 < col_lim
// A d2 is priced with the reference's expressions (one rounding per operation, as the kernel's).
// Each predicate switches at most once over the d2 a 16-bit voxel can hold: sqrt, the product with
// a positive res and the difference with radius are each monotone under rounding to nearest, so
// dist and dist - radius never decrease with d2.  The first d2 at which a predicate holds is
// therefore found by bisection (a request re-plans every sphere on the host: 17 evaluations per
// threshold instead of 65536), and the kernel's integer compares give the same answers as the
// potential itself.
template <class Pred>
int first_d2(Pred pred)   // the first d2 in [0, 65535] with pred(d2), or 65536
{
    int lo = 0, hi = 65536;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (pred(mid)) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

bool sphere_thresholds(double radius, double clearance, double res, int* zero_lim, int* col_lim)
{
    if (!(radius >= 0.0 && clearance > 0.0 && std::isfinite(radius) && std::isfinite(clearance))) return false;
    *zero_lim = first_d2([&](int d2) { return std::sqrt((double)d2) * res - radius >= clearance; });
    *col_lim = first_d2([&](int d2) { return !(std::sqrt((double)d2) * res <= radius); });
    return true;
}

// FK program: frames of the segments that carry spheres or are their ancestors, in
// DFS order, each composed from its parent's live slot; sphere runs emitted in list
// order right after their segment's frame (requires sphere segments non-decreasing).
int plan_fk(stomp_engine* e, const std::vector<DevSegment>& segs, int N, const stomp_sphere* spheres, int S,
            ModelTables& t)
{
    const int ns = (int)segs.size();
    std::vector<FkOp>& ops = t.ops;
    ops.clear();
    t.nslots = 0;
    t.sphere_slot.assign(std::max(S, 1), 0);
    std::vector<char> needed(ns, 0);
    int prev = -1;
    for (int j = 0; j < S; ++j) {
        int s = spheres[j].segment;
        if (s < prev)
            return fail(e, STOMP_E_UNSUPPORTED,
                        "sphere list must be ordered by segment (sphere %d on segment %d after segment %d)", j, s, prev);
        prev = s;
        for (int a = s; a >= 0 && !needed[a]; a = segs[a].parent) needed[a] = 1;
    }
    // DFS order: the next needed segment after s is its first needed child, so a chain
    // continues from the running frame C; a segment with several needed children is saved
    // and its later children start from the saved copy.
    std::vector<int> remaining(ns, 0), slot_of(ns, -1);
    for (int s = 0; s < ns; ++s)
        if (needed[s] && segs[s].parent >= 0) remaining[segs[s].parent]++;
    bool used[kSaves] = {false, false};
    const int runmax = run_max(N);
    int sph = 0, cur = -1;
    for (int s = 0; s < ns; ++s) {
        if (!needed[s]) continue;
        const int p = segs[s].parent;
        int base;
        if (p < 0) base = kBaseRoot;
        else if (p == cur) base = kBaseChain;
        else if (slot_of[p] >= 0) base = slot_of[p];
        else return fail(e, STOMP_E_UNSUPPORTED, "FK planner: parent frame of segment %d not available", s);
        if (p >= 0 && --remaining[p] == 0 && slot_of[p] >= 0) {
            used[slot_of[p]] = false;   // read by this step before any save below overwrites it
            slot_of[p] = -1;
        }
        int save = -1;
        if (remaining[s] >= 2) {
            for (int k = 0; k < kSaves; ++k)
                if (!used[k]) { used[k] = true; save = k; break; }
            if (save < 0) return fail(e, STOMP_E_UNSUPPORTED, "kinematic tree needs more than %d saved frames", kSaves);
            slot_of[s] = save;
        }
        cur = s;
        int b = sph;
        while (sph < S && spheres[sph].segment == s) ++sph;
        const int slot = sph > b ? t.nslots++ : -1;
        for (int j = b; j < sph; ++j) t.sphere_slot[j] = slot;
        bool first = true;
        for (int a = b; a < sph || first; a += runmax) {
            FkOp o;
            o.seg = first ? s : -1;
            o.base = first ? base : kBaseChain;
            o.save = first ? save : -1;
            o.slot = first ? slot : -1;
            o.sph_begin = std::min(a, sph);
            o.sph_end = std::min(a + runmax, sph);
            ops.push_back(o);
            first = false;
        }
    }
    return 0;
}

// the torque term's chain (stomp_robot_model.cpp:185-189): segments below torque_root up to
// torque_tip, root side first; its joints must be the group's joints in order.  Returns an
// error message, or nullptr.
const char* torque_chain(const stomp_engine_desc* d, std::vector<int>& path)
{
    path.clear();
    if (!d->inertias) return "torque term needs segment inertias";
    if (d->torque_root < 0 || d->torque_root >= d->num_segments || d->torque_tip < 0 ||
        d->torque_tip >= d->num_segments)
        return "torque chain root/tip out of range";
    for (int sgi = d->torque_tip; sgi != d->torque_root; sgi = d->segments[sgi].parent) {
        if (sgi < 0 || (int)path.size() == kMaxChain) return "torque tip is not below the torque root (or chain too long)";
        path.push_back(sgi);
    }
    std::reverse(path.begin(), path.end());
    int nj = 0;
    for (int sgi : path)
        if (d->segments[sgi].q_index >= 0 && d->segments[sgi].q_index != nj++) return "torque chain joints must be the group joints in order";
    if (nj != d->num_joints) return "torque chain joints must be the group joints in order";
    return nullptr;
}

// OrientationConstraintEvaluator ctor (constraint_evaluator.cpp:50-73): tf::quaternionMsgToTF
// (normalises when |q|^2 is off by more than 0.1), btMatrix3x3(btQuaternion), inverse()
// (bullet LinearMath, double precision), restated as in the oracle
void oc_nominal_inverse(const double* q, double* O)
{
    double x = q[0], y = q[1], z = q[2], w = q[3];
    const double l2 = x * x + y * y + z * z + w * w;
    if (std::fabs(l2 - 1.0) > 0.1f) {
        const double inv = 1.0 / std::sqrt(l2);
        x *= inv; y *= inv; z *= inv; w *= inv;
    }
    const double d = x * x + y * y + z * z + w * w;
    const double s = 2.0 / d;
    const double xs = x * s, ys = y * s, zs = z * s;
    const double wx = w * xs, wy = w * ys, wz = w * zs;
    const double xx = x * xs, xy = x * ys, xz = x * zs;
    const double yy = y * ys, yz = y * zs, zz = z * zs;
    const double M[9] = {1.0 - (yy + zz), xy - wz, xz + wy, xy + wz, 1.0 - (xx + zz), yz - wx,
                         xz - wy, yz + wx, 1.0 - (xx + yy)};
    auto cof = [&](int r1, int c1, int r2, int c2) { return M[3 * r1 + c1] * M[3 * r2 + c2] - M[3 * r1 + c2] * M[3 * r2 + c1]; };
    const double co0 = cof(1, 1, 2, 2), co1 = cof(1, 2, 2, 0), co2 = cof(1, 0, 2, 1);
    const double det = M[0] * co0 + M[1] * co1 + M[2] * co2;
    const double sc = 1.0 / det;
    O[0] = co0 * sc; O[1] = cof(0, 2, 2, 1) * sc; O[2] = cof(0, 1, 1, 2) * sc;
    O[3] = co1 * sc; O[4] = cof(0, 0, 2, 2) * sc; O[5] = cof(0, 2, 1, 0) * sc;
    O[6] = co2 * sc; O[7] = cof(0, 1, 2, 0) * sc; O[8] = cof(0, 0, 1, 1) * sc;
}

}  // namespace

// The stages that depend on the collision points and the path constraints.  Creation runs them on
// the engine under construction and stomp_engine_retarget_request on a live one (e: the engine
// whose scalars, kinematic tree and joint limits they read; err: where a refusal's message goes,
// null on a live engine, which must stay as it was).  None of them touches a device.
namespace stomp {

int validate_spheres(const stomp_sphere* spheres, int n, int num_segments, double resolution)
{
    for (int j = 0; j < n; ++j) {
        if (spheres[j].segment < 0 || spheres[j].segment >= num_segments)
            return fail(nullptr, STOMP_E_INVALID, "sphere %d: bad segment", j);
        int zl, cl;
        if (!sphere_thresholds(spheres[j].radius, spheres[j].clearance, resolution, &zl, &cl))
            return fail(nullptr, STOMP_E_INVALID, "sphere %d: radius / clearance not finite and positive", j);
    }
    return 0;
}

int validate_constraints(const stomp_orientation_constraint* oc, int n, int num_segments)
{
    if (n < 0 || (n > 0 && !oc)) return fail(nullptr, STOMP_E_INVALID, "invalid orientation constraints");
    for (int c = 0; c < n; ++c)
        if (oc[c].segment < 0 || oc[c].segment >= num_segments)
            return fail(nullptr, STOMP_E_INVALID, "orientation constraint %d: bad segment", c);
    return 0;
}

// the FK program, the spheres as the kernels hold them, each published frame slot's first sphere
int plan_model_tables(stomp_engine* err, const stomp_engine* e, const stomp_sphere* spheres, int S, ModelTables& t)
{
    t.S = S;
    if (int rc = plan_fk(err, e->h_segs, e->N, spheres, S, t)) return rc;
    t.sph.assign(std::max(S, 1), DevSphere{});
    for (int j = 0; j < S; ++j) {
        const stomp_sphere& g = spheres[j];
        DevSphere& o = t.sph[j];
        o.slot = t.sphere_slot[j];
        o.radius = g.radius; o.clearance = g.clearance;
        o.inv_clearance = 1.0 / g.clearance;   // stomp_collision_point.cpp:50
        std::memcpy(o.pos, g.pos, sizeof g.pos);
        sphere_thresholds(g.radius, g.clearance, e->model.res, &o.zero_lim, &o.col_lim);
        o.pad_ = 0;
    }
    // slots are numbered in sphere order, so each slot owns a contiguous sphere range
    t.slot_sph.assign(t.nslots + 1, S);
    for (int j = S - 1; j >= 0; --j) t.slot_sph[t.sphere_slot[j]] = j;
    return 0;
}

// the path constraints (OrientationConstraintEvaluator) as k_terms holds them
int plan_constraints(stomp_engine* err, const stomp_engine* e, const stomp_orientation_constraint* ocs, int n,
                     std::vector<OcDev>& oc)
{
    oc.assign(std::max(n, 0), OcDev{});
    for (int c = 0; c < n; ++c) {
        const stomp_orientation_constraint& in = ocs[c];
        OcDev& o = oc[c];
        std::vector<int> path;
        for (int sgi = in.segment; sgi >= 0; sgi = e->h_segs[sgi].parent) path.push_back(sgi);
        if ((int)path.size() > kMaxChain)
            return fail(err, STOMP_E_UNSUPPORTED, "constraint segment deeper than %d", kMaxChain);
        std::reverse(path.begin(), path.end());
        o.seg = in.segment; o.body_fixed = in.body_fixed ? 1 : 0; o.path_len = (int)path.size();
        for (size_t k = 0; k < path.size(); ++k) o.path[k] = path[k];
        oc_nominal_inverse(in.orientation, o.ninv);
        o.tol[0] = in.absolute_roll_tolerance; o.tol[1] = in.absolute_pitch_tolerance;
        o.tol[2] = in.absolute_yaw_tolerance; o.weight = in.weight;
        o.rw = o.pw = o.yw = 1.0;   // constraint_evaluator.cpp:66-72
        if (o.tol[1] >= M_PI) o.pw = 0.0;
        if (o.tol[0] >= M_PI) o.rw = 0.0;
        if (o.tol[2] >= M_PI) o.yw = 0.0;
    }
    return 0;
}

// what every terms model holds besides its chain and its constraints; the kernel's LDS limit for
// an engine whose terms run (terms_on)
int plan_terms(stomp_engine* err, const stomp_engine* e, TermsModel& t, bool terms_on)
{
    t.J = e->J; t.N = e->N;
    const double invTime = 1.0 / e->disc, invTime2 = 1.0 / (e->disc * e->disc);   // stomp_trajectory.h:289, 301
    for (int k = 0; k < 7; ++k) {
        t.cv[k] = invTime * kDiffRules[0][k];
        t.ca[k] = invTime2 * kDiffRules[1][k];
    }
    t.start = e->d_start; t.goal = e->d_goal;
    t.w_con = e->w_con; t.w_tq = e->w_tq;
    if (terms_on && terms_lds_bytes(t) > 160 * 1024)
        return fail(err, STOMP_E_UNSUPPORTED, "state-terms kernel needs %zu B of LDS", terms_lds_bytes(t));
    return 0;
}

// the rollout kernel's LDS table image for a model (RolloutLds from .sph on, padding positions last)
RolloutLds model_image_layout(const stomp_engine* e, const DevModel& m)
{
    return rollout_lds(e->J, e->N, m.S, m.sph_chunk, m.nsaves, m.nseg, m.nops, m.nslots, 1);
}

size_t model_image_bytes(const stomp_engine* e, const DevModel& m)
{
    const RolloutLds L = model_image_layout(e, m);
    return L.total - L.sph;
}

// the image's tables (everything before the padding positions), [0, L.pad - L.sph)
std::vector<unsigned char> build_model_image(const stomp_engine* e, const ModelTables& t, const DevModel& m)
{
    const int J = e->J;
    const RolloutLds L = model_image_layout(e, m);
    std::vector<unsigned char> img(L.pad - L.sph, 0);
    auto put = [&](size_t off, const void* src, size_t bytes) {
        if (bytes) std::memcpy(img.data() + (off - L.sph), src, bytes);
    };
    std::vector<double> jlim(2 * (size_t)J);
    for (int j = 0; j < J; ++j) { jlim[2 * j] = e->h_jmin[j]; jlim[2 * j + 1] = e->h_jmax[j]; }
    put(L.sph, t.sph.data(), sizeof(DevSphere) * t.S);
    put(L.seg, e->h_segs.data(), sizeof(DevSegment) * e->h_segs.size());
    put(L.ops, t.ops.data(), sizeof(FkOp) * t.ops.size());
    put(L.slot, t.slot_sph.data(), sizeof(int) * t.slot_sph.size());
    put(L.hl, e->h_has_lim.data(), sizeof(int) * J);
    put(L.jlim, jlim.data(), sizeof(double) * jlim.size());
    return img;
}

// the model's pointers into its image at d_img (every one of them moves with S)
void point_model_into_image(const stomp_engine* e, DevModel& m, unsigned long long* d_img)
{
    const RolloutLds L = model_image_layout(e, m);
    const unsigned char* base = (const unsigned char*)d_img;
    m.img = d_img;
    m.img_words = (int)(((m.pad_lds ? L.total : L.pad) - L.sph) / 8);
    m.sph = (const DevSphere*)(base + (L.sph - L.sph));
    m.segs = (const DevSegment*)(base + (L.seg - L.sph));
    m.ops = (const FkOp*)(base + (L.ops - L.sph));
    m.slot_sph = (const int*)(base + (L.slot - L.sph));
    m.pad_pos = (const double*)(base + (L.pad - L.sph));
}

}  // namespace stomp

namespace {

// The host tables several stages read, alive until creation's last synchronisation (they are
// pageable sources of asynchronous uploads): the transposed setup matrices.  (The kinematic tree,
// the joint limits and the sphere tables stay with the engine: h_segs, h_has_lim, h_jmin / h_jmax, mt.)
struct HostTables {
    std::vector<double> LT, MT, QT;
    std::vector<double> Rb, RinvT;   // stomp_engine_retarget's tables (engine_internal.h)
};

// Owner of the engine under construction: a stage that fails leaves its message in the engine,
// and letting go of the engine publishes it as the thread's last error and frees what was built.
struct AbandonEngine {
    void operator()(stomp_engine* e) const
    {
        g_last_error = e->err;
        release(e);
        delete e;
    }
};

int world_of(const stomp_engine_desc* d) { return d->world_size > 0 ? d->world_size : 1; }

// Stage 1: everything that can be refused before a device is touched
int validate_desc(const stomp_engine_desc* d)
{
    if (d->abi_version != STOMP_ENGINE_ABI_VERSION)
        return fail(nullptr, STOMP_E_INVALID, "abi_version %d != %d", d->abi_version, STOMP_ENGINE_ABI_VERSION);
    if (d->num_joints <= 0 || d->num_joints > kMaxJoints)
        return fail(nullptr, STOMP_E_INVALID, "num_joints must be in [1, %d]", kMaxJoints);
    if (d->num_time_steps <= 0 || d->num_time_steps > 256)
        return fail(nullptr, STOMP_E_INVALID, "num_time_steps must be in [1, 256]");
    if (d->num_rollouts <= 0) return fail(nullptr, STOMP_E_INVALID, "num_rollouts must be positive");
    if (d->num_reused_rollouts < 0 || d->num_reused_rollouts >= d->num_rollouts)
        return fail(nullptr, STOMP_E_INVALID, "Number of reused rollouts must be strictly less than number of rollouts.");
    if (int rc = validate_constraints(d->orientation_constraints, d->num_orientation_constraints, d->num_segments))
        return rc;
    if (d->num_segments <= 0 || !d->segments || (d->num_spheres > 0 && !d->spheres) || !d->joints || !d->noise_stddev ||
        !d->noise_decay || !d->start || !d->goal || !d->grid.data)
        return fail(nullptr, STOMP_E_INVALID, "missing table pointer");
    if (d->grid.nx < 3 || d->grid.ny < 3 || d->grid.nz < 3 || !(d->grid.resolution > 0))
        return fail(nullptr, STOMP_E_INVALID, "invalid grid");
    if ((uint64_t)d->grid.nx * (uint64_t)d->grid.ny * (uint64_t)d->grid.nz > 0xFFFFFFFFull)
        return fail(nullptr, STOMP_E_UNSUPPORTED, "distance field larger than 2^32 cells");
    for (int s = 0; s < d->num_segments; ++s)
        if (d->segments[s].parent >= s || d->segments[s].q_index >= d->num_joints)
            return fail(nullptr, STOMP_E_INVALID, "segment %d: parent must precede it (DFS order), q_index < J", s);
    if (int rc = validate_spheres(d->spheres, d->num_spheres, d->num_segments, d->grid.resolution)) return rc;
    if (d->torque_cost_weight > 1e-9) {
        std::vector<int> path;
        if (const char* why = torque_chain(d, path)) return fail(nullptr, STOMP_E_UNSUPPORTED, "%s", why);
    }
    const int world = world_of(d);
    if (world > 1) {
        if (!d->comm_id) return fail(nullptr, STOMP_E_INVALID, "world_size > 1 needs a comm_id");
        if (d->rank < 0 || d->rank >= world)
            return fail(nullptr, STOMP_E_INVALID, "rank %d outside [0, world_size %d)", d->rank, world);
        if (d->num_rollouts % (world * kSumBlock) != 0)
            return fail(nullptr, STOMP_E_INVALID, "num_rollouts must be a multiple of 64 * world_size");
        if (!kWithRccl && !is_local_comm_id(d->comm_id))
            return fail(nullptr, STOMP_E_UNSUPPORTED, "built without RCCL (use stomp_comm_local_id)");
    }
    return 0;
}

// the engine's stream and the descriptor's scalars
int open_engine(stomp_engine* e, const stomp_engine_desc* d)
{
    e->device = d->device;
    if (hipSetDevice(d->device) != hipSuccess) return fail(e, STOMP_E_DEVICE, "hipSetDevice(%d) failed", d->device);
    if (d->stream) {
        e->stream = (hipStream_t)d->stream;
    } else {
        hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
        e->own_stream = true;
    }
    const int world = world_of(d);
    e->J = d->num_joints; e->N = d->num_time_steps; e->Nall = e->N + 2 * kPad;
    e->K = d->num_rollouts; e->Kr = d->num_reused_rollouts;
    e->world = world; e->rank = world > 1 ? d->rank : 0;
    e->K_loc = e->K / world; e->first = e->rank * e->K_loc;
    e->S = d->num_spheres; e->nseg = d->num_segments; e->seed = d->seed;
    e->model.res = d->grid.resolution;   // (the sphere thresholds read it before finish_model)
    e->disc = d->discretization; e->w_smooth = d->smoothness_cost_weight; e->w_obs = d->obstacle_cost_weight;
    e->w_con = d->constraint_cost_weight; e->w_tq = d->torque_cost_weight;
    for (int r = 0; r < 3; ++r) e->smooth[r] = d->smoothness_costs[r];
    e->use_cum = d->use_cumulative_costs; e->max_it = d->max_iterations;
    e->max_it_cf = d->max_iterations_after_collision_free;
    e->sig_std.assign(d->noise_stddev, d->noise_stddev + e->J);
    e->sig_dec.assign(d->noise_decay, d->noise_decay + e->J);
    e->start.assign(d->start, d->start + e->J);
    e->goal.assign(d->goal, d->goal + e->J);
    return 0;
}

// Stage 2: the K-sharded decomposition.  gather: one all-gather of the state-cost rows
// per iteration, every rank making and pricing all K noise rows; partials: three exchanges
// of 64-rollout block partials (MINMAX / PSUM / USUM weights phases).  Default: gather while
// the state rows of all K rollouts are at most 1 MiB (cfg2: 396 KB; cfg3's 6.5 MB stay
// partials), STOMP_SHARD_MODE=gather|partials to choose.  Gather needs the pregen rows in
// the rollout launch and no reuse.  Every environment variable that shapes it is read here.
int choose_decomposition(stomp_engine* e, const stomp_engine_desc* d, bool local_id)
{
    const int world = e->world;
    if (e->K_loc > kSumBlock * 64) return fail(e, STOMP_E_INVALID, "at most %d rollouts per device", kSumBlock * 64);
    // rows made ahead by the previous rollout launch (the fused noise phase takes J <= 16); with
    // reused rollouts on one device too (the generated rows' noise does not depend on the reuse)
    e->pre_on = (e->Kr == 0 || world == 1) && e->J <= 16;
    const bool can = e->pre_on && e->Kr == 0 && e->K <= kSumBlock * 64;
    const char* sm = std::getenv("STOMP_SHARD_MODE");
    if (world > 1 && sm && std::strcmp(sm, "gather") == 0 && !can)
        // not honoured silently: a rank falling back to partials would post other collectives
        return fail(e, STOMP_E_UNSUPPORTED, "STOMP_SHARD_MODE=gather needs the pregen rows in the rollout launch "
                                            "and no reused rollouts (K_r = %d, J = %d)", e->Kr, e->J);
    // STOMP_DEBUG_GATHER_RANKS=W: a one-device engine times rank 0 of W gather-mode ranks (its
    // K / W rollouts, all K rows made and weighted; nothing exchanged, so results are not the
    // sharded ones: a timing hook)
    const char* sim = std::getenv("STOMP_DEBUG_GATHER_RANKS");
    const int W = (world == 1 && sim) ? std::atoi(sim) : 0;
    if (W > 1 && can && e->K % (W * kSumBlock) == 0) {
        e->gather = true;
        e->K_loc = e->K / W;
    } else if (world > 1 && can) {
        // requested (STOMP_SHARD_MODE), or, where nothing is measured (an in-process group without
        // STOMP_DEBUG_CALIBRATE_LOCAL), gather while the K N state rows fit 1 MiB
        e->gather = sm ? std::strcmp(sm, "gather") == 0 : (size_t)e->K * e->N * sizeof(double) <= (1u << 20);
    }
    // over RCCL, with both decompositions possible and none requested, the choice is measured at
    // the end of creation (calibrate_shard_mode); until then gather mode's layout, which holds every
    // row (shrink_rows gives the buffers back when partials wins)
    // (the in-process exchange group calibrates only on request, STOMP_DEBUG_CALIBRATE_LOCAL=1:
    // its ranks must then be created on host threads of their own, as the measurement exchanges)
    const char* cl = std::getenv("STOMP_DEBUG_CALIBRATE_LOCAL");
    e->calibrate = world > 1 && can && !sm && (!local_id || (cl && cl[0] == '1'));
    if (e->calibrate) e->gather = true;
    e->rows = e->gather ? e->K : e->K_loc;
    e->row0 = (e->gather && world > 1) ? e->first : 0;
    // STOMP_DEBUG_SHARDED_MODES=1: a one-device engine runs the multi-GPU weights phases
    // (test hook for the MINMAX / PSUM / USUM kernels; needs whole 64-rollout blocks, no reuse)
    const char* dbg = std::getenv("STOMP_DEBUG_SHARDED_MODES");
    e->split_modes = (world > 1 && !e->gather) ||
                     (world == 1 && !e->gather && dbg && dbg[0] == '1' && d->num_rollouts % kSumBlock == 0 &&
                      d->num_reused_rollouts == 0);
    return 0;
}

// Stage 3: the FK program, the setup matrices (R^-1, its Cholesky factor, the projection M) and
// the host tables
int setup_tables(stomp_engine* e, const stomp_engine_desc* d, HostTables& t)
{
    e->h_segs.resize(e->nseg);
    for (int s = 0; s < e->nseg; ++s) {
        const stomp_segment& g = d->segments[s];
        DevSegment& o = e->h_segs[s];
        o.parent = g.parent; o.q_index = g.q_index;
        std::memcpy(o.rot, g.rot, sizeof g.rot);
        // as the oracle's so_rot_identity: products with it are skipped on both sides
        o.rot_identity = g.rot[0] == 1.0 && g.rot[1] == 0.0 && g.rot[2] == 0.0 && g.rot[3] == 0.0 &&
                         g.rot[4] == 1.0 && g.rot[5] == 0.0 && g.rot[6] == 0.0 && g.rot[7] == 0.0 &&
                         g.rot[8] == 1.0;
        o.pad_ = 0;
        std::memcpy(o.trans, g.trans, sizeof g.trans);
        std::memcpy(o.axis, g.axis, sizeof g.axis);
    }
    if (int rc = plan_model_tables(e, e, d->spheres, e->S, e->mt)) return rc;
    SetupInput si;
    si.J = e->J; si.N = e->N; si.discretization = e->disc;
    for (int r = 0; r < 3; ++r) si.smoothness_costs[r] = e->smooth[r];
    si.ridge_factor = d->ridge_factor;
    for (int j = 0; j < e->J; ++j) si.joint_cost.push_back(d->joints[j].joint_cost);
    si.start = e->start; si.goal = e->goal;
    std::string msg = compute_setup(si, e->su);
    if (!msg.empty()) return fail(e, STOMP_E_INVALID, "%s", msg.c_str());

    const int J = e->J, N = e->N;
    // LT / MT carry kMatPadRows zero rows past N for the noise kernel's unclamped look-ahead loads
    t.LT.assign((size_t)(N + kMatPadRows) * N, 0.0);
    t.MT.assign((size_t)(N + kMatPadRows) * N, 0.0);
    t.QT.resize((size_t)J * N * N);
    for (int i = 0; i < N; ++i)
        for (int k = 0; k < N; ++k) {
            t.LT[(size_t)k * N + i] = e->su.L[(size_t)i * N + k];
            t.MT[(size_t)k * N + i] = e->su.M[(size_t)i * N + k];
        }
    for (int j = 0; j < J; ++j)
        for (int i = 0; i < N; ++i)
            for (int k = 0; k < N; ++k)
                t.QT[((size_t)j * N + k) * N + i] = e->su.Qinv[((size_t)j * N + i) * N + k];
    // what theta_0 reads (compute_setup, setToMinControlCost): the start-side and goal-side
    // boundary rows of R over the free columns, and R^-1 with lane i's entries consecutive
    t.Rb.resize((size_t)2 * kPad * N);
    t.RinvT.resize((size_t)N * N);
    for (int i = 0; i < kPad; ++i)
        for (int c = 0; c < N; ++c) {
            t.Rb[(size_t)i * N + c] = e->su.Rall[(size_t)i * e->Nall + (c + kPad)];
            t.Rb[(size_t)(kPad + i) * N + c] = e->su.Rall[(size_t)(N + kPad + i) * e->Nall + (c + kPad)];
        }
    for (int i = 0; i < N; ++i)
        for (int k = 0; k < N; ++k) t.RinvT[(size_t)k * N + i] = e->su.Rinv[(size_t)i * N + k];
    e->h_has_lim.resize(J);
    e->h_jmin.resize(J);
    e->h_jmax.resize(J);
    for (int j = 0; j < J; ++j) {
        e->h_has_lim[j] = d->joints[j].has_limits;
        e->h_jmin[j] = d->joints[j].min;
        e->h_jmax[j] = d->joints[j].max;
    }
    return 0;
}

// the reuse step's buffers: one device ranks in k_reuse, several exchange totals and slots
int alloc_reuse_buffers(stomp_engine* e)
{
    const int J = e->J, N = e->N;
    if (e->world == 1 && e->Kr > 0) {   // k_reuse's per-candidate totals and its counter (zeroed)
        if (int rc = dev_alloc(e, &e->d_reuse_costs, (size_t)e->K + 1)) return rc;
        if (int rc = dev_alloc(e, &e->d_reuse_count, 1)) return rc;
        const char* no_spec = std::getenv("STOMP_DEBUG_NO_SPEC");
        if (!(no_spec && std::strcmp(no_spec, "1") == 0)) {
            const size_t n = ((size_t)e->K + 1) * J * N;
            if (int rc = dev_alloc(e, &e->d_spec_params, n)) return rc;
            if (int rc = dev_alloc(e, &e->d_spec_noise, n)) return rc;
            if (int rc = dev_alloc(e, &e->d_spec_ctl, n)) return rc;
            e->spec_on = true;
        }
        const char* no_fuse = std::getenv("STOMP_DEBUG_NO_PICK_FUSE");
        e->pick_fuse = !(no_fuse && std::strcmp(no_fuse, "1") == 0);
    }
    if (e->world > 1 && e->Kr > 0) {
        const size_t slot = (size_t)e->Kr * ((size_t)J * N + N);
        if (int rc = dev_alloc(e, &e->d_tot_loc, (size_t)e->K_loc)) return rc;
        if (int rc = dev_alloc(e, &e->d_tot_all, (size_t)e->K)) return rc;
        if (int rc = dev_alloc(e, &e->d_tot_x, 1)) return rc;
        if (int rc = dev_alloc(e, &e->d_sel, (size_t)e->Kr)) return rc;
        if (int rc = dev_alloc(e, &e->d_slot, slot)) return rc;
        if (int rc = dev_alloc(e, &e->d_slot_all, slot * e->world)) return rc;
    }
    return 0;
}

// Stage 4: the setup matrices, theta and the field on the device; the rollout rows and every
// other per-engine buffer
int alloc_buffers(stomp_engine* e, const stomp_engine_desc* d, const HostTables& tab)
{
    const int J = e->J, N = e->N;
    if (int rc = upload(e, &e->d_QT, tab.QT.data(), tab.QT.size())) return rc;
    if (int rc = upload(e, &e->d_LT, tab.LT.data(), tab.LT.size())) return rc;
    if (int rc = upload(e, &e->d_MT, tab.MT.data(), tab.MT.size())) return rc;
    if (int rc = upload(e, &e->d_Rb, tab.Rb.data(), tab.Rb.size())) return rc;
    if (int rc = upload(e, &e->d_RinvT, tab.RinvT.data(), tab.RinvT.size())) return rc;
    if (int rc = upload(e, &e->d_theta, e->su.theta.data(), e->su.theta.size())) return rc;
    if (int rc = upload(e, &e->d_start, e->start.data(), e->start.size())) return rc;
    if (int rc = upload(e, &e->d_goal, e->goal.data(), e->goal.size())) return rc;
    const size_t ncell = (size_t)d->grid.nx * d->grid.ny * d->grid.nz;
    e->grid_n[0] = d->grid.nx; e->grid_n[1] = d->grid.ny; e->grid_n[2] = d->grid.nz;
    if (d->grid.data_on_device) {
        e->d_sdf = (uint16_t*)d->grid.data;
        e->d_sdf_caller = d->grid.data;
    } else {
        if (int rc = upload(e, &e->d_sdf, d->grid.data, ncell)) return rc;
    }
    const size_t KJN = (size_t)e->rows * J * N;
    if (int rc = dev_alloc(e, &e->d_params, KJN)) return rc;
    if (int rc = dev_alloc(e, &e->d_noise, KJN)) return rc;
    if (int rc = dev_alloc(e, &e->d_control, KJN)) return rc;
    if (int rc = dev_alloc(e, &e->d_prob, KJN)) return rc;
    if (int rc = dev_alloc(e, &e->d_state, (size_t)e->rows * N)) return rc;
    if (e->gather && hipMemsetAsync(e->d_state, 0, sizeof(double) * e->rows * N, e->stream) != hipSuccess)
        return fail(e, STOMP_E_DEVICE, "memset failed");
    if (e->Kr > 0) {
        if (int rc = dev_alloc(e, &e->d_params_b, KJN)) return rc;
        if (int rc = dev_alloc(e, &e->d_noise_b, KJN)) return rc;
        if (int rc = dev_alloc(e, &e->d_control_b, KJN)) return rc;
        if (int rc = dev_alloc(e, &e->d_state_b, (size_t)e->K_loc * N)) return rc;
    }
    if (e->use_cum)
        if (int rc = dev_alloc(e, &e->d_cum, KJN)) return rc;
    if (int rc = dev_alloc(e, &e->d_u, (size_t)J * N)) return rc;
    if (e->split_modes || e->calibrate) {
        const size_t nb_loc = (size_t)e->K_loc / kSumBlock, nb_tot = (size_t)e->K / kSumBlock;
        if (int rc = dev_alloc(e, &e->d_mm, 2 * (size_t)J * N)) return rc;
        if (int rc = dev_alloc(e, &e->d_psum_part, nb_loc * J * N)) return rc;
        if (int rc = dev_alloc(e, &e->d_psum_all, nb_tot * J * N)) return rc;
        if (int rc = dev_alloc(e, &e->d_u_part, nb_loc * J * N)) return rc;
        if (int rc = dev_alloc(e, &e->d_u_all, nb_tot * J * N)) return rc;
    }
    if (e->pre_on) {
        for (int b = 0; b < 2; ++b) {
            if (int rc = dev_alloc(e, &e->d_pre_eps[b], KJN)) return rc;
            if (int rc = dev_alloc(e, &e->d_pre_meps[b], KJN)) return rc;
        }
        if (int rc = dev_alloc(e, &e->d_theta_gen, (size_t)J * N)) return rc;
    }
    if (int rc = dev_alloc(e, &e->d_x_params, (size_t)J * N)) return rc;
    if (int rc = dev_alloc(e, &e->d_x_noise, (size_t)J * N)) return rc;
    if (int rc = dev_alloc(e, &e->d_x_control, (size_t)J * N)) return rc;
    if (int rc = dev_alloc(e, &e->d_x_state, (size_t)N)) return rc;
    if (int rc = dev_alloc(e, &e->d_last_traj, (size_t)J * N)) return rc;
    if (int rc = dev_alloc(e, &e->d_best_traj, (size_t)J * N)) return rc;
    if (int rc = dev_alloc(e, &e->d_total, 1)) return rc;
    if (int rc = dev_alloc(e, &e->d_cf, 1)) return rc;
    if (int rc = dev_alloc(e, &e->d_cs, 1)) return rc;
    if (int rc = dev_alloc(e, &e->d_track, 1)) return rc;
    e->d_stop = &e->d_track->stop;
    if (int rc = dev_alloc(e, &e->d_opt_costs, (size_t)std::max(e->max_it, 1))) return rc;
    if (hipHostMalloc((void**)&e->h_track, sizeof(DevTrack) * 4) != hipSuccess)
        return fail(e, STOMP_E_DEVICE, "hipHostMalloc failed");
    if (hipMemsetAsync(e->d_track, 0, sizeof(DevTrack), e->stream) != hipSuccess)
        return fail(e, STOMP_E_DEVICE, "memset failed");
    if (hipMemsetAsync(e->d_cs, 1, 1, e->stream) != hipSuccess) return fail(e, STOMP_E_DEVICE, "memset failed");
    if (int rc = dev_alloc(e, &e->d_pad_cf, 1)) return rc;
    if (int rc = alloc_reuse_buffers(e)) return rc;
    if (hipHostMalloc((void**)&e->h_total, sizeof(double)) != hipSuccess ||
        hipHostMalloc((void**)&e->h_cf, 16) != hipSuccess)
        return fail(e, STOMP_E_DEVICE, "hipHostMalloc failed");
    return 0;
}

// the torque term's chain (stomp_robot_model.cpp:185-189): segments below torque_root up to
// torque_tip, whose joints must be the group's joints in order.  Built whenever the inertias
// describe a valid chain: the term itself runs only with torque_cost_weight > 1e-9, the
// final torque statistics of optimize() always (stomp_optimizer.cpp:384-398)
int build_torque_chain(stomp_engine* e, const stomp_engine_desc* d, const HostTables& tab)
{
    std::vector<int> path;
    if (torque_chain(d, path) != nullptr) return 0;
    std::vector<ChainSeg> cs(path.size());
    for (size_t i = 0; i < path.size(); ++i) {
        cs[i].seg = e->h_segs[path[i]];
        // KDL::RigidBodyInertia(m, c, Ic): h = m c, I = Ic - m (c c^T - (c.c) 1)
        const stomp_inertia& in = d->inertias[path[i]];
        const double* c = in.com;
        const double* v = in.inertia;
        const double Ic[9] = {v[0], v[3], v[4], v[3], v[1], v[5], v[4], v[5], v[2]};
        const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
        cs[i].m = in.mass;
        for (int a = 0; a < 3; ++a) {
            cs[i].h[a] = in.mass * c[a];
            for (int b = 0; b < 3; ++b) cs[i].I[3 * a + b] = Ic[3 * a + b] - in.mass * (c[a] * c[b] - (a == b ? cc : 0.0));
        }
    }
    ChainSeg* d_chain;
    if (int rc = upload(e, &d_chain, cs.data(), cs.size())) return rc;
    TermsModel& t = e->terms;
    t.torque = d->torque_cost_weight > 1e-9 ? 1 : 0;
    t.nchain = (int)cs.size();
    t.chain = d_chain;
    for (int k = 0; k < 3; ++k) t.g[k] = d->gravity[k];
    if (t.torque) e->terms_on = true;
    e->torque_stats = true;
    return 0;
}

// the path constraints (OrientationConstraintEvaluator) as k_terms holds them
int build_constraints(stomp_engine* e, const stomp_engine_desc* d)
{
    if (d->num_orientation_constraints <= 0) return 0;
    std::vector<OcDev> oc;
    if (int rc = plan_constraints(e, e, d->orientation_constraints, d->num_orientation_constraints, oc)) return rc;
    if (int rc = upload(e, &e->d_oc, oc.data(), oc.size())) return rc;
    e->oc_cap = oc.size();
    e->terms.noc = (int)oc.size();
    e->terms.oc = e->d_oc;
    e->terms_on = true;
    return 0;
}

// Stage 5: the state-cost terms' models (k_terms): the torque chain, the path constraints, their
// buffers; the PolicyImprovement API's update buffer
int build_terms(stomp_engine* e, const stomp_engine_desc* d, const HostTables& tab)
{
    const int J = e->J, N = e->N;
    if (int rc = build_torque_chain(e, d, tab)) return rc;
    if (int rc = build_constraints(e, d)) return rc;
    if (e->terms_on || e->torque_stats) {
        TermsModel& t = e->terms;
        if (int rc = plan_terms(e, e, t, e->terms_on)) return rc;
        if (terms_lds_bytes(t) > 160 * 1024)
            e->torque_stats = false;   // the chain stays in e->terms: get_best_torques says why it cannot run
        if (getenv("STOMP_DEBUG_LEAN_PRINT"))   // the launch launch_terms takes (read-only: tests and tables)
            fprintf(stderr, "stomp: terms J %d N %d nchain %d noc %d torque %d stats %d, k_terms<%d>, LDS %zu B, "
                            "opt-in %d\n", J, N, t.nchain, t.noc, t.torque, e->torque_stats ? 1 : 0, N <= 128 ? 128 : 256,
                    terms_lds_bytes(t), terms_lds_bytes(t) > 64 * 1024 ? 1 : 0);
        if (e->terms_on)
            if (int rc = dev_alloc(e, &e->d_terms_traj, (size_t)e->K_loc * J * N)) return rc;
        if (e->torque_stats) {
            e->tq_model = t;
            e->tq_model.torque = 1;
            e->tq_model.noc = 0;   // torques only
            if (int rc = dev_alloc(e, &e->d_tq, (size_t)N)) return rc;
            if (int rc = dev_alloc(e, &e->d_tq_state, (size_t)N)) return rc;
        }
    }
    if (int rc = dev_alloc(e, &e->d_delta, (size_t)J * N)) return rc;
    e->pi_weight = e->w_smooth;
    if (hipDeviceGetAttribute(&e->wall_khz, hipDeviceAttributeWallClockRate, d->device) != hipSuccess) e->wall_khz = 0;
    return 0;
}

}  // namespace

namespace stomp {

// Stage 6: the rollout kernel's layout for this model and launch size: the sincos pre-pass, the
// padding rows' positions in LDS or not, the LDS-lean slot-loop layouts
// (a shared stage as those above: m is the model under construction, or on a live engine a copy of
// its model whose compute-unit count is already known; the kernels' attributes are asked of the
// current device, the engine's)
int choose_layout(stomp_engine* err, const stomp_engine* e, const ModelTables& t, DevModel& m)
{
    const int J = e->J, N = e->N;
    const std::vector<FkOp>& ops = t.ops;
    m.J = J; m.N = N; m.Nall = e->Nall; m.S = t.S; m.nops = (int)ops.size(); m.nseg = e->nseg;
    m.nslots = t.nslots;
    m.sph_chunk = 1;   // the a-value buffer holds the longest sphere run
    for (const FkOp& o : ops) m.sph_chunk = std::max(m.sph_chunk, o.sph_end - o.sph_begin);
    if (m.sph_chunk * N > 65535)
        return fail(err, STOMP_E_UNSUPPORTED, "%d spheres on one segment x %d waypoints exceed 16-bit pair ids",
                    m.sph_chunk, N);
    m.nsaves = 0;
    for (const FkOp& o : ops) m.nsaves = std::max(m.nsaves, o.save + 1);
    // the sincos pre-pass parks the cosines in the saved-frame area: only when that area
    // holds J x N doubles and the first save comes after the last joint segment
    int last_joint = -1, first_save = (int)ops.size();
    for (int i = 0; i < (int)ops.size(); ++i) {
        const FkOp& o = ops[i];
        if (o.seg >= 0 && e->h_segs[o.seg].q_index >= 0) last_joint = i;
        if (o.save >= 0 && first_save == (int)ops.size()) first_save = i;
    }
    m.sincos_pre = m.nsaves >= 1 && J <= 12 * m.nsaves && first_save > last_joint ? 1 : 0;
    // padding-row positions go to LDS unless that costs a workgroup per CU the launch
    // would use: one rollout launch has K_loc + 1 workgroups over the device's CUs
    const size_t stat = rollout_static_lds();
    const size_t with_pad = rollout_lds_bytes(m, 1) + stat, without = rollout_lds_bytes(m, 0) + stat;
    int cus = m.cus;
    if (cus <= 0 &&
        (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || cus <= 0))
        cus = 256;
    m.cus = cus;
    // every workgroup of the launch counts: the rollouts, the noiseless one, the pregen blocks
    // and the reuse candidates' totals blocks beside them (K = 448 with its 449 pregen blocks
    // ran two workgroups per CU at 54.6 us against three at K = 512, 47.1 us: the padding
    // positions took the slot the pregen blocks need)
    const int blocks = e->K_loc + 1 + (e->pre_on ? e->rows : 0) + (e->Kr > 0 && e->world == 1 ? e->K : 0);
    const int need = (blocks + cus - 1) / cus;
    m.pad_lds = (with_pad <= kRolloutLdsMax &&
                 rollout_blocks_per_cu(with_pad) >= std::min(need, rollout_blocks_per_cu(without))) ? 1 : 0;
    const size_t lds = rollout_lds_bytes(m, m.pad_lds) + stat;
    m.phased_lds = (int)rollout_phased_lds_bytes(m);
    if (getenv("STOMP_DEBUG_PHASED")) fprintf(stderr, "stomp: phased rollout LDS %d B\n", m.phased_lds);
    if (lds > kRolloutLdsMax)
        return fail(err, STOMP_E_UNSUPPORTED, "rollout kernel needs %zu B of LDS (J=%d, N=%d, S=%d, %d spheres "
                                              "on one segment), more than %zu", lds, J, N, m.S, m.sph_chunk,
                    kRolloutLdsMax);
    // the LDS-lean slot-loop layout (DevModel::lean) when it puts more rollout workgroups on a
    // CU and the launch has more workgroups than the full layout's slots: cfg3's N = 199 (71.7
    // KB per workgroup, two per CU; lean 2 46.5 KB, three) and cfg4's two-arm tree (two saved
    // frames, a 12 KB table)
    m.lean = 0;
    const int per_cu_full = rollout_blocks_per_cu(lds);
    int per_cu[3] = {per_cu_full, 0, 0};
    for (int lv = 1; lv <= 2; ++lv)
        if (rollout_lean_allowed(m, lv)) per_cu[lv] = rollout_blocks_per_cu(rollout_lds_bytes(m, 0, lv) + stat, lv);
    if (need > per_cu_full) {
        int best = per_cu_full;
        for (int lv = 1; lv <= 2; ++lv)
            if (per_cu[lv] > best) {
                best = per_cu[lv];
                m.lean = lv;
            }
    }
    if (const char* v = getenv("STOMP_DEBUG_LEAN")) {   // tests / A/B: force a layout
        const int lv = atoi(v);
        if (lv >= 0 && lv <= 2 && rollout_lean_allowed(m, lv)) m.lean = lv;
    }
    if (getenv("STOMP_DEBUG_LEAN_PRINT"))
        fprintf(stderr, "stomp: rollout LDS full %zu / lean1 %zu / lean2 %zu B, workgroups per CU %d / %d / %d, "
                        "needed %d, layout lean %d\n", lds, rollout_lds_bytes(m, 0, 1) + stat,
                rollout_lds_bytes(m, 0, 2) + stat, per_cu[0], per_cu[1], per_cu[2], need, m.lean);
    if (!cost_supported(m)) return fail(err, STOMP_E_UNSUPPORTED, "FK program too large (%d ops, %d segments)",
                                        m.nops, m.nseg);
    return 0;
}

// the lean layout's saved-frame blocks, [nsaves][12][N] per rollout workgroup of a launch, in the
// buffer held for them (d_sv, sv_cap: the engine's fields at creation, a commit's copies of them on
// a live engine; grown when this model needs more, as grow_buffer does)
int place_saved_frames(stomp_engine* e, DevModel& m, double** d_sv, size_t* sv_cap, LiveAlloc* live)
{
    m.sv_glob = nullptr;
    m.sv_rows = 0;
    if (!(m.lean && m.nsaves > 0)) return 0;
    m.sv_rows = e->K_loc + 1;
    if (int rc = grow_buffer(e, d_sv, sv_cap, (size_t)m.sv_rows * m.nsaves * 12 * e->N, live)) return rc;
    m.sv_glob = *d_sv;
    return 0;
}

}  // namespace stomp

namespace {

// Stage 7: the rollout kernel's LDS table image (RolloutLds from .sph on), padding positions last
int upload_lds_image(stomp_engine* e)
{
    DevModel& m = e->model;
    std::vector<unsigned char> img = build_model_image(e, e->mt, m);
    img.resize(model_image_bytes(e, m), 0);
    if (int rc = upload(e, &e->d_img, (const unsigned long long*)img.data(), img.size() / 8)) return rc;
    e->img_cap = img.size() / 8;
    if (hipStreamSynchronize(e->stream) != hipSuccess)   // img is pageable and goes out of scope
        return fail(e, STOMP_E_DEVICE, "table upload failed");
    point_model_into_image(e, m, e->d_img);
    e->d_pad_pos = (double*)m.pad_pos;
    m.sdf = e->d_sdf;
    return 0;
}

// Stage 8: the field as 4^3 bricks (one 128-B line per brick) when it is large: the SDF gathers of
// neighbouring rollouts' spheres, which differ in x and y as much as in z, then land on
// shared lines (a z-fastest line holds 64 cells along z only).  STOMP_SDF_LAYOUT =
// brick | linear overrides.  The engine keeps its own bricked copy; the caller's field
// ([x][y][z], the ABI's layout) is only read here.
int place_field(stomp_engine* e, const stomp_engine_desc* d)
{
    DevModel& m = e->model;
    const size_t ncell = (size_t)d->grid.nx * d->grid.ny * d->grid.nz;
    const char* lay = std::getenv("STOMP_SDF_LAYOUT");
    const bool brick = lay ? std::strcmp(lay, "brick") == 0 : ncell * sizeof(uint16_t) > ((size_t)64 << 20);
    m.brick = 0;
    m.nby = (d->grid.ny + 3) / 4;
    m.nbz = (d->grid.nz + 3) / 4;
    if (!brick) return 0;
    uint16_t* bricks = nullptr;
    if (int rc = dev_alloc(e, &bricks, sdf_brick_cells(d->grid.nx, d->grid.ny, d->grid.nz))) return rc;
    launch_sdf_bricks(e->d_sdf, bricks, d->grid.nx, d->grid.ny, d->grid.nz, e->stream);
    if (hipStreamSynchronize(e->stream) != hipSuccess)
        return fail(e, STOMP_E_DEVICE, "distance-field brick layout failed");
    if (!d->grid.data_on_device) {   // the linear upload is no longer needed
        auto it = std::find(e->allocs.begin(), e->allocs.end(), (void*)e->d_sdf);
        if (it != e->allocs.end()) {
            hipFree(*it);
            e->allocs.erase(it);
        }
    }
    e->d_sdf = bricks;
    m.sdf = bricks;
    m.brick = 1;
    return 0;
}

// the rest of the device model, once the tables and the field are placed: the grid's geometry, the
// velocity stencil, the split launches' piece counters and the lean layout's saved-frame blocks
// (allocated after the field's bricks), the debug knobs of the launch
int finish_model(stomp_engine* e, const stomp_engine_desc* d)
{
    const int J = e->J, N = e->N;
    DevModel& m = e->model;
    e->terms.segs = m.segs;
    e->tq_model.segs = m.segs;
    m.nx = d->grid.nx; m.ny = d->grid.ny; m.nz = d->grid.nz;
    m.ny_d = (double)m.ny; m.nz_d = (double)m.nz;
    m.hi_x = m.nx - 1.5; m.hi_y = m.ny - 1.5; m.hi_z = m.nz - 1.5;
    m.ox = d->grid.origin[0]; m.oy = d->grid.origin[1]; m.oz = d->grid.origin[2]; m.res = d->grid.resolution;
    m.inv_res = 1.0 / d->grid.resolution;
    m.start = e->d_start; m.goal = e->d_goal;
    const double invTime = 1.0 / e->disc;   // stomp_optimizer.cpp:620
    for (int k = 0; k < 7; ++k) {
        m.vel_coef[k] = invTime * kDiffRules[0][k];
        if ((k < kVelTap0 || k > kVelTap1) && kDiffRules[0][k] != 0.0)
            return fail(e, STOMP_E_UNSUPPORTED, "velocity rule tap %d outside the kernel's stencil", k);
    }
    m.w_obs = e->w_obs; m.w_con = e->w_con; m.w_tq = e->w_tq;
    m.QT = e->d_QT;
    // piece counters of the waypoint-split rollout launches (zeroed; the last piece resets its own)
    // one per rollout of any split launch: split_pieces takes nro <= cus / 2 (two pieces or more
    // per rollout), and an eval batch may hold more rows than K_loc + 1
    m.split_cap = std::max(e->K_loc + 2, m.cus / 2 + 1);
    if (int rc = dev_alloc(e, &m.split_cnt, (size_t)m.split_cap)) return rc;
    if (int rc = place_saved_frames(e, m, &e->d_sv, &e->sv_cap, nullptr)) return rc;
    {
        const char* env = std::getenv("STOMP_DEBUG_SPLIT_MAX");
        m.split_max = env ? std::atoi(env) : 0;
        const char* xi = std::getenv("STOMP_DEBUG_XCTL_INLINE");
        m.x_ctl_inline = xi && std::strcmp(xi, "1") == 0 ? 1 : 0;
    }
    if (getenv("STOMP_DEBUG_LEAN_PRINT")) {
        // what creation chose for this model, and the body launch_cost takes for an iteration's
        // K_loc rollouts + the noiseless one beside the pregen blocks (read-only: tests and tables).
        // The weights kernel is that of the rows the launch covers now (gather: all K).  Where the
        // decomposition is still to be measured (e->calibrate) that is gather's layout: if the
        // calibration then picks partials, the phases run the K_loc-row kernel, not the one named here
        const int nro = e->K_loc + 1, extra = e->pre_on ? e->rows : 0;
        const int P = rollout_split_pieces(m, nro, extra, false);
        const char* body = P ? "split" : nro <= m.cus ? (m.phased_lds > 0 ? "phased" : "wide")
                                                      : (m.lean ? "lean slot loop" : "slot loop");
        fprintf(stderr, "stomp: model J %d N %d S %d nseg %d nops %d nsaves %d sincos_pre %d sph_chunk %d lean %d "
                        "pregen %d fused_noise %d brick %d, launch of %d rollouts: %s, %d pieces, weights %s\n",
                J, N, e->S, m.nseg, m.nops, m.nsaves, m.sincos_pre, m.sph_chunk, m.lean, e->pre_on ? 1 : 0,
                J <= 16 ? 1 : 0, m.brick, nro, body, P, weights_kernel_name(e->rows, !e->split_modes, false));
    }
    return 0;
}

// Stage 9: the padding rows' FK (start / goal poses: sphere positions and whether they collide),
// and theta as the last and the best trajectory so far
int pad_fk(stomp_engine* e)
{
    const int J = e->J, N = e->N;
    DevModel& m = e->model;
    m.pad_collision = 0;
    launch_pad_fk(m, e->d_start, e->d_goal, e->d_pad_pos, e->d_pad_cf, e->stream);
    int pad_cf = 0;
    if (hipMemcpyAsync(&pad_cf, e->d_pad_cf, sizeof(int), hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess)
        return fail(e, STOMP_E_DEVICE, "padding FK failed: %s", hipGetErrorString(hipGetLastError()));
    m.pad_collision = pad_cf;
    e->pad_collision = pad_cf;
    if (hipMemcpyAsync(e->d_last_traj, e->d_theta, sizeof(double) * J * N, hipMemcpyDeviceToDevice, e->stream) !=
            hipSuccess ||
        hipMemcpyAsync(e->d_best_traj, e->d_theta, sizeof(double) * J * N, hipMemcpyDeviceToDevice, e->stream) !=
            hipSuccess)
        return fail(e, STOMP_E_DEVICE, "trajectory copies failed");
    return 0;
}

// Stage 11: everything enqueued so far has run; the decomposition is measured when both are possible
int settle_and_calibrate(stomp_engine* e)
{
    if (hipStreamSynchronize(e->stream) != hipSuccess) return fail(e, STOMP_E_DEVICE, "setup failed");
    return e->calibrate ? calibrate_shard_mode(e) : 0;
}

}  // namespace

extern "C" int stomp_engine_create(const stomp_engine_desc* d, stomp_engine** out)
{
    if (!d || !out) return fail(nullptr, STOMP_E_INVALID, "null argument");
    *out = nullptr;
    if (int rc = validate_desc(d)) return rc;

    DeviceGuard dg(d->device);
    std::unique_ptr<stomp_engine, AbandonEngine> owner(new stomp_engine());
    stomp_engine* e = owner.get();
    const bool local_id = world_of(d) > 1 && is_local_comm_id(d->comm_id);
    HostTables tab;
    if (int rc = open_engine(e, d)) return rc;
    if (int rc = choose_decomposition(e, d, local_id)) return rc;
    if (int rc = setup_tables(e, d, tab)) return rc;
    if (int rc = alloc_buffers(e, d, tab)) return rc;
    if (int rc = build_terms(e, d, tab)) return rc;
    if (int rc = choose_layout(e, e, e->mt, e->model)) return rc;
    if (int rc = upload_lds_image(e)) return rc;
    if (int rc = place_field(e, d)) return rc;
    if (int rc = finish_model(e, d)) return rc;
    if (int rc = pad_fk(e)) return rc;
    if (int rc = join_exchange(e, d->comm_id, local_id)) return rc;
    if (int rc = settle_and_calibrate(e)) return rc;
    *out = owner.release();
    return 0;
}
