// engine_chomp.cpp -- stomp_chomp_*: CHOMP mode (k_chomp.hip) on a live engine's model, field and
// cost.  A stomp_chomp borrows its engine: it reads the engine's tables, start, goal, Q^-1 and field
// on the engine's stream and writes only buffers of its own -- one device slab for the descents'
// state, one for the tables, one pinned block for uploads and read-backs, each held with a capacity.
// Nothing the engine's iterations read or write is touched: no flush, no swap, no counter of theirs.
#include "engine_internal.h"
#include "chomp.h"

using namespace stomp;

struct stomp_chomp {
    stomp_engine* e = nullptr;
    std::string err;
    double lr = 0, w_smooth = 0, ridge = 0, bias[3] = {0, 0, 0};
    int use_pinv = 0;
    std::vector<double> upd;
    int B = 0;
    bool ready = false;                 // a reset has run and the engine is as it was then
    long long model_epoch = 0, target_epoch = 0;
    int iterations = 0;                 // stepped since the reset
    long long launches = 0, allocs = 0;
    DevModel model{};                   // the engine's model at the reset
    ChompArgs args{};
    unsigned char *d_state = nullptr, *d_tab = nullptr, *h_pin = nullptr;
    size_t state_cap = 0, tab_cap = 0, pin_cap = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
};

namespace {

constexpr size_t kChompLdsMax = 64 * 1024;   // dynamic LDS without an opt-in

int cfail(stomp_chomp* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    g_last_error = buf;
    return code;
}

#define CH_TRY(c, x)                                                                              \
    do {                                                                                          \
        hipError_t _st = (x);                                                                     \
        if (_st != hipSuccess)                                                                    \
            return cfail((c), STOMP_E_DEVICE, "%s failed: %s", #x, hipGetErrorString(_st));       \
    } while (0)

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// where the descents' state lies in the device slab (bytes)
struct StateMap {
    size_t track, mirror, traj, sinc, cinc, finc, scales, pos, dist, pot, vmag, fgrad, pgrad, vel, acc, col, wp_col,
        jorg, jax, wcost, cost, cf, hist, best, total;
    StateMap(size_t B, size_t J, size_t N, size_t S, size_t max_it)
    {
        size_t o = 0;
        auto take = [&](size_t& at, size_t bytes) {
            at = o;
            o += align256(bytes);
        };
        const size_t d = sizeof(double), S1 = std::max<size_t>(S, 1);
        take(track, sizeof(ChompTrack) * B);
        take(mirror, sizeof(int) * B);
        take(traj, d * B * J * N); take(sinc, d * B * J * N); take(cinc, d * B * J * N); take(finc, d * B * J * N);
        take(scales, d * B * J);
        take(pos, d * B * N * S1 * 3);
        take(dist, d * B * N * S1); take(pot, d * B * N * S1); take(vmag, d * B * N * S1);
        take(fgrad, d * B * N * S1 * 3); take(pgrad, d * B * N * S1 * 3);
        take(vel, d * B * N * S1 * 3); take(acc, d * B * N * S1 * 3);
        take(col, B * N * S1);
        take(wp_col, sizeof(int) * B * N);
        take(jorg, d * B * N * J * 3); take(jax, d * B * N * J * 3);
        take(wcost, d * B * N); take(cost, d * B); take(cf, sizeof(int) * B);
        take(hist, d * B * std::max<size_t>(max_it, 1));
        take(best, d * B * J * N);
        total = o;
    }
};

// the tables (device slab and its pinned source)
struct TabMap {
    size_t sph_seg, seg_mask, joint_seg, hl, jlim, upd, band, total;
    TabMap(size_t J, size_t Nall, size_t S, size_t nseg)
    {
        size_t o = 0;
        auto take = [&](size_t& at, size_t bytes) {
            at = o;
            o += align256(bytes);
        };
        take(sph_seg, sizeof(int) * std::max<size_t>(S, 1));
        take(seg_mask, sizeof(unsigned) * nseg);
        take(joint_seg, sizeof(int) * J);
        take(hl, sizeof(int) * J);
        take(jlim, sizeof(double) * 2 * J);
        take(upd, sizeof(double) * J);
        take(band, sizeof(double) * J * Nall * 13);
        total = o;
    }
};

// the pinned block: the tables' source, then the initial tracks and trajectories (uploads), the two
// stop-flag slots of the optimize loop and its results (read-backs)
struct PinMap {
    size_t tab, track, traj, mirror[2], hist, best, total;
    PinMap(const TabMap& t, size_t B, size_t J, size_t N, size_t max_it)
    {
        size_t o = 0;
        auto take = [&](size_t& at, size_t bytes) {
            at = o;
            o += align256(bytes);
        };
        take(tab, t.total);
        take(track, sizeof(ChompTrack) * B);
        take(traj, sizeof(double) * B * J * N);
        take(mirror[0], sizeof(int) * B);
        take(mirror[1], sizeof(int) * B);
        take(hist, sizeof(double) * B * std::max<size_t>(max_it, 1));
        take(best, sizeof(double) * B * J * N);
        total = o;
    }
};

// `bytes` of device (pinned: host) memory held with a capacity; an allocation counts in c->allocs
int reserve(stomp_chomp* c, unsigned char** p, size_t* cap, size_t bytes, bool pinned)
{
    if (bytes <= *cap) return 0;
    // (no launch reads the old block: every call that grows one has waited for the stream)
    if (*p) {
        if (pinned) hipHostFree(*p);
        else hipFree(*p);
        *p = nullptr;
        *cap = 0;
    }
    void* q = nullptr;
    const hipError_t st = pinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes);
    if (st != hipSuccess)
        return cfail(c, STOMP_E_DEVICE, "chomp: allocation of %zu bytes failed: %s", bytes, hipGetErrorString(st));
    *p = (unsigned char*)q;
    *cap = bytes;
    ++c->allocs;
    return 0;
}

// the refusals every call after a reset shares (host only)
int check_live(stomp_chomp* c, const char* call)
{
    const stomp_engine* e = c->e;
    if (e->tracking) return cfail(c, STOMP_E_INVALID, "chomp %s: the engine is inside its optimize loop", call);
    if (!c->ready) return cfail(c, STOMP_E_INVALID, "chomp %s: no reset yet", call);
    if (c->model_epoch != e->model_epoch)
        return cfail(c, STOMP_E_INVALID, "chomp %s: the engine's model changed since the last reset (a request "
                     "replaced its collision points or constraints); call stomp_chomp_reset", call);
    if (c->target_epoch != e->target_epoch)
        return cfail(c, STOMP_E_INVALID, "chomp %s: the engine was retargeted or its field refreshed since the last "
                     "reset; call stomp_chomp_reset", call);
    return 0;
}

// one iteration (doChompOptimization) of every descent whose stop flag is down
void enqueue_step(stomp_chomp* c, int member, int it)
{
    ChompArgs& a = c->args;
    hipStream_t s = c->e->stream;
    a.member = member;
    a.it = it;
    launch_chomp_grad(c->model, a, s);
    launch_chomp_update(c->model, a, s);
    launch_chomp_fk(c->model, a, s);
    launch_chomp_vel(c->model, a, s);
    launch_chomp_track(c->model, a, s);
    c->launches += 5;
}

int chomp_reset(stomp_chomp* c, int B, const double* trajectories)
{
    stomp_engine* e = c->e;
    const int J = e->J, N = e->N, Nall = e->Nall, S = e->model.S, nseg = e->nseg;
    hipStream_t s = e->stream;
    c->ready = false;
    c->launches = 0;
    const StateMap sm((size_t)B, J, N, S, e->max_it);
    const TabMap tm(J, Nall, S, nseg);
    const PinMap pm(tm, (size_t)B, J, N, e->max_it);
    if (sm.total > c->state_cap || tm.total > c->tab_cap || pm.total > c->pin_cap)
        CH_TRY(c, hipStreamSynchronize(s));   // before a block that a launch may still read is replaced
    if (int rc = reserve(c, &c->d_state, &c->state_cap, sm.total, false)) return rc;
    if (int rc = reserve(c, &c->d_tab, &c->tab_cap, tm.total, false)) return rc;
    if (int rc = reserve(c, &c->h_pin, &c->pin_cap, pm.total, true)) return rc;
    for (hipEvent_t& ev : c->ev)
        if (!ev) {
            CH_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            ++c->allocs;
        }
    unsigned char *d = c->d_state, *t = c->d_tab, *h = c->h_pin;

    // the tables: each sphere's segment from the FK program, the joints on each segment's path, the
    // segment each joint drives, the limits, the update limits and the smoothness band
    unsigned char* ht = h + pm.tab;
    {
        int* sph_seg = (int*)(ht + tm.sph_seg);
        int cur = -1;
        for (const FkOp& o : e->mt.ops) {
            if (o.seg >= 0) cur = o.seg;
            for (int j = o.sph_begin; j < o.sph_end; ++j) sph_seg[j] = cur;
        }
        unsigned* mask = (unsigned*)(ht + tm.seg_mask);
        int* joint_seg = (int*)(ht + tm.joint_seg);
        std::fill(joint_seg, joint_seg + J, -1);
        for (int g = 0; g < nseg; ++g) {
            const DevSegment& sg = e->h_segs[g];
            unsigned m = sg.parent >= 0 ? mask[sg.parent] : 0u;
            if (sg.q_index >= 0) {
                m |= 1u << sg.q_index;
                if (joint_seg[sg.q_index] < 0) joint_seg[sg.q_index] = g;
            }
            mask[g] = m;
        }
        int* hl = (int*)(ht + tm.hl);
        double* jlim = (double*)(ht + tm.jlim);
        for (int j = 0; j < J; ++j) {
            hl[j] = e->h_has_lim[j];
            jlim[2 * j] = e->h_jmin[j];
            jlim[2 * j + 1] = e->h_jmax[j];
        }
        std::memcpy(ht + tm.upd, c->upd.data(), sizeof(double) * J);
        std::memcpy(ht + tm.band, e->su.Qband.data(), sizeof(double) * (size_t)J * Nall * 13);
    }
    CH_TRY(c, hipMemcpyAsync(t, ht, tm.total, hipMemcpyHostToDevice, s));

    ChompArgs a{};
    a.B = B; a.J = J; a.N = N; a.Nall = Nall; a.S = S; a.nseg = nseg;
    a.member = 0; a.it = -1;
    a.max_it = e->max_it; a.max_it_cf = e->max_it_cf;
    a.use_pinv = c->use_pinv;
    a.lr = c->lr; a.w_smooth = c->w_smooth; a.w_obs = e->w_obs; a.ridge = c->ridge;
    for (int k = 0; k < 3; ++k) a.bias[k] = c->bias[k];
    const double invTime = 1.0 / e->disc;          // stomp_optimizer.cpp:620-621
    const double invTimeSq = invTime * invTime;
    for (int k = 0; k < 7; ++k) {
        a.cv[k] = invTime * kDiffRules[0][k];
        a.ca[k] = invTimeSq * kDiffRules[1][k];
    }
    a.sph_seg = (const int*)(t + tm.sph_seg);
    a.seg_mask = (const unsigned*)(t + tm.seg_mask);
    a.joint_seg = (const int*)(t + tm.joint_seg);
    a.hl = (const int*)(t + tm.hl);
    a.jlim = (const double*)(t + tm.jlim);
    a.upd = (const double*)(t + tm.upd);
    a.band = (const double*)(t + tm.band);
    a.track = (ChompTrack*)(d + sm.track);
    a.mirror = (int*)(d + sm.mirror);
    a.traj = (double*)(d + sm.traj);
    a.sinc = (double*)(d + sm.sinc); a.cinc = (double*)(d + sm.cinc); a.finc = (double*)(d + sm.finc);
    a.scales = (double*)(d + sm.scales);
    a.pos = (double*)(d + sm.pos);
    a.dist = (double*)(d + sm.dist); a.pot = (double*)(d + sm.pot); a.vmag = (double*)(d + sm.vmag);
    a.fgrad = (double*)(d + sm.fgrad); a.pgrad = (double*)(d + sm.pgrad);
    a.vel = (double*)(d + sm.vel); a.acc = (double*)(d + sm.acc);
    a.col = d + sm.col;
    a.wp_col = (int*)(d + sm.wp_col);
    a.jorg = (double*)(d + sm.jorg); a.jax = (double*)(d + sm.jax);
    a.wcost = (double*)(d + sm.wcost); a.cost = (double*)(d + sm.cost); a.cf = (int*)(d + sm.cf);
    a.hist = (double*)(d + sm.hist);
    a.best_traj = (double*)(d + sm.best);
    c->model = e->model;
    if (chomp_fk_lds(a) > kChompLdsMax || chomp_grad_lds(a) > kChompLdsMax || chomp_update_lds(a) > kChompLdsMax)
        return cfail(c, STOMP_E_UNSUPPORTED, "chomp: a kernel needs more than %zu B of LDS (FK %zu, gradient %zu, "
                     "update %zu)", kChompLdsMax, chomp_fk_lds(a), chomp_grad_lds(a), chomp_update_lds(a));

    // the loop's initial bookkeeping, the increments at zero, the trajectories
    ChompTrack* ht0 = (ChompTrack*)(h + pm.track);
    for (int b = 0; b < B; ++b) ht0[b] = ChompTrack{0, 0, 0, 0, -1, -1, -1, 0, 0.0};
    CH_TRY(c, hipMemcpyAsync(a.track, ht0, sizeof(ChompTrack) * B, hipMemcpyHostToDevice, s));
    CH_TRY(c, hipMemsetAsync(a.mirror, 0, sizeof(int) * B, s));
    CH_TRY(c, hipMemsetAsync(d + sm.sinc, 0, sm.scales + align256(sizeof(double) * B * J) - sm.sinc, s));
    const size_t JN = (size_t)J * N;
    if (trajectories) {
        std::memcpy(h + pm.traj, trajectories, sizeof(double) * B * JN);
        CH_TRY(c, hipMemcpyAsync(a.traj, h + pm.traj, sizeof(double) * B * JN, hipMemcpyHostToDevice, s));
    } else {
        for (int b = 0; b < B; ++b)
            CH_TRY(c, hipMemcpyAsync(a.traj + b * JN, e->d_theta, sizeof(double) * JN, hipMemcpyDeviceToDevice, s));
    }
    CH_TRY(c, hipMemcpyAsync(a.best_traj, a.traj, sizeof(double) * B * JN, hipMemcpyDeviceToDevice, s));
    // optimize()'s pass before the loop (:267-271)
    launch_chomp_limits(c->model, a, s);
    launch_chomp_fk(c->model, a, s);
    launch_chomp_vel(c->model, a, s);
    launch_chomp_track(c->model, a, s);
    c->launches = 4;
    CH_TRY(c, hipGetLastError());
    // the uploads' pinned sources are free again, and a failure of the pass is this call's
    CH_TRY(c, hipStreamSynchronize(s));
    c->args = a;
    c->B = B;
    c->iterations = 0;
    c->model_epoch = e->model_epoch;
    c->target_epoch = e->target_epoch;
    c->ready = true;
    return 0;
}

int chomp_optimize(stomp_chomp* c, stomp_stats* stats, double* costs, int stride, double* best)
{
    stomp_engine* e = c->e;
    hipStream_t s = e->stream;
    const int B = c->B, max_it = e->max_it;
    const size_t JN = (size_t)e->J * e->N;
    const TabMap tm(e->J, e->Nall, e->model.S, e->nseg);
    const PinMap pm(tm, (size_t)B, e->J, e->N, max_it);
    unsigned char* h = c->h_pin;
    c->launches = 0;
    int chunk = 0;
    for (int it = 0; it < max_it; ++chunk) {
        const int n = std::min(STOMP_GROUP_OPTIMIZE_CHUNK, max_it - it);
        for (int k = 0; k < n; ++k) enqueue_step(c, it + k, it + k);
        it += n;
        c->iterations = it;
        CH_TRY(c, hipGetLastError());
        CH_TRY(c, hipMemcpyAsync(h + pm.mirror[chunk & 1], c->args.mirror, sizeof(int) * B, hipMemcpyDeviceToHost, s));
        CH_TRY(c, hipEventRecord(c->ev[chunk & 1], s));
        if (chunk == 0) continue;
        // one chunk behind: the flags of the chunk before the one just enqueued
        CH_TRY(c, hipEventSynchronize(c->ev[(chunk - 1) & 1]));
        const int* flags = (const int*)(h + pm.mirror[(chunk - 1) & 1]);
        bool all = true;
        for (int b = 0; b < B; ++b) all = all && flags[b] != 0;
        if (all) break;
    }
    ChompTrack* tr = (ChompTrack*)(h + pm.track);
    CH_TRY(c, hipMemcpyAsync(tr, c->args.track, sizeof(ChompTrack) * B, hipMemcpyDeviceToHost, s));
    if (costs)
        CH_TRY(c, hipMemcpyAsync(h + pm.hist, c->args.hist, sizeof(double) * B * max_it, hipMemcpyDeviceToHost, s));
    if (best) CH_TRY(c, hipMemcpyAsync(h + pm.best, c->args.best_traj, sizeof(double) * B * JN, hipMemcpyDeviceToHost, s));
    CH_TRY(c, hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) {
        stomp_stats st{};
        st.iterations = tr[b].iterations;
        st.success = tr[b].success;
        st.success_iteration = tr[b].success_iteration;
        st.collision_success_iteration = tr[b].collision_success_iteration;
        st.last_improvement_iteration = tr[b].last_improvement_iteration;
        st.best_cost = tr[b].best;
        stats[b] = st;
        if (costs)
            std::memcpy(costs + (size_t)b * stride, (const double*)(h + pm.hist) + (size_t)b * max_it,
                        sizeof(double) * tr[b].iterations);
    }
    if (best) std::memcpy(best, h + pm.best, sizeof(double) * B * JN);
    return 0;
}

}  // namespace

extern "C" int stomp_chomp_create(stomp_engine* e, const stomp_chomp_params* p, stomp_chomp** out)
{
    // (up to here e is not touched)
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    if (!p || !out) return fail(nullptr, STOMP_E_INVALID, "chomp: null argument");
    if (p->struct_size != (int32_t)sizeof(stomp_chomp_params))
        return fail(nullptr, STOMP_E_INVALID, "chomp: struct_size is not sizeof(stomp_chomp_params)");
    if (!p->joint_update_limits) return fail(nullptr, STOMP_E_INVALID, "chomp: null joint_update_limits");
    const double vals[] = {p->learning_rate, p->smoothness_cost_weight, p->pseudo_inverse_ridge_factor,
                           p->field_bias[0], p->field_bias[1], p->field_bias[2]};
    for (double v : vals)
        if (!std::isfinite(v)) return fail(nullptr, STOMP_E_INVALID, "chomp: a parameter is not finite");
    for (int j = 0; j < e->J; ++j)
        if (!(std::isfinite(p->joint_update_limits[j]) && p->joint_update_limits[j] > 0.0))
            return fail(nullptr, STOMP_E_INVALID, "chomp: joint_update_limits[%d] is not positive and finite", j);
    if (p->use_hamiltonian_monte_carlo)
        return fail(nullptr, STOMP_E_UNSUPPORTED, "chomp: use_hamiltonian_monte_carlo is not supported (the reference's "
                    "HMC updates, stomp_optimizer.cpp:219-226, are not built)");
    if (e->world > 1 || e->gather)
        return fail(nullptr, STOMP_E_UNSUPPORTED, "chomp: a sharded engine (world_size > 1) is not supported");
    if (e->N > kChompMaxN)
        return fail(nullptr, STOMP_E_UNSUPPORTED, "chomp: N = %d is above %d", e->N, kChompMaxN);
    if (e->grid_n[0] < 3 || e->grid_n[1] < 3 || e->grid_n[2] < 3)
        return fail(nullptr, STOMP_E_UNSUPPORTED, "chomp: the field has fewer than 3 cells on an axis");
    stomp_chomp* c = new stomp_chomp();
    c->e = e;
    c->lr = p->learning_rate;
    c->w_smooth = p->smoothness_cost_weight;
    c->use_pinv = p->use_pseudo_inverse ? 1 : 0;
    c->ridge = p->pseudo_inverse_ridge_factor;
    for (int k = 0; k < 3; ++k) c->bias[k] = p->field_bias[k];
    c->upd.assign(p->joint_update_limits, p->joint_update_limits + e->J);
    *out = c;
    return 0;
}

extern "C" int stomp_chomp_reset(stomp_chomp* c, int32_t num_trajectories, const double* trajectories)
{
    if (!c) return fail(nullptr, STOMP_E_INVALID, "null chomp");
    if (num_trajectories < 1) return cfail(c, STOMP_E_INVALID, "chomp reset: num_trajectories %d is below 1", num_trajectories);
    const stomp_engine* e = c->e;
    if (trajectories) {
        const size_t n = (size_t)num_trajectories * e->J * e->N;
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(trajectories[i]))
                return cfail(c, STOMP_E_INVALID, "chomp reset: trajectory %zu has a value that is not finite",
                             i / ((size_t)e->J * e->N));
    }
    if (e->tracking) return cfail(c, STOMP_E_INVALID, "chomp reset: the engine is inside its optimize loop");
    DeviceGuard dg(e->device);
    return chomp_reset(c, num_trajectories, trajectories);
}

extern "C" int stomp_chomp_step(stomp_chomp* c, int32_t count)
{
    if (!c) return fail(nullptr, STOMP_E_INVALID, "null chomp");
    if (count < 0) return cfail(c, STOMP_E_INVALID, "chomp step: count %d is negative", count);
    if (int rc = check_live(c, "step")) return rc;
    DeviceGuard dg(c->e->device);
    c->launches = 0;
    for (int k = 0; k < count; ++k) enqueue_step(c, c->iterations + k, -1);
    c->iterations += count;
    CH_TRY(c, hipGetLastError());
    return 0;
}

extern "C" int stomp_chomp_synchronize(stomp_chomp* c)
{
    if (!c) return fail(nullptr, STOMP_E_INVALID, "null chomp");
    DeviceGuard dg(c->e->device);
    CH_TRY(c, hipStreamSynchronize(c->e->stream));
    return 0;
}

extern "C" int stomp_chomp_optimize(stomp_chomp* c, stomp_stats* stats, double* costs, int32_t costs_stride,
                                    double* best_trajectories)
{
    if (!c) return fail(nullptr, STOMP_E_INVALID, "null chomp");
    if (!stats) return cfail(c, STOMP_E_INVALID, "chomp optimize: null stats");
    if (costs && costs_stride < c->e->max_it)
        return cfail(c, STOMP_E_INVALID, "chomp optimize: costs_stride %d is below max_iterations %d", costs_stride,
                     c->e->max_it);
    if (int rc = check_live(c, "optimize")) return rc;
    if (c->iterations != 0)
        return cfail(c, STOMP_E_INVALID, "chomp optimize: %d iterations since the last reset; the loop starts from a "
                     "fresh reset", c->iterations);
    if (c->e->max_it < 1) return cfail(c, STOMP_E_INVALID, "chomp optimize: max_iterations is below 1");
    DeviceGuard dg(c->e->device);
    return chomp_optimize(c, stats, costs, costs_stride, best_trajectories);
}

extern "C" int stomp_chomp_get(stomp_chomp* c, const char* which, double* out)
{
    if (!c) return fail(nullptr, STOMP_E_INVALID, "null chomp");
    if (!which || !out) return cfail(c, STOMP_E_INVALID, "chomp get: null argument");
    if (int rc = check_live(c, "get")) return rc;
    const ChompArgs& a = c->args;
    const size_t B = a.B, J = a.J, N = a.N, S = a.S;
    struct Name {
        const char* name;
        const double* p;
        size_t n;
    };
    const Name names[] = {{"trajectory", a.traj, J * N}, {"smoothness_increments", a.sinc, J * N},
                          {"collision_increments", a.cinc, J * N}, {"final_increments", a.finc, J * N},
                          {"scales", a.scales, J}, {"distances", a.dist, N * S}, {"field_gradients", a.fgrad, N * S * 3},
                          {"potentials", a.pot, N * S}, {"potential_gradients", a.pgrad, N * S * 3},
                          {"velocities", a.vel, N * S * 3}, {"accelerations", a.acc, N * S * 3},
                          {"vel_mags", a.vmag, N * S}, {"joint_origins", a.jorg, N * J * 3},
                          {"joint_axes", a.jax, N * J * 3}, {"costs", a.wcost, N}, {"cost", a.cost, 1}};
    DeviceGuard dg(c->e->device);
    hipStream_t s = c->e->stream;
    for (const Name& nm : names)
        if (!std::strcmp(which, nm.name)) {
            if (nm.n) CH_TRY(c, hipMemcpyAsync(out, nm.p, sizeof(double) * B * nm.n, hipMemcpyDeviceToHost, s));
            CH_TRY(c, hipStreamSynchronize(s));
            return 0;
        }
    if (!std::strcmp(which, "collision_free")) {
        std::vector<int> cf(B);
        CH_TRY(c, hipMemcpyAsync(cf.data(), a.cf, sizeof(int) * B, hipMemcpyDeviceToHost, s));
        CH_TRY(c, hipStreamSynchronize(s));
        for (size_t b = 0; b < B; ++b) out[b] = cf[b] ? 1.0 : 0.0;
        return 0;
    }
    if (!std::strcmp(which, "sphere_positions")) {
        // the whole trajectory's centres: the model's padding centres around each descent's free block
        std::vector<double> pad((size_t)36 * S), pos(B * N * S * 3);
        if (S) {
            CH_TRY(c, hipMemcpyAsync(pad.data(), c->model.pad_pos, sizeof(double) * 36 * S, hipMemcpyDeviceToHost, s));
            CH_TRY(c, hipMemcpyAsync(pos.data(), a.pos, sizeof(double) * pos.size(), hipMemcpyDeviceToHost, s));
        }
        CH_TRY(c, hipStreamSynchronize(s));
        const size_t row = S * 3;
        for (size_t b = 0; b < B; ++b) {
            double* o = out + b * (N + 12) * row;
            std::copy(pad.begin(), pad.begin() + 6 * row, o);
            std::copy(pos.begin() + b * N * row, pos.begin() + (b + 1) * N * row, o + 6 * row);
            std::copy(pad.begin() + 6 * row, pad.end(), o + (6 + N) * row);
        }
        return 0;
    }
    return cfail(c, STOMP_E_INVALID, "chomp get: unknown name '%s'", which);
}

extern "C" int stomp_chomp_info(stomp_chomp* c, int64_t info[8])
{
    if (!c || !info) return fail(nullptr, STOMP_E_INVALID, "null argument");
    info[0] = c->B;
    info[1] = c->iterations;
    info[2] = c->launches;
    info[3] = c->allocs;
    info[4] = c->B ? (int64_t)chomp_fk_lds(c->args) : 0;
    info[5] = c->B ? (int64_t)chomp_grad_lds(c->args) : 0;
    info[6] = c->B ? (int64_t)chomp_update_lds(c->args) : 0;
    info[7] = c->B ? (int64_t)chomp_track_lds(c->args) : 0;
    return 0;
}

extern "C" const char* stomp_chomp_last_error(const stomp_chomp* c) { return c ? c->err.c_str() : ""; }

extern "C" void stomp_chomp_destroy(stomp_chomp* c)
{
    if (!c) return;
    if (c->d_state || c->d_tab || c->h_pin || c->ev[0] || c->ev[1]) {
        DeviceGuard dg(c->e->device);
        (void)hipStreamSynchronize(c->e->stream);   // no launch of this object is left reading its blocks
        if (c->d_state) hipFree(c->d_state);
        if (c->d_tab) hipFree(c->d_tab);
        if (c->h_pin) hipHostFree(c->h_pin);
        for (hipEvent_t ev : c->ev)
            if (ev) hipEventDestroy(ev);
    }
    delete c;
}
