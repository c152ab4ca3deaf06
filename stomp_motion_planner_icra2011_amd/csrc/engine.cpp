// engine.cpp -- host side of the C ABI in include/stomp_engine.h: the iteration and the entry
// points on an engine (engine_internal.h lists the files beside this one).
//
// One stomp_engine = one planning problem resident on one device: setup matrices,
// distance field, rollout arrays and the policy theta live in HBM for the
// engine's lifetime; an iteration is a fixed sequence of kernel launches on the
// engine stream with no host synchronisation (stomp_engine_run), or with one
// 9-byte read-back (stomp_engine_iterate, the runSingleIteration contract).
#include "engine_internal.h"

#include <algorithm>

using namespace stomp;

namespace stomp {

thread_local std::string g_last_error;

int fail(stomp_engine* e, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (e) e->err = buf;
    g_last_error = buf;
    return code;
}

void release(stomp_engine* e)
{
    if (!e) return;
    if (e->stream) hipStreamSynchronize(e->stream);
    for (auto& v : e->evs) { hipEventDestroy(v.a); hipEventDestroy(v.b); }
    for (auto ev : e->pool) hipEventDestroy(ev);
    for (void* p : e->allocs) hipFree(p);
    if (e->h_total) hipHostFree(e->h_total);
    if (e->h_cf) hipHostFree(e->h_cf);
    if (e->h_track) hipHostFree(e->h_track);
    if (e->h_stall) hipHostFree(e->h_stall);
    if (e->h_rq) hipHostFree(e->h_rq);
    if (e->d_rq) hipFree(e->d_rq);
    if (e->h_qs) hipHostFree(e->h_qs);
    if (e->d_qs) hipFree(e->d_qs);
    for (hipEvent_t ev : e->q_ev)
        if (ev) hipEventDestroy(ev);
    for (auto& r : e->coll_ring)
        if (r.ev) hipEventDestroy(r.ev);
    comm_destroy(e);
    if (e->ev_ready) hipEventDestroy(e->ev_ready);
    if (e->ev_done) hipEventDestroy(e->ev_done);
    if (e->own_stream && e->stream) hipStreamDestroy(e->stream);
}

}  // namespace stomp

namespace {

void collect_timing(stomp_engine* e)
{
    if (e->evs.empty()) return;
    hipStreamSynchronize(e->stream);
    for (auto& v : e->evs) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, v.a, v.b);
        e->tot_ms[v.id] += ms;
        e->launches[v.id] += 1;
        e->pool.push_back(v.a);
        e->pool.push_back(v.b);
    }
    e->evs.clear();
}

// Task::execute of a launch's rollouts
void launch_rollouts(stomp_engine* e, const CostArgs& ca)
{
    DevModel& m = e->model;
    const int nro = ca.num_noisy + (ca.x_params ? 1 : 0);
    if (m.lean && m.nsaves > 0 && nro > m.sv_rows) {
        // an eval batch with more rollouts than the lean layout's saved-frame blocks: grow them (the
        // old blocks stay allocated until the engine is destroyed, launches before may use them).
        // Without the memory the engine takes the full layout, which is valid for every launch.
        void* q = nullptr;
        if (hipMalloc(&q, sizeof(double) * (size_t)nro * m.nsaves * 12 * m.N) == hipSuccess) {
            e->allocs.push_back(q);
            m.sv_glob = (double*)q;
            m.sv_rows = nro;
        } else {
            (void)hipGetLastError();
            m.lean = 0;
        }
    }
    launch_cost(m, ca, e->stream);
}

// the state-cost terms after the collision cost (k_terms), on the rollouts a k_rollout
// launch with these arguments evaluated; its trajectories must have been written
void launch_terms_for(stomp_engine* e, const CostArgs& ca, uint8_t* cs = nullptr)
{
    if (!e->terms_on) return;
    Timed tm(e, T_TERMS);
    TermsArgs ta{};
    ta.stop = e->d_stop;
    ta.traj = ca.traj_out; ta.state = ca.state_out; ta.total = ca.total_out; ta.num_noisy = ca.num_noisy;
    ta.cs = cs;
    if (ca.x_params) {
        ta.x_traj = ca.x_traj; ta.x_state = ca.x_state; ta.x_total = ca.x_total; ta.x_cs = e->d_cs;
    }
    launch_terms(e->terms, ta, e->stream);
}

// the optimize loop's bookkeeping for the noiseless rollout a launch with these arguments
// evaluated (its iteration_ is ca.x_member)
void track_noiseless(stomp_engine* e, const CostArgs& ca)
{
    if (!e->tracking || !ca.x_params) return;
    launch_track(e->d_track, ca.x_member, e->max_it_cf, e->d_total, e->d_cf, e->d_cs, e->d_opt_costs, e->d_last_traj,
                 e->d_best_traj, e->J * e->N, e->stream);
}

}  // namespace

namespace stomp {

// noiseless rollout of the current theta (policy_improvement_loop.cpp:180-182), alone
void launch_noiseless(stomp_engine* e, int member)
{
    CostArgs ca{};
    ca.stop = e->d_stop;
    ca.num_noisy = 0;
    set_noiseless(e, ca, member, true, e->Kr > 0);
    if (e->Kr > 0) ca.nz = noise_args(e, member + 1);   // it is also the extra rollout of the next reuse ranking
    {
        Timed tm(e, T_NOISELESS);
        launch_rollouts(e, ca);
    }
    launch_terms_for(e, ca);
    track_noiseless(e, ca);
}

// the reuse step: rank the previous rows and the extra (noiseless) rollout, copy the best K_r
// into rows K_gen.. of this iteration's set (the extra rollout's state costs must be evaluated)
int run_reuse(stomp_engine* e)
{
    Timed tm(e, T_REUSE);
    const int with_extra = e->extra_added ? 1 : 0;
    e->extra_added = false;
    if (e->world == 1) {
        if (int rc = launch_reuse(e->K, e->J, e->N, e->Kr, e->K_gen, with_extra, e->d_params_b, e->d_state_b, e->d_control_b,
                         e->d_params, e->d_noise, e->d_state, e->d_x_params, e->d_x_state, e->d_x_control, e->d_theta,
                         e->d_reuse_costs, e->d_reuse_count, e->d_stop, e->stream))
            return fail(e, STOMP_E_INVALID, rc == -1 ? "reuse: the source and destination rollout rows alias"
                                                     : "reuse: the cost rows of one candidate exceed the LDS");
        return 0;
    }
    const size_t slot = (size_t)e->Kr * ((size_t)e->J * e->N + e->N);
    launch_reuse_totals(e->K_loc, e->J, e->N, e->d_state_b, e->d_control_b, e->d_x_state, e->d_x_control,
                        e->d_tot_loc, e->d_tot_x, e->d_stop, e->stream);
    int rc = exchange_gather(e, e->d_tot_loc, e->d_tot_all, (size_t)e->K_loc);
    if (rc) return rc;
    launch_reuse_select(e->K, e->Kr, with_extra, e->d_tot_all, e->d_tot_x, e->d_sel, e->d_stop, e->stream);
    launch_reuse_pack(e->Kr, e->J, e->N, e->first, e->K_loc, e->d_sel, e->d_params_b, e->d_state_b, e->d_slot,
                      e->d_stop, e->stream);
    if ((rc = exchange_gather(e, e->d_slot, e->d_slot_all, slot))) return rc;
    launch_reuse_unpack(e->Kr, e->K_gen, e->J, e->N, e->first, e->K_loc, e->d_sel, e->d_slot_all, e->d_x_params,
                        e->d_x_state, e->d_theta, e->d_params, e->d_noise, e->d_state, e->d_stop, e->stream);
    return 0;
}

}  // namespace stomp

namespace {

// One runSingleIteration (policy_improvement_loop.cpp:143-202) enqueued on the engine stream.
// pipelined: the noiseless rollout of the updated theta is not launched here but evaluated by
// the next iteration's rollout-cost launch (extra workgroup) or by flush_noiseless().
int enqueue_iteration(stomp_engine* e, int it, bool pipelined)
{
    if (e->comm_aborted) return fail(e, STOMP_E_COMM, "%s", e->comm_msg.c_str());
    e->cur_it = it;
    // setRolloutCosts with the loop's weight (policy_improvement_loop.cpp:173): every row of this
    // iteration is priced with it, and a stomp_pi_add_extra_rollouts after it prices with it too
    e->pi_weight = e->w_smooth;
    const int member = it - 1;
    const bool fused = e->J <= 16;   // rollout_project: at most four 4-joint column groups
    // With fused noise the reuse step runs after the rollout launch: the generated rows go to
    // the other row set, and the launch also evaluates the pending noiseless rollout that the
    // ranking needs (so K_r > 0 iterations pipeline like K_r = 0 ones).  Otherwise k_noise
    // makes every row before the launch and the reuse step has to come first.
    if (e->Kr > 0 && !fused) pipelined = false;
    const bool reuse = plan_generate(e);
    const bool reuse_late = reuse && fused;
    if (reuse && !reuse_late) {
        flush_noiseless(e);
        if (int rc = run_reuse(e)) return rc;
    }
    NoiseArgs na = noise_args(e, it);
    na.K_gen_global = e->K_gen;
    // generated rows [0, g1 - g0) of this shard: their noise is made by the rollout kernel
    // itself (fused), k_noise only projects and prices the reused rows after them
    const int g0 = e->first, g1 = std::min(e->first + e->K_loc, e->K_gen);
    const int num_gen = std::max(g1 - g0, 0);
    if (fused) na.row_begin = e->gather ? e->rows : num_gen;
    // the generated rows' eps and M eps come from the pregen buffers (every local row, or with
    // reuse on one device the rows before the reused ones)
    const bool pre = fused && e->pre_on && (num_gen == e->K_loc || (e->Kr > 0 && num_gen > 0));
    if (e->gather && !pre) return fail(e, STOMP_E_INVALID, "gather mode needs the pregen rows");
    // outside the optimize loop and without reuse the rows stay in the pregen buffer: the weights
    // read eps there and nothing else needs the noise / params rows on the device (the reuse step
    // ranks and copies the previous rows, so with K_r > 0 they are written).  The optimize loop
    // keeps the copies: after its stop the pregen blocks of the iterations enqueued past it still
    // overwrite the buffers.
    const bool rows_pre = pre && !e->tracking && e->Kr == 0;
    na.rows_in_pre = rows_pre ? 1 : 0;
    if (!rows_pre) e->rows_in_pre = false;
    if (pre) {
        if (e->pre_it != it) {   // not made ahead by the previous iteration's launches
            Timed tm(e, T_PREGEN);
            launch_pregen(pregen_args(e, it), e->rows, e->stream);
        }
        e->pre_it = -1;
    }
    if (na.row_begin < na.K_loc && !reuse_late) {
        Timed tm(e, T_NOISE);
        launch_noise(na, e->stream);
    }
    // the candidates priced by the rollout launch (launch_reuse_pick) when its blocks still fit
    // the CUs beside the rollouts, pregen and totals blocks (more pricing blocks than idle CUs
    // would lengthen the launch)
    const int spec_nro = num_gen + (e->pending_member >= 0 ? 1 : 0);
    const int spec_extra = (pre ? e->rows : 0) + e->K + (e->K + 1);
    const bool spec = reuse_late && e->spec_on && !e->x_foreign && e->world == 1 && launch_reuse_pick_ok(na, e->K, e->Kr) &&
                      spec_nro + spec_extra <= e->model.cus &&
                      rollout_split_pieces(e->model, spec_nro, spec_extra, true) > 0;
    // Task::execute for the generated rollouts of this shard (+ the pending noiseless rollout)
    {
        CostArgs ca{};
        ca.stop = e->d_stop;
        ca.fused_noise = pre ? 2 : (fused ? 1 : 0);
        ca.nz = na;
        ca.params = e->d_params; ca.stride = (long long)e->J * e->N; ca.num_noisy = num_gen;
        ca.member = member; ca.state_out = e->d_state;
        if (pre) {
            ca.pre_rows = e->rows;
            ca.pre_next = pregen_args(e, it + 1);
            ca.ctl_by_pre = 1;
            ca.ctl_rows = e->Kr > 0 ? num_gen : e->rows;   // the reused rows are priced by k_noise
            ca.row0 = e->row0;
            ca.state_out = e->d_state + (size_t)e->row0 * e->N;
            e->pre_it = it + 1;
        }
        if (reuse_late && e->world == 1 && launch_reuse_rows_ok(na, e->K, e->Kr)) {
            // the reuse candidates' totals (the previous rows, complete) made beside the rollouts
            ca.tot_rows = e->K;
            ca.tot_state = e->d_state_b; ca.tot_control = e->d_control_b; ca.tot_out = e->d_reuse_costs;
            if (spec) {
                // and every candidate re-based on theta and priced, so that the reuse step only
                // ranks and copies
                ca.spec_rows = e->K + 1;
                ca.spec_src = e->d_params_b;
                ca.spec_params = e->d_spec_params; ca.spec_noise = e->d_spec_noise; ca.spec_ctl = e->d_spec_ctl;
            }
        }
        if (e->terms_on) ca.traj_out = e->d_terms_traj;
        if (e->pending_member >= 0) {
            // the pipelined noiseless rollout's costs.sum() and collision flag are read only by
            // the optimize loop's bookkeeping (k_track); stomp_engine_iterate and the flush
            // evaluate their own, so without tracking the launch skips them
            set_noiseless(e, ca, e->pending_member, e->tracking, e->Kr > 0);
            e->pending_member = -1;
        }
        {
            Timed tm(e, T_COST);
            launch_rollouts(e, ca);
        }
        if (rows_pre) {
            e->rows_in_pre = true;
            e->rows_eps = na.pre_eps;
        }
        launch_terms_for(e, ca);
        // before this iteration's weights / update: a break decided on the previous
        // iteration's noiseless rollout leaves theta where the reference leaves it
        track_noiseless(e, ca);
    }
    if (e->gather)
        if (int rc = exchange_state(e)) return rc;
    // the reuse step folded into the one-wave-per-column weights (launch_weights_pick)
    ReuseArgs pick_ra{};
    bool pick_in_weights = false;
    if (reuse_late) {
        // the previous rows and the extra rollout (evaluated just now) ranked; the reused rows'
        // projection and control costs after them.  On one device the candidates' totals are
        // made by k_reuse and the reused rows' kernel ranks, copies and prices each row itself
        if (e->world == 1 && launch_reuse_rows_ok(na, e->K, e->Kr)) {
            ReuseArgs ra{};
            ra.K = e->K; ra.Kr = e->Kr; ra.K_gen = e->K_gen; ra.with_extra = e->extra_added ? 1 : 0;
            e->extra_added = false;
            ra.costs = e->d_reuse_costs;
            ra.src_params = e->d_params_b; ra.src_state = e->d_state_b;
            ra.x_params = e->d_x_params; ra.x_state = e->d_x_state; ra.x_control = e->d_x_control;
            ra.state = e->d_state;
            Timed tm(e, T_NOISE);
            if (spec) {
                ra.spec_params = e->d_spec_params; ra.spec_noise = e->d_spec_noise; ra.spec_ctl = e->d_spec_ctl;
                // (launch_weights_pick_ok decides at the weights launch; otherwise k_reuse_pick runs there)
                if (e->pick_fuse && !e->split_modes && !e->use_cum) {
                    pick_ra = ra;
                    pick_in_weights = true;
                } else {
                    launch_reuse_pick(na, ra, e->stream);
                }
            } else {
                launch_reuse_rows(na, ra, e->stream);
            }
        } else {
            if (int rc = run_reuse(e)) return rc;
            if (na.row_begin < na.K_loc) {
                Timed tm(e, T_NOISE);
                launch_noise(na, e->stream);
            }
        }
    }
    WeightArgs wa = weight_args(e, e->rows, rows_pre ? na.pre_eps : e->d_noise);
    wa.use_cumulative = e->use_cum;
    wa.cum = e->use_cum ? e->d_cum : nullptr;
    wa.mm = e->d_mm; wa.psum_part = e->d_psum_part; wa.psum_all = e->d_psum_all; wa.u_part = e->d_u_part;
    {
        Timed tm(e, T_WEIGHTS);
        if (e->use_cum) launch_cumulative(wa, e->d_cum, e->stream);
        if (!e->split_modes) {
            wa.mode = W_FUSED;
            if (pick_in_weights && launch_weights_pick_ok(wa, pick_ra)) {
                launch_weights_pick(wa, pick_ra, na.params, na.noise, na.control, e->stream);
            } else {
                if (pick_in_weights) launch_reuse_pick(na, pick_ra, e->stream);
                launch_weights(wa, e->stream);
            }
        } else {
            // the sharded decomposition; with one rank (debug hook) the all-reduce is the
            // identity and the all-gathers are device copies
            const size_t JN = (size_t)e->J * e->N;
            const size_t nb_loc = (size_t)e->K_loc / kSumBlock;
            wa.mode = W_MINMAX;
            launch_weights(wa, e->stream);
            int rc = exchange_max(e, e->d_mm, 2 * JN);
            if (rc) return rc;
            wa.mode = W_PSUM;
            launch_weights(wa, e->stream);
            if ((rc = exchange_gather(e, e->d_psum_part, e->d_psum_all, nb_loc * JN))) return rc;
            wa.mode = W_USUM;
            launch_weights(wa, e->stream);
            if ((rc = exchange_gather(e, e->d_u_part, e->d_u_all, nb_loc * JN))) return rc;
        }
    }
    {
        Timed tm(e, T_UPDATE);
        launch_update(e->J, e->N, e->d_MT, e->d_u, e->split_modes ? e->d_u_all : nullptr, e->K / kSumBlock,
                      e->d_theta, e->d_stop, e->stream);
    }
    if (pipelined) {
        e->pending_member = member;
    } else {
        launch_noiseless(e, member);
    }
    if (e->Kr > 0) {
        // addExtraRollouts (policy_improvement.cpp:443-462): params = theta, noise = 0 — the
        // noiseless rollout of theta, whose workgroup (this iteration's noiseless launch, or the
        // next rollout launch's extra workgroup) also writes the extra rollout's params / noise /
        // control rows (x_ctl) before the next reuse ranking reads them
        e->extra_added = true;
    }
    e->x_foreign = false;   // the extra rollout is this iteration's noiseless rollout of theta
    hipError_t st = hipGetLastError();
    if (st != hipSuccess)
        return fail(e, STOMP_E_DEVICE, "kernel launch failed: %s%s%s", hipGetErrorString(st),
                    lds_opt_in_error()[0] ? "; " : "", lds_opt_in_error());
    return 0;
}

}  // namespace

extern "C" {

const char* stomp_last_error(void) { return g_last_error.c_str(); }

const char* stomp_engine_last_error(const stomp_engine* e) { return e ? e->err.c_str() : g_last_error.c_str(); }
// stomp_engine_source_hash: in the object _build.py generates at link time (build/source_hash.cpp)

void stomp_engine_destroy(stomp_engine* e)
{
    if (!e) return;
    DeviceGuard dg(e->device);
    release(e);
    delete e;
}

int stomp_engine_refresh_field(stomp_engine* e)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    if (!e->d_sdf_caller)
        return fail(e, STOMP_E_UNSUPPORTED, "the distance field was uploaded from the host at creation (data_on_device = 0)");
    ++e->target_epoch;
    if (!e->model.brick) return 0;   // read in place
    DeviceGuard dg(e->device);
    launch_sdf_bricks(e->d_sdf_caller, e->d_sdf, e->grid_n[0], e->grid_n[1], e->grid_n[2], e->stream);
    HIP_TRY(e, hipGetLastError());
    return 0;
}

int stomp_engine_get_theta(stomp_engine* e, double* theta)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    DeviceGuard dg(e->device);
    HIP_TRY(e, hipMemcpyAsync(theta, e->d_theta, sizeof(double) * e->J * e->N, hipMemcpyDeviceToHost, e->stream));
    SYNC_TRY(e);
    return 0;
}

int stomp_engine_set_theta(stomp_engine* e, const double* theta)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    DeviceGuard dg(e->device);
    flush_noiseless(e);   // a pending noiseless rollout belongs to the theta being replaced
    HIP_TRY(e, hipMemcpyAsync(e->d_theta, theta, sizeof(double) * e->J * e->N, hipMemcpyHostToDevice, e->stream));
    SYNC_TRY(e);
    e->x_foreign = true;   // the extra rollout keeps the parameters it was added with
    return 0;
}

int stomp_engine_iterate(stomp_engine* e, int32_t it, stomp_iter_out* out)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    DeviceGuard dg(e->device);
    flush_noiseless(e);
    int rc = enqueue_iteration(e, it, false);
    if (rc) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->h_total, e->d_total, sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipMemcpyAsync(e->h_cf, e->d_cf, 1, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipMemcpyAsync(e->h_cf + 1, e->d_cs, 1, hipMemcpyDeviceToHost, e->stream));
    SYNC_TRY(e);
    if (out) {
        out->cost = *e->h_total;
        out->collision_free = e->h_cf[0];
        out->constraints_satisfied = e->h_cf[1];
    }
    return 0;
}

int stomp_engine_run(stomp_engine* e, int32_t first_iteration, int32_t count)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    DeviceGuard dg(e->device);
    // the last iteration's noiseless rollout stays pending: it rides in the next rollout
    // launch, or is flushed by synchronize, iterate, set_theta and the trajectory reads
    for (int i = 0; i < count; ++i) {
        int rc = enqueue_iteration(e, first_iteration + i, true);
        if (rc) return rc;
    }
    return 0;
}

int stomp_engine_synchronize(stomp_engine* e)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    DeviceGuard dg(e->device);
    flush_noiseless(e);
    SYNC_TRY(e);
    return 0;
}

int stomp_engine_eval(stomp_engine* e, const double* params, int32_t num, double* costs, uint8_t* collision_free,
                      double* traj_out, int32_t iteration_member, uint8_t* constraints_satisfied)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    DeviceGuard dg(e->device);
    if (num <= 0) return 0;
    const size_t JN = (size_t)e->J * e->N;
    if (num > e->eval_cap) {
        for (void* p : {(void*)e->d_eval_params, (void*)e->d_eval_costs, (void*)e->d_eval_traj, (void*)e->d_eval_cf,
                        (void*)e->d_eval_cs}) {
            if (!p) continue;
            hipFree(p);
            e->allocs.erase(std::remove(e->allocs.begin(), e->allocs.end(), p), e->allocs.end());
        }
        int rc;
        if ((rc = dev_alloc(e, &e->d_eval_params, num * JN))) return rc;
        if ((rc = dev_alloc(e, &e->d_eval_costs, (size_t)num * e->N))) return rc;
        if ((rc = dev_alloc(e, &e->d_eval_traj, num * JN))) return rc;
        if ((rc = dev_alloc(e, &e->d_eval_cf, (size_t)num))) return rc;
        if ((rc = dev_alloc(e, &e->d_eval_cs, (size_t)num))) return rc;
        e->eval_cap = num;
    }
    HIP_TRY(e, hipMemcpyAsync(e->d_eval_params, params, sizeof(double) * num * JN, hipMemcpyHostToDevice, e->stream));
    CostArgs ca{};
    ca.params = e->d_eval_params; ca.stride = (long long)JN; ca.num_noisy = num; ca.member = iteration_member;
    ca.state_out = e->d_eval_costs; ca.cf_out = e->d_eval_cf;
    ca.traj_out = (traj_out || e->terms_on) ? e->d_eval_traj : nullptr;
    {
        Timed tm(e, T_COST);
        launch_rollouts(e, ca);
    }
    if (constraints_satisfied && !e->terms_on) HIP_TRY(e, hipMemsetAsync(e->d_eval_cs, 1, (size_t)num, e->stream));
    launch_terms_for(e, ca, e->d_eval_cs);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, hipMemcpyAsync(costs, e->d_eval_costs, sizeof(double) * num * e->N, hipMemcpyDeviceToHost, e->stream));
    if (collision_free)
        HIP_TRY(e, hipMemcpyAsync(collision_free, e->d_eval_cf, num, hipMemcpyDeviceToHost, e->stream));
    if (constraints_satisfied)
        HIP_TRY(e, hipMemcpyAsync(constraints_satisfied, e->d_eval_cs, num, hipMemcpyDeviceToHost, e->stream));
    if (traj_out)
        HIP_TRY(e, hipMemcpyAsync(traj_out, e->d_eval_traj, sizeof(double) * num * JN, hipMemcpyDeviceToHost, e->stream));
    SYNC_TRY(e);
    return 0;
}

// StompOptimizer::optimize loop (stomp_optimizer.cpp:284-359), device-resident: every iteration is
// followed by k_track, which keeps the loop's bookkeeping in HBM and sets the stop flag when the
// reference loop would break; all later launches of the loop then return at once.  The host
// enqueues iterations in chunks, one chunk ahead of the stop flag it reads back, so the stream
// never waits on the host.
int stomp_engine_optimize(stomp_engine* e, stomp_stats* st, double* costs_per_it)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    DeviceGuard dg(e->device);
    materialize_rows(e);
    flush_noiseless(e);
    DevTrack init{};
    init.stop = 0; init.cfi = 0; init.iterations = 0; init.success = 0;
    init.success_iteration = -1; init.collision_success_iteration = -1; init.last_improvement_iteration = -1;
    init.best = 0.0;
    e->h_track[3] = init;
    HIP_TRY(e, hipMemcpyAsync(e->d_track, &e->h_track[3], sizeof(DevTrack), hipMemcpyHostToDevice, e->stream));
    launch_track_start(e->d_track, e->stream);   // stomp_optimizer.cpp:251 start_time
    const int max_it = e->max_it;
    // host-side generateRollouts state after each iteration, to restore the one the device stopped at
    struct HostState { bool reused_next, extra_added; int row_set; };
    std::vector<HostState> after((size_t)std::max(max_it, 1));
    const int chunk = 8;
    int next = 0, checked = 0;
    hipEvent_t ev[2] = {get_event(e), get_event(e)};
    int slot_end[2] = {0, 0};
    int inflight = 0, head = 0;
    auto enqueue_chunk = [&](int slot) -> int {
        const int end = std::min(next + chunk, max_it);
        for (; next < end; ++next) {
            // K_r = 0: the noiseless rollout of iteration next rides in the next iteration's
            // rollout launch (pipelined), its k_track right after that launch
            int rc = enqueue_iteration(e, next + 1, true);
            if (rc) return rc;
            after[next] = {e->reused_next, e->extra_added, e->row_set};
        }
        HIP_TRY(e, hipMemcpyAsync(&e->h_track[slot], e->d_track, sizeof(DevTrack), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(e, hipEventRecord(ev[slot], e->stream));
        slot_end[slot] = next;
        return 0;
    };
    int rc = 0;
    bool stopped = false;
    e->tracking = true;
    while (!stopped && checked < max_it) {
        while (inflight < 2 && next < max_it) {
            if ((rc = enqueue_chunk((head + inflight) & 1))) break;
            ++inflight;
        }
        if (rc || inflight == 0) break;
        HIP_TRY(e, hipEventSynchronize(ev[head]));
        const DevTrack& h = e->h_track[head];
        checked = slot_end[head];
        stopped = h.stop != 0;
        head ^= 1;
        --inflight;
    }
    if (!rc) rc = flush_noiseless(e);   // the last iteration's noiseless rollout and its bookkeeping
    e->tracking = false;
    SYNC_TRY(e);
    e->pool.push_back(ev[0]);
    e->pool.push_back(ev[1]);
    if (rc) return rc;
    DevTrack& t = e->h_track[2];
    HIP_TRY(e, hipMemcpy(&t, e->d_track, sizeof(DevTrack), hipMemcpyDeviceToHost));
    if (t.iterations > 0) {
        e->reused_next = after[t.iterations - 1].reused_next;
        e->extra_added = after[t.iterations - 1].extra_added;
        if (e->row_set != after[t.iterations - 1].row_set) swap_row_sets(e);   // iterations past the stop were no-ops
    }
    if (costs_per_it && t.iterations > 0)
        HIP_TRY(e, hipMemcpy(costs_per_it, e->d_opt_costs, sizeof(double) * t.iterations, hipMemcpyDeviceToHost));
    // later launches (iterate / run / eval) are not gated
    HIP_TRY(e, hipMemsetAsync(e->d_track, 0, sizeof(int), e->stream));
    SYNC_TRY(e);
    if (st) *st = stats_from_track(e, t);
    return 0;
}

int stomp_engine_get_best_torques(stomp_engine* e, double* torques)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    DeviceGuard dg(e->device);
    if (!e->torque_stats && e->terms.nchain > 0)   // a valid chain that build_terms found too large
        return fail(e, STOMP_E_UNSUPPORTED, "torque statistics kernel needs %zu B of LDS", terms_lds_bytes(e->terms));
    if (!e->torque_stats) return fail(e, STOMP_E_UNSUPPORTED, "no torque chain (segment inertias not given)");
    flush_noiseless(e);
    HIP_TRY(e, hipMemsetAsync(e->d_tq_state, 0, sizeof(double) * e->N, e->stream));
    TermsArgs ta{};
    ta.traj = e->d_best_traj; ta.state = e->d_tq_state; ta.num_noisy = 1; ta.tq_out = e->d_tq;
    launch_terms(e->tq_model, ta, e->stream);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, hipMemcpyAsync(torques, e->d_tq, sizeof(double) * e->N, hipMemcpyDeviceToHost, e->stream));
    SYNC_TRY(e);
    return 0;
}

// ---------------------------------------------------------------- PolicyImprovement API
// policy_improvement.h:86-126 step by step on the engine's rollout set, for callers that run
// their own Task::execute between the steps (the fused stomp_engine_iterate does the same work
// in one launch sequence)
int stomp_pi_get_rollouts(stomp_engine* e, int32_t iteration, const double* noise_stddev, double* rollouts,
                          int32_t* num_generated)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    if (e->world > 1 || e->gather) return fail(e, STOMP_E_UNSUPPORTED, "the PolicyImprovement API is single-rank");
    DeviceGuard dg(e->device);
    materialize_rows(e);
    if (!noise_stddev) return fail(e, STOMP_E_INVALID, "null noise_stddev");
    flush_noiseless(e);
    if (int rc = begin_generate(e)) return rc;
    NoiseArgs na = noise_args(e, iteration);
    for (int d = 0; d < e->J; ++d) na.sigma.v[d] = noise_stddev[d];   // generateRollouts(noise_stddev)
    na.stop = nullptr;
    na.row_begin = 0;
    na.K_gen_global = e->K_gen;
    {
        Timed tm(e, T_NOISE);
        launch_noise(na, e->stream);
    }
    e->pi_weight = e->w_smooth;
    HIP_TRY(e, hipGetLastError());
    if (rollouts)
        HIP_TRY(e, hipMemcpyAsync(rollouts, e->d_params, sizeof(double) * e->K_gen * e->J * e->N,
                                  hipMemcpyDeviceToHost, e->stream));
    SYNC_TRY(e);
    if (num_generated) *num_generated = e->K_gen;
    return 0;
}

int stomp_pi_set_rollout_costs(stomp_engine* e, const double* costs, double control_cost_weight, double* totals)
{
    if (!e || !costs) return fail(e, STOMP_E_INVALID, "null argument");
    // before anything moves: a rank's row buffers hold K_loc rows, the copies below take K
    if (e->world > 1 || e->gather) return fail(e, STOMP_E_UNSUPPORTED, "the PolicyImprovement API is single-rank");
    DeviceGuard dg(e->device);
    materialize_rows(e);
    const int K = e->K, J = e->J, N = e->N;
    // state costs of the generated rows; reused rows keep theirs (policy_improvement.cpp:270-273)
    HIP_TRY(e, hipMemcpyAsync(e->d_state, costs, sizeof(double) * e->K_gen * N, hipMemcpyHostToDevice, e->stream));
    if (control_cost_weight != e->pi_weight) {
        // computeRolloutControlCosts with another weight (:264-266): every row's noise is kept,
        // its projection and control cost recomputed
        NoiseArgs na = noise_args(e, 1);
        na.stop = nullptr; na.row_begin = 0; na.K_gen_global = 0;
        for (int r = 0; r < 3; ++r) na.wr[r] = 0.5 * control_cost_weight * e->smooth[r];
        launch_noise(na, e->stream);
        e->pi_weight = control_cost_weight;
    }
    HIP_TRY(e, hipGetLastError());
    if (totals) {
        // Rollout::getCost (:149-156): state sum, then each joint's control sum
        std::vector<double> st((size_t)K * N), ct((size_t)K * J * N);
        HIP_TRY(e, hipMemcpyAsync(st.data(), e->d_state, sizeof(double) * st.size(), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(e, hipMemcpyAsync(ct.data(), e->d_control, sizeof(double) * ct.size(), hipMemcpyDeviceToHost, e->stream));
        SYNC_TRY(e);
        for (int r = 0; r < K; ++r) {
            const double* sr = st.data() + (size_t)r * N;
            double c = sr[0];
            for (int t = 1; t < N; ++t) c += sr[t];
            for (int d = 0; d < J; ++d) {
                const double* x = ct.data() + ((size_t)r * J + d) * N;
                double sd = x[0];
                for (int t = 1; t < N; ++t) sd += x[t];
                c += sd;
            }
            totals[r] = c;
        }
    }
    SYNC_TRY(e);
    return 0;
}

int stomp_pi_improve_policy(stomp_engine* e, double* updates)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    if (e->world > 1 || e->gather) return fail(e, STOMP_E_UNSUPPORTED, "the PolicyImprovement API is single-rank");
    DeviceGuard dg(e->device);
    materialize_rows(e);
    WeightArgs wa{};
    wa.stop = nullptr;
    wa.J = e->J; wa.N = e->N; wa.K_loc = e->K_loc; wa.use_cumulative = e->use_cum;
    wa.state = e->d_state; wa.control = e->d_control; wa.noise = e->d_noise;
    wa.cum = e->use_cum ? e->d_cum : nullptr; wa.prob = e->d_prob; wa.u = e->d_u;
    wa.tc = weights_tile(e->K_loc);
    wa.nb_total = e->K / kSumBlock;
    wa.mode = W_FUSED;
    {
        Timed tm(e, T_WEIGHTS);
        if (e->use_cum) launch_cumulative(wa, e->d_cum, e->stream);
        launch_weights(wa, e->stream);
    }
    {
        Timed tm(e, T_UPDATE);
        launch_update(e->J, e->N, e->d_MT, e->d_u, nullptr, e->K / kSumBlock, nullptr, nullptr, e->stream, e->d_delta);
    }
    HIP_TRY(e, hipGetLastError());
    if (updates)
        HIP_TRY(e, hipMemcpyAsync(updates, e->d_delta, sizeof(double) * e->J * e->N, hipMemcpyDeviceToHost, e->stream));
    SYNC_TRY(e);
    return 0;
}

// setNumRollouts with the engine's counts (policy_improvement.cpp:139-141): rollouts_reused_next_
// and extra_rollouts_added_ cleared
int stomp_pi_reset(stomp_engine* e)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    // on a rank the two flags decide which collectives the next iteration posts
    if (e->world > 1 || e->gather) return fail(e, STOMP_E_UNSUPPORTED, "the PolicyImprovement API is single-rank");
    DeviceGuard dg(e->device);
    SYNC_TRY(e);
    e->reused_next = false;
    e->extra_added = false;
    return 0;
}

int stomp_pi_add_extra_rollouts(stomp_engine* e, int32_t num, const double* params, const double* costs)
{
    if (!e || !params || !costs) return fail(e, STOMP_E_INVALID, "null argument");
    if (e->world > 1 || e->gather) return fail(e, STOMP_E_UNSUPPORTED, "the PolicyImprovement API is single-rank");
    DeviceGuard dg(e->device);
    materialize_rows(e);
    if (num != 1) return fail(e, STOMP_E_INVALID, "one extra rollout (the loop's noiseless rollout)");
    const int J = e->J, N = e->N;
    const size_t JN = (size_t)J * N;
    // copyParametersFromPolicy, then noise = parameters - theta (policy_improvement.cpp:446-449, 464-469)
    std::vector<double> th(JN), nz(JN);
    flush_noiseless(e);
    HIP_TRY(e, hipMemcpyAsync(th.data(), e->d_theta, sizeof(double) * JN, hipMemcpyDeviceToHost, e->stream));
    SYNC_TRY(e);
    for (size_t k = 0; k < JN; ++k) nz[k] = params[k] - th[k];
    HIP_TRY(e, hipMemcpyAsync(e->d_x_params, params, sizeof(double) * JN, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(e->d_x_noise, nz.data(), sizeof(double) * JN, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(e->d_x_state, costs, sizeof(double) * N, hipMemcpyHostToDevice, e->stream));
    // computeProjectedNoise + computeRolloutControlCosts of the extra row (:452-453)
    NoiseArgs xa = noise_args(e, 1);
    xa.stop = nullptr;
    xa.K_loc = 1; xa.first_global = 0; xa.K_gen_global = 0; xa.zero_noise = 0; xa.row_begin = 0;
    for (int r = 0; r < 3; ++r) xa.wr[r] = 0.5 * e->pi_weight * e->smooth[r];
    xa.params = e->d_x_params; xa.noise = e->d_x_noise; xa.control = e->d_x_control;
    launch_noise(xa, e->stream);
    HIP_TRY(e, hipGetLastError());
    SYNC_TRY(e);   // nz is a pageable host buffer
    e->extra_added = true;
    e->x_foreign = true;
    return 0;
}

int stomp_engine_get_best_trajectory(stomp_engine* e, double* traj)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    DeviceGuard dg(e->device);
    flush_noiseless(e);
    HIP_TRY(e, hipMemcpyAsync(traj, e->d_best_traj, sizeof(double) * e->J * e->N, hipMemcpyDeviceToHost, e->stream));
    SYNC_TRY(e);
    return 0;
}

int stomp_engine_get_last_trajectory(stomp_engine* e, double* traj)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    DeviceGuard dg(e->device);
    flush_noiseless(e);
    HIP_TRY(e, hipMemcpyAsync(traj, e->d_last_traj, sizeof(double) * e->J * e->N, hipMemcpyDeviceToHost, e->stream));
    SYNC_TRY(e);
    return 0;
}

int stomp_engine_get_rollouts(stomp_engine* e, const char* which, double* out)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    DeviceGuard dg(e->device);
    // this rank's rows (gather mode holds all K: its own start at row0)
    const size_t JN = (size_t)e->J * e->N, KJN = (size_t)e->K_loc * JN, o = (size_t)e->row0 * JN;
    const double* src = nullptr;
    size_t n = KJN;
    if (!std::strcmp(which, "params") || !std::strcmp(which, "noise")) materialize_rows(e);
    if (!std::strcmp(which, "params")) src = e->d_params + o;
    else if (!std::strcmp(which, "noise")) src = e->d_noise + o;
    else if (!std::strcmp(which, "control_costs")) src = e->d_control + o;
    else if (!std::strcmp(which, "probabilities")) src = e->d_prob + o;
    else if (!std::strcmp(which, "cumulative_costs")) {
        // the rows the last weights launch read (k_cumulative / k_cumulative_group)
        if (!e->use_cum) return fail(e, STOMP_E_INVALID, "the engine was created without use_cumulative_costs");
        src = e->d_cum + o;
    }
    else if (!std::strcmp(which, "state_costs")) { src = e->d_state + (size_t)e->row0 * e->N; n = (size_t)e->K_loc * e->N; }
    else if (!std::strncmp(which, "x_", 2)) {
        // the extra (noiseless) rollout of addExtraRollouts (policy_improvement.cpp:443-462);
        // x_state_costs is written by every noiseless rollout, the others only with reuse
        flush_noiseless(e);
        n = (size_t)e->J * e->N;
        if (!std::strcmp(which, "x_params")) src = e->d_x_params;
        else if (!std::strcmp(which, "x_noise")) src = e->d_x_noise;
        else if (!std::strcmp(which, "x_control_costs")) src = e->d_x_control;
        else if (!std::strcmp(which, "x_state_costs")) { src = e->d_x_state; n = (size_t)e->N; }
        else return fail(e, STOMP_E_INVALID, "unknown rollout field '%s'", which);
    }
    else return fail(e, STOMP_E_INVALID, "unknown rollout field '%s'", which);
    HIP_TRY(e, hipMemcpyAsync(out, src, n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    SYNC_TRY(e);
    return 0;
}

int stomp_engine_get_matrix(stomp_engine* e, const char* which, int32_t joint, double* out)
{
    const size_t NN = (size_t)e->N * e->N;
    if (!std::strcmp(which, "Rinv")) std::memcpy(out, e->su.Rinv.data(), NN * 8);
    else if (!std::strcmp(which, "L")) std::memcpy(out, e->su.L.data(), NN * 8);
    else if (!std::strcmp(which, "M")) std::memcpy(out, e->su.M.data(), NN * 8);
    else if (!std::strcmp(which, "R")) {
        // free block of the control-cost matrix (CovariantTrajectoryPolicy::getControlCosts)
        for (int i = 0; i < e->N; ++i)
            for (int k = 0; k < e->N; ++k)
                out[(size_t)i * e->N + k] = e->su.Rall[(size_t)(i + kPad) * e->Nall + k + kPad];
    } else if (which[0] == 'D' && which[1] >= '0' && which[1] <= '2' && which[2] == 0) {
        // policy differentiation matrix D_i (Nall x Nall), covariant_trajectory_policy.cpp:204-226
        const int r = which[1] - '0', A = e->Nall;
        std::memset(out, 0, sizeof(double) * A * A);
        for (int i = 0; i < A; ++i)
            for (int j = 0; j < kDiffRuleLength; ++j) {
                const int c = i + j - kDiffRuleLength / 2;
                if (c >= 0 && c < A) out[(size_t)i * A + c] = e->su.dcoef[r][j];
            }
    } else if (!std::strcmp(which, "Qinv")) {
        if (joint < 0 || joint >= e->J) return fail(e, STOMP_E_INVALID, "joint out of range");
        std::memcpy(out, e->su.Qinv.data() + (size_t)joint * NN, NN * 8);
    } else return fail(e, STOMP_E_INVALID, "unknown matrix '%s'", which);
    return 0;
}

int stomp_engine_get_pad_positions(stomp_engine* e, double* out)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    DeviceGuard dg(e->device);
    HIP_TRY(e, hipMemcpyAsync(out, e->d_pad_pos, sizeof(double) * 12 * e->S * 3, hipMemcpyDeviceToHost, e->stream));
    SYNC_TRY(e);
    return 0;
}

int stomp_engine_set_timing(stomp_engine* e, int32_t enable)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    DeviceGuard dg(e->device);
    collect_timing(e);
    e->timing = enable != 0;
    for (int i = 0; i < T_COUNT; ++i) { e->tot_ms[i] = 0; e->launches[i] = 0; }
    return 0;
}

int stomp_engine_get_timing(stomp_engine* e, const char* name, double* total_ms, int32_t* launches)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    DeviceGuard dg(e->device);
    collect_timing(e);
    double t = 0;
    int n = 0;
    bool found = false;
    for (int i = 0; i < T_COUNT; ++i)
        if (!std::strcmp(name, "all") || !std::strcmp(name, kTimerNames[i])) {
            t += e->tot_ms[i];
            n += e->launches[i];
            found = true;
        }
    if (!found) return fail(e, STOMP_E_INVALID, "unknown timer '%s'", name);
    if (total_ms) *total_ms = t;
    if (launches) *launches = n;
    return 0;
}

int stomp_engine_local_rollouts(stomp_engine* e, int32_t* first, int32_t* count)
{
    if (first) *first = e->first;
    if (count) *count = e->K_loc;
    return 0;
}

int stomp_engine_shard_mode(stomp_engine* e, int32_t* mode)
{
    if (!e || !mode) return fail(e, STOMP_E_INVALID, "null argument");
    *mode = e->world == 1 ? STOMP_SHARD_NONE : (e->gather ? STOMP_SHARD_GATHER : STOMP_SHARD_PARTIALS);
    return 0;
}

int stomp_engine_shard_info(stomp_engine* e, double* info)
{
    if (!e || !info) return fail(e, STOMP_E_INVALID, "null argument");
    for (int k = 0; k < 6; ++k) info[k] = e->shard_info[k];
    if (!e->calibrate) info[0] = e->world == 1 ? STOMP_SHARD_NONE : (e->gather ? STOMP_SHARD_GATHER : STOMP_SHARD_PARTIALS);
    return 0;
}

// ---------------------------------------------------------------- device utilities
int stomp_diff_rules(double* out)
{
    if (!out) return fail(nullptr, STOMP_E_INVALID, "null argument");
    std::memcpy(out, kDiffRules, sizeof(double) * kNumDiffRules * kDiffRuleLength);
    return 0;
}

int stomp_device_alloc(int32_t device, uint64_t bytes, void** out)
{
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, STOMP_E_DEVICE, "hipSetDevice(%d) failed", device);
    hipError_t st = hipMalloc(out, bytes ? bytes : 1);
    if (st != hipSuccess) return fail(nullptr, STOMP_E_DEVICE, "hipMalloc: %s", hipGetErrorString(st));
    return 0;
}

int stomp_device_free(void* p)
{
    hipError_t st = hipFree(p);
    return st == hipSuccess ? 0 : fail(nullptr, STOMP_E_DEVICE, "hipFree: %s", hipGetErrorString(st));
}

int stomp_device_copy_to_host(void* dst, const void* src, uint64_t bytes)
{
    hipError_t st = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    return st == hipSuccess ? 0 : fail(nullptr, STOMP_E_DEVICE, "hipMemcpy: %s", hipGetErrorString(st));
}

int stomp_device_count(int32_t* count)
{
    int n = 0;
    hipError_t st = hipGetDeviceCount(&n);
    *count = st == hipSuccess ? n : 0;
    return 0;
}

int stomp_stream_create(int32_t device, void** out)
{
    if (!out) return fail(nullptr, STOMP_E_INVALID, "null argument");
    DeviceGuard dg(device);
    hipStream_t s = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess)
        return fail(nullptr, STOMP_E_DEVICE, "hipStreamCreate failed");
    *out = (void*)s;
    return 0;
}

int stomp_stream_destroy(void* stream)
{
    if (stream && hipStreamDestroy((hipStream_t)stream) != hipSuccess)
        return fail(nullptr, STOMP_E_DEVICE, "hipStreamDestroy failed");
    return 0;
}

}  // extern "C"
