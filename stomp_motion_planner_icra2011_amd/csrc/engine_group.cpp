// engine_group.cpp -- engine groups (stomp_group_*).
// Several engines of one shape driven in lockstep by shared launches: per iteration one rollout
// launch covering every engine's rollout workgroups and pregen blocks, one weights launch and one
// update launch (k_rollout_group, k_weights_rows_group, k_update_group), so a batch of independent
// planning problems costs three dispatches per iteration instead of three per problem.  Each
// engine's results are the ones its own stomp_engine_run gives, bit for bit.
// One grouped step is described by a StepLaunch and issued by launch_step, the only place that
// knows the launches and their order: per iteration of stomp_group_run, per staged step of
// stomp_group_optimize (with the flush cohort and k_track_group, the bookkeeping of every engine,
// each stopping on its own), and for stomp_group_synchronize's flush.  stage_step writes a step's
// per-engine kernel arguments through an Arena over a pinned buffer and its device twin; a run or
// a chunk of steps is uploaded once.  What a group may hold adds launches to the step:
//   reused rollouts (one K_r for the group): the candidates' totals blocks in the rollout launch and
//     k_reuse_rows_group on the reusing iterations; the host keeps every engine's generateRollouts
//     state in step with the staged iterations and, after an optimize loop, puts back the state of
//     the iteration each engine stopped at
//   state-cost terms (stomp_group_create_with): k_terms_group after every grouped rollout launch
//     and flush, each engine with its own TermsModel (an engine without terms has no workgroup
//     that writes)
//   cumulative costs (stomp_group_create_flags): k_cumulative_group before the weights launch, in
//     its timed scope (an engine without has no workgroup that writes)
// stomp_group_retarget and stomp_group_retarget_requests put every engine of the group onto its next
// request in one launch and one read-back (group_retarget, over engine_retarget.cpp); the launch
// also writes the padding-collision flags of the group's own DevModel list, which the grouped
// launches of a run and a synchronize read, and rewrites the entries of a replaced model.
// The engines of a step need not be at one iteration: stage_step takes the iteration per engine, a
// StepLaunch carries the largest counts and the kernels take an engine's own from its arguments.
// stomp_group_run and stomp_group_optimize stage equal iterations; stomp_group_serve
// (engine_serve.cpp) runs the optimize loop's stages (engine_group.h) with every slot at its own.
#include "engine_group.h"

#include <algorithm>
#include <optional>

using namespace stomp;

namespace stomp {
int gfail(stomp_group* g, int code, const char* msg)
{
    g_last_error = msg;
    if (g) g->err = msg;
    return code;
}

namespace {
// the group's buffers are made with hipMalloc / hipHostMalloc and freed here, pointer reset
template <class... T>
void free_device(T*&... p) { ((p ? (void)hipFree(p) : (void)0, p = nullptr), ...); }
template <class... T>
void free_pinned(T*&... p) { ((p ? (void)hipHostFree(p) : (void)0, p = nullptr), ...); }
}  // namespace

// The launches of one grouped step, in the order everything depends on.  With timing on for the
// group's first engine, its timers hold the group's launches.
int launch_step(stomp_group* g, const StepLaunch& L)
{
    stomp_engine* e0 = g->e[0];
    hipStream_t s = g->stream;
    const int J = e0->J, N = e0->N, K = e0->K_loc;
    const DevModel& shape = e0->model;   // the engines of a group have one shape and one field layout
    int n = 0;
    if (L.nc > 0) {
        // every cohort engine's pending noiseless rollout in one launch (one workgroup per engine)
        std::optional<Timed> tm;
        if (L.time_flush) tm.emplace(e0, T_NOISELESS, s);
        launch_cost_group(shape, L.clists.models, L.ccs, L.nc, 1, 0, s);
        ++n;
    }
    if (L.nc > 0 && L.clists.nx > 0) {
        Timed tm(e0, T_TERMS, s);
        launch_terms_group(L.clists.tmodels, L.cxas, L.nc, 1, N, g->terms_lds, s);
        ++n;
    }
    if (L.nm > 0) {
        // (the grid by the step's largest counts; an engine's block roles are its own CostArgs')
        Timed tm(e0, T_COST, s);
        launch_cost_group(shape, L.lists.models, L.cas, L.nm, L.nro, K + L.ntot, s);
        ++n;
    }
    if (L.nm > 0 && L.lists.nx > 0) {
        // the state-cost terms of both rollout launches before the bookkeeping reads the noiseless
        // rollouts' totals and constraints-satisfied flags, the reuse ranking and the weights the rows
        Timed tm(e0, T_TERMS, s);
        launch_terms_group(L.lists.tmodels, L.xas, L.nm, L.nro, N, g->terms_lds, s);
        ++n;
    }
    // before this step's weights / update: a break decided on the previous iteration's noiseless
    // rollout leaves theta where the reference leaves it
    if (L.ntrack > 0) {
        launch_track_group(L.tas, L.ntrack, -1, J * N, s);
        ++n;
    }
    if (L.nm <= 0) return n;
    if (L.reuse) {
        // every engine's reuse step (an engine on its own records its reused rows' launch on this
        // timer too); after the bookkeeping, as the engine's own loop: a stopped engine's reused
        // rows stay the ones of the iteration it stopped at.  An engine of the step that does not
        // reuse (a serve loop's fresh slot) has an empty entry: no workgroup of it writes
        Timed tm(e0, T_NOISE, s);
        launch_reuse_rows_group(g->shape, L.ras, L.nm, e0->K, e0->Kr, s);
        ++n;
    }
    {
        // the cumulative rows of the engines that use them, on the control costs the reuse launch
        // re-priced, in the weights' scope as an engine's own launch_cumulative (the step's own
        // list: compacted, or a stopped engine a no-op at its flag)
        Timed tm(e0, T_WEIGHTS, s);
        if (g->ncum > 0) launch_cumulative_group(L.was, L.nm, J, N, K, s), ++n;
        launch_weights_group(L.was, L.nm, J, N, K, s);
        ++n;
    }
    {
        Timed tm(e0, T_UPDATE, s);
        launch_update_group(J, N, L.uas, L.nm, s);
        ++n;
    }
    return n;
}

namespace {
// one step's staged arrays over nm engines that run the iteration and nc of the flush cohort (the
// arrays a group has no use for are empty): the host side; L gets the device side and the counts
struct StepHost {
    CostArgs* cas; WeightArgs* was; UpdateArgs* uas; ReuseRowArgs* ras; TermsArgs* xas;
    CostArgs* ccs; TermsArgs* cxas; TrackArgs* tas;
};

StepHost take_step(Arena& a, const stomp_group* g, int nm, int nc, bool track, StepLaunch& L)
{
    const int terms = g->nterms > 0 ? 1 : 0, reuse = g->e[0]->Kr > 0 ? 1 : 0;
    L.nm = nm; L.nc = nc;
    return StepHost{a.take(nm, L.cas), a.take(nm, L.was), a.take(nm, L.uas), a.take(reuse * nm, L.ras),
                    a.take(terms * nm, L.xas), a.take(nc, L.ccs), a.take(terms * nc, L.cxas),
                    a.take(track ? nm + nc : 0, L.tas)};   // (stage_step fills L.ntrack of them)
}

// the model lists of a launch over the n engines `of`, staged (of == nullptr: measured only)
ModelLists take_models(Arena& a, const stomp_group* g, const int* of, int n)
{
    ModelLists l;
    DevModel* ms = a.take(n, l.models);
    TermsModel* xs = a.take(g->nterms > 0 ? n : 0, l.tmodels);
    if (a.overflowed() || !of) return l;
    for (int k = 0; k < n; ++k) ms[k] = g->e[of[k]]->model;
    for (int k = 0; k < n && g->nterms > 0; ++k) {
        xs[k] = g->e[of[k]]->terms;
        l.nx += g->e[of[k]]->terms_on ? 1 : 0;
    }
    return l;
}
}  // namespace

// the capacity one staged step needs, with `lists` its two launches' model lists too
size_t step_bytes(const stomp_group* g, int nm, int nc, bool track, bool lists)
{
    Arena measure;
    StepLaunch L;
    take_step(measure, g, nm, nc, track, L);
    if (lists) take_models(measure, g, nullptr, nm), take_models(measure, g, nullptr, nc);
    return measure.used();
}

namespace {

// h_args / d_args of at least `bytes` and h_args free again: the last upload has left it; a device
// buffer is freed once the stream's launches have read it
int reserve_args(stomp_group* g, size_t bytes)
{
    if (g->staged && hipEventSynchronize(g->staged) != hipSuccess)
        return gfail(g, STOMP_E_DEVICE, "group staging wait failed");
    if (bytes > g->h_cap) {
        free_pinned(g->h_args);
        g->h_cap = hipHostMalloc((void**)&g->h_args, bytes) == hipSuccess ? bytes : 0;
        if (!g->h_cap) return gfail(g, STOMP_E_DEVICE, "hipHostMalloc failed");
    }
    if (bytes > g->d_cap) {
        if (g->d_args) hipStreamSynchronize(g->stream);
        free_device(g->d_args);
        g->d_cap = hipMalloc(&g->d_args, bytes) == hipSuccess ? bytes : 0;
        if (!g->d_cap) return gfail(g, STOMP_E_DEVICE, "hipMalloc failed");
    }
    return 0;
}

// the arena's staged bytes on their way to the device; `done` (or none) recorded behind them
int upload(stomp_group* g, const Arena& a, hipEvent_t done)
{
    hipError_t err = a.used() ? hipMemcpyAsync(a.d, a.h, a.used(), hipMemcpyHostToDevice, g->stream) : hipSuccess;
    if (err == hipSuccess && done) err = hipEventRecord(done, g->stream);
    if (err != hipSuccess) return gfail(g, STOMP_E_DEVICE, "group argument upload failed");
    return 0;
}

// what one engine's staged iteration adds to the step's launches
struct StagedIteration {
    int nro;      // rollout workgroups (the generated rows and the pending noiseless rollout)
    int ntot;     // totals blocks (K on a reusing iteration)
    bool reuse;   // the grouped reuse launch has an entry of this engine
};

// One engine's arguments of iteration `it` in a group's step: enqueue_iteration's pipelined
// one-device path with pregen rows, arguments only.  The engine's generateRollouts state
// (plan_generate: K_gen, reused_next, the row-set swap; extra_added) advances as its own
// iteration advances it.  keep_in_pre: without reuse the rows stay in the pregen buffer (a run
// outside the optimize loop); with K_r > 0 they are written, the next reuse step ranks and copies
// them.  On a reusing iteration the rollout launch carries the K totals blocks of the previous
// rows and `rr` is the engine's entry of the grouped reuse launch (between the rollout and the
// weights launches); no candidates are priced ahead and no launch splits, the rows are the same
// bit for bit.
StagedIteration stage_iteration(stomp_engine* e, int it, bool keep_in_pre, CostArgs& ca_out, WeightArgs& wa_out,
                                UpdateArgs& ua_out, ReuseRowArgs* rr)
{
    const bool reuse = plan_generate(e);   // K_r = 0: every row generated
    NoiseArgs na = noise_args(e, it);
    na.K_gen_global = e->K_gen;
    na.row_begin = e->K_gen;   // the rows after the generated ones are the reuse launch's
    const bool rows_pre = keep_in_pre && e->Kr == 0;
    na.rows_in_pre = rows_pre ? 1 : 0;
    CostArgs ca{};
    ca.stop = e->d_stop;
    ca.fused_noise = 2;
    ca.nz = na;
    ca.params = e->d_params; ca.stride = (long long)e->J * e->N; ca.num_noisy = e->K_gen;
    ca.member = it - 1; ca.state_out = e->d_state;
    ca.pre_rows = e->K_loc;
    ca.pre_next = pregen_args(e, it + 1);
    // the grouped launch is throughput-bound: its rollout workgroups price their own rows
    // (pricing in the pregen blocks re-reads theta and eps: cfg5 55.7k vs 53.9-54.5k
    // problem-it/s)
    ca.ctl_by_pre = 0;
    e->pre_it = it + 1;
    if (reuse) {
        // the reuse candidates' totals (the previous rows, complete) made beside the rollouts
        ca.tot_rows = e->K;
        ca.tot_state = e->d_state_b; ca.tot_control = e->d_control_b; ca.tot_out = e->d_reuse_costs;
    }
    if (e->terms_on) ca.traj_out = e->d_terms_traj;
    if (e->pending_member >= 0) {
        // with K_r > 0 it is also the extra rollout of this iteration's ranking (priced with ca.nz)
        set_noiseless(e, ca, e->pending_member, true, e->Kr > 0);
        e->pending_member = -1;
    }
    if (rows_pre) {
        e->rows_in_pre = true;
        e->rows_eps = na.pre_eps;
    } else {
        e->rows_in_pre = false;
    }
    ca_out = ca;
    if (reuse) {
        ReuseArgs ra{};
        ra.K = e->K; ra.Kr = e->Kr; ra.K_gen = e->K_gen; ra.with_extra = e->extra_added ? 1 : 0;
        e->extra_added = false;
        ra.costs = e->d_reuse_costs;
        ra.src_params = e->d_params_b; ra.src_state = e->d_state_b;
        ra.x_params = e->d_x_params; ra.x_state = e->d_x_state; ra.x_control = e->d_x_control;
        ra.state = e->d_state;
        rr->nz = na;
        rr->ra = ra;
    } else if (rr) {
        // no reuse in this iteration (the generate-all one): with neighbours that reuse in the same
        // step the engine's entry of the grouped reuse launch is empty (ra.K == 0: no workgroup writes)
        *rr = ReuseRowArgs{};
    }
    WeightArgs wa = weight_args(e, e->K_loc, rows_pre ? na.pre_eps : e->d_noise);
    wa.mode = W_FUSED;
    // enqueue_iteration's: the grouped cumulative launch makes the rows the weights read
    wa.use_cumulative = e->use_cum;
    wa.cum = e->use_cum ? e->d_cum : nullptr;
    wa_out = wa;
    ua_out = UpdateArgs{e->d_MT, e->d_u, e->d_theta, e->d_stop};
    e->pending_member = it - 1;
    if (e->Kr > 0) e->extra_added = true;   // addExtraRollouts: the noiseless rollout pending now
    e->x_foreign = false;
    e->pi_weight = e->w_smooth;   // (enqueue_iteration's)
    return StagedIteration{ca.num_noisy + (ca.x_params ? 1 : 0), ca.tot_rows, reuse};
}

// an engine's pending noiseless rollout alone in a grouped launch (launch_noiseless' arguments):
// with K_r > 0 its workgroup also writes the extra rollout's rows of the next reuse ranking
CostArgs noiseless_args(stomp_engine* e)
{
    CostArgs ca{};
    ca.stop = e->d_stop;
    ca.num_noisy = 0;
    if (e->terms_on) ca.traj_out = e->d_terms_traj;
    set_noiseless(e, ca, e->pending_member, true, e->Kr > 0);
    if (e->Kr > 0) ca.nz = noise_args(e, e->pending_member + 1);
    e->pending_member = -1;
    return ca;
}

// the engine's entry of the grouped terms launch after a grouped rollout launch with its
// arguments `ca` (launch_terms_for's arguments); an engine without terms gets an entry of no
// rollouts: none of its rows is touched
TermsArgs terms_args(const stomp_engine* e, const CostArgs& ca)
{
    TermsArgs ta{};
    if (!e->terms_on) return ta;
    ta.stop = e->d_stop;
    ta.traj = ca.traj_out; ta.state = ca.state_out; ta.total = ca.total_out; ta.num_noisy = ca.num_noisy;
    if (ca.x_params) {
        ta.x_traj = ca.x_traj; ta.x_state = ca.x_state; ta.x_total = ca.x_total; ta.x_cs = e->d_cs;
    }
    return ta;
}

// d_models' padding-collision flags brought up to the engines' own (changed by a
// stomp_engine_retarget on a member): rare, so a wait and a blocking 4-byte copy per changed entry
int sync_model_flags(stomp_group* g)
{
    for (size_t p = 0; p < g->e.size(); ++p) {
        if (g->pad_flags[p] == g->e[p]->pad_collision) continue;
        const int f = g->e[p]->pad_collision;
        if (hipStreamSynchronize(g->stream) != hipSuccess ||
            hipMemcpy(&g->d_models[p].pad_collision, &f, sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
            return gfail(g, STOMP_E_DEVICE, "group model refresh failed");
        g->pad_flags[p] = f;
    }
    return 0;
}

// An engine whose model stomp_engine_retarget_request replaced on its own: the group's lists
// (d_models, d_tmodels, nterms, terms_lds) still describe the old one.  Refused before anything is
// touched; stomp_group_retarget_requests brings the group back in step.
}  // namespace
int check_epochs(stomp_group* g)
{
    for (size_t p = 0; p < g->e.size(); ++p)
        if (g->epochs[p] != g->e[p]->model_epoch) {
            char buf[200];
            snprintf(buf, sizeof buf, "engine %d of the group changed its model on its own (stomp_engine_retarget_request): "
                                      "stomp_group_retarget_requests brings the group back in step", (int)p);
            return gfail(g, STOMP_E_INVALID, buf);
        }
    return 0;
}
namespace {

// what stomp_group_create_flags tells an engine the group does not take, by what the group accepts
const char* refusal_text(bool state_terms, bool cumulative)
{
    if (state_terms && cumulative) return "groups run single-device engines of at most 16 joints";
    if (cumulative) return "groups run single-device engines of at most 16 joints without state-cost terms";
    if (state_terms) return "groups run single-device engines of at most 16 joints without cumulative costs";
    return "groups run single-device engines of at most 16 joints without state-cost terms or cumulative costs";
}

// What both group retarget calls do once their arguments are checked: every engine onto its
// request (none with a null start or goal) in one upload, one launch and one read-back; every engine
// leaves in the freshly created iteration state, whichever iteration its optimize loop stopped at.
int group_retarget(stomp_group* g, const stomp_request* rs)
{
    const int P = (int)g->e.size();
    // host only: before any engine or device is touched
    for (int p = 0; p < P; ++p)
        if (int rc = request_validate(g->e[p], &rs[p], p)) return gfail(g, rc, std::string(g_last_error).c_str());
    // (the plans ask the rollout kernels' attributes of the current device: the group's)
    DeviceGuard dg(g->device);
    std::vector<ModelPlan> plans(P);
    for (int p = 0; p < P; ++p)
        if (int rc = request_plan(g->e[p], &rs[p], plans[p])) return gfail(g, rc, std::string(g_last_error).c_str());
    // stomp_group_create_flags' shape rule and accept rule on the planned models
    const DevModel& m0 = plans[0].m;
    const size_t lds0 = rollout_lds_bytes(m0, m0.pad_lds);
    int nterms = 0;
    size_t terms_lds = 0;
    bool behind = false;   // an engine's model was replaced on its own: the lists are rewritten whatever the requests keep
    for (int p = 0; p < P; ++p) {
        const DevModel& m = plans[p].m;
        if (m.S != m0.S || rollout_lds_bytes(m, m.pad_lds) != lds0 || m.pad_lds != m0.pad_lds || m.lean != m0.lean)
            return gfail(g, STOMP_E_INVALID,
                         "the engines of a group have one shape (J, N, K, K_r, spheres, model, field layout)");
        if (plans[p].terms_on && !g->state_terms)
            return gfail(g, STOMP_E_UNSUPPORTED, refusal_text(false, g->ncum > 0));
        behind = behind || g->epochs[p] != g->e[p]->model_epoch;
        if (!plans[p].terms_on) continue;
        ++nterms;
        terms_lds = std::max(terms_lds, terms_lds_bytes(plans[p].terms));
    }
    const size_t cap = g->rq_cap;
    if (!reserve_stage(&g->h_rq, &g->d_rq, &g->rq_cap, request_stage_bytes(g->e.data(), P, plans)))
        return gfail(g, STOMP_E_DEVICE, "group retarget allocation failed");
    if (g->rq_cap != cap)
        for (stomp_engine* e : g->e) e->rq_allocs += 2;
    // the launch rewrites the group's own entries of a replaced model, so nothing staged from the
    // old models outlives this call
    if (int rc = request_engines(g->e.data(), P, rs, plans, g->h_rq, g->d_rq, g->d_models, g->d_tmodels, behind))
        return gfail(g, rc, std::string(g_last_error).c_str());
    g->nterms = nterms;
    g->terms_lds = terms_lds;
    for (int p = 0; p < P; ++p) {
        g->pad_flags[p] = g->e[p]->pad_collision;
        g->epochs[p] = g->e[p]->model_epoch;
    }
    return 0;
}

}  // namespace

// engine p's bookkeeping arguments; it: the iteration index of a launch's entry (negative: the
// launch's own, as the start and clear launches leave it)
TrackArgs track_args(const stomp_group* g, int p, int it)
{
    const stomp_engine* e = g->e[p];
    return TrackArgs{e->d_track, e->d_total, e->d_cf, e->d_cs, e->d_opt_costs, e->d_last_traj, e->d_best_traj,
                     e->max_it_cf, e->max_it, g->d_mirror + 2 * p, it};
}

namespace {
// One step's arguments into the arena, host only: engine main[k] at its iteration its[k]
// (stage_iteration and its terms arguments; the step's counts are the largest of the engines'),
// the flush of the engines `cohort`, and with `track` the bookkeeping arguments: iteration index
// its[k] - 2 of a main engine past its first iteration, max_iterations - 1 of a cohort engine (the
// table above stomp_group_optimize, per engine).
int stage_step(stomp_group* g, Arena& a, const std::vector<int>& main, const std::vector<int>& its,
               const std::vector<int>& cohort, bool keep_in_pre, bool track, StepLaunch& L)
{
    const int nm = (int)main.size(), nc = (int)cohort.size();
    const StepHost h = take_step(a, g, nm, nc, track, L);
    if (a.overflowed()) return gfail(g, STOMP_E_INVALID, "group optimize staging overflow");
    L.nro = L.ntot = L.ntrack = 0;
    L.reuse = false;
    for (int k = 0; k < nm; ++k) {
        stomp_engine* e = g->e[main[k]];
        const StagedIteration si = stage_iteration(e, its[k], keep_in_pre, h.cas[k], h.was[k], h.uas[k],
                                                   e->Kr > 0 ? h.ras + k : nullptr);
        if (g->nterms > 0) h.xas[k] = terms_args(e, h.cas[k]);
        L.nro = std::max(L.nro, si.nro);
        L.ntot = std::max(L.ntot, si.ntot);
        L.reuse = L.reuse || si.reuse;
        if (track && its[k] >= 2) h.tas[L.ntrack++] = track_args(g, main[k], its[k] - 2);
    }
    for (int k = 0; k < nc; ++k) {
        stomp_engine* e = g->e[cohort[k]];
        h.ccs[k] = noiseless_args(e);   // with K_r > 0 the extra rollout's rows too
        if (g->nterms > 0) h.cxas[k] = terms_args(e, h.ccs[k]);
        if (track) h.tas[L.ntrack++] = track_args(g, cohort[k], e->max_it - 1);
    }
    return 0;
}

// ---- stomp_group_optimize's stages (OptimizeLoop: engine_group.h)

// The model lists of the rollout launch within a chunk: staged once, again where an engine's
// max_iterations takes it out of the set (the upload of a chunk carries them once, not per step).
struct MainLists {
    std::vector<int> of;
    ModelLists lists;
    const ModelLists& get(Arena& a, const stomp_group* g, const std::vector<int>& main)
    {
        if (!main.empty() && main != of) {
            lists = take_models(a, g, main.data(), (int)main.size());
            of = main;
        }
        return lists;
    }
};

}  // namespace

// first-call allocations and the track arguments' upload
int optimize_prepare(stomp_group* g)
{
    if (g->d_mirror) return 0;
    const int P = (int)g->e.size();
    // one chunk of steps with every engine in both sets at most, and both launches' model lists;
    // a serve loop's chunk also carries a turnover's arguments
    const size_t slot_bytes = step_bytes(g, P, P, true, true) * (size_t)STOMP_GROUP_OPTIMIZE_CHUNK +
                              serve_chunk_bytes(P, g->e[0]->J);
    if (hipMalloc((void**)&g->d_mirror, sizeof(int) * 2 * P) != hipSuccess ||
        hipHostMalloc((void**)&g->h_mirror, sizeof(int) * 4 * P) != hipSuccess ||
        hipMalloc((void**)&g->d_track_all, sizeof(TrackArgs) * P) != hipSuccess ||
        hipMalloc((void**)&g->d_opt, 2 * slot_bytes) != hipSuccess ||
        hipHostMalloc((void**)&g->h_opt, 2 * slot_bytes) != hipSuccess ||
        hipEventCreateWithFlags(&g->opt_ev[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&g->opt_ev[1], hipEventDisableTiming) != hipSuccess)
        return gfail(g, STOMP_E_DEVICE, "group optimize allocation failed");
    g->opt_slot = slot_bytes;
    // every engine's track arguments, for the start and clear launches
    std::vector<TrackArgs> ta(P);
    for (int p = 0; p < P; ++p) ta[p] = track_args(g, p);
    if (hipMemcpy(g->d_track_all, ta.data(), sizeof(TrackArgs) * P, hipMemcpyHostToDevice) != hipSuccess)
        return gfail(g, STOMP_E_DEVICE, "group argument upload failed");
    return 0;
}

namespace {
// The engines enter in any state: rows out of the pregen buffers, pending noiseless rollouts
// evaluated, the pregen rows of iteration 1 made where another iteration's are held.
void optimize_enter(stomp_group* g)
{
    for (stomp_engine* e : g->e) {
        materialize_rows(e);
        flush_noiseless(e);
        if (e->max_it > 0 && e->pre_it != 1) {
            launch_pregen(pregen_args(e, 1), e->K_loc, g->stream);
            e->pre_it = 1;
        }
    }
    launch_track_start_group(g->d_track_all, (int)g->e.size(), false, g->stream);   // stomp_optimizer.cpp:251 start_time
}

// the staged entries of engines whose padding-collision flag the host does not know (a serve
// loop's turned slots): listed for launch_serve_flags
void note_flag_copies(OptimizeLoop& o, const ModelLists& l, const std::vector<int>& of)
{
    if (!o.flag_unknown || !l.models) return;
    for (size_t k = 0; k < of.size(); ++k)
        if ((*o.flag_unknown)[of[k]])
            o.flag_copies.push_back({o.g->e[of[k]]->d_pad_cf, (int*)((const unsigned char*)(l.models + k) +
                                                                      offsetof(DevModel, pad_collision))});
}

// The next chunk of steps into the arena and onto o.steps, host only.  In step `step` engine p is
// at its iteration it = step - o.start[p] + 1: the engines of o.main run theirs, the ones of
// o.cohort, which ended with it - 1, get their flush (the table above stomp_group_optimize).
int optimize_stage_chunk(OptimizeLoop& o, Arena& a)
{
    stomp_group* g = o.g;
    MainLists lists;
    o.steps.clear();
    o.flag_copies.clear();
    const int end = std::min(o.next + STOMP_GROUP_OPTIMIZE_CHUNK, o.last_step + 1);
    for (int step = o.next; step < end; ++step) {
        o.main.clear();
        o.main_it.clear();
        o.cohort.clear();
        for (int p : o.live) {
            const int it = step - o.start[p] + 1;
            if (it >= 1 && g->e[p]->max_it >= it) {
                o.main.push_back(p);
                o.main_it.push_back(it);
            } else if (g->e[p]->max_it == it - 1 && it >= 2) {
                o.cohort.push_back(p);
            }
        }
        // inside the optimize loop the noise / params rows are copied out of the pregen buffer
        // (pregen blocks enqueued past a stop overwrite the ping-pong buffers), the weights read
        // d_noise
        for (size_t k = 0; k < o.main.size(); ++k)
            if (g->e[o.main[k]]->pre_it != o.main_it[k]) return gfail(g, STOMP_E_INVALID, "group pregen rows out of step");
        StepLaunch L;
        if (int rc = stage_step(g, a, o.main, o.main_it, o.cohort, false, true, L)) return rc;
        L.clists = take_models(a, g, o.cohort.data(), (int)o.cohort.size());
        const DevModel* held = lists.lists.models;
        L.lists = lists.get(a, g, o.main);
        if (a.overflowed()) return gfail(g, STOMP_E_INVALID, "group optimize staging overflow");
        note_flag_copies(o, L.clists, o.cohort);
        if (L.lists.models != held) note_flag_copies(o, L.lists, o.main);
        for (size_t k = 0; k < o.main.size(); ++k) {
            const stomp_engine* e = g->e[o.main[k]];
            if (e->Kr > 0) o.after[o.main[k]][o.main_it[k] - 1] = {e->reused_next, e->extra_added, e->row_set};
        }
        o.steps.push_back(L);
    }
    o.next = end;
    return 0;
}
}  // namespace

// one chunk of steps staged into `slot`, uploaded and enqueued, then the mirror's read-back
int optimize_enqueue_chunk(OptimizeLoop& o, int slot, const ChunkExtra* extra)
{
    stomp_group* g = o.g;
    const int P = (int)g->e.size();
    Arena a{g->h_opt + (size_t)slot * g->opt_slot, g->d_opt + (size_t)slot * g->opt_slot, g->opt_slot};
    if (int rc = optimize_stage_chunk(o, a)) return rc;
    if (extra)
        if (int rc = extra->stage(a)) return rc;
    if (int rc = upload(g, a, nullptr)) return rc;
    if (extra) extra->launch();
    for (const StepLaunch& L : o.steps) o.launches += launch_step(g, L);
    if (hipMemcpyAsync(g->h_mirror + (size_t)slot * 2 * P, g->d_mirror, sizeof(int) * 2 * P, hipMemcpyDeviceToHost,
                       g->stream) != hipSuccess ||
        hipEventRecord(g->opt_ev[slot], g->stream) != hipSuccess)
        return gfail(g, STOMP_E_DEVICE, "group read-back failed");
    return 0;
}

void optimize_restore(OptimizeLoop& o, int p, int iterations)
{
    stomp_engine* e = o.g->e[p];
    if (e->Kr <= 0 || iterations <= 0) return;
    const OptimizeLoop::HostState& h = o.after[p][iterations - 1];
    e->reused_next = h.reused_next;
    e->extra_added = h.extra_added;
    if (e->row_set != h.row_set) swap_row_sets(e);
}

namespace {
// The loop is over (rc: how): pipeline state reset, every engine's DevTrack read back, its
// generateRollouts state put back to the iteration it stopped at, cost histories and stats out.
int optimize_finish(OptimizeLoop& o, int rc, stomp_stats* stats, double* costs_per_iteration, int32_t costs_stride)
{
    stomp_group* g = o.g;
    const int P = (int)g->e.size();
    hipStream_t s = g->stream;
    // the steps enqueued past an engine's stop were no-ops; the engines stopped at different
    // iterations, so every engine leaves with no pregen rows held and nothing pending (the next
    // run, the group's or the engine's own, makes its rows with a standalone pregen launch)
    for (stomp_engine* e : g->e) {
        e->pending_member = -1;
        e->pre_it = -1;
        e->rows_in_pre = false;
    }
    hipError_t err = hipGetLastError();
    if (!rc && err != hipSuccess) rc = gfail(g, STOMP_E_DEVICE, hipGetErrorString(err));
    for (int p = 0; p < P && !rc; ++p)
        if (hipMemcpyAsync(&g->e[p]->h_track[2], g->e[p]->d_track, sizeof(DevTrack), hipMemcpyDeviceToHost, s) != hipSuccess)
            rc = gfail(g, STOMP_E_DEVICE, "group read-back failed");
    // later launches (iterate / run / eval) are not gated
    launch_track_start_group(g->d_track_all, P, true, s);
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = gfail(g, STOMP_E_DEVICE, "group synchronize failed");
    if (rc) return rc;
    for (int p = 0; p < P; ++p) {
        stomp_engine* e = g->e[p];
        const DevTrack& t = e->h_track[2];
        optimize_restore(o, p, t.iterations);
        if (costs_per_iteration && t.iterations > 0 &&
            hipMemcpy(costs_per_iteration + (size_t)p * costs_stride, e->d_opt_costs, sizeof(double) * t.iterations,
                      hipMemcpyDeviceToHost) != hipSuccess)
            return gfail(g, STOMP_E_DEVICE, "group cost history read-back failed");
        stats[p] = stats_from_track(e, t);
    }
    return 0;
}
}  // namespace
}  // namespace stomp

extern "C" {

void stomp_group_destroy(stomp_group* g)
{
    if (!g) return;
    DeviceGuard dg(g->device);
    if (g->staged) {
        hipEventSynchronize(g->staged);
        hipEventDestroy(g->staged);
    }
    free_device(g->d_models, g->d_tmodels, g->d_args, g->d_opt, g->d_mirror, g->d_track_all, g->d_rq, g->d_slab);
    free_pinned(g->h_args, g->h_opt, g->h_mirror, g->h_rq);
    for (hipEvent_t ev : g->opt_ev)
        if (ev) hipEventDestroy(ev);
    delete g;
}

int stomp_group_create(stomp_engine* const* engines, int32_t n, stomp_group** out)
{
    const stomp_group_options o = {(int32_t)sizeof(stomp_group_options), 0, -1};
    return stomp_group_create_with(engines, n, &o, out);
}

int stomp_group_create_with(stomp_engine* const* engines, int32_t n, const stomp_group_options* options,
                            stomp_group** out)
{
    if (!engines || n <= 0 || !out) return gfail(nullptr, STOMP_E_INVALID, "invalid group arguments");
    if (!options || options->struct_size != (int32_t)sizeof(stomp_group_options))
        return gfail(nullptr, STOMP_E_INVALID, "invalid group options (null, or struct_size is not sizeof(stomp_group_options))");
    return stomp_group_create_flags(engines, n, options->state_terms ? STOMP_GROUP_ACCEPT_STATE_TERMS : 0u,
                                    options->compact, out);
}

int stomp_group_create_flags(stomp_engine* const* engines, int32_t n, uint32_t accept, int32_t compact,
                             stomp_group** out)
{
    // all of this before any engine or device is touched
    if (!engines || n <= 0 || !out) return gfail(nullptr, STOMP_E_INVALID, "invalid group arguments");
    if (accept & ~(STOMP_GROUP_ACCEPT_STATE_TERMS | STOMP_GROUP_ACCEPT_CUMULATIVE))
        return gfail(nullptr, STOMP_E_INVALID, "invalid group arguments: unknown bits in accept");
    if (compact < -1 || compact > 1)
        return gfail(nullptr, STOMP_E_INVALID, "invalid group arguments: compact is -1, 0 or 1");
    const bool state_terms = (accept & STOMP_GROUP_ACCEPT_STATE_TERMS) != 0;
    const bool cumulative = (accept & STOMP_GROUP_ACCEPT_CUMULATIVE) != 0;
    stomp_engine* e0 = engines[0];
    if (!e0) return gfail(nullptr, STOMP_E_INVALID, "null engine");
    const size_t lds0 = rollout_lds_bytes(e0->model, e0->model.pad_lds);
    for (int p = 0; p < n; ++p) {
        stomp_engine* e = engines[p];
        if (!e) return gfail(nullptr, STOMP_E_INVALID, "null engine");
        if (e->device != e0->device || e->stream != e0->stream)
            return gfail(nullptr, STOMP_E_INVALID, "the engines of a group share one device and one stream");
        if (e->J != e0->J || e->N != e0->N || e->K != e0->K || e->Kr != e0->Kr || e->S != e0->S ||
            rollout_lds_bytes(e->model, e->model.pad_lds) != lds0 || e->model.brick != e0->model.brick)
            return gfail(nullptr, STOMP_E_INVALID,
                         "the engines of a group have one shape (J, N, K, K_r, spheres, model, field layout)");
        if (e->world != 1 || !e->pre_on || (e->terms_on && !state_terms) || e->split_modes || e->gather ||
            (e->use_cum && !cumulative) || e->J > 16)
            return gfail(nullptr, STOMP_E_UNSUPPORTED,
                         refusal_text(state_terms, cumulative));
        if (e->use_cum && cumulative_group_rows(e->N) <= 0)
            return gfail(nullptr, STOMP_E_UNSUPPORTED, "groups with cumulative costs take at most 256 time steps");
        if (e->Kr > 0) {
            // the reuse step is the reused rows' kernel (launch_reuse_rows_ok: K + 1 candidates
            // ranked by a workgroup, J <= 16, the row kernel's LDS)
            NoiseArgs na = noise_args(e, 1);
            na.K_gen_global = e->K - e->Kr;
            na.row_begin = e->K - e->Kr;
            if (!launch_reuse_rows_ok(na, e->K, e->Kr))
                return gfail(nullptr, STOMP_E_UNSUPPORTED,
                             "groups with reused rollouts take at most 1023 rollouts and a reused row's kernel "
                             "that fits the LDS");
        }
    }
    const int nt = weights_group_tiles(e0->J, e0->N, e0->K_loc);
    if (nt <= 0) return gfail(nullptr, STOMP_E_UNSUPPORTED, "rollouts per engine beyond the weights tiles");
    DeviceGuard dg(e0->device);
    stomp_group* g = new stomp_group();
    g->e.assign(engines, engines + n);
    for (int p = 0; p < n; ++p) g->all.push_back(p);
    g->device = e0->device;
    g->stream = e0->stream;
    g->nt = nt;
    g->shape = noise_args(e0, 1);
    if (compact >= 0) g->compact = compact != 0;
    else if (const char* c = getenv("STOMP_DEBUG_GROUP_COMPACT")) g->compact = c[0] == '1';
    g->state_terms = state_terms;
    for (int p = 0; p < n; ++p) g->ncum += engines[p]->use_cum ? 1 : 0;
    std::vector<DevModel> ms(n);
    for (int p = 0; p < n; ++p) ms[p] = engines[p]->model;
    for (int p = 0; p < n; ++p) g->pad_flags.push_back(engines[p]->pad_collision);
    for (int p = 0; p < n; ++p) g->epochs.push_back(engines[p]->model_epoch);
    if (hipMalloc(&g->d_models, sizeof(DevModel) * n) != hipSuccess ||
        hipMemcpy(g->d_models, ms.data(), sizeof(DevModel) * n, hipMemcpyHostToDevice) != hipSuccess ||
        hipEventCreateWithFlags(&g->staged, hipEventDisableTiming) != hipSuccess) {
        stomp_group_destroy(g);
        return gfail(nullptr, STOMP_E_DEVICE, "group allocation failed");
    }
    if (state_terms) {
        std::vector<TermsModel> ts(n);
        for (int p = 0; p < n; ++p) {
            ts[p] = engines[p]->terms;
            if (!engines[p]->terms_on) continue;
            ++g->nterms;
            g->terms_lds = std::max(g->terms_lds, terms_lds_bytes(ts[p]));
        }
        if (hipMalloc(&g->d_tmodels, sizeof(TermsModel) * n) != hipSuccess ||
            hipMemcpy(g->d_tmodels, ts.data(), sizeof(TermsModel) * n, hipMemcpyHostToDevice) != hipSuccess) {
            stomp_group_destroy(g);
            return gfail(nullptr, STOMP_E_DEVICE, "group allocation failed");
        }
    }
    if (getenv("STOMP_DEBUG_LEAN_PRINT")) {
        // the group's own choices and the launches launch_terms_group / launch_cumulative_group
        // take (read-only: tests and tables)
        fprintf(stderr, "stomp: group of %d engines J %d N %d K %d brick %d, %d weights tiles per engine, "
                        "weights %s\n", (int)n, e0->J, e0->N, e0->K_loc, e0->model.brick, nt,
                weights_kernel_name(e0->K_loc, true, true));
        if (state_terms)
            fprintf(stderr, "stomp: group terms k_terms_group<%d>, LDS %zu B, opt-in %d, engines with terms %d of %d\n",
                    e0->N <= 128 ? 128 : 256, g->terms_lds, g->terms_lds > 64 * 1024 ? 1 : 0, g->nterms, (int)n);
        if (g->ncum > 0)
            fprintf(stderr, "stomp: group cumulative k_cumulative_group<%d>, rows per workgroup %d, LDS %zu B, "
                            "engines with cumulative costs %d of %d\n", cumulative_group_rows(e0->N),
                    cumulative_group_rows(e0->N), cumulative_group_lds_bytes(e0->N), g->ncum, (int)n);
    }
    *out = g;
    return 0;
}

int stomp_group_retarget(stomp_group* g, const double* starts, const double* goals, const uint64_t* seeds)
{
    // all of this before any engine or device is touched
    if (!g) return gfail(nullptr, STOMP_E_INVALID, "null group");
    if (!starts || !goals || !seeds) return gfail(nullptr, STOMP_E_INVALID, "retarget: null starts, goals or seeds");
    if (int rc = check_epochs(g)) return rc;
    const size_t P = g->e.size(), J = (size_t)g->e[0]->J;
    std::vector<stomp_request> rs(P);
    for (size_t p = 0; p < P; ++p) rs[p] = kept_request(starts + p * J, goals + p * J, seeds[p]);
    return group_retarget(g, rs.data());
}

int stomp_group_retarget_requests(stomp_group* g, const stomp_request* rs)
{
    // all of this before any engine or device is touched
    if (!g) return gfail(nullptr, STOMP_E_INVALID, "null group");
    if (!rs) return gfail(nullptr, STOMP_E_INVALID, "retarget: null requests");
    for (size_t p = 0; p < g->e.size(); ++p) {
        if (rs[p].struct_size != (int32_t)sizeof(stomp_request))
            return gfail(g, STOMP_E_INVALID, "retarget: struct_size is not sizeof(stomp_request)");
        if (!rs[p].start || !rs[p].goal) return gfail(g, STOMP_E_INVALID, "retarget: null start or goal");
    }
    return group_retarget(g, rs);
}

const char* stomp_group_last_error(const stomp_group* g) { return g ? g->err.c_str() : g_last_error.c_str(); }

int stomp_group_run(stomp_group* g, int32_t first, int32_t count)
{
    if (!g) return gfail(nullptr, STOMP_E_INVALID, "null group");
    if (count <= 0) return 0;
    if (int rc = check_epochs(g)) return rc;
    DeviceGuard dg(g->device);
    const int P = (int)g->e.size();
    stomp_engine* e0 = g->e[0];
    for (stomp_engine* e : g->e) {
        // lockstep: the engines enter the run in one pipeline state, and with reuse in one
        // generateRollouts state (which row set an engine writes next is its own: the engines of
        // a group leave stomp_group_optimize at either parity of the swap)
        if (e->pending_member != e0->pending_member || e->pre_it != e0->pre_it || e->tracking ||
            (e->Kr > 0 && (e->reused_next != e0->reused_next || e->extra_added != e0->extra_added)))
            return gfail(g, STOMP_E_INVALID, "the engines of a group are not at the same iteration state");
    }
    const size_t bytes = step_bytes(g, P, 0, false, false) * (size_t)count;
    if (int rc = sync_model_flags(g)) return rc;
    if (int rc = reserve_args(g, bytes)) return rc;
    Arena a{g->h_args, g->d_args, bytes};
    std::vector<StepLaunch> steps(count);
    std::vector<char> pregen_first(P, 0);
    std::vector<int> its(P);
    for (int i = 0; i < count; ++i) {
        const int it = first + i;
        std::fill(its.begin(), its.end(), it);   // a run's engines are in lockstep
        for (int p = 0; p < P; ++p) {
            if (g->e[p]->pre_it == it) continue;
            if (i > 0) return gfail(g, STOMP_E_INVALID, "group pregen rows out of step");
            pregen_first[p] = 1;
        }
        if (int rc = stage_step(g, a, g->all, its, {}, true, false, steps[i])) return rc;
        steps[i].lists = {g->d_models, g->d_tmodels, g->nterms};
    }
    for (int p = 0; p < P; ++p)
        if (pregen_first[p]) launch_pregen(pregen_args(g->e[p], first), g->e[p]->K_loc, g->stream);
    if (int rc = upload(g, a, g->staged)) return rc;
    for (const StepLaunch& L : steps) launch_step(g, L);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return gfail(g, STOMP_E_DEVICE, hipGetErrorString(err));
    return 0;
}

int stomp_group_synchronize(stomp_group* g)
{
    if (!g) return gfail(nullptr, STOMP_E_INVALID, "null group");
    if (int rc = check_epochs(g)) return rc;
    DeviceGuard dg(g->device);
    const int P = (int)g->e.size();
    if (int rc = sync_model_flags(g)) return rc;
    bool pending = true;
    for (stomp_engine* e : g->e) pending = pending && e->pending_member >= 0 && !e->tracking;
    const size_t cap = std::min(g->h_cap, g->d_cap);
    if (pending && step_bytes(g, 0, P, false, false) <= cap) {
        // every engine's pending noiseless rollout in one step of the flush cohort alone, staged in
        // a run's buffers (no run has sized them yet: the per-engine flushes below); its rollout
        // launch is on no timer, as an engine's own flush here
        if (g->staged && hipEventSynchronize(g->staged) != hipSuccess)
            return gfail(g, STOMP_E_DEVICE, "group staging wait failed");
        Arena a{g->h_args, g->d_args, cap};
        StepLaunch L;
        if (int rc = stage_step(g, a, {}, {}, g->all, false, false, L)) return rc;
        L.clists = {g->d_models, g->d_tmodels, g->nterms};
        L.time_flush = false;
        if (int rc = upload(g, a, g->staged)) return rc;
        launch_step(g, L);
    }
    for (stomp_engine* e : g->e) flush_noiseless(e);
    if (hipStreamSynchronize(g->stream) != hipSuccess) return gfail(g, STOMP_E_DEVICE, "group synchronize failed");
    return 0;
}

int32_t stomp_group_optimize_chunk(void) { return STOMP_GROUP_OPTIMIZE_CHUNK; }

// StompOptimizer::optimize (stomp_optimizer.cpp:249-401) for every engine of the group:
// stomp_engine_optimize's chunked loop over the grouped launches.  Step `it` (1-based iteration,
// the engines in lockstep) is
//   the grouped rollout launch of `it` with the noiseless rollouts of it - 1   (engines with max_it >= it)
//   a grouped noiseless flush                                                  (engines with max_it == it - 1)
//   k_track_group(it - 2) over both sets, weights and update of the first set
// so an engine whose own max_iterations ends the loop gets the flush and the bookkeeping that
// stomp_engine_optimize ends with, in the step after its last iteration; the last step of all is
// that flush alone.  With g->compact no arguments are staged for an engine seen stopped; otherwise
// its blocks stay in the launches and return at its stop flag (the default: DESIGN.md 7).
int stomp_group_optimize(stomp_group* g, stomp_stats* stats, double* costs_per_iteration, int32_t costs_stride)
{
    if (!g) return gfail(nullptr, STOMP_E_INVALID, "null group");
    if (!stats) return gfail(g, STOMP_E_INVALID, "null stats");
    if (int rc = check_epochs(g)) return rc;
    const int P = (int)g->e.size();
    stomp_engine* e0 = g->e[0];
    int maxcap = 0;
    for (stomp_engine* e : g->e) {
        if (e->tracking) return gfail(g, STOMP_E_INVALID, "an engine of the group is inside its own optimize loop");
        maxcap = std::max(maxcap, e->max_it);
    }
    if (costs_per_iteration && costs_stride < maxcap)
        return gfail(g, STOMP_E_INVALID, "costs_stride is smaller than an engine's max_iterations");
    DeviceGuard dg(g->device);
    if (int rc = optimize_prepare(g)) return rc;
    // with reuse the engines are at one point of generateRollouts (all reuse in iteration 1, or
    // none does)
    for (stomp_engine* e : g->e)
        if (e->Kr > 0 && e->reused_next != e0->reused_next)
            return gfail(g, STOMP_E_INVALID, "the engines of a group are not at the same iteration state");
    OptimizeLoop o;
    o.g = g;
    o.after.resize(P);
    o.start.assign(P, 1);   // lockstep: every engine's iteration 1 in step 1
    if (e0->Kr > 0)
        for (int p = 0; p < P; ++p) o.after[p].resize((size_t)std::max(g->e[p]->max_it, 0));
    for (int p = 0; p < P; ++p)
        if (!g->compact || g->e[p]->max_it > 0) o.live.push_back(p);
    o.last_step = maxcap > 0 ? maxcap + 1 : 0;
    optimize_enter(g);

    // two chunks in flight: the host stages and enqueues one while the device runs the other, and
    // reads the mirror of the older one
    int rc = 0, inflight = 0, head = 0;
    bool all_stopped = false;
    while (!all_stopped) {
        while (inflight < 2 && o.next <= o.last_step) {
            if ((rc = optimize_enqueue_chunk(o, (head + inflight) & 1))) break;
            ++inflight;
        }
        if (rc || inflight == 0) break;
        if (hipEventSynchronize(g->opt_ev[head]) != hipSuccess) {
            rc = gfail(g, STOMP_E_DEVICE, "group read-back wait failed");
            break;
        }
        const int* hm = g->h_mirror + (size_t)head * 2 * P;
        all_stopped = true;
        for (int p = 0; p < P; ++p) all_stopped = all_stopped && hm[2 * p] != 0;
        if (g->compact)   // the engines seen stopped leave every chunk staged from here on
            o.live.erase(std::remove_if(o.live.begin(), o.live.end(), [hm](int p) { return hm[2 * p] != 0; }), o.live.end());
        head ^= 1;
        --inflight;
    }
    return optimize_finish(o, rc, stats, costs_per_iteration, costs_stride);
}

}  // extern "C"
