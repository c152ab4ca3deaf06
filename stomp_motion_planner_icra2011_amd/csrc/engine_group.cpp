// engine_group.cpp -- engine groups (stomp_group_*).
// Several engines of one shape driven in lockstep by shared launches: per iteration one rollout
// launch covering every engine's rollout workgroups and pregen blocks, one weights launch and one
// update launch (k_rollout_group, k_weights_rows_group, k_update_group), so a batch of independent
// planning problems costs three dispatches per iteration instead of three per problem.  The
// per-engine kernel arguments of a whole run are staged in pinned memory and uploaded once; each
// engine's results are the ones its own stomp_engine_run gives, bit for bit.  stomp_group_optimize
// runs the whole optimize loop that way, the bookkeeping of every engine in one more launch per
// iteration (k_track_group), each engine stopping on its own.
// Engines with reused rollouts (one K_r for the group) add the reuse candidates' totals blocks to
// the rollout launch and one launch for every engine's reused rows (k_reuse_rows_group) on the
// reusing iterations; the host keeps every engine's generateRollouts state (reused_next,
// extra_added, the row-set swap) in step with the staged iterations and, after an optimize loop,
// puts back the state of the iteration each engine stopped at.
// A group created with state_terms (stomp_group_create_with) also takes engines with the torque
// term and / or orientation path constraints: every grouped rollout launch and every grouped
// noiseless flush is followed by one launch of the state-cost terms for all of its engines
// (k_terms_group, each engine with its own TermsModel; an engine without terms has no workgroup
// that writes), before anything reads the state costs, the noiseless total or the
// constraints-satisfied flag.
// A group created accepting cumulative costs (stomp_group_create_flags) also takes engines with
// use_cumulative_costs, mixed freely with engines without: every grouped weights launch is then
// preceded, inside the same timed scope, by one launch of the cumulative rows of all of its
// engines (k_cumulative_group; an engine without cumulative costs has no workgroup that writes).
// stomp_group_retarget puts every engine of the group onto a new start, goal and seed in one launch
// and one read-back (engine_retarget.cpp); the launch also writes the padding-collision flags of
// the group's own DevModel list, which the grouped launches of a run and a synchronize read.
#include "engine_internal.h"

#include <algorithm>

using namespace stomp;

struct stomp_group {
    std::vector<stomp_engine*> e;
    int device = 0;
    hipStream_t stream = nullptr;
    int nt = 0;                           // weights tiles per engine
    DevModel* d_models = nullptr;         // [P]
    bool state_terms = false;             // engines with terms accepted (stomp_group_create_with)
    TermsModel* d_tmodels = nullptr;      // [P] every engine's terms model (state_terms)
    int nterms = 0;                       // engines with terms
    int ncum = 0;                         // engines with cumulative costs (stomp_group_create_flags)
    size_t terms_lds = 0;                 // the largest terms_lds_bytes among them: k_terms_group's dynamic LDS
    unsigned char* d_args = nullptr;      // [iterations][P] CostArgs, WeightArgs, UpdateArgs, (K_r > 0) ReuseRowArgs,
                                          // (engines with terms) TermsArgs
    size_t d_cap = 0;
    unsigned char* h_args = nullptr;      // pinned staging of one run's arguments
    size_t h_cap = 0;
    hipEvent_t staged = nullptr;          // the last upload from h_args is done
    // stomp_group_optimize: two slots of one chunk's arguments each (pinned and device), the
    // engines' (stop, iterations) mirror with a pinned read-back per slot, all P track arguments
    bool compact = false;                 // stopped engines leave the launches (STOMP_DEBUG_GROUP_COMPACT=1 / 0)
    unsigned char *h_opt = nullptr, *d_opt = nullptr;
    size_t opt_slot = 0;                  // bytes per slot
    int* d_mirror = nullptr;              // [P][2]
    int* h_mirror = nullptr;              // [2][P][2]
    TrackArgs* d_track_all = nullptr;     // [P]
    hipEvent_t opt_ev[2] = {nullptr, nullptr};
    // stomp_group_retarget: one call's staging (pinned and device); the padding-collision flag each
    // entry of d_models holds, so that an engine retargeted on its own (stomp_engine_retarget knows
    // no group) gets its entry refreshed before the next launch that reads the list
    unsigned char *h_rt = nullptr, *d_rt = nullptr;
    std::vector<int> pad_flags;
    std::string err;
};

namespace {
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

int gfail(stomp_group* g, int code, const char* msg)
{
    g_last_error = msg;
    if (g) g->err = msg;
    return code;
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
}  // namespace

extern "C" {

void stomp_group_destroy(stomp_group* g)
{
    if (!g) return;
    DeviceGuard dg(g->device);
    if (g->staged) {
        hipEventSynchronize(g->staged);
        hipEventDestroy(g->staged);
    }
    if (g->d_models) hipFree(g->d_models);
    if (g->d_tmodels) hipFree(g->d_tmodels);
    if (g->d_args) hipFree(g->d_args);
    if (g->h_args) hipHostFree(g->h_args);
    if (g->d_opt) hipFree(g->d_opt);
    if (g->h_opt) hipHostFree(g->h_opt);
    if (g->d_mirror) hipFree(g->d_mirror);
    if (g->h_mirror) hipHostFree(g->h_mirror);
    if (g->d_track_all) hipFree(g->d_track_all);
    if (g->d_rt) hipFree(g->d_rt);
    if (g->h_rt) hipHostFree(g->h_rt);
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
                         cumulative ? (state_terms ? "groups run single-device engines of at most 16 joints"
                                                   : "groups run single-device engines of at most 16 joints without "
                                                     "state-cost terms")
                         : state_terms ? "groups run single-device engines of at most 16 joints without cumulative costs"
                                       : "groups run single-device engines of at most 16 joints without state-cost "
                                         "terms or cumulative costs");
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
    g->device = e0->device;
    g->stream = e0->stream;
    g->nt = nt;
    if (compact >= 0) g->compact = compact != 0;
    else if (const char* c = getenv("STOMP_DEBUG_GROUP_COMPACT")) g->compact = c[0] == '1';
    g->state_terms = state_terms;
    for (int p = 0; p < n; ++p) g->ncum += engines[p]->use_cum ? 1 : 0;
    std::vector<DevModel> ms(n);
    for (int p = 0; p < n; ++p) ms[p] = engines[p]->model;
    for (int p = 0; p < n; ++p) g->pad_flags.push_back(engines[p]->pad_collision);
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
    if (getenv("STOMP_DEBUG_LEAN_PRINT"))   // the group's own choices (read-only: tests and tables)
        fprintf(stderr, "stomp: group of %d engines J %d N %d K %d brick %d, %d weights tiles per engine, "
                        "weights %s\n", (int)n, e0->J, e0->N, e0->K_loc, e0->model.brick, nt,
                weights_kernel_name(e0->K_loc, true, true));
    if (state_terms && getenv("STOMP_DEBUG_LEAN_PRINT"))   // the launch launch_terms_group takes (read-only)
        fprintf(stderr, "stomp: group terms k_terms_group<%d>, LDS %zu B, opt-in %d, engines with terms %d of %d\n",
                e0->N <= 128 ? 128 : 256, g->terms_lds, g->terms_lds > 64 * 1024 ? 1 : 0, g->nterms, (int)n);
    if (g->ncum > 0 && getenv("STOMP_DEBUG_LEAN_PRINT"))   // the launch launch_cumulative_group takes (read-only)
        fprintf(stderr, "stomp: group cumulative k_cumulative_group<%d>, rows per workgroup %d, LDS %zu B, engines "
                        "with cumulative costs %d of %d\n", cumulative_group_rows(e0->N), cumulative_group_rows(e0->N),
                cumulative_group_lds_bytes(e0->N), g->ncum, (int)n);
    *out = g;
    return 0;
}

int stomp_group_retarget(stomp_group* g, const double* starts, const double* goals, const uint64_t* seeds)
{
    // all of this before any engine or device is touched
    if (!g) return gfail(nullptr, STOMP_E_INVALID, "null group");
    if (!starts || !goals || !seeds) return gfail(nullptr, STOMP_E_INVALID, "retarget: null starts, goals or seeds");
    const int P = (int)g->e.size();
    if (int rc = retarget_validate(g->e.data(), P, starts, goals)) return gfail(g, rc, std::string(g_last_error).c_str());
    DeviceGuard dg(g->device);
    if (!g->d_rt) {
        const size_t bytes = retarget_stage_bytes(P, g->e[0]->J);
        if ((!g->h_rt && hipHostMalloc((void**)&g->h_rt, bytes) != hipSuccess) ||
            hipMalloc((void**)&g->d_rt, bytes) != hipSuccess)
            return gfail(g, STOMP_E_DEVICE, "group retarget allocation failed");
    }
    // one launch and one read-back for the whole group; every engine leaves in the freshly created
    // iteration state, whichever iteration its optimize loop stopped at
    if (int rc = retarget_engines(g->e.data(), P, starts, goals, seeds, g->h_rt, g->d_rt, g->d_models))
        return gfail(g, rc, std::string(g_last_error).c_str());
    for (int p = 0; p < P; ++p) g->pad_flags[p] = g->e[p]->pad_collision;
    return 0;
}

const char* stomp_group_last_error(const stomp_group* g) { return g ? g->err.c_str() : g_last_error.c_str(); }

int stomp_group_run(stomp_group* g, int32_t first, int32_t count)
{
    if (!g) return gfail(nullptr, STOMP_E_INVALID, "null group");
    if (count <= 0) return 0;
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
    const size_t szc = align256(sizeof(CostArgs) * P), szw = align256(sizeof(WeightArgs) * P),
                 szu = align256(sizeof(UpdateArgs) * P),
                 szr = e0->Kr > 0 ? align256(sizeof(ReuseRowArgs) * P) : 0,
                 szt = g->nterms > 0 ? align256(sizeof(TermsArgs) * P) : 0, per = szc + szw + szu + szr + szt;
    const size_t bytes = per * (size_t)count;
    if (int rc = sync_model_flags(g)) return rc;
    if (g->staged && hipEventSynchronize(g->staged) != hipSuccess)   // h_args free again
        return gfail(g, STOMP_E_DEVICE, "group staging wait failed");
    if (bytes > g->h_cap) {
        if (g->h_args) hipHostFree(g->h_args);
        g->h_args = nullptr;
        g->h_cap = 0;
        if (hipHostMalloc((void**)&g->h_args, bytes) != hipSuccess) return gfail(g, STOMP_E_DEVICE, "hipHostMalloc failed");
        g->h_cap = bytes;
    }
    if (bytes > g->d_cap) {
        if (g->d_args) {
            hipStreamSynchronize(g->stream);
            hipFree(g->d_args);
        }
        g->d_args = nullptr;
        g->d_cap = 0;
        if (hipMalloc(&g->d_args, bytes) != hipSuccess) return gfail(g, STOMP_E_DEVICE, "hipMalloc failed");
        g->d_cap = bytes;
    }
    std::vector<StagedIteration> steps(count);
    std::vector<char> pregen_first(P, 0);
    for (int i = 0; i < count; ++i) {
        const int it = first + i;
        CostArgs* cas = (CostArgs*)(g->h_args + per * i);
        WeightArgs* was = (WeightArgs*)(g->h_args + per * i + szc);
        UpdateArgs* uas = (UpdateArgs*)(g->h_args + per * i + szc + szw);
        ReuseRowArgs* ras = (ReuseRowArgs*)(g->h_args + per * i + szc + szw + szu);
        TermsArgs* tas = (TermsArgs*)(g->h_args + per * i + szc + szw + szu + szr);
        for (int p = 0; p < P; ++p) {
            stomp_engine* e = g->e[p];
            if (e->pre_it != it) {
                if (i > 0) return gfail(g, STOMP_E_INVALID, "group pregen rows out of step");
                pregen_first[p] = 1;
            }
            const StagedIteration st = stage_iteration(e, it, true, cas[p], was[p], uas[p], ras + p);
            if (szt) tas[p] = terms_args(e, cas[p]);
            if (p == 0) steps[i] = st;
            else if (st.nro != steps[i].nro || st.ntot != steps[i].ntot || st.reuse != steps[i].reuse)
                return gfail(g, STOMP_E_INVALID, "group engines out of step");
        }
    }
    hipStream_t s = g->stream;
    for (int p = 0; p < P; ++p)
        if (pregen_first[p]) launch_pregen(pregen_args(g->e[p], first), g->e[p]->K_loc, s);
    hipError_t err = hipMemcpyAsync(g->d_args, g->h_args, bytes, hipMemcpyHostToDevice, s);
    if (err == hipSuccess) err = hipEventRecord(g->staged, s);
    if (err != hipSuccess) return gfail(g, STOMP_E_DEVICE, "group argument upload failed");
    const int J = e0->J, N = e0->N, K = e0->K_loc;
    const NoiseArgs shape = noise_args(e0, first);   // J, N, Nall of the reuse launches
    for (int i = 0; i < count; ++i) {
        unsigned char* base = g->d_args + per * i;
        // with timing on for the group's first engine, its timers hold the group's launches
        {
            Timed tm(e0, T_COST, s);
            launch_cost_group(e0->model, g->d_models, (const CostArgs*)base, P, steps[i].nro, K + steps[i].ntot, s);
        }
        if (szt) {
            // every engine's state-cost terms on the rollouts just evaluated, before the reuse
            // ranking, the weights (and the next flush's bookkeeping) read them
            Timed tm(e0, T_TERMS, s);
            launch_terms_group(g->d_tmodels, (const TermsArgs*)(base + szc + szw + szu + szr), P, steps[i].nro, N,
                               g->terms_lds, s);
        }
        if (steps[i].reuse) {
            // every engine's reuse step (an engine on its own records its reused rows' launch on
            // this timer too)
            Timed tm(e0, T_NOISE, s);
            launch_reuse_rows_group(shape, (const ReuseRowArgs*)(base + szc + szw + szu), P, e0->K, e0->Kr, s);
        }
        {
            // the cumulative rows of the engines that use them, on the control costs the reuse
            // launch re-priced, in the weights' scope as an engine's own launch_cumulative
            Timed tm(e0, T_WEIGHTS, s);
            if (g->ncum > 0) launch_cumulative_group((const WeightArgs*)(base + szc), P, J, N, K, s);
            launch_weights_group((const WeightArgs*)(base + szc), P, J, N, K, s);
        }
        {
            Timed tm(e0, T_UPDATE, s);
            launch_update_group(J, N, (const UpdateArgs*)(base + szc + szw), P, s);
        }
    }
    err = hipGetLastError();
    if (err != hipSuccess) return gfail(g, STOMP_E_DEVICE, hipGetErrorString(err));
    return 0;
}

int stomp_group_synchronize(stomp_group* g)
{
    if (!g) return gfail(nullptr, STOMP_E_INVALID, "null group");
    DeviceGuard dg(g->device);
    const int P = (int)g->e.size();
    if (int rc = sync_model_flags(g)) return rc;
    bool all = true;
    for (stomp_engine* e : g->e) all = all && e->pending_member >= 0 && !e->tracking;
    if (all) {
        // every engine's pending noiseless rollout in one launch (one workgroup per engine)
        const size_t szc = align256(sizeof(CostArgs) * P);
        const size_t bytes = szc + (g->nterms > 0 ? align256(sizeof(TermsArgs) * P) : 0);
        if (g->staged && hipEventSynchronize(g->staged) != hipSuccess)
            return gfail(g, STOMP_E_DEVICE, "group staging wait failed");
        if (bytes > g->h_cap || bytes > g->d_cap) {
            all = false;   // the arrays of a run are larger; no run yet: per-engine flushes
        } else {
            CostArgs* cas = (CostArgs*)g->h_args;
            TermsArgs* tas = (TermsArgs*)(g->h_args + szc);
            for (int p = 0; p < P; ++p) {
                cas[p] = noiseless_args(g->e[p]);
                if (g->nterms > 0) tas[p] = terms_args(g->e[p], cas[p]);
            }
            hipError_t err = hipMemcpyAsync(g->d_args, g->h_args, bytes, hipMemcpyHostToDevice, g->stream);
            if (err == hipSuccess) err = hipEventRecord(g->staged, g->stream);
            if (err != hipSuccess) return gfail(g, STOMP_E_DEVICE, "group argument upload failed");
            launch_cost_group(g->e[0]->model, g->d_models, (const CostArgs*)g->d_args, P, 1, 0, g->stream);
            if (g->nterms > 0) {
                Timed tm(g->e[0], T_TERMS, g->stream);
                launch_terms_group(g->d_tmodels, (const TermsArgs*)(g->d_args + szc), P, 1, g->e[0]->N, g->terms_lds,
                                   g->stream);
            }
        }
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
// that flush alone.  The host reads the engines' (stop, iterations) mirror one chunk behind the
// chunk it stages.  With g->compact it stages no arguments for an engine it has seen stopped;
// otherwise a stopped engine's blocks stay in the launches and return at its stop flag (the
// default: DESIGN.md 7 has the measurement).
int stomp_group_optimize(stomp_group* g, stomp_stats* stats, double* costs_per_iteration, int32_t costs_stride)
{
    if (!g) return gfail(nullptr, STOMP_E_INVALID, "null group");
    if (!stats) return gfail(g, STOMP_E_INVALID, "null stats");
    const int P = (int)g->e.size();
    int maxcap = 0;
    for (stomp_engine* e : g->e) {
        if (e->tracking) return gfail(g, STOMP_E_INVALID, "an engine of the group is inside its own optimize loop");
        maxcap = std::max(maxcap, e->max_it);
    }
    if (costs_per_iteration && costs_stride < maxcap)
        return gfail(g, STOMP_E_INVALID, "costs_stride is smaller than an engine's max_iterations");
    DeviceGuard dg(g->device);
    hipStream_t s = g->stream;
    stomp_engine* e0 = g->e[0];
    const int J = e0->J, N = e0->N, K = e0->K_loc, chunk = STOMP_GROUP_OPTIMIZE_CHUNK;
    // one step's arguments at most: both rollout launches' CostArgs and DevModel lists, the
    // weights, update and track arguments
    const size_t szc = align256(sizeof(CostArgs) * P), szw = align256(sizeof(WeightArgs) * P),
                 szu = align256(sizeof(UpdateArgs) * P), szt = align256(sizeof(TrackArgs) * P),
                 szm = align256(sizeof(DevModel) * P), szr = e0->Kr > 0 ? align256(sizeof(ReuseRowArgs) * P) : 0,
                 // both rollout launches' TermsArgs and TermsModel lists
                 szx = g->nterms > 0 ? 2 * (align256(sizeof(TermsArgs) * P) + align256(sizeof(TermsModel) * P)) : 0;
    const size_t slot_bytes = (2 * szc + 2 * szm + szw + szu + szt + szr + szx) * (size_t)chunk;
    auto track_args = [&](int p) {
        stomp_engine* e = g->e[p];
        return TrackArgs{e->d_track, e->d_total, e->d_cf, e->d_cs, e->d_opt_costs, e->d_last_traj, e->d_best_traj,
                         e->max_it_cf, e->max_it, g->d_mirror + 2 * p};
    };
    if (!g->d_mirror) {
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
        for (int p = 0; p < P; ++p) ta[p] = track_args(p);
        if (hipMemcpy(g->d_track_all, ta.data(), sizeof(TrackArgs) * P, hipMemcpyHostToDevice) != hipSuccess)
            return gfail(g, STOMP_E_DEVICE, "group argument upload failed");
    }
    // the engines enter in any state: rows out of the pregen buffers, pending noiseless rollouts
    // evaluated, the pregen rows of iteration 1 made where another iteration's are held.  With
    // reuse they are at one point of generateRollouts (all reuse in iteration 1, or none does)
    for (stomp_engine* e : g->e)
        if (e->Kr > 0 && e->reused_next != e0->reused_next)
            return gfail(g, STOMP_E_INVALID, "the engines of a group are not at the same iteration state");
    // host-side generateRollouts state after each staged iteration, to restore for every engine
    // the one of the iteration the device stopped it at (stomp_engine_optimize's)
    struct HostState { bool reused_next, extra_added; int row_set; };
    std::vector<std::vector<HostState>> after(P);
    if (e0->Kr > 0)
        for (int p = 0; p < P; ++p) after[p].resize((size_t)std::max(g->e[p]->max_it, 0));
    const NoiseArgs shape = noise_args(e0, 1);   // J, N, Nall of the reuse launches
    for (stomp_engine* e : g->e) {
        materialize_rows(e);
        flush_noiseless(e);
        if (e->max_it > 0 && e->pre_it != 1) {
            launch_pregen(pregen_args(e, 1), e->K_loc, s);
            e->pre_it = 1;
        }
    }
    launch_track_start_group(g->d_track_all, P, false, s);   // stomp_optimizer.cpp:251 start_time

    std::vector<int> live;
    for (int p = 0; p < P; ++p)
        if (!g->compact || g->e[p]->max_it > 0) live.push_back(p);
    const int last_step = maxcap > 0 ? maxcap + 1 : 0;   // the flush of the engines that ran maxcap iterations
    int next = 1;
    // one chunk of steps staged into `slot`, uploaded and enqueued, then the mirror's read-back
    auto enqueue_chunk = [&](int slot) -> int {
        unsigned char* hb = g->h_opt + (size_t)slot * g->opt_slot;
        unsigned char* db = g->d_opt + (size_t)slot * g->opt_slot;
        size_t used = 0;
        auto take = [&](size_t bytes) {
            const size_t o = used;
            used += align256(bytes);
            return o;
        };
        struct Step {
            int it, nm, nc, nro, ntot;
            bool reuse;
            size_t cas, was, uas, tas, ccs, mms, cms, ras;
            const DevModel* m0;
            // the terms launches after the rollout launch and after the flush: arguments, models,
            // engines with terms among the launch's (0: no launch)
            size_t xas, xms, cxas, cxms;
            int nx, ncx;
        };
        std::vector<Step> steps;
        std::vector<int> prev_main;
        size_t prev_mms = 0, prev_xms = 0;
        int prev_nx = 0;
        const int end = std::min(next + chunk, last_step + 1);
        for (int it = next; it < end; ++it) {
            Step st{};
            st.it = it;
            std::vector<int> main, cohort;
            for (int p : live) {
                if (g->e[p]->max_it >= it) main.push_back(p);
                else if (g->e[p]->max_it == it - 1 && it >= 2) cohort.push_back(p);
            }
            st.nm = (int)main.size();
            st.nc = (int)cohort.size();
            st.cas = take(sizeof(CostArgs) * st.nm);
            st.was = take(sizeof(WeightArgs) * st.nm);
            st.uas = take(sizeof(UpdateArgs) * st.nm);
            st.tas = take(sizeof(TrackArgs) * (st.nm + st.nc));
            st.ccs = take(sizeof(CostArgs) * st.nc);
            st.cms = take(sizeof(DevModel) * st.nc);
            st.ras = e0->Kr > 0 ? take(sizeof(ReuseRowArgs) * st.nm) : 0;
            const bool terms = g->nterms > 0;
            st.xas = terms ? take(sizeof(TermsArgs) * st.nm) : 0;
            st.cxas = terms ? take(sizeof(TermsArgs) * st.nc) : 0;
            st.cxms = terms ? take(sizeof(TermsModel) * st.nc) : 0;
            // the DevModel list of the rollout launch: once per chunk, again where an engine's
            // max_iterations takes it out within the chunk
            if (st.nm > 0 && main != prev_main) {
                prev_mms = take(sizeof(DevModel) * st.nm);
                DevModel* ms = (DevModel*)(hb + prev_mms);
                for (int k = 0; k < st.nm; ++k) ms[k] = g->e[main[k]]->model;
                if (terms) {
                    prev_xms = take(sizeof(TermsModel) * st.nm);
                    TermsModel* xs = (TermsModel*)(hb + prev_xms);
                    prev_nx = 0;
                    for (int k = 0; k < st.nm; ++k) {
                        xs[k] = g->e[main[k]]->terms;
                        prev_nx += g->e[main[k]]->terms_on ? 1 : 0;
                    }
                }
                prev_main = main;
            }
            st.mms = prev_mms;
            st.xms = prev_xms;
            st.nx = st.nm > 0 ? prev_nx : 0;
            if (st.nm > 0) st.m0 = &g->e[main[0]]->model;
            CostArgs* cas = (CostArgs*)(hb + st.cas);
            WeightArgs* was = (WeightArgs*)(hb + st.was);
            UpdateArgs* uas = (UpdateArgs*)(hb + st.uas);
            TrackArgs* tas = (TrackArgs*)(hb + st.tas);
            ReuseRowArgs* ras = (ReuseRowArgs*)(hb + st.ras);
            TermsArgs* xas = (TermsArgs*)(hb + st.xas);
            for (int k = 0; k < st.nm; ++k) {
                stomp_engine* e = g->e[main[k]];
                // inside the optimize loop the noise / params rows are copied out of the pregen
                // buffer (pregen blocks enqueued past a stop overwrite the ping-pong buffers), the
                // weights read d_noise
                if (e->pre_it != it) return gfail(g, STOMP_E_INVALID, "group pregen rows out of step");
                const StagedIteration si = stage_iteration(e, it, false, cas[k], was[k], uas[k], ras + k);
                if (terms) xas[k] = terms_args(e, cas[k]);
                if (k == 0) {
                    st.nro = si.nro;
                    st.ntot = si.ntot;
                    st.reuse = si.reuse;
                } else if (si.nro != st.nro || si.ntot != st.ntot || si.reuse != st.reuse) {
                    return gfail(g, STOMP_E_INVALID, "group engines out of step");
                }
                if (e->Kr > 0) after[main[k]][it - 1] = {e->reused_next, e->extra_added, e->row_set};
                tas[k] = track_args(main[k]);
            }
            CostArgs* ccs = (CostArgs*)(hb + st.ccs);
            DevModel* cms = (DevModel*)(hb + st.cms);
            TermsArgs* cxas = (TermsArgs*)(hb + st.cxas);
            TermsModel* cxms = (TermsModel*)(hb + st.cxms);
            for (int k = 0; k < st.nc; ++k) {
                stomp_engine* e = g->e[cohort[k]];
                ccs[k] = noiseless_args(e);   // with K_r > 0 the extra rollout's rows too
                cms[k] = e->model;
                if (terms) {
                    cxas[k] = terms_args(e, ccs[k]);
                    cxms[k] = e->terms;
                    st.ncx += e->terms_on ? 1 : 0;
                }
                tas[st.nm + k] = track_args(cohort[k]);
            }
            steps.push_back(st);
        }
        next = end;
        if (used > g->opt_slot) return gfail(g, STOMP_E_INVALID, "group optimize staging overflow");
        if (used && hipMemcpyAsync(db, hb, used, hipMemcpyHostToDevice, s) != hipSuccess)
            return gfail(g, STOMP_E_DEVICE, "group argument upload failed");
        for (const Step& st : steps) {
            // with timing on for the group's first engine, its timers hold the group's launches
            if (st.nc > 0) {
                Timed tm(e0, T_NOISELESS, s);
                launch_cost_group(g->e[0]->model, (const DevModel*)(db + st.cms), (const CostArgs*)(db + st.ccs), st.nc,
                                  1, 0, s);
            }
            if (st.ncx > 0) {
                Timed tm(e0, T_TERMS, s);
                launch_terms_group((const TermsModel*)(db + st.cxms), (const TermsArgs*)(db + st.cxas), st.nc, 1, N,
                                   g->terms_lds, s);
            }
            if (st.nm > 0) {
                Timed tm(e0, T_COST, s);
                launch_cost_group(*st.m0, (const DevModel*)(db + st.mms), (const CostArgs*)(db + st.cas), st.nm, st.nro,
                                  K + st.ntot, s);
            }
            // the state-cost terms of both launches before the bookkeeping reads the noiseless
            // rollouts' totals and constraints-satisfied flags
            if (st.nx > 0) {
                Timed tm(e0, T_TERMS, s);
                launch_terms_group((const TermsModel*)(db + st.xms), (const TermsArgs*)(db + st.xas), st.nm, st.nro, N,
                                   g->terms_lds, s);
            }
            // before this step's weights / update: a break decided on the previous iteration's
            // noiseless rollout leaves theta where the reference leaves it
            if (st.it >= 2) launch_track_group((const TrackArgs*)(db + st.tas), st.nm + st.nc, st.it - 2, J * N, s);
            if (st.nm > 0) {
                if (st.reuse) {
                    // after the bookkeeping, as the engine's own loop: a stopped engine's reused
                    // rows stay the ones of the iteration it stopped at
                    Timed tm(e0, T_NOISE, s);
                    launch_reuse_rows_group(shape, (const ReuseRowArgs*)(db + st.ras), st.nm, e0->K, e0->Kr, s);
                }
                {
                    // (the step's own list: compacted, or a stopped engine a no-op at its flag)
                    Timed tm(e0, T_WEIGHTS, s);
                    if (g->ncum > 0) launch_cumulative_group((const WeightArgs*)(db + st.was), st.nm, J, N, K, s);
                    launch_weights_group((const WeightArgs*)(db + st.was), st.nm, J, N, K, s);
                }
                {
                    Timed tm(e0, T_UPDATE, s);
                    launch_update_group(J, N, (const UpdateArgs*)(db + st.uas), st.nm, s);
                }
            }
        }
        if (hipMemcpyAsync(g->h_mirror + (size_t)slot * 2 * P, g->d_mirror, sizeof(int) * 2 * P, hipMemcpyDeviceToHost,
                           s) != hipSuccess ||
            hipEventRecord(g->opt_ev[slot], s) != hipSuccess)
            return gfail(g, STOMP_E_DEVICE, "group read-back failed");
        return 0;
    };
    int rc = 0, inflight = 0, head = 0;
    bool all_stopped = false;
    while (!all_stopped) {
        while (inflight < 2 && next <= last_step) {
            if ((rc = enqueue_chunk((head + inflight) & 1))) break;
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
        if (g->compact) {
            // the engines seen stopped leave every chunk staged from here on
            std::vector<int> keep;
            for (int p : live)
                if (!hm[2 * p]) keep.push_back(p);
            live.swap(keep);
        }
        head ^= 1;
        --inflight;
    }
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
        if (e->Kr > 0 && t.iterations > 0) {
            // the steps staged past the engine's stop were no-ops on the device
            const HostState& h = after[p][t.iterations - 1];
            e->reused_next = h.reused_next;
            e->extra_added = h.extra_added;
            if (e->row_set != h.row_set) swap_row_sets(e);
        }
        if (costs_per_iteration && t.iterations > 0 &&
            hipMemcpy(costs_per_iteration + (size_t)p * costs_stride, e->d_opt_costs, sizeof(double) * t.iterations,
                      hipMemcpyDeviceToHost) != hipSuccess)
            return gfail(g, STOMP_E_DEVICE, "group cost history read-back failed");
        stomp_stats st;
        st.iterations = t.iterations;
        st.success = t.success;
        st.success_iteration = t.success_iteration;
        st.collision_success_iteration = t.collision_success_iteration;
        st.last_improvement_iteration = t.last_improvement_iteration;
        st.best_cost = t.best;
        const double tick_s = e->wall_khz > 0 ? 1.0 / (1000.0 * e->wall_khz) : 0.0;
        st.success_duration = t.success_iteration >= 0 ? (double)(t.t_success - t.t0) * tick_s : 0.0;
        st.collision_success_duration =
            t.collision_success_iteration >= 0 ? (double)(t.t_collision_success - t.t0) * tick_s : 0.0;
        stats[p] = st;
    }
    return 0;
}

}  // extern "C"
