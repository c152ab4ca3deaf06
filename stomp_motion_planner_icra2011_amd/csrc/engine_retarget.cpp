// engine_retarget.cpp -- the one path behind the four retarget entry points: live engines put onto
// their next requests.  A request is a new start, goal and seed and, where it replaces them, the
// collision points and the path constraints; stomp_engine_retarget and stomp_group_retarget make
// requests that keep both.  Only four things in an engine depend on the start and goal: the two
// vectors, theta_0, the padding rows' sphere positions with their collision flag, and the noise
// seed.  Every request is validated and its model planned on the host (request_validate,
// request_plan); then one upload, one launch (k_retarget) and one read-back of the P flags remake
// the device side of all P engines of a call (request_engines), and the host drops every piece of
// iteration state that was made with the old problem (retarget_host_state), so that the engine is
// the one stomp_engine_create would return for the new one.  For a kept model the plan is a copy of
// the engine's fields: nothing is allocated but the call's staging, and that once.
#include "engine_internal.h"

using namespace stomp;

namespace stomp {

// the host side of a retarget, once the launch has run: the new vectors, seed and flag, and every
// piece of iteration state dropped
void retarget_host_state(stomp_engine* e, const double* start, const double* goal, const uint64_t* seed, int flag)
{
    e->start.assign(start, start + e->J);
    e->goal.assign(goal, goal + e->J);
    if (seed) e->seed = *seed;
    e->model.pad_collision = flag;
    e->pad_collision = flag;
    ++e->target_epoch;
    // made with the old theta, start, goal and seed: the noiseless rollout not evaluated yet,
    // the rows made ahead, the reuse ranking's inputs (which row set is written next is the
    // engine's own and stays), the step API's state (stomp_pi_reset's, and its weight)
    e->pending_member = -1;
    e->pre_it = -1;
    e->rows_in_pre = false;
    e->rows_eps = nullptr;
    e->reused_next = false;
    e->extra_added = false;
    e->x_foreign = false;
    e->K_gen = 0;
    e->pi_weight = e->w_smooth;
    e->cur_it = -1;
}

// k_retarget's arguments for an engine that keeps its model, outside a retarget call (a serve
// loop's turnover): request_launch's entry of a request that replaces nothing
RequestArgs kept_request_args(const stomp_engine* e, const double* d_vec, int* d_flag_out, DevModel* list_entry)
{
    RequestArgs r;
    std::memset(&r, 0, sizeof r);
    r.model = e->model;
    r.stage = d_vec;
    r.Rb = e->d_Rb; r.RinvT = e->d_RinvT;
    r.theta = e->d_theta; r.last_traj = e->d_last_traj; r.best_traj = e->d_best_traj;
    r.start = e->d_start; r.goal = e->d_goal;
    r.pad_pos = (double*)e->model.pad_pos; r.pad_cf = e->d_pad_cf;
    r.model_flag = list_entry ? &list_entry->pad_collision : nullptr;
    r.flag_out = d_flag_out;
    r.stage_img = e->model.img;   // the tables are the engine's own, which no workgroup writes
    r.img_out = e->d_img;
    r.oc_out = (unsigned long long*)e->d_oc;
    r.cs = e->d_cs;
    r.terms = e->terms;
    return r;
}

namespace {

bool all_finite(const double* v, int n)
{
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// where one call's staging holds what: [P] RequestArgs, [P][2][J] vectors, engine p's image tables
// and constraint table, [P] flags (the upload ends where the flags begin)
struct StageMap {
    size_t vec = 0, flag = 0, total = 0;
    std::vector<size_t> img, oc;
    StageMap(int P, int J, const std::vector<ModelPlan>& plans) : img(P, 0), oc(P, 0)
    {
        vec = align256(sizeof(RequestArgs) * P);
        size_t o = vec + align256(sizeof(double) * 2 * J * P);
        for (int p = 0; p < P; ++p) {
            img[p] = o;
            o += align256(plans[p].spheres ? plans[p].img.size() : 0);
            oc[p] = o;
            o += align256(plans[p].constraints ? sizeof(OcDev) * plans[p].oc.size() : 0);
        }
        flag = o;
        total = flag + align256(sizeof(int) * P);
    }
};

}  // namespace

int request_validate(const stomp_engine* e, const stomp_request* r, int p)
{
    for (int d = 0; d < e->J; ++d)
        if (!std::isfinite(r->start[d]) || !std::isfinite(r->goal[d]))
            return fail(nullptr, STOMP_E_INVALID, "retarget: start / goal of engine %d, joint %d is not finite", p, d);
    if (r->num_spheres < -1 || (r->num_spheres > 0 && !r->spheres))
        return fail(nullptr, STOMP_E_INVALID, "retarget: request %d has %d spheres and no sphere array", p, r->num_spheres);
    if (r->num_orientation_constraints < -1)
        return fail(nullptr, STOMP_E_INVALID, "invalid orientation constraints");
    for (int j = 0; j < r->num_spheres; ++j)
        if (!all_finite(r->spheres[j].pos, 3))
            return fail(nullptr, STOMP_E_INVALID, "retarget: sphere %d of request %d is not finite", j, p);
    if (r->num_spheres > 0)
        if (int rc = validate_spheres(r->spheres, r->num_spheres, e->nseg, e->model.res)) return rc;
    if (r->num_orientation_constraints >= 0) {
        if (int rc = validate_constraints(r->orientation_constraints, r->num_orientation_constraints, e->nseg)) return rc;
        for (int c = 0; c < r->num_orientation_constraints; ++c) {
            const stomp_orientation_constraint& oc = r->orientation_constraints[c];
            // (a tolerance may be infinite: at pi and above its axis is unconstrained)
            if (!all_finite(oc.orientation, 4) || !std::isfinite(oc.weight) || std::isnan(oc.absolute_roll_tolerance) ||
                std::isnan(oc.absolute_pitch_tolerance) || std::isnan(oc.absolute_yaw_tolerance))
                return fail(nullptr, STOMP_E_INVALID, "retarget: orientation constraint %d of request %d is not finite", c, p);
        }
    }
    if (e->world > 1 || e->gather)
        return fail(nullptr, STOMP_E_UNSUPPORTED, "retargeting is single-rank (a sharded engine's ranks would "
                                                  "have to retarget in lockstep)");
    if (e->tracking) return fail(nullptr, STOMP_E_INVALID, "retarget: an engine is inside its optimize loop");
    return 0;
}

int request_plan(const stomp_engine* e, const stomp_request* r, ModelPlan& plan)
{
    plan.spheres = r->num_spheres >= 0;
    plan.constraints = r->num_orientation_constraints >= 0;
    plan.m = e->model;
    plan.terms = e->terms;
    plan.terms_on = e->terms_on;
    // creation's order, so that a request two stages would refuse gets creation's message
    if (plan.spheres)
        if (int rc = plan_model_tables(nullptr, e, r->spheres, r->num_spheres, plan.mt)) return rc;
    if (plan.constraints) {
        if (int rc = plan_constraints(nullptr, e, r->orientation_constraints, r->num_orientation_constraints, plan.oc))
            return rc;
        plan.terms.noc = (int)plan.oc.size();
        plan.terms_on = plan.terms.torque != 0 || plan.terms.noc > 0;
        if (int rc = plan_terms(nullptr, e, plan.terms, plan.terms_on)) return rc;
    }
    if (plan.spheres) {
        if (int rc = choose_layout(nullptr, e, plan.mt, plan.m)) return rc;
        plan.img = build_model_image(e, plan.mt, plan.m);
    }
    return 0;
}

size_t request_stage_bytes(stomp_engine* const* es, int P, const std::vector<ModelPlan>& plans)
{
    return StageMap(P, es[0]->J, plans).total;
}

namespace {

// the device memory the new models need, grown before anything is enqueued -- into the plans' own
// copies of the engines' buffer fields: no engine is touched, and nothing an enqueued launch reads
// is freed or rewritten (a replaced buffer waits in the plan's `retired`)
int request_buffers(stomp_engine* const* es, int P, std::vector<ModelPlan>& plans)
{
    for (int p = 0; p < P; ++p) {
        stomp_engine* e = es[p];
        ModelPlan& pl = plans[p];
        pl.d_img = e->d_img; pl.img_cap = e->img_cap;
        pl.d_oc = e->d_oc; pl.oc_cap = e->oc_cap;
        pl.d_sv = e->d_sv; pl.sv_cap = e->sv_cap;
        pl.d_terms_traj = e->d_terms_traj;
        if (pl.spheres) {
            if (int rc = grow_buffer(e, &pl.d_img, &pl.img_cap, model_image_bytes(e, pl.m) / 8, &pl.live)) return rc;
            point_model_into_image(e, pl.m, pl.d_img);
            if (int rc = place_saved_frames(e, pl.m, &pl.d_sv, &pl.sv_cap, &pl.live)) return rc;
        }
        if (pl.constraints) {
            if (int rc = grow_buffer(e, &pl.d_oc, &pl.oc_cap, pl.oc.size(), &pl.live)) return rc;
            pl.terms.oc = pl.oc.empty() ? nullptr : pl.d_oc;
        }
        pl.terms.segs = pl.m.segs;
        if (pl.terms_on && !pl.d_terms_traj) {   // the first time this engine gets terms
            size_t cap = 0;
            if (int rc = grow_buffer(e, &pl.d_terms_traj, &cap, (size_t)e->K_loc * e->J * e->N, &pl.live)) return rc;
        }
    }
    return 0;
}

int request_launch(stomp_engine* const* es, int P, const stomp_request* rs, const std::vector<ModelPlan>& plans,
                   unsigned char* h, unsigned char* d, DevModel* d_models, TermsModel* d_tmodels, bool replaces,
                   const int** flags_out)
{
    stomp_engine* e0 = es[0];
    const int J = e0->J, N = e0->N;
    hipStream_t s = e0->stream;
    const StageMap at(P, J, plans);
    RequestArgs* as = (RequestArgs*)h;
    double* vec = (double*)(h + at.vec);
    int* flags = (int*)(h + at.flag);
    for (int p = 0; p < P; ++p) {
        stomp_engine* e = es[p];
        const ModelPlan& pl = plans[p];
        replaces = replaces || pl.spheres || pl.constraints;
        RequestArgs& r = as[p];
        std::memset(&r, 0, sizeof r);
        r.model = pl.m;
        r.stage = (const double*)(d + at.vec) + (size_t)p * 2 * J;
        r.Rb = e->d_Rb; r.RinvT = e->d_RinvT;
        r.theta = e->d_theta; r.last_traj = e->d_last_traj; r.best_traj = e->d_best_traj;
        r.start = e->d_start; r.goal = e->d_goal;
        r.pad_pos = (double*)pl.m.pad_pos; r.pad_cf = e->d_pad_cf;
        r.model_flag = d_models ? &d_models[p].pad_collision : nullptr;
        r.flag_out = (int*)(d + at.flag) + p;
        // collision points kept: the tables are the engine's own, which no workgroup writes
        r.stage_img = pl.spheres ? (const unsigned long long*)(d + at.img[p]) : pl.m.img;
        r.img_out = pl.d_img;
        r.img_words = pl.spheres ? (int)(pl.img.size() / 8) : 0;
        r.stage_oc = (const unsigned long long*)(d + at.oc[p]);
        r.oc_out = (unsigned long long*)pl.d_oc;
        r.oc_words = pl.constraints ? (int)(sizeof(OcDev) * pl.oc.size() / 8) : 0;
        r.cs = e->d_cs;
        r.terms = pl.terms;
        r.model_out = d_models ? &d_models[p] : nullptr;
        r.terms_out = d_tmodels ? &d_tmodels[p] : nullptr;
        // what the launch writes stays inside the buffers it is given
        if ((size_t)r.img_words > pl.img_cap || (pl.constraints && pl.oc.size() > pl.oc_cap) ||
            (pl.spheres && model_image_bytes(e, pl.m) / 8 > pl.img_cap))
            return fail(nullptr, STOMP_E_DEVICE, "retarget: a model buffer is smaller than its model");
        std::memcpy(vec + (size_t)p * 2 * J, rs[p].start, sizeof(double) * J);
        std::memcpy(vec + (size_t)p * 2 * J + J, rs[p].goal, sizeof(double) * J);
        if (pl.spheres && !pl.img.empty()) std::memcpy(h + at.img[p], pl.img.data(), pl.img.size());
        if (pl.constraints && !pl.oc.empty()) std::memcpy(h + at.oc[p], pl.oc.data(), sizeof(OcDev) * pl.oc.size());
    }
    // ordered on the stream after everything enqueued before: iterations still in flight read the
    // old image, the old constraint table and the group's old model entries, and a
    // stomp_engine_refresh_field's bricks are the ones the padding FK reads
    HIP_TRY(nullptr, hipMemcpyAsync(d, h, at.flag, hipMemcpyHostToDevice, s));
    launch_retarget((const RequestArgs*)d, P, J, N, replaces, s);
    HIP_TRY(nullptr, hipGetLastError());
    HIP_TRY(nullptr, hipMemcpyAsync(flags, d + at.flag, sizeof(int) * P, hipMemcpyDeviceToHost, s));
    HIP_TRY(nullptr, hipStreamSynchronize(s));
    *flags_out = flags;
    return 0;
}

}  // namespace

int request_engines(stomp_engine* const* es, int P, const stomp_request* rs, std::vector<ModelPlan>& plans,
                    unsigned char* h, unsigned char* d, DevModel* d_models, TermsModel* d_tmodels, bool lists_behind)
{
    const int* flags = nullptr;
    int rc = request_buffers(es, P, plans);
    if (!rc) rc = request_launch(es, P, rs, plans, h, d, d_models, d_tmodels, lists_behind, &flags);
    if (rc) {
        // nothing was handed to an engine yet: what the call allocated is given back (the stream is
        // waited for first, a launch of this call may still write the new buffers)
        (void)hipStreamSynchronize(es[0]->stream);
        for (ModelPlan& pl : plans) live_alloc_abort(pl.live);
        es[0]->err = g_last_error;
        return rc;
    }
    for (int p = 0; p < P; ++p) {
        stomp_engine* e = es[p];
        ModelPlan& pl = plans[p];
        e->d_img = pl.d_img; e->img_cap = pl.img_cap;
        e->d_oc = pl.d_oc; e->oc_cap = pl.oc_cap;
        e->d_sv = pl.d_sv; e->sv_cap = pl.sv_cap;
        e->d_terms_traj = pl.d_terms_traj;
        if (pl.spheres) {
            e->S = pl.m.S;
            e->mt = std::move(pl.mt);
            e->model = pl.m;
            e->d_pad_pos = (double*)pl.m.pad_pos;
            e->tq_model.segs = pl.m.segs;
        }
        e->terms = pl.terms;
        e->terms_on = pl.terms_on;
        if (pl.spheres || pl.constraints) ++e->model_epoch;
        retarget_host_state(e, rs[p].start, rs[p].goal, &rs[p].seed, flags[p]);
        live_alloc_commit(e, pl.live);   // (the stream has passed every launch that read the replaced buffers)
    }
    return 0;
}

bool reserve_stage(unsigned char** h, unsigned char** d, size_t* cap, size_t bytes)
{
    if (bytes <= *cap) return true;
    const size_t grown = std::max(bytes, 2 * *cap);
    // (no launch reads the old staging: every call that used it waited for the stream)
    if (*h) hipHostFree(*h);
    if (*d) hipFree(*d);
    *h = *d = nullptr;
    *cap = 0;
    if (hipHostMalloc((void**)h, grown) != hipSuccess || hipMalloc((void**)d, grown) != hipSuccess) return false;
    *cap = grown;
    return true;
}

}  // namespace stomp

namespace {

// What both engine entry points do once their arguments are checked: e onto request r.  A refusal
// writes nothing of the engine, not even its message (stomp_last_error has it), so the "inside its
// optimize loop" refusal may be made from another host thread than the loop's (stomp_engine_retarget
// copies the message into the engine afterwards, as its callers expect).
int retarget_engine(stomp_engine* e, const stomp_request* r)
{
    if (int rc = request_validate(e, r, 0)) return rc;   // host only: no device is touched yet
    // the plan asks the rollout kernels' attributes of the current device: the engine's
    DeviceGuard dg(e->device);
    std::vector<ModelPlan> plans(1);
    if (int rc = request_plan(e, r, plans[0])) return rc;
    const size_t cap = e->rq_cap;
    if (!reserve_stage(&e->h_rq, &e->d_rq, &e->rq_cap, request_stage_bytes(&e, 1, plans)))
        return fail(e, STOMP_E_DEVICE, "retarget staging allocation failed");
    if (e->rq_cap != cap) e->rq_allocs += 2;
    return request_engines(&e, 1, r, plans, e->h_rq, e->d_rq, nullptr, nullptr, false);
}

}  // namespace

extern "C" int stomp_engine_retarget_request(stomp_engine* e, const stomp_request* r)
{
    // (up to here e is not touched)
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    if (!r) return fail(nullptr, STOMP_E_INVALID, "retarget: null request");
    if (r->struct_size != (int32_t)sizeof(stomp_request))
        return fail(nullptr, STOMP_E_INVALID, "retarget: struct_size is not sizeof(stomp_request)");
    if (!r->start || !r->goal) return fail(nullptr, STOMP_E_INVALID, "retarget: null start or goal");
    return retarget_engine(e, r);
}

extern "C" int stomp_engine_model_info(stomp_engine* e, int64_t info[12])
{
    if (!e || !info) return fail(nullptr, STOMP_E_INVALID, "null argument");
    const DevModel& m = e->model;
    const int64_t v[12] = {m.S, m.nops, m.nslots, m.nsaves, m.sph_chunk, m.pad_lds, m.lean, m.sincos_pre,
                           e->terms.noc, e->terms_on ? 1 : 0, e->model_epoch, e->rq_allocs};
    std::memcpy(info, v, sizeof v);
    return 0;
}

extern "C" int stomp_engine_retarget(stomp_engine* e, const double* start, const double* goal, uint64_t seed)
{
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    if (!start || !goal) return fail(nullptr, STOMP_E_INVALID, "retarget: null start or goal");   // (e not touched)
    const stomp_request r = kept_request(start, goal, seed);
    const int rc = retarget_engine(e, &r);
    if (rc) e->err = g_last_error;
    return rc;
}
