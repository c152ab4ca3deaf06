// engine_retarget.cpp -- stomp_engine_retarget, and the part of it stomp_group_retarget shares:
// a live engine put onto a new start, goal and seed.  Only four things in an engine depend on the
// request: the start / goal vectors, theta_0, the padding rows' sphere positions with their
// collision flag, and the noise seed.  One launch (k_retarget) remakes the device side of all P
// engines of a call, one read-back fetches the P flags, and the host drops every piece of
// iteration state that was made with the old problem, so that the engine is the one
// stomp_engine_create would return for the new one.
#include "engine_internal.h"

using namespace stomp;

namespace stomp {

size_t retarget_stage_bytes(int P, int J)
{
    return align256(sizeof(RetargetArgs) * P) + align256(sizeof(double) * 2 * J * P) + align256(sizeof(int) * P);
}

int retarget_validate(stomp_engine* const* es, int P, const double* starts, const double* goals)
{
    if (!starts || !goals) return fail(nullptr, STOMP_E_INVALID, "retarget: null start or goal");
    for (int p = 0; p < P; ++p) {
        const int J = es[p]->J;
        for (int d = 0; d < J; ++d)
            if (!std::isfinite(starts[(size_t)p * J + d]) || !std::isfinite(goals[(size_t)p * J + d]))
                return fail(nullptr, STOMP_E_INVALID, "retarget: start / goal of engine %d, joint %d is not finite", p, d);
    }
    for (int p = 0; p < P; ++p)
        if (es[p]->world > 1 || es[p]->gather)
            // its ranks would have to retarget in lockstep (as the PolicyImprovement API on ranks)
            return fail(nullptr, STOMP_E_UNSUPPORTED, "retargeting is single-rank (a sharded engine's ranks would "
                                                      "have to retarget in lockstep)");
    for (int p = 0; p < P; ++p)
        if (es[p]->tracking) return fail(nullptr, STOMP_E_INVALID, "retarget: an engine is inside its optimize loop");
    return 0;
}

int retarget_engines(stomp_engine* const* es, int P, const double* starts, const double* goals,
                     const uint64_t* seeds, unsigned char* h, unsigned char* d, DevModel* d_models)
{
    stomp_engine* e0 = es[0];
    const int J = e0->J, N = e0->N;
    hipStream_t s = e0->stream;
    const size_t o_vec = align256(sizeof(RetargetArgs) * P), o_flag = o_vec + align256(sizeof(double) * 2 * J * P);
    RetargetArgs* as = (RetargetArgs*)h;
    double* vec = (double*)(h + o_vec);
    int* flags = (int*)(h + o_flag);
    for (int p = 0; p < P; ++p) {
        stomp_engine* e = es[p];
        RetargetArgs& a = as[p];
        a.model = e->model;
        a.stage = (const double*)(d + o_vec) + (size_t)p * 2 * J;
        a.Rb = e->d_Rb; a.RinvT = e->d_RinvT;
        a.theta = e->d_theta; a.last_traj = e->d_last_traj; a.best_traj = e->d_best_traj;
        a.start = e->d_start; a.goal = e->d_goal;
        a.pad_pos = e->d_pad_pos; a.pad_cf = e->d_pad_cf;
        a.model_flag = d_models ? &d_models[p].pad_collision : nullptr;
        a.flag_out = (int*)(d + o_flag) + p;
        std::memcpy(vec + (size_t)p * 2 * J, starts + (size_t)p * J, sizeof(double) * J);
        std::memcpy(vec + (size_t)p * 2 * J + J, goals + (size_t)p * J, sizeof(double) * J);
    }
    // ordered on the stream after everything enqueued before: iterations still in flight, and a
    // stomp_engine_refresh_field whose bricks the padding FK reads
    HIP_TRY(e0, hipMemcpyAsync(d, h, o_flag, hipMemcpyHostToDevice, s));
    launch_retarget((const RetargetArgs*)d, P, J, N, s);
    HIP_TRY(e0, hipGetLastError());
    HIP_TRY(e0, hipMemcpyAsync(flags, d + o_flag, sizeof(int) * P, hipMemcpyDeviceToHost, s));
    HIP_TRY(e0, hipStreamSynchronize(s));
    for (int p = 0; p < P; ++p)
        retarget_host_state(es[p], starts + (size_t)p * J, goals + (size_t)p * J, seeds ? &seeds[p] : nullptr, flags[p]);
    return 0;
}

// the host side of a retarget, once the launch has run: the new vectors, seed and flag, and every
// piece of iteration state dropped
void retarget_host_state(stomp_engine* e, const double* start, const double* goal, const uint64_t* seed, int flag)
{
    e->start.assign(start, start + e->J);
    e->goal.assign(goal, goal + e->J);
    if (seed) e->seed = *seed;
    e->model.pad_collision = flag;
    e->pad_collision = flag;
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

// ---------------------------------------------------------------- requests with a model
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
    const int J = e->J;
    if (!all_finite(r->start, J) || !all_finite(r->goal, J))
        return fail(nullptr, STOMP_E_INVALID, "retarget: start / goal of engine %d is not finite", p);
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

int request_plan(const stomp_engine* e, const stomp_request* r, int p, ModelPlan& plan)
{
    if (int rc = request_validate(e, r, p)) return rc;
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
                   unsigned char* h, unsigned char* d, DevModel* d_models, TermsModel* d_tmodels, const int** flags_out)
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
        RequestArgs& r = as[p];
        std::memset(&r, 0, sizeof r);
        RetargetArgs& a = r.rt;
        a.model = pl.m;
        a.stage = (const double*)(d + at.vec) + (size_t)p * 2 * J;
        a.Rb = e->d_Rb; a.RinvT = e->d_RinvT;
        a.theta = e->d_theta; a.last_traj = e->d_last_traj; a.best_traj = e->d_best_traj;
        a.start = e->d_start; a.goal = e->d_goal;
        a.pad_pos = (double*)pl.m.pad_pos; a.pad_cf = e->d_pad_cf;
        a.model_flag = d_models ? &d_models[p].pad_collision : nullptr;
        a.flag_out = (int*)(d + at.flag) + p;
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
    // old image, the old constraint table and the group's old model entries
    HIP_TRY(nullptr, hipMemcpyAsync(d, h, at.flag, hipMemcpyHostToDevice, s));
    launch_retarget_model((const RequestArgs*)d, P, J, N, s);
    HIP_TRY(nullptr, hipGetLastError());
    HIP_TRY(nullptr, hipMemcpyAsync(flags, d + at.flag, sizeof(int) * P, hipMemcpyDeviceToHost, s));
    HIP_TRY(nullptr, hipStreamSynchronize(s));
    *flags_out = flags;
    return 0;
}

}  // namespace

int request_engines(stomp_engine* const* es, int P, const stomp_request* rs, std::vector<ModelPlan>& plans,
                    unsigned char* h, unsigned char* d, DevModel* d_models, TermsModel* d_tmodels)
{
    const int* flags = nullptr;
    int rc = request_buffers(es, P, plans);
    if (!rc) rc = request_launch(es, P, rs, plans, h, d, d_models, d_tmodels, &flags);
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

}  // namespace stomp

namespace {

// one call's staging of `bytes`, pinned and on the device, held with a capacity
int reserve_request_stage(stomp_engine* e, size_t bytes)
{
    if (bytes <= e->rq_cap) return 0;
    const size_t cap = std::max(bytes, 2 * e->rq_cap);
    // (no launch reads the old staging: every call that used it waited for the stream)
    if (e->h_rq) hipHostFree(e->h_rq);
    if (e->d_rq) hipFree(e->d_rq);
    e->h_rq = e->d_rq = nullptr;
    e->rq_cap = 0;
    if (hipHostMalloc((void**)&e->h_rq, cap) != hipSuccess || hipMalloc((void**)&e->d_rq, cap) != hipSuccess)
        return fail(e, STOMP_E_DEVICE, "retarget staging allocation failed");
    e->rq_cap = cap;
    e->rq_allocs += 2;
    return 0;
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
    if (r->num_spheres == -1 && r->num_orientation_constraints == -1)   // the model kept: retarget's own launch
        return stomp_engine_retarget(e, r->start, r->goal, r->seed);
    // the plan asks the rollout kernels' attributes of the current device: the engine's.  A refusal
    // writes nothing of the engine, not even its message (stomp_last_error has it), so the "inside
    // its optimize loop" refusal may be made from another host thread than the loop's
    DeviceGuard dg(e->device);
    std::vector<ModelPlan> plans(1);
    if (int rc = request_plan(e, r, 0, plans[0])) return rc;
    if (int rc = reserve_request_stage(e, request_stage_bytes(&e, 1, plans))) return rc;
    return request_engines(&e, 1, r, plans, e->h_rq, e->d_rq, nullptr, nullptr);
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
    if (int rc = retarget_validate(&e, 1, start, goal)) {
        e->err = g_last_error;
        return rc;
    }
    DeviceGuard dg(e->device);
    if (!e->d_rt) {
        const size_t bytes = retarget_stage_bytes(1, e->J);
        if (!e->h_rt && hipHostMalloc((void**)&e->h_rt, bytes) != hipSuccess)
            return fail(e, STOMP_E_DEVICE, "hipHostMalloc failed");
        if (int rc = dev_alloc(e, &e->d_rt, bytes)) return rc;
    }
    return retarget_engines(&e, 1, start, goal, &seed, e->h_rt, e->d_rt, nullptr);
}
