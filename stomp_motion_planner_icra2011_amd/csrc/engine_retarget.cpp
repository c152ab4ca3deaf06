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
    for (int p = 0; p < P; ++p) {
        stomp_engine* e = es[p];
        e->start.assign(starts + (size_t)p * J, starts + (size_t)(p + 1) * J);
        e->goal.assign(goals + (size_t)p * J, goals + (size_t)(p + 1) * J);
        if (seeds) e->seed = seeds[p];
        e->model.pad_collision = flags[p];
        e->pad_collision = flags[p];
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
    return 0;
}

}  // namespace stomp

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
