// engine_internal.h -- what the engine's host translation units share: the engine struct, the
// error / device / timing helpers every entry point uses, the small per-iteration helpers (inline:
// stomp_engine_run and stomp_group_run call them once per engine and iteration), and the
// declarations of the helpers one file defines for another.
//   engine.cpp           release, the launch helpers, enqueue_iteration, the C-ABI entry points
//   engine_create.cpp    descriptor validation and stomp_engine_create's stages
//   engine_exchange.cpp  the in-process group, the RCCL path, the collectives, calibration
//   engine_group.cpp     stomp_group: one launcher of a grouped step (launch_step) and one arena of
//                        staged arguments behind run, synchronize and optimize (engine_group.h: what
//                        it shares with engine_serve.cpp)
//   engine_serve.cpp     stomp_group_serve: the optimize loop over a queue, a slot that stops taking
//                        the next request; stomp_serve_schedule, its decisions as a host-only function
//   engine_retarget.cpp  the one retarget path (validate, plan, stage, launch, commit) behind
//                        stomp_engine_retarget, stomp_engine_retarget_request and the two group calls
//   engine_query.cpp     stomp_engine_query_states: a batch of joint states against the engine's
//                        current model and field (k_query.hip), chunked through one staging block
//   sdf_build.cpp        the distance-field builders (does not include this header)
//   scene.cpp            stomp_scene: the field kept in a static and a dynamic layer (uses fail and
//                        DeviceGuard only)
#pragma once

#include "stomp_engine.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "kernels.h"
#include "setup.h"

struct ncclComm;   // RCCL's communicator (ncclComm_t is a pointer to it)

namespace stomp {

enum TimerId { T_NOISE = 0, T_COST, T_WEIGHTS, T_UPDATE, T_NOISELESS, T_REUSE, T_TERMS, T_PREGEN, T_COUNT };
inline constexpr const char* kTimerNames[T_COUNT] = {"noise", "rollout_cost", "weights", "update", "noiseless", "reuse",
                                                     "state_terms", "pregen"};

// In-process exchange group: the ranks of one sharded problem as engines of ONE process, each
// driven by its own host thread (one per device, or several on one device).  The collectives are
// device-to-device copies on the ranks' own streams, ordered by HIP events and two host barriers
// per collective (publish -> copy -> done), in place of RCCL.  Created by stomp_comm_local_id.
struct LocalGroup {
    int world = 0;
    std::mutex mu;
    std::condition_variable cv;
    struct Slot {
        const void* src = nullptr;
        hipEvent_t ready = nullptr, done = nullptr;
        int device = 0;
    };
    std::vector<Slot> slot;
    std::vector<char> joined;
    long long phase = 0;    // completed barrier phases
    int arrived = 0;
    // the decomposition every rank must run (gather, K, J, N), set by the first rank to join: a
    // rank that disagrees would post different collectives, so its creation fails instead
    bool has_sig = false;
    long long sig[6] = {0, 0, 0, 0, 0, 0};   // gather, K, J, N, K_r, split_modes (join_exchange)
    bool broken = false;    // a rank timed out: every later barrier fails at once
    // all ranks arrive (or the wait times out: a rank not driven from a thread of its own)
    bool barrier(std::unique_lock<std::mutex>& lk)
    {
        if (broken) return false;
        const long long my = phase;
        if (++arrived == world) {
            arrived = 0;
            ++phase;
            cv.notify_all();
            return true;
        }
        if (!cv.wait_for(lk, std::chrono::seconds(120), [&] { return phase != my || broken; }) || broken) {
            broken = true;
            cv.notify_all();
            return false;
        }
        return true;
    }
};

// The host tables that depend on the collision points: the FK program, each sphere's published
// frame slot, each slot's first sphere, the spheres as the kernels hold them.  Made by
// plan_model_tables at creation and again, on a live engine, by stomp_engine_retarget_request.
struct ModelTables {
    int S = 0, nslots = 0;
    std::vector<FkOp> ops;
    std::vector<int> sphere_slot, slot_sph;
    std::vector<DevSphere> sph;
};

}  // namespace stomp

struct stomp_engine {
    std::string err;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int J = 0, N = 0, Nall = 0, K = 0, Kr = 0, K_loc = 0, first = 0, S = 0, nseg = 0;
    int world = 1, rank = 0;
    bool split_modes = false;   // weights in the MINMAX / PSUM / USUM phases (world > 1, or the debug hook)
    // gather mode (world > 1, small K N): every rank makes and prices the noise rows of all K rollouts
    // (counter-based, so no noise moves), evaluates its own K_loc, and one all-gather of the state-cost
    // rows per iteration gives every rank the whole cost matrix for the fused weights and the update
    bool gather = false;
    int rows = 0, row0 = 0;   // rollout rows held per iteration (K_loc, or K in gather mode); own rows' offset
    // the decomposition measured at creation (calibrate_shard_mode): both are possible and none was
    // requested, so the buffers hold all K rows and the ranks time each decomposition's compute and
    // collectives, then pick the faster.  shard_info: mode, T_gather, T_partials (us per iteration
    // without exchanges), L_allreduce, L_allgather_state, L_allgather_partials (us per collective)
    bool calibrate = false;
    double shard_info[6] = {0, 0, 0, 0, 0, 0};
    uint64_t seed = 0;
    double disc = 0.05, w_smooth = 0, w_obs = 0, w_con = 0, w_tq = 0;
    double smooth[3] = {0, 0, 0};
    int use_cum = 0, max_it = 0, max_it_cf = 0;
    std::vector<double> sig_std, sig_dec, start, goal;
    stomp::SetupOutput su;
    stomp::DevModel model{};
    stomp::TermsModel terms{};
    bool terms_on = false;      // torque term / path constraints: k_terms after every k_rollout
    double* d_terms_traj = nullptr;   // [K_loc][J][N] joint-limited trajectories for k_terms
    uint8_t* d_cs = nullptr;          // last_trajectory_constraints_satisfied_ of the noiseless rollout
    stomp::DevTrack* d_track = nullptr;   // device-resident optimize loop state; d_track->stop gates every launch
    const int* d_stop = nullptr;
    double* d_opt_costs = nullptr;    // [max_iterations] last_trajectory_cost_ per iteration
    stomp::DevTrack* h_track = nullptr;   // pinned read-back slots
    // inside stomp_engine_optimize: k_track after each noiseless rollout.  Atomic: the retarget
    // calls' "inside its optimize loop" refusal may come from another host thread than the loop's
    std::atomic<bool> tracking{false};
    stomp::ModelTables mt;          // the FK program and the sphere tables of the current collision points
    // what the model stages read again on a live engine (stomp_engine_retarget_request): the
    // kinematic tree and the joint limits as the LDS image holds them
    std::vector<stomp::DevSegment> h_segs;
    std::vector<int> h_has_lim;
    std::vector<double> h_jmin, h_jmax;
    // held with a capacity, reallocated only when a request needs more than every earlier one: the
    // LDS image (8-byte words), the path constraints' table (entries), the lean layout's saved-frame
    // blocks (doubles), one retarget call's staging (pinned and device, bytes; allocated by the
    // engine's first call -- a group stages its engines in buffers of its own)
    unsigned long long* d_img = nullptr;
    size_t img_cap = 0;
    stomp::OcDev* d_oc = nullptr;
    size_t oc_cap = 0;
    double* d_sv = nullptr;
    size_t sv_cap = 0;
    unsigned char *h_rq = nullptr, *d_rq = nullptr;
    size_t rq_cap = 0;
    // model changes so far (a group compares it with the epoch it last saw), and the device or
    // pinned allocations made inside retarget calls of either kind (the staging's included)
    long long model_epoch = 0, rq_allocs = 0;
    // retargets of either kind and stomp_engine_refresh_field calls so far: with model_epoch, what a
    // CHOMP object (engine_chomp.cpp) compares with the values of its last reset
    long long target_epoch = 0;
    // the state query (engine_query.cpp): one chunk's staging, pinned and on the device, held with a
    // capacity; the events around a chunk's launches; the last call's chunks, launches, states per
    // chunk and device time (ms), and the allocations made inside query calls so far
    unsigned char *h_qs = nullptr, *d_qs = nullptr;
    size_t qs_cap = 0;
    hipEvent_t q_ev[2] = {nullptr, nullptr};
    long long q_chunks = 0, q_launches = 0, q_allocs = 0, q_chunk_states = 0;
    double q_kernel_ms = 0.0;
    std::vector<void*> allocs;
    double *d_theta = nullptr, *d_LT = nullptr, *d_MT = nullptr, *d_QT = nullptr;
    double *d_params = nullptr, *d_noise = nullptr, *d_control = nullptr, *d_prob = nullptr, *d_state = nullptr;
    // K_r > 0: a second set of rollout rows.  Each reusing iteration swaps the sets, so the
    // previous iteration's rows (ranked and copied by the reuse kernels) stay intact while this
    // iteration's rollout launch writes its generated rows; row_set counts the swaps mod 2
    double *d_params_b = nullptr, *d_noise_b = nullptr, *d_control_b = nullptr, *d_state_b = nullptr;
    int row_set = 0;
    double *d_cum = nullptr, *d_u = nullptr;
    double *d_x_params = nullptr, *d_x_noise = nullptr, *d_x_control = nullptr, *d_x_state = nullptr;
    double *d_last_traj = nullptr, *d_best_traj = nullptr, *d_total = nullptr;
    double *d_pad_pos = nullptr, *d_start = nullptr, *d_goal = nullptr;
    // sharded reuse (world > 1, K_r > 0): per-rank totals, all totals, the extra's total, the
    // chosen rows' slots [Kr][J N + N] and their all-gather [world][Kr][J N + N], the ranking
    double *d_tot_loc = nullptr, *d_tot_all = nullptr, *d_tot_x = nullptr, *d_slot = nullptr, *d_slot_all = nullptr;
    double* d_reuse_costs = nullptr;   // one device: k_reuse's totals [K + 1] and its counter
    int* d_reuse_count = nullptr;
    // one device, reuse: every candidate priced ahead by the rollout launch (CostArgs::spec_*),
    // [K + 1][J][N] each (row K the extra rollout); spec_on: allocated (STOMP_DEBUG_NO_SPEC=1: not)
    double *d_spec_params = nullptr, *d_spec_noise = nullptr, *d_spec_ctl = nullptr;
    bool spec_on = false;
    // the copy of the chosen candidates in the weights launch (STOMP_DEBUG_NO_PICK_FUSE=1: k_reuse_pick)
    bool pick_fuse = true;
    int* d_sel = nullptr;
    uint8_t* d_cf = nullptr;
    uint16_t* d_sdf = nullptr;   // d2 per voxel (the engine's bricked copy when model.brick)
    const uint16_t* d_sdf_caller = nullptr;   // the caller's device field (data_on_device), or null
    int grid_n[3] = {0, 0, 0};
    int* d_pad_cf = nullptr;
    int pad_collision = 0;
    // a retarget's theta_0: the boundary rows of R cut to the free columns [12][N] and R^-1
    // transposed [N][N] (uploaded at creation)
    double *d_Rb = nullptr, *d_RinvT = nullptr;
    bool reused_next = false, extra_added = false;
    // the extra rollout's params are not the current theta (stomp_engine_set_theta after its
    // noiseless rollout, stomp_pi_add_extra_rollouts with rows of the caller's): the next reuse step
    // cannot price that candidate ahead as theta + 0 and takes the reused rows' kernel
    bool x_foreign = false;
    int pending_member = -1;   // iteration_ of a noiseless rollout of theta not evaluated yet
    double *d_mm = nullptr, *d_psum_part = nullptr, *d_psum_all = nullptr, *d_u_part = nullptr, *d_u_all = nullptr;
    int K_gen = 0;
    // pregen (K_r = 0, fused noise phase): the normals, eps = sigma L z and M eps of iteration
    // it + 1 are made by extra low-priority blocks of iteration it's rollout launch; the rollout
    // launch of it + 1 reads them.  Two buffers, by iteration parity: a rollout launch reads one
    // and fills the other.
    bool pre_on = false;
    int pre_it = -1;                  // iteration whose rows are in d_pre_eps / d_pre_meps[it & 1] (enqueued)
    double *d_pre_eps[2] = {nullptr, nullptr}, *d_pre_meps[2] = {nullptr, nullptr};
    // the last iteration left its rows in d_pre_eps (rows_eps) instead of copying them into
    // d_noise / d_params (run / iterate with pregen rows); materialize_rows writes them on demand
    bool rows_in_pre = false;
    const double* rows_eps = nullptr;
    double* d_theta_gen = nullptr;
    double* h_total = nullptr;
    uint8_t* h_cf = nullptr;
    // eval scratch
    int eval_cap = 0;
    double *d_eval_params = nullptr, *d_eval_costs = nullptr, *d_eval_traj = nullptr;
    uint8_t* d_eval_cf = nullptr;
    uint8_t* d_eval_cs = nullptr;
    // timing
    bool timing = false;
    struct Ev {
        int id;
        hipEvent_t a, b;
    };
    std::vector<Ev> evs;
    std::vector<hipEvent_t> pool;
    double tot_ms[stomp::T_COUNT] = {0};
    int launches[stomp::T_COUNT] = {0};
    ncclComm* comm = nullptr;   // the RCCL communicator (a build without RCCL leaves it null)
    // bounded waits over RCCL (sync_stream): the last collective posted (name, iteration, count),
    // the deadline (STOMP_COMM_TIMEOUT_S, default 300 s), and the aborted communicator's message
    const char* coll_name = "none";
    int coll_it = -1;
    long long coll_count = 0;
    int cur_it = -1;
    double comm_timeout_s = 300.0;
    bool comm_aborted = false;
    std::string comm_msg;
    // STOMP_DEBUG_STALL_COLLECTIVE=n (tests): the n-th collective is withheld and the stream made
    // to wait on h_stall instead (a rank that never posts it); released after the abort
    long long stall_at = 0;
    unsigned* h_stall = nullptr;
    // an event behind each of the last kCollRing collectives: the message names the first one not
    // complete (the stuck one), not only the last one posted
    static constexpr int kCollRing = 32;
    struct CollRec {
        hipEvent_t ev = nullptr;
        const char* name = "";
        int it = -1;
        long long n = 0;
    } coll_ring[kCollRing];
    // PolicyImprovement API (stomp_pi_*): the weight the control-cost rows were priced with,
    // improvePolicy's update (J x N)
    double pi_weight = 0.0;
    double* d_delta = nullptr;
    // STOMPStatistics.torques (stomp_optimizer.cpp:384-398): the torque chain's model whenever
    // inertias are given (also with the torque term off), its per-waypoint output
    bool torque_stats = false;
    stomp::TermsModel tq_model{};
    double *d_tq = nullptr, *d_tq_state = nullptr;
    int wall_khz = 0;
    std::shared_ptr<stomp::LocalGroup> local;   // in-process exchange group (stomp_comm_local_id), or null
    hipEvent_t ev_ready = nullptr, ev_done = nullptr;
    double* d_mm_all = nullptr;          // [world][2][J][N] gathered (max, -min) of a local group
};

namespace stomp {

// ---- engine.cpp
extern thread_local std::string g_last_error;   // stomp_last_error
int fail(stomp_engine* e, int code, const char* fmt, ...);   // (sdf_build.cpp declares it too)
void release(stomp_engine* e);
void launch_noiseless(stomp_engine* e, int member);
int run_reuse(stomp_engine* e);

// ---- engine_retarget.cpp
// the request stomp_engine_retarget / stomp_group_retarget make of their arguments: it keeps the
// engine's collision points and path constraints
inline stomp_request kept_request(const double* start, const double* goal, uint64_t seed)
{
    return stomp_request{(int32_t)sizeof(stomp_request), start, goal, seed, -1, nullptr, -1, nullptr};
}
// the host side of a retarget once its launch has run: the new vectors, seed (null: kept) and
// padding-collision flag, every piece of iteration state dropped
void retarget_host_state(stomp_engine* e, const double* start, const double* goal, const uint64_t* seed, int flag);
// k_retarget's arguments for an engine that keeps its model: d_vec [2][J] the new start and goal
// on the device, d_flag_out the read-back slot, list_entry the engine's entry of a group's DevModel
// list or null
RequestArgs kept_request_args(const stomp_engine* e, const double* d_vec, int* d_flag_out, DevModel* list_entry);

// A request's model for one engine, planned on the host before anything is touched: the tables
// and the layout of the new collision points (spheres), the new path constraints (constraints),
// the model and the terms model the engine will hold (their device pointers are set at the commit).
// The device buffers a commit made for one engine and the ones they replace.  Until the call's
// stream wait has succeeded the engine knows neither: a failed call frees `fresh` and the engine is
// as it was; a finished one hands `fresh` to the engine and frees `retired` (live_alloc_*).
struct LiveAlloc {
    std::vector<void*> fresh, retired;
};
struct ModelPlan {
    bool spheres = false, constraints = false;   // which of the two the request replaces
    ModelTables mt;
    DevModel m{};
    std::vector<OcDev> oc;
    TermsModel terms{};
    bool terms_on = false;
    std::vector<unsigned char> img;   // the image's tables (build_model_image)
    // the commit's view of the buffers the engine holds with a capacity (the engine's own until one
    // has to grow), swapped into the engine after the stream wait
    unsigned long long* d_img = nullptr;
    size_t img_cap = 0;
    OcDev* d_oc = nullptr;
    size_t oc_cap = 0;
    double* d_sv = nullptr;
    size_t sv_cap = 0;
    double* d_terms_traj = nullptr;
    LiveAlloc live;
};
// everything the retarget calls refuse about request r (start and goal not null) for engine e
// on the host alone, before an engine or a device is touched (p: the engine's index in the messages)
int request_validate(const stomp_engine* e, const stomp_request* r, int p);
// the plan of a validated request, with the engine's device current; for a request that keeps both
// lists a copy of the engine's model and terms model
int request_plan(const stomp_engine* e, const stomp_request* r, ModelPlan& plan);
// the staging of one call for these plans (bytes): [P] RequestArgs, [P][2][J] vectors, each
// engine's image tables and constraint table, [P] flags
size_t request_stage_bytes(stomp_engine* const* es, int P, const std::vector<ModelPlan>& plans);
// one retarget call's staging of at least `bytes`, pinned (*h) and on the device (*d), held with a
// capacity (*cap) that at least doubles when it grows; false: an allocation failed, nothing is held
bool reserve_stage(unsigned char** h, unsigned char** d, size_t* cap, size_t bytes);
// the commit: the P engines (one shape, one stream, validated and planned) onto their requests in
// one upload, one launch and one read-back of the P flags; h / d: staging of request_stage_bytes,
// free for this call; d_models / d_tmodels: a group's lists, whose flags the launch also writes and
// whose entries it rewrites when a request replaces something or the lists are behind an engine's
// model (lists_behind), or null
int request_engines(stomp_engine* const* es, int P, const stomp_request* rs, std::vector<ModelPlan>& plans,
                    unsigned char* h, unsigned char* d, DevModel* d_models, TermsModel* d_tmodels, bool lists_behind);

// ---- engine_create.cpp: the stages that depend on the collision points and the path
// constraints, shared by creation and stomp_engine_retarget_request (err: where a refusal's message
// goes -- the engine under construction, or null on a live engine, which stays as it was)
int validate_spheres(const stomp_sphere* spheres, int n, int num_segments, double resolution);
int validate_constraints(const stomp_orientation_constraint* oc, int n, int num_segments);
int plan_model_tables(stomp_engine* err, const stomp_engine* e, const stomp_sphere* spheres, int S, ModelTables& t);
int plan_constraints(stomp_engine* err, const stomp_engine* e, const stomp_orientation_constraint* ocs, int n,
                     std::vector<OcDev>& oc);
int plan_terms(stomp_engine* err, const stomp_engine* e, TermsModel& t, bool terms_on);
int choose_layout(stomp_engine* err, const stomp_engine* e, const ModelTables& t, DevModel& m);
RolloutLds model_image_layout(const stomp_engine* e, const DevModel& m);
size_t model_image_bytes(const stomp_engine* e, const DevModel& m);
std::vector<unsigned char> build_model_image(const stomp_engine* e, const ModelTables& t, const DevModel& m);
void point_model_into_image(const stomp_engine* e, DevModel& m, unsigned long long* d_img);
int place_saved_frames(stomp_engine* e, DevModel& m, double** d_sv, size_t* sv_cap, LiveAlloc* live);

// ---- engine_exchange.cpp
extern const bool kWithRccl;
bool is_local_comm_id(const void* comm_id);
int sync_stream(stomp_engine* e);
int exchange_max(stomp_engine* e, double* buf, size_t n);
int exchange_gather(stomp_engine* e, const double* send, double* recv, size_t n);
int exchange_state(stomp_engine* e);
int join_exchange(stomp_engine* e, const void* comm_id, bool local_id);
void comm_destroy(stomp_engine* e);
int calibrate_shard_mode(stomp_engine* e);

// Every C-ABI entry on an engine runs with the engine's device current (allocations, launches
// and attribute opt-ins land there) and restores the caller's device on return.
struct DeviceGuard {
    int prev = -1, dev;
    explicit DeviceGuard(int d) : dev(d)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard()
    {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
};

#define HIP_TRY(e, x)                                                                          \
    do {                                                                                       \
        hipError_t _st = (x);                                                                  \
        if (_st != hipSuccess)                                                                 \
            return fail((e), STOMP_E_DEVICE, "%s failed: %s", #x, hipGetErrorString(_st));     \
    } while (0)

#define SYNC_TRY(e)                        \
    do {                                   \
        const int _rc = sync_stream(e);    \
        if (_rc) return _rc;               \
    } while (0)

template <class T>
int dev_alloc(stomp_engine* e, T** p, size_t n)
{
    void* q = nullptr;
    if (n == 0) n = 1;
    hipError_t st = hipMalloc(&q, n * sizeof(T));
    if (st != hipSuccess) return fail(e, STOMP_E_DEVICE, "hipMalloc(%zu bytes): %s", n * sizeof(T), hipGetErrorString(st));
    hipMemsetAsync(q, 0, n * sizeof(T), e->stream);
    e->allocs.push_back(q);
    *p = (T*)q;
    return 0;
}

template <class T>
int upload(stomp_engine* e, T** p, const T* src, size_t n)
{
    int rc = dev_alloc(e, p, n);
    if (rc) return rc;
    if (n) HIP_TRY(e, hipMemcpyAsync(*p, src, n * sizeof(T), hipMemcpyHostToDevice, e->stream));
    return 0;
}

// A buffer the engine holds with a capacity (in elements): reallocated only when `need` exceeds it.
// live == null (creation): exactly `need`, the engine's own allocation (p, cap: the engine's
// fields).  On a live engine p and cap are the commit's copies of those fields: the capacity at
// least doubles, the new buffer goes to live->fresh and the old one -- launches already enqueued
// may read it -- to live->retired; the engine itself is not touched.
template <class T>
int grow_buffer(stomp_engine* e, T** p, size_t* cap, size_t need, LiveAlloc* live)
{
    if (need <= *cap) return 0;
    const size_t n = live ? std::max(need, 2 * *cap) : need;
    T* q = nullptr;
    if (!live) {
        if (int rc = dev_alloc(e, &q, n)) return rc;
    } else {
        if (hipMalloc((void**)&q, n * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(nullptr, STOMP_E_DEVICE, "hipMalloc(%zu bytes) failed", n * sizeof(T));
        }
        hipMemsetAsync(q, 0, n * sizeof(T), e->stream);
        live->fresh.push_back(q);
        if (*p) live->retired.push_back(*p);
    }
    *p = q;
    *cap = n;
    return 0;
}

// a failed call: what it allocated is given back, the engine was never told of it
inline void live_alloc_abort(LiveAlloc& live)
{
    for (void* q : live.fresh) hipFree(q);
    live.fresh.clear();
    live.retired.clear();
}

// a finished call, after the engine's stream has passed every launch that could read the retired
// buffers: the new ones are the engine's (counted in rq_allocs), the replaced ones are freed
inline void live_alloc_commit(stomp_engine* e, LiveAlloc& live)
{
    for (void* q : live.fresh) e->allocs.push_back(q);
    e->rq_allocs += (long long)live.fresh.size();
    for (void* q : live.retired) {
        auto it = std::find(e->allocs.begin(), e->allocs.end(), q);
        if (it != e->allocs.end()) e->allocs.erase(it);
        hipFree(q);
    }
    live.fresh.clear();
    live.retired.clear();
}

inline hipEvent_t get_event(stomp_engine* e)
{
    if (!e->pool.empty()) {
        hipEvent_t ev = e->pool.back();
        e->pool.pop_back();
        return ev;
    }
    hipEvent_t ev;
    hipEventCreate(&ev);
    return ev;
}

struct Timed {
    stomp_engine* e;
    int id;
    hipStream_t s;
    hipEvent_t a = nullptr, b = nullptr;
    Timed(stomp_engine* e_, int id_, hipStream_t s_ = nullptr) : e(e_), id(id_), s(s_ ? s_ : e_->stream)
    {
        if (e->timing) {
            a = get_event(e);
            b = get_event(e);
            hipEventRecord(a, s);
        }
    }
    ~Timed()
    {
        if (e->timing) {
            hipEventRecord(b, s);
            e->evs.push_back({id, a, b});
        }
    }
};

// staged argument arrays start at multiples of 256 bytes (engine_group.cpp's arena, the retarget
// staging)
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// STOMPStatistics of an optimize loop from the engine's device-resident bookkeeping, read back
inline stomp_stats stats_from_track(const stomp_engine* e, const DevTrack& t)
{
    stomp_stats s;
    s.iterations = t.iterations;
    s.success = t.success;
    s.success_iteration = t.success_iteration;
    s.collision_success_iteration = t.collision_success_iteration;
    s.last_improvement_iteration = t.last_improvement_iteration;
    s.best_cost = t.best;
    const double tick_s = e->wall_khz > 0 ? 1.0 / (1000.0 * e->wall_khz) : 0.0;
    s.success_duration = t.success_iteration >= 0 ? (double)(t.t_success - t.t0) * tick_s : 0.0;
    s.collision_success_duration =
        t.collision_success_iteration >= 0 ? (double)(t.t_collision_success - t.t0) * tick_s : 0.0;
    return s;
}

// generateRollouts' sampling arguments of iteration it (policy_improvement_loop.cpp:155-160:
// sigma_d * decay_d^(it - 1))
inline NoiseArgs noise_args(const stomp_engine* e, int it)
{
    NoiseArgs na{};
    // gather mode: the noise rows of all K rollouts (global ids from 0)
    na.J = e->J; na.N = e->N; na.Nall = e->Nall; na.K_loc = e->rows; na.first_global = e->first - e->row0;
    na.iteration = it; na.seed = e->seed;
    for (int d = 0; d < e->J; ++d) na.sigma.v[d] = e->sig_std[d] * std::pow(e->sig_dec[d], it - 1);
    na.theta = e->d_theta; na.LT = e->d_LT; na.MT = e->d_MT; na.start = e->d_start; na.goal = e->d_goal;
    std::memcpy(na.dcoef, e->su.dcoef, sizeof na.dcoef);
    const double w = 0.5 * e->w_smooth;   // policy_improvement.cpp:487
    for (int r = 0; r < 3; ++r) na.wr[r] = w * e->smooth[r];
    na.params = e->d_params; na.noise = e->d_noise; na.control = e->d_control; na.zero_noise = 0; na.row_begin = 0;
    na.stop = e->d_stop;
    na.pre_eps = e->d_pre_eps[it & 1]; na.pre_meps = e->d_pre_meps[it & 1];
    na.rows_in_pre = 0; na.theta_gen = e->d_theta_gen;
    return na;
}

// k_pregen's arguments for iteration it: no stop flag, so the rows stay valid for pre_it
// whatever the optimize loop decides
inline NoiseArgs pregen_args(const stomp_engine* e, int it)
{
    NoiseArgs na = noise_args(e, it);
    na.stop = nullptr;
    return na;
}

// The noiseless rollout of theta (iteration_ = member) in a rollout launch's arguments.  totals:
// its costs.sum() and collision flag are written too; extra_rows: it is also the extra rollout of
// the next reuse ranking (K_r > 0), whose params / noise / control rows its workgroup writes.
inline void set_noiseless(const stomp_engine* e, CostArgs& ca, int member, bool totals, bool extra_rows)
{
    ca.x_params = e->d_theta; ca.x_member = member;
    ca.x_state = e->d_x_state; ca.x_traj = e->d_last_traj;
    if (totals) { ca.x_cf = e->d_cf; ca.x_total = e->d_total; }
    if (extra_rows) { ca.x_ctl = e->d_x_control; ca.x_prm = e->d_x_params; ca.x_nse = e->d_x_noise; }
}

// The weights launch's arguments over `rows` rollout rows whose noise is at `noise`: the fields
// every caller sets alike (the cumulative costs, the sharded phases' buffers and the mode are the
// caller's)
inline WeightArgs weight_args(const stomp_engine* e, int rows, const double* noise)
{
    WeightArgs wa{};
    wa.stop = e->d_stop;
    wa.J = e->J; wa.N = e->N; wa.K_loc = rows;
    wa.state = e->d_state; wa.control = e->d_control; wa.noise = noise;
    wa.prob = e->d_prob; wa.u = e->d_u;
    wa.tc = weights_tile(rows);
    wa.nb_total = e->K / kSumBlock;
    return wa;
}

// noise / params rows of an iteration that left them in its pregen buffer
inline void materialize_rows(stomp_engine* e)
{
    if (!e->rows_in_pre) return;
    launch_materialize_rows(e->rows, e->J * e->N, e->rows_eps, e->d_theta_gen, e->d_noise, e->d_params, e->stream);
    e->rows_in_pre = false;
}

inline int flush_noiseless(stomp_engine* e)
{
    if (e->pending_member >= 0) {
        launch_noiseless(e, e->pending_member);
        e->pending_member = -1;
    }
    return 0;
}

// generateRollouts bookkeeping (policy_improvement.cpp:167-225): the first call generates all K;
// later ones rank the K previous rollouts and the extra (noiseless) one, keep the best K_r in rows
// K_gen.. with their noise re-based on the current theta, and generate the rest.  With the rows
// sharded over ranks the ranking runs on all-gathered totals and the chosen rows travel in slots
// (k_misc.hip), so every rank ends with exactly its rows of the single-device result.
inline void swap_row_sets(stomp_engine* e)
{
    std::swap(e->d_params, e->d_params_b);
    std::swap(e->d_noise, e->d_noise_b);
    std::swap(e->d_control, e->d_control_b);
    std::swap(e->d_state, e->d_state_b);
    e->row_set ^= 1;
}

// generateRollouts' bookkeeping: K_gen, and whether the reuse step runs this iteration; when it
// does the row sets swap, so the previous rows are the reuse source (d_*_b) and this iteration's
// rows are written into the other set
inline bool plan_generate(stomp_engine* e)
{
    e->K_gen = e->K - e->Kr;
    if (!e->reused_next) {
        e->K_gen = e->K;
        if (e->Kr > 0) e->reused_next = true;
        return false;
    }
    swap_row_sets(e);
    return true;
}

// plan + reuse at once (callers that evaluate no rollouts of their own before the ranking)
inline int begin_generate(stomp_engine* e)
{
    if (!plan_generate(e)) return 0;
    flush_noiseless(e);
    return run_reuse(e);
}

}  // namespace stomp
