// engine_exchange.cpp -- what the ranks of a K-sharded problem exchange, and how: the in-process
// group and its registry, the RCCL communicator with its bounded waits, the collectives an
// iteration posts, joining either at creation (join_exchange), and the decomposition measured at
// creation (calibrate_shard_mode).  The only file that sees RCCL.
#include "engine_internal.h"

#include <algorithm>
#include <cstdlib>
#include <map>
#include <thread>

#ifdef STOMP_WITH_RCCL
#include <rccl/rccl.h>
#endif

namespace stomp {

#ifdef STOMP_WITH_RCCL
const bool kWithRccl = true;
#else
const bool kWithRccl = false;
#endif

namespace {

constexpr char kLocalMagic[8] = {'S', 'T', 'O', 'M', 'P', 'L', 'O', 'C'};

std::mutex g_groups_mu;
std::map<uint64_t, std::shared_ptr<LocalGroup>> g_groups;   // created, not yet joined by every rank
uint64_t g_next_group = 1;

}  // namespace

bool is_local_comm_id(const void* comm_id) { return std::memcmp(comm_id, kLocalMagic, sizeof kLocalMagic) == 0; }

// hipStreamSynchronize of the engine stream, bounded when collectives are in it: over RCCL the
// wait polls the stream and the communicator's asynchronous error, and after STOMP_COMM_TIMEOUT_S
// seconds without completion (a rank that never posts its side of a collective, a mismatched
// sequence) or on an RCCL error it aborts the communicator (ncclCommAbort also releases RCCL
// kernels still waiting) and fails with STOMP_E_COMM naming the last collective posted.  Every
// later call on the engine fails the same way.
int sync_stream(stomp_engine* e)
{
#ifdef STOMP_WITH_RCCL
    if (e->comm_aborted) return fail(e, STOMP_E_COMM, "%s", e->comm_msg.c_str());
    if (e->comm) {
        const auto t0 = std::chrono::steady_clock::now();
        for (long long n = 0;; ++n) {
            const hipError_t q = hipStreamQuery(e->stream);
            if (q == hipSuccess) return 0;
            if (q != hipErrorNotReady)
                return fail(e, STOMP_E_DEVICE, "hipStreamQuery failed: %s", hipGetErrorString(q));
            ncclResult_t ae = ncclSuccess;
            const ncclResult_t qr = ncclCommGetAsyncError(e->comm, &ae);
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            const bool err = qr != ncclSuccess || (ae != ncclSuccess && ae != ncclInProgress);
            if (err || el > e->comm_timeout_s) {
                char buf[400];
                if (err)
                    snprintf(buf, sizeof buf, "rank %d: RCCL error (%s) with collectives in flight",
                             e->rank, ncclGetErrorString(qr != ncclSuccess ? qr : ae));
                else
                    snprintf(buf, sizeof buf, "rank %d: collectives did not complete within %.1f s (STOMP_COMM_TIMEOUT_S)",
                             e->rank, e->comm_timeout_s);
                std::string stuck = "unknown (older than the last 32)";
                for (long long k = std::max(1LL, e->coll_count - stomp_engine::kCollRing + 1); k <= e->coll_count; ++k) {
                    const auto& r = e->coll_ring[k % stomp_engine::kCollRing];
                    if (r.n == k && r.ev && hipEventQuery(r.ev) == hipErrorNotReady) {
                        stuck = std::string(r.name) + " of iteration " + std::to_string(r.it) + " (#" + std::to_string(k) + ")";
                        break;
                    }
                }
                (void)hipGetLastError();
                e->comm_msg = std::string(buf) + "; first collective not complete: " + stuck + "; last posted: " +
                              e->coll_name + " of iteration " + std::to_string(e->coll_it) + " (#" +
                              std::to_string(e->coll_count) + "); communicator aborted";
                // the test hook's wait first: its withheld collective's successors are queued behind
                // it and have not started, so the abort would wait for them
                if (e->h_stall) __atomic_store_n(e->h_stall, 1u, __ATOMIC_SEQ_CST);
                ncclCommAbort(e->comm);
                e->comm = nullptr;
                e->comm_aborted = true;
                (void)hipStreamSynchronize(e->stream);   // the aborted collectives drain
                (void)hipGetLastError();
                return fail(e, STOMP_E_COMM, "%s", e->comm_msg.c_str());
            }
            if (n > 2000) std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
    }
#endif
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return 0;
}

void comm_destroy(stomp_engine* e)
{
#ifdef STOMP_WITH_RCCL
    if (e->comm) ncclCommDestroy(e->comm);   // null once aborted (sync_stream)
#else
    (void)e;
#endif
}

namespace {

#ifdef STOMP_WITH_RCCL
#define NCCL_TRY(e, x)                                                                       \
    do {                                                                                     \
        ncclResult_t _r = (x);                                                               \
        if (_r != ncclSuccess) return fail((e), STOMP_E_COMM, "%s: %s", #x, ncclGetErrorString(_r)); \
    } while (0)

// a collective about to be posted on the engine stream: recorded for sync_stream's message;
// returns 1 when the STOMP_DEBUG_STALL_COLLECTIVE hook withholds it (the stream then waits on
// h_stall, as behind a rank that never posts it)
int coll_post(stomp_engine* e, const char* name)
{
    e->coll_name = name;
    e->coll_it = e->cur_it;
    ++e->coll_count;
    if (e->stall_at > 0 && e->coll_count == e->stall_at && e->h_stall) {
        void* dp = nullptr;
        if (hipHostGetDevicePointer(&dp, e->h_stall, 0) == hipSuccess &&
            hipStreamWaitValue32(e->stream, dp, 1u, hipStreamWaitValueEq, 0xFFFFFFFFu) == hipSuccess)
            return 1;
        (void)hipGetLastError();
    }
    return 0;
}

// the event behind the collective coll_post just recorded (or withheld)
void coll_mark(stomp_engine* e)
{
    auto& r = e->coll_ring[e->coll_count % stomp_engine::kCollRing];
    if (!r.ev && hipEventCreateWithFlags(&r.ev, hipEventDisableTiming) != hipSuccess) {
        r.ev = nullptr;
        (void)hipGetLastError();
        return;
    }
    r.name = e->coll_name;
    r.it = e->coll_it;
    r.n = e->coll_count;
    (void)hipEventRecord(r.ev, e->stream);
}
#endif

// all-gather of n doubles per rank, rank order, over the in-process group: publish the send
// buffer with an event recorded after its producer; after the first barrier every rank copies
// every rank's buffer behind that rank's event; after the second barrier every rank's stream
// waits for every rank's copies, so no rank overwrites a buffer another still reads
int local_gather(stomp_engine* e, const double* send, double* recv, size_t n)
{
    LocalGroup& g = *e->local;
    HIP_TRY(e, hipEventRecord(e->ev_ready, e->stream));
    std::unique_lock<std::mutex> lk(g.mu);
    g.slot[e->rank].src = send;
    g.slot[e->rank].ready = e->ev_ready;
    g.slot[e->rank].done = e->ev_done;
    if (!g.barrier(lk)) return fail(e, STOMP_E_COMM, "local exchange group: a rank did not arrive (each rank needs a host thread of its own)");
    std::vector<LocalGroup::Slot> sl = g.slot;
    lk.unlock();
    for (int q = 0; q < g.world; ++q) {
        if (q != e->rank) HIP_TRY(e, hipStreamWaitEvent(e->stream, sl[q].ready, 0));
        if (recv + (size_t)q * n != sl[q].src)   // in place (gather mode: the rank's own rows)
            HIP_TRY(e, hipMemcpyAsync(recv + (size_t)q * n, sl[q].src, n * sizeof(double), hipMemcpyDeviceToDevice,
                                      e->stream));
    }
    HIP_TRY(e, hipEventRecord(e->ev_done, e->stream));
    lk.lock();
    if (!g.barrier(lk)) return fail(e, STOMP_E_COMM, "local exchange group: a rank did not arrive");
    lk.unlock();
    for (int q = 0; q < g.world; ++q)
        if (q != e->rank) HIP_TRY(e, hipStreamWaitEvent(e->stream, sl[q].done, 0));
    return 0;
}

}  // namespace

// all-reduce(max) in place of n doubles over the ranks (RCCL, or the in-process group; with one
// rank the identity)
int exchange_max(stomp_engine* e, double* buf, size_t n)
{
#ifdef STOMP_WITH_RCCL
    if (e->comm_aborted) return fail(e, STOMP_E_COMM, "%s", e->comm_msg.c_str());
    if (e->comm) {
        if (!coll_post(e, "all-reduce(max)"))
            NCCL_TRY(e, ncclAllReduce(buf, buf, n, ncclFloat64, ncclMax, e->comm, e->stream));
        coll_mark(e);
        return 0;
    }
#endif
    if (e->local) {
        int rc = local_gather(e, buf, e->d_mm_all, n);
        if (rc) return rc;
        launch_gather_max(e->d_mm_all, e->world, (int)n, buf, e->stream);
    }
    return 0;
}

// all-gather of n doubles per rank into recv [world][n] (send may be recv's own slot: in place)
int exchange_gather(stomp_engine* e, const double* send, double* recv, size_t n)
{
#ifdef STOMP_WITH_RCCL
    if (e->comm_aborted) return fail(e, STOMP_E_COMM, "%s", e->comm_msg.c_str());
    if (e->comm) {
        if (!coll_post(e, "all-gather")) NCCL_TRY(e, ncclAllGather(send, recv, n, ncclFloat64, e->comm, e->stream));
        coll_mark(e);
        return 0;
    }
#endif
    if (e->local) return local_gather(e, send, recv, n);
    if (recv != send) HIP_TRY(e, hipMemcpyAsync(recv, send, sizeof(double) * n, hipMemcpyDeviceToDevice, e->stream));
    return 0;
}

// gather mode: every rank's state-cost rows into every rank's [K][N] state buffer (in place;
// with one rank, the STOMP_DEBUG_GATHER_RANKS timing hook, nothing moves)
int exchange_state(stomp_engine* e)
{
    if (e->world == 1) return 0;
    const size_t n = (size_t)e->K_loc * e->N;
    return exchange_gather(e, e->d_state + (size_t)e->row0 * e->N, e->d_state, n);
}

namespace {

// a rank of world_size > 1 created with a stomp_comm_local_id: joins its in-process group
int join_local_group(stomp_engine* e, const void* comm_id)
{
    const int world = e->world, J = e->J, N = e->N;
    uint64_t gid = 0;
    std::memcpy(&gid, (const char*)comm_id + 8, sizeof gid);
    std::shared_ptr<LocalGroup> g;
    {
        std::lock_guard<std::mutex> lk(g_groups_mu);
        auto it = g_groups.find(gid);
        if (it != g_groups.end()) g = it->second;
    }
    if (!g) return fail(e, STOMP_E_COMM, "unknown local exchange group (stomp_comm_local_id)");
    {
        std::lock_guard<std::mutex> lk(g->mu);
        if (g->world != world) return fail(e, STOMP_E_COMM, "local group of %d ranks, engine world_size %d",
                                           g->world, world);
        if (g->joined[e->rank]) return fail(e, STOMP_E_COMM, "rank %d joined the local group twice", e->rank);
        // everything that changes the per-iteration exchange sequence: the decomposition, the
        // shapes, the reused rollouts (two more all-gathers) and the weights phases
        const long long sig[6] = {e->gather ? 1 : 0, e->K, J, N, e->Kr, e->split_modes ? 1 : 0};
        if (g->has_sig && std::memcmp(sig, g->sig, sizeof sig) != 0)
            return fail(e, STOMP_E_COMM, "rank %d: decomposition (%s, K=%lld, J=%d, N=%d, K_r=%d) differs from the "
                        "group's (%s, K=%lld, J=%lld, N=%lld, K_r=%lld)", e->rank, e->gather ? "gather" : "partials",
                        (long long)e->K, J, N, e->Kr, g->sig[0] ? "gather" : "partials", g->sig[1], g->sig[2],
                        g->sig[3], g->sig[4]);
        std::memcpy(g->sig, sig, sizeof sig);
        g->has_sig = true;
        g->joined[e->rank] = 1;
        g->slot[e->rank].device = e->device;
        for (int q = 0; q < world; ++q)   // copies between the ranks' devices go peer to peer
            if (g->joined[q] && g->slot[q].device != e->device) {
                (void)hipDeviceEnablePeerAccess(g->slot[q].device, 0);
                (void)hipGetLastError();   // already enabled is fine
            }
        bool all = true;
        for (int q = 0; q < world; ++q) all = all && g->joined[q];
        if (all) {
            std::lock_guard<std::mutex> lk2(g_groups_mu);
            g_groups.erase(gid);   // every rank holds it now
        }
    }
    e->local = g;
    if (hipEventCreateWithFlags(&e->ev_ready, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_done, hipEventDisableTiming) != hipSuccess)
        return fail(e, STOMP_E_DEVICE, "hipEventCreate failed");
    return dev_alloc(e, &e->d_mm_all, (size_t)world * 2 * J * N);
}

#ifdef STOMP_WITH_RCCL
// a rank of world_size > 1 created with a stomp_comm_unique_id: joins the communicator, and the
// ranks check that they agree on the decomposition
int join_communicator(stomp_engine* e, const void* comm_id)
{
    ncclUniqueId id;
    std::memcpy(&id, comm_id, sizeof id);
    if (ncclCommInitRank(&e->comm, e->world, id, e->rank) != ncclSuccess)
        return fail(e, STOMP_E_COMM, "ncclCommInitRank failed");
    // every rank must run the same decomposition and shape, or the per-iteration collectives
    // would not pair up (one all-gather against an all-reduce and two all-gathers): one
    // all-reduce(max) of (x, -x) pairs at creation
    // (K_r and the weights phases too: they change the exchange sequence)
    const double sm = e->split_modes ? 1.0 : 0.0;
    const double h[12] = {e->gather ? 1.0 : 0.0, e->gather ? -1.0 : 0.0, (double)e->K, -(double)e->K,
                          (double)e->J,          -(double)e->J,          (double)e->N, -(double)e->N,
                          (double)e->Kr,         -(double)e->Kr,         sm,           -sm};
    double* d_sig = nullptr;
    if (int rc = dev_alloc(e, &d_sig, 12)) return rc;
    double r[12];
    if (hipMemcpyAsync(d_sig, h, sizeof h, hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        (!coll_post(e, "decomposition check (all-reduce(max))") &&
         ncclAllReduce(d_sig, d_sig, 12, ncclFloat64, ncclMax, e->comm, e->stream) != ncclSuccess))
        return fail(e, STOMP_E_COMM, "decomposition check across ranks failed");
    coll_mark(e);
    if (hipMemcpyAsync(r, d_sig, sizeof r, hipMemcpyDeviceToHost, e->stream) != hipSuccess)
        return fail(e, STOMP_E_COMM, "decomposition check across ranks failed");
    if (int rc = sync_stream(e)) return rc;   // bounded: a rank that never gets here fails the others
    for (int k = 0; k < 12; k += 2)
        if (r[k] != -r[k + 1])
            return fail(e, STOMP_E_COMM, "ranks disagree on the K-sharded decomposition (gather, K, J, N, K_r, "
                        "weights phases; "
                        "entry %d: max %g, min %g)", k / 2, r[k], -r[k + 1]);
    return 0;
}
#endif

}  // namespace

// stomp_engine_create's join stage: the in-process group or the RCCL communicator of a sharded
// engine, and the bounded waits' settings (read for every engine of an RCCL build)
int join_exchange(stomp_engine* e, const void* comm_id, bool local_id)
{
    if (local_id)
        if (int rc = join_local_group(e, comm_id)) return rc;
#ifdef STOMP_WITH_RCCL
    if (const char* to = std::getenv("STOMP_COMM_TIMEOUT_S")) {
        const double v = std::atof(to);
        if (v > 0.0) e->comm_timeout_s = v;
    }
    if (const char* st = std::getenv("STOMP_DEBUG_STALL_COLLECTIVE")) {
        e->stall_at = std::atoll(st);
        if (e->stall_at > 0 && hipHostMalloc((void**)&e->h_stall, sizeof(unsigned), hipHostMallocMapped) != hipSuccess)
            return fail(e, STOMP_E_DEVICE, "hipHostMalloc (stall hook) failed");
        if (e->h_stall) *e->h_stall = 0u;
    }
    if (e->world > 1 && !local_id) {
        if (int rc = join_communicator(e, comm_id)) return rc;
    } else if (e->split_modes && e->world == 1) {
        // STOMP_DEBUG_RCCL_ONE_RANK=1 (with the sharded-modes hook): a one-rank communicator,
        // so the sharded path's RCCL all-reduce / all-gathers run on a one-GPU box
        const char* one = std::getenv("STOMP_DEBUG_RCCL_ONE_RANK");
        if (one && one[0] == '1') {
            ncclUniqueId id;
            if (ncclGetUniqueId(&id) != ncclSuccess || ncclCommInitRank(&e->comm, 1, id, 0) != ncclSuccess)
                return fail(e, STOMP_E_COMM, "one-rank ncclCommInitRank failed");
        }
    }
#endif
    return 0;
}

namespace {

// partials chosen after a calibration that ran in gather mode's layout: the row buffers drop from
// K rows to the rank's K_loc (about world_size times less memory); nothing in them is read again
// (every row is rewritten by the iterations, the pregen rows are remade)
int shrink_rows(stomp_engine* e)
{
    const size_t JN = (size_t)e->J * e->N, KJN = (size_t)e->rows * JN;
    auto re = [&](double*& p, size_t n) -> int {
        if (!p) return 0;
        HIP_TRY(e, hipStreamSynchronize(e->stream));   // the calibration launches used it
        auto it = std::find(e->allocs.begin(), e->allocs.end(), (void*)p);
        if (it != e->allocs.end()) {
            hipFree(*it);
            e->allocs.erase(it);
        }
        p = nullptr;
        return dev_alloc(e, &p, n);
    };
    int rc = 0;
    for (double** p : {&e->d_params, &e->d_noise, &e->d_control, &e->d_prob, &e->d_cum, &e->d_pre_eps[0],
                       &e->d_pre_eps[1], &e->d_pre_meps[0], &e->d_pre_meps[1]})
        if ((rc = re(*p, KJN))) return rc;
    return re(e->d_state, (size_t)e->rows * e->N);
}

}  // namespace

// The K-sharded decomposition from measurements, at the end of stomp_engine_create when
// both are possible and none was requested.  Every rank times, on its own device and stream:
//   T_g  one iteration's rollout launch and fused weights in gather mode (its K_loc rollouts, all K
//        pregen / pricing rows, the weights over all K), no exchange;
//   T_p  the same in partials mode (its K_loc rows, the MINMAX / PSUM / USUM weights phases);
//   L_ar, L_ag, L_agp  the collectives each posts: the all-reduce(max) of 2 J N doubles, the
//        all-gather of the K_loc N state rows, the all-gather of the block partials;
// the maxima over the ranks are taken (one all-reduce), so every rank decides alike:
//   gather  <=>  T_g + L_ag <= T_p + L_ar + 2 L_agp          (stomp_shard_decide)
// The calibration launches leave no state the first iteration reads: theta is untouched, the pregen
// rows are remade (pre_it stays -1), and every row buffer is rewritten by the iterations.
// STOMP_DEBUG_SHARD_LATENCY_US=x adds x us to every measured collective (tests: both selections).
int calibrate_shard_mode(stomp_engine* e)
{
    const int J = e->J, N = e->N;
    const size_t JN = (size_t)J * N;
    hipEvent_t ev0 = get_event(e), ev1 = get_event(e);
    auto elapsed_us = [&]() -> double {
        float ms = 0.0f;
        if (hipEventSynchronize(ev1) != hipSuccess || hipEventElapsedTime(&ms, ev0, ev1) != hipSuccess) return -1.0;
        return 1000.0 * ms;
    };
    auto median = [](std::vector<double> v) {
        std::sort(v.begin(), v.end());
        return v[v.size() / 2];
    };
    auto set_mode = [&](bool gather) {
        e->gather = gather;
        e->rows = gather ? e->K : e->K_loc;
        e->row0 = gather ? e->first : 0;
        e->split_modes = !gather;
    };
    // one iteration's compute in the current mode (enqueue_iteration's launches for K_r = 0 with
    // pregen rows, the exchanges left out)
    auto compute = [&]() -> double {
        NoiseArgs na = noise_args(e, 1);
        na.K_gen_global = e->K;
        na.row_begin = e->rows;
        na.rows_in_pre = 1;
        CostArgs ca{};
        ca.stop = e->d_stop;
        ca.fused_noise = 2;
        ca.nz = na;
        ca.params = e->d_params; ca.stride = (long long)JN; ca.num_noisy = e->K_loc;
        ca.member = 0;
        ca.pre_rows = e->rows;
        ca.pre_next = pregen_args(e, 2);
        ca.ctl_by_pre = 1;
        ca.ctl_rows = e->rows;
        ca.row0 = e->row0;
        ca.state_out = e->d_state + (size_t)e->row0 * N;
        WeightArgs wa = weight_args(e, e->rows, na.pre_eps);
        wa.use_cumulative = e->use_cum;
        wa.cum = e->use_cum ? e->d_cum : nullptr;
        wa.mm = e->d_mm; wa.psum_part = e->d_psum_part; wa.psum_all = e->d_psum_all; wa.u_part = e->d_u_part;
        hipEventRecord(ev0, e->stream);
        launch_cost(e->model, ca, e->stream);
        if (e->use_cum) launch_cumulative(wa, e->d_cum, e->stream);
        if (!e->split_modes) {
            wa.mode = W_FUSED;
            launch_weights(wa, e->stream);
        } else {
            for (int mode : {W_MINMAX, W_PSUM, W_USUM}) {
                wa.mode = mode;
                launch_weights(wa, e->stream);
            }
        }
        hipEventRecord(ev1, e->stream);
        return elapsed_us();
    };
    auto timed = [&](auto&& f, int reps) -> double {
        f();   // warm
        std::vector<double> v;
        for (int r = 0; r < reps; ++r) v.push_back(f());
        return median(v);
    };
    double m[5];
    set_mode(true);
    m[0] = timed(compute, 3);
    set_mode(false);
    m[1] = timed(compute, 3);
    int rc = 0;
    auto coll = [&](auto&& post) -> double {
        hipEventRecord(ev0, e->stream);
        if (int r = post()) rc = r;
        hipEventRecord(ev1, e->stream);
        return elapsed_us();
    };
    m[2] = timed([&]() { return coll([&]() { return exchange_max(e, e->d_mm, 2 * JN); }); }, 8);
    m[3] = timed([&]() {
        return coll([&]() { return exchange_gather(e, e->d_state + (size_t)e->first * N, e->d_state,
                                                   (size_t)e->K_loc * N); });
    }, 8);
    m[4] = timed([&]() {
        return coll([&]() { return exchange_gather(e, e->d_psum_part, e->d_psum_all,
                                                   (size_t)(e->K_loc / kSumBlock) * JN); });
    }, 8);
    e->pool.push_back(ev0);
    e->pool.push_back(ev1);
    if (rc) return rc;
    for (double x : m)
        if (!(x >= 0.0)) return fail(e, STOMP_E_DEVICE, "decomposition calibration: event timing failed");
    if (const char* lat = std::getenv("STOMP_DEBUG_SHARD_LATENCY_US"))
        for (int k = 2; k < 5; ++k) m[k] += std::atof(lat);
    // every rank decides on the maxima over the ranks
    HIP_TRY(e, hipMemcpyAsync(e->d_mm, m, sizeof m, hipMemcpyHostToDevice, e->stream));
    if ((rc = exchange_max(e, e->d_mm, 5))) return rc;
    HIP_TRY(e, hipMemcpyAsync(m, e->d_mm, sizeof m, hipMemcpyDeviceToHost, e->stream));
    SYNC_TRY(e);
    int32_t mode = 0;
    stomp_shard_decide(m, &mode);
    set_mode(mode == STOMP_SHARD_GATHER);
    if (e->gather) HIP_TRY(e, hipMemsetAsync(e->d_state, 0, sizeof(double) * e->rows * N, e->stream));
    else if ((rc = shrink_rows(e))) return rc;
    e->shard_info[0] = mode;
    for (int k = 0; k < 5; ++k) e->shard_info[1 + k] = m[k];
    return 0;
}

}  // namespace stomp

using namespace stomp;

extern "C" {

int stomp_shard_decide(const double* measured, int32_t* mode)
{
    if (!measured || !mode) return STOMP_E_INVALID;
    const double gather = measured[0] + measured[3];
    const double partials = measured[1] + measured[2] + 2.0 * measured[4];
    *mode = gather <= partials ? STOMP_SHARD_GATHER : STOMP_SHARD_PARTIALS;
    return 0;
}

int stomp_comm_local_id(int32_t world_size, void* out128)
{
    if (world_size < 1 || !out128) return fail(nullptr, STOMP_E_INVALID, "invalid local group arguments");
    auto g = std::make_shared<LocalGroup>();
    g->world = world_size;
    g->slot.resize(world_size);
    g->joined.assign(world_size, 0);
    uint64_t gid;
    {
        std::lock_guard<std::mutex> lk(g_groups_mu);
        gid = g_next_group++;
        g_groups[gid] = g;
    }
    std::memset(out128, 0, 128);
    std::memcpy(out128, kLocalMagic, sizeof kLocalMagic);
    std::memcpy((char*)out128 + 8, &gid, sizeof gid);
    std::memcpy((char*)out128 + 16, &world_size, sizeof world_size);
    return 0;
}

int stomp_comm_unique_id(void* out128)
{
#ifdef STOMP_WITH_RCCL
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return fail(nullptr, STOMP_E_COMM, "ncclGetUniqueId failed");
    std::memcpy(out128, &id, sizeof id);
    return 0;
#else
    (void)out128;
    return fail(nullptr, STOMP_E_UNSUPPORTED, "built without RCCL");
#endif
}

}  // extern "C"
