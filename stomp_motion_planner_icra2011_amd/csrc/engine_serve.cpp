// engine_serve.cpp -- stomp_group_serve: a queue of requests served by a group's engines as slots.
// stomp_group_optimize is a batch, and a batch ends with its slowest problem; here a slot whose
// request has stopped takes the next waiting request.  The loop is stomp_group_optimize's (the
// chunks of staged steps, two in flight, the stop flags read one chunk behind: engine_group.cpp)
// with every slot at its own iteration: OptimizeLoop::start[p] is the group step of slot p's
// iteration 1.  Which slot takes which request, and in which step it starts, is decided by
// ServeSchedule from what the mirror showed stopped at which chunk boundary, and by nothing else;
// serve_drive is the one loop around it, run by stomp_group_serve over the device and by
// stomp_serve_schedule over given iteration counts.  A turnover is a fixed number of launches for
// all the slots that turn at one boundary, in stream order between the chunks: k_serve_turnover
// (the finished requests' records into the result slab, the DevTracks re-initialised), k_retarget
// (the kept-model retarget of engine_retarget.cpp), the grouped pregen of iteration 1, and the
// copies of the new padding-collision flags into the model entries the chunk staged from host
// copies that do not know them yet.  Nothing waits per request: the results stay in the slab until
// the loop is over and come back in one copy.
#include "engine_group.h"

#include <algorithm>

using namespace stomp;

namespace {

struct Turn {
    int slot, request, prev;   // prev: the request the slot leaves (-1: its first of the call)
};

// The decision procedure.  A slot is free when it has no request yet or its request has been seen
// stopped; free slots take the waiting requests in ascending slot order, and a request's
// iteration 1 is the first step staged after the decision.
struct ServeSchedule {
    int P, n;
    int next_req = 0;
    int staged_end = 0;             // the last step staged so far
    std::vector<int> cur;           // slot -> its request (-1: none)
    std::vector<char> seen;         // slot -> its request has been seen stopped
    std::vector<int> slot, start;   // request -> its slot and start step
    ServeSchedule(int P_, int n_) : P(P_), n(n_), cur(P_, -1), seen(P_, 0), slot(n_, -1), start(n_, 0) {}
    bool waiting() const { return next_req < n; }
    std::vector<Turn> assign()
    {
        std::vector<Turn> t;
        for (int p = 0; p < P && next_req < n; ++p) {
            if (cur[p] >= 0 && !seen[p]) continue;
            t.push_back({p, next_req, cur[p]});
            slot[next_req] = p;
            start[next_req] = staged_end + 1;
            cur[p] = next_req++;
            seen[p] = 0;
        }
        return t;
    }
    // the mirror read behind the chunk that ended with step `end`: it speaks of a slot's request
    // only if that request's turnover was enqueued ahead of the chunk (an older mirror still shows
    // the request the slot has left)
    void saw(int end, const std::vector<char>& stopped)
    {
        for (int p = 0; p < P; ++p)
            if (cur[p] >= 0 && !seen[p] && start[cur[p]] <= end && stopped[p]) seen[p] = 1;
    }
    bool done() const
    {
        if (waiting()) return false;
        for (int p = 0; p < P; ++p)
            if (cur[p] >= 0 && !seen[p]) return false;
        return true;
    }
};

// The loop: two chunks in flight, the stop flags read behind the older one, the turnovers decided
// there enqueued ahead of the next chunk staged.  Backend: the device (ServeDevice) or given
// iteration counts (ServeCounts).  While requests wait every chunk is enqueued whole; afterwards
// the backend says whether steps with work remain.
template <class Backend>
int serve_drive(ServeSchedule& s, Backend& b)
{
    int rc = 0, inflight = 0, head = 0;
    int ends[2] = {0, 0};
    std::vector<Turn> turns = s.assign();
    std::vector<char> stopped(s.P, 0);
    for (;;) {
        while (inflight < 2 && (s.waiting() || !turns.empty() || b.more(s))) {
            const int slot = (head + inflight) & 1;
            if ((rc = b.enqueue(s, slot, turns))) break;   // (advances s.staged_end)
            ends[slot] = s.staged_end;
            turns.clear();
            ++inflight;
        }
        if (rc || inflight == 0) break;
        if ((rc = b.read(head, ends[head], stopped))) break;
        s.saw(ends[head], stopped);
        turns = s.assign();
        head ^= 1;
        --inflight;
        if (s.done()) break;
    }
    return rc;
}

// the schedule over given iteration counts: a request that starts in step s and runs n iterations
// raises its stop flag in step s + n (the bookkeeping of iteration n runs in the step after it)
struct ServeCounts {
    const int32_t* iterations;
    const ServeSchedule* sched;
    bool more(const ServeSchedule&) const { return false; }   // no request waits: nothing left to decide
    int enqueue(ServeSchedule& s, int, const std::vector<Turn>&)
    {
        s.staged_end += STOMP_GROUP_OPTIMIZE_CHUNK;
        return 0;
    }
    int read(int, int end, std::vector<char>& stopped) const
    {
        for (int p = 0; p < sched->P; ++p) {
            const int r = sched->cur[p];
            stopped[p] = r >= 0 && sched->start[r] + iterations[r] <= end;
        }
        return 0;
    }
};

// where the result slab holds what: [n] DevTrack, [n][JN] best trajectories, [n][cap] cost
// histories, [P] padding-collision flags of the slots' last retargets
struct SlabMap {
    size_t best, costs, flags, total;
    SlabMap(int n, int JN, int cap, int P)
    {
        best = align256(sizeof(DevTrack) * n);
        costs = best + align256(sizeof(double) * (size_t)n * JN);
        flags = costs + align256(sizeof(double) * (size_t)n * cap);
        total = flags + align256(sizeof(int) * P);
    }
};

// the device side of the loop
struct ServeDevice {
    stomp_group* g;
    OptimizeLoop& o;
    const double *starts, *goals;
    const uint64_t* seeds;
    SlabMap at;
    int cap;                          // cost history entries per request in the slab
    std::vector<char> flag_unknown;   // slots retargeted by this call
    int last_read = -1;               // the pipeline slot read last: its staging is free again
    // the turnover of the chunk being enqueued, device side
    const TurnArgs* d_turn = nullptr; const RequestArgs* d_req = nullptr; const NoiseArgs* d_nz = nullptr;
    const FlagCopy* d_fc = nullptr;
    int nturn = 0, nfc = 0;

    TurnArgs turn_args(int p, int prev, bool reinit) const
    {
        const int JN = g->e[0]->J * g->e[0]->N;
        TurnArgs t{};
        t.t = track_args(g, p);
        if (prev >= 0) {
            t.out_track = (DevTrack*)g->d_slab + prev;
            t.out_best = (double*)(g->d_slab + at.best) + (size_t)prev * JN;
            t.out_costs = (double*)(g->d_slab + at.costs) + (size_t)prev * cap;
        }
        t.reinit = reinit ? 1 : 0;
        return t;
    }

    bool more(const ServeSchedule& s) const { return o.next <= last_work(s); }
    // the last step in which a slot has work: its request's flush, the step after its max_iterations
    int last_work(const ServeSchedule& s) const
    {
        int last = 0;
        for (int p = 0; p < s.P; ++p)
            if (s.cur[p] >= 0) last = std::max(last, o.start[p] + g->e[p]->max_it);
        return last;
    }

    int enqueue(ServeSchedule& s, int slot, const std::vector<Turn>& turns)
    {
        const int J = g->e[0]->J;
        // the host side of the turnovers first: the chunk's steps are staged from it
        for (const Turn& t : turns) {
            stomp_engine* e = g->e[t.slot];
            // (the flag: the one the host holds, until the call's end brings the device's back)
            retarget_host_state(e, starts + (size_t)t.request * J, goals + (size_t)t.request * J, &seeds[t.request],
                                e->pad_collision);
            e->pre_it = 1;   // the turnover's grouped pregen
            o.start[t.slot] = o.next;
            flag_unknown[t.slot] = 1;
        }
        o.live.clear();
        for (int p = 0; p < s.P; ++p)
            if (s.cur[p] >= 0 && !(g->compact && s.seen[p])) o.live.push_back(p);
        o.last_step = s.waiting() ? (1 << 30) : last_work(s);
        ChunkExtra extra;
        extra.stage = [&](Arena& a) -> int {
            const double* d_vec = nullptr;
            nturn = (int)turns.size();
            nfc = (int)o.flag_copies.size();
            TurnArgs* ht = a.take(nturn, d_turn);
            RequestArgs* hr = a.take(nturn, d_req);
            NoiseArgs* hn = a.take(nturn, d_nz);
            double* hv = a.take((size_t)nturn * 2 * J, d_vec);
            FlagCopy* hf = a.take(nfc, d_fc);
            if (a.overflowed()) return gfail(g, STOMP_E_INVALID, "group serve staging overflow");
            for (int k = 0; k < nturn; ++k) {
                const Turn& t = turns[k];
                stomp_engine* e = g->e[t.slot];
                ht[k] = turn_args(t.slot, t.prev, true);
                std::memcpy(hv + (size_t)k * 2 * J, starts + (size_t)t.request * J, sizeof(double) * J);
                std::memcpy(hv + (size_t)k * 2 * J + J, goals + (size_t)t.request * J, sizeof(double) * J);
                hr[k] = kept_request_args(e, d_vec + (size_t)k * 2 * J, (int*)(g->d_slab + at.flags) + t.slot,
                                          g->d_models + t.slot);
                hn[k] = pregen_args(e, 1);
            }
            if (nfc) std::memcpy(hf, o.flag_copies.data(), sizeof(FlagCopy) * nfc);
            return 0;
        };
        extra.launch = [&]() {
            stomp_engine* e0 = g->e[0];
            if (nturn > 0) {
                launch_serve_turnover(d_turn, nturn, e0->J * e0->N, g->stream);
                launch_retarget(d_req, nturn, e0->J, e0->N, false, g->stream);
                launch_pregen_group(g->shape, d_nz, nturn, e0->K_loc, g->stream);
                o.launches += 3;
            }
            if (nfc > 0) {
                launch_serve_flags(d_fc, nfc, g->stream);
                ++o.launches;
            }
        };
        if (int rc = optimize_enqueue_chunk(o, slot, &extra)) return rc;
        s.staged_end = o.next - 1;
        return 0;
    }

    int read(int head, int, std::vector<char>& stopped)
    {
        const int P = (int)g->e.size();
        if (hipEventSynchronize(g->opt_ev[head]) != hipSuccess) return gfail(g, STOMP_E_DEVICE, "group read-back wait failed");
        const int* hm = g->h_mirror + (size_t)head * 2 * P;
        for (int p = 0; p < P; ++p) stopped[p] = hm[2 * p] != 0;
        last_read = head;
        return 0;
    }
};

// what stomp_group_serve_info reports of a finished schedule
void serve_report(stomp_group* g, const ServeSchedule& s, const std::vector<int>& iterations, long long launches,
                  long long slab_bytes, long long allocs)
{
    long long steps = 0, occupied = 0, gap = 0;
    for (int r = 0; r < s.n; ++r) {
        steps = std::max<long long>(steps, s.start[r] + iterations[r]);
        occupied += iterations[r];
    }
    // a slot's requests in the order it took them: the gap between a stop and the next iteration 1
    std::vector<int> last(s.P, -1);
    for (int r = 0; r < s.n; ++r) {
        const int q = last[s.slot[r]];
        if (q >= 0) gap = std::max<long long>(gap, s.start[r] - (s.start[q] + iterations[q]));
        last[s.slot[r]] = r;
    }
    // steps in which two live slots ran different iteration numbers: requests that overlap in time
    // and did not start in the same step
    std::vector<int> lo(steps + 2, 1 << 30), hi(steps + 2, -1);
    for (int r = 0; r < s.n; ++r)
        for (int st = s.start[r]; st < s.start[r] + iterations[r]; ++st) {
            lo[st] = std::min(lo[st], st - s.start[r] + 1);
            hi[st] = std::max(hi[st], st - s.start[r] + 1);
        }
    long long mixed = 0;
    for (long long st = 1; st <= steps; ++st) mixed += hi[st] > lo[st] ? 1 : 0;
    const long long v[8] = {steps, occupied, s.n - std::min(s.P, s.n), mixed, gap, launches, slab_bytes, allocs};
    std::memcpy(g->serve_info, v, sizeof v);
}

}  // namespace

extern "C" {

int stomp_serve_schedule(int32_t num_slots, int32_t num_requests, const int32_t* iterations, int32_t* slot,
                         int32_t* start_step, int32_t* total_steps)
{
    if (num_slots <= 0 || num_requests <= 0 || !iterations || !slot || !start_step)
        return gfail(nullptr, STOMP_E_INVALID, "serve schedule: invalid arguments");
    for (int r = 0; r < num_requests; ++r)
        if (iterations[r] < 1) return gfail(nullptr, STOMP_E_INVALID, "serve schedule: a request runs at least one iteration");
    ServeSchedule s(num_slots, num_requests);
    ServeCounts b{iterations, &s};
    serve_drive(s, b);
    int total = 0;
    for (int r = 0; r < num_requests; ++r) {
        slot[r] = s.slot[r];
        start_step[r] = s.start[r];
        total = std::max(total, s.start[r] + iterations[r]);
    }
    if (total_steps) *total_steps = total;
    return 0;
}

int stomp_group_serve_info(stomp_group* g, int64_t info[8])
{
    if (!g || !info) return gfail(nullptr, STOMP_E_INVALID, "null argument");
    for (int i = 0; i < 8; ++i) info[i] = g->serve_info[i];
    return 0;
}

int stomp_group_serve(stomp_group* g, const double* starts, const double* goals, const uint64_t* seeds,
                      int32_t num_requests, stomp_serve_result* results, double* best_trajectories,
                      double* costs_per_iteration, int32_t costs_stride)
{
    // all of this before any engine or device is touched
    if (!g) return gfail(nullptr, STOMP_E_INVALID, "null group");
    // (the group is not touched either, not even for the message: stomp_last_error has it)
    if (!starts || !goals || !seeds) return gfail(nullptr, STOMP_E_INVALID, "serve: null starts, goals or seeds");
    if (!results || !best_trajectories)
        return gfail(nullptr, STOMP_E_INVALID, "serve: null results or best_trajectories");
    if (num_requests <= 0) return gfail(nullptr, STOMP_E_INVALID, "serve: num_requests is not positive");
    const int P = (int)g->e.size(), n = num_requests;
    stomp_engine* e0 = g->e[0];
    const int J = e0->J, N = e0->N, JN = J * N;
    for (int r = 0; r < n; ++r)
        for (int d = 0; d < J; ++d)
            if (!std::isfinite(starts[(size_t)r * J + d]) || !std::isfinite(goals[(size_t)r * J + d])) {
                char buf[120];
                snprintf(buf, sizeof buf, "serve: start / goal of request %d, joint %d is not finite", r, d);
                return gfail(g, STOMP_E_INVALID, buf);
            }
    int maxcap = 0;
    for (stomp_engine* e : g->e) {
        if (e->world > 1 || e->gather)
            return gfail(g, STOMP_E_UNSUPPORTED, "retargeting is single-rank (a sharded engine's ranks would have to "
                                                 "retarget in lockstep)");
        if (e->tracking) return gfail(g, STOMP_E_INVALID, "an engine of the group is inside its own optimize loop");
        if (e->max_it <= 0) return gfail(g, STOMP_E_INVALID, "serve: an engine of the group has no iterations to run");
        maxcap = std::max(maxcap, e->max_it);
    }
    if (costs_per_iteration && costs_stride < maxcap)
        return gfail(g, STOMP_E_INVALID, "costs_stride is smaller than an engine's max_iterations");
    if (int rc = check_epochs(g)) return rc;

    DeviceGuard dg(g->device);
    long long allocs = g->d_mirror ? 0 : 5;
    if (int rc = optimize_prepare(g)) return rc;
    const SlabMap at(n, JN, maxcap, P);
    if (at.total > g->slab_cap) {
        // (no launch reads the old slab: every call that used it waited for the stream)
        const size_t grown = std::max(at.total, 2 * g->slab_cap);
        if (g->d_slab) hipFree(g->d_slab);
        g->d_slab = nullptr;
        g->slab_cap = 0;
        if (hipMalloc((void**)&g->d_slab, grown) != hipSuccess) return gfail(g, STOMP_E_DEVICE, "group serve allocation failed");
        g->slab_cap = grown;
        ++allocs;
    }

    OptimizeLoop o;
    o.g = g;
    o.after.resize(P);
    o.start.assign(P, 1);
    if (e0->Kr > 0)
        for (int p = 0; p < P; ++p) o.after[p].resize((size_t)g->e[p]->max_it);
    ServeSchedule s(P, n);
    ServeDevice dev{g, o, starts, goals, seeds, at, maxcap, std::vector<char>(P, 0)};
    o.flag_unknown = &dev.flag_unknown;
    int rc = serve_drive(s, dev);

    // The loop is over (rc: how).  Every used slot leaves as stomp_group_optimize leaves an engine:
    // the steps enqueued past its stop were no-ops, it holds no pregen rows and nothing pending.
    hipStream_t st = g->stream;
    std::vector<int> used;
    for (int p = 0; p < P; ++p)
        if (s.cur[p] >= 0) used.push_back(p);
    for (int p : used) {
        stomp_engine* e = g->e[p];
        e->pending_member = -1;
        e->pre_it = -1;
        e->rows_in_pre = false;
    }
    hipError_t err = hipGetLastError();
    if (!rc && err != hipSuccess) rc = gfail(g, STOMP_E_DEVICE, hipGetErrorString(err));
    if (!rc && dev.last_read >= 0) {
        // the slots' last requests into the slab, staged where the chunk read last was staged: the
        // loop ends behind a read, before that pipeline slot is staged again, so its upload and its
        // launches are done
        Arena a{g->h_opt + (size_t)dev.last_read * g->opt_slot, g->d_opt + (size_t)dev.last_read * g->opt_slot, g->opt_slot};
        const TurnArgs* d_turn = nullptr;
        TurnArgs* ht = a.take(used.size(), d_turn);
        for (size_t k = 0; k < used.size(); ++k) ht[k] = dev.turn_args(used[k], s.cur[used[k]], false);
        if (hipMemcpyAsync(a.d, a.h, a.used(), hipMemcpyHostToDevice, st) != hipSuccess)
            rc = gfail(g, STOMP_E_DEVICE, "group argument upload failed");
        else {
            launch_serve_turnover(d_turn, (int)used.size(), JN, st);
            ++o.launches;
        }
    }
    // later launches (iterate / run / eval) are not gated
    launch_track_start_group(g->d_track_all, P, true, st);
    ++o.launches;
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = gfail(g, STOMP_E_DEVICE, "group synchronize failed");
    std::vector<unsigned char> slab;
    if (!rc) {
        slab.resize(at.total);
        if (hipMemcpy(slab.data(), g->d_slab, at.total, hipMemcpyDeviceToHost) != hipSuccess)
            rc = gfail(g, STOMP_E_DEVICE, "group serve read-back failed");
    }
    if (rc) return rc;
    const DevTrack* tracks = (const DevTrack*)slab.data();
    const double* best = (const double*)(slab.data() + at.best);
    const double* costs = (const double*)(slab.data() + at.costs);
    const int* flags = (const int*)(slab.data() + at.flags);
    std::vector<int> iterations(n);
    for (int r = 0; r < n; ++r) {
        const DevTrack& t = tracks[r];
        iterations[r] = t.iterations;
        results[r].slot = s.slot[r];
        results[r].start_step = s.start[r];
        results[r].stats = stats_from_track(g->e[s.slot[r]], t);
        std::memcpy(best_trajectories + (size_t)r * JN, best + (size_t)r * JN, sizeof(double) * JN);
        if (costs_per_iteration && t.iterations > 0)
            std::memcpy(costs_per_iteration + (size_t)r * costs_stride, costs + (size_t)r * maxcap,
                        sizeof(double) * std::min(t.iterations, maxcap));
    }
    for (int p : used) {
        stomp_engine* e = g->e[p];
        optimize_restore(o, p, iterations[s.cur[p]]);
        // the flag of the slot's last retarget, which the device has held since its turnover
        e->model.pad_collision = e->pad_collision = g->pad_flags[p] = flags[p];
    }
    serve_report(g, s, iterations, o.launches, (long long)g->slab_cap, allocs);
    return 0;
}

}  // extern "C"
