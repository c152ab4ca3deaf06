// engine_query.cpp -- stomp_engine_query_states: a batch of joint states against the model and the
// field the engine holds now (k_query.hip).  The call validates on the host, then works through the
// states in chunks: a chunk's states go joint-major into one pinned staging block, one upload, the
// query launch and the transposes of the per-sphere outputs on the engine's stream, one download,
// one wait, and the caller's arrays are filled from the staging.  Nothing the engine's iterations
// read or write is touched: the call has no flush, no swap, no counter of theirs.
#include "engine_internal.h"
#include "query.h"

#include <cstdlib>

using namespace stomp;

namespace {

constexpr size_t kQueryStageBudget = (size_t)48 << 20;   // device staging of one chunk (the contract: <= 64 MiB)
constexpr long long kQueryChunkMax = 65536;

// which outputs a query names
struct Want {
    bool pos, dist, pot, col, link, cost, clear, min_s, in_col, lim;
    explicit Want(const stomp_state_query& q)
        : pos(q.positions), dist(q.distances), pot(q.potentials), col(q.sphere_collides),
          link(q.link_costs && q.num_links > 0), cost(q.state_cost), clear(q.min_clearance), min_s(q.min_sphere),
          in_col(q.in_collision), lim(q.limits_violated)
    {
    }
};

// Where one chunk's staging of capacity C states holds what (bytes): the inputs (uploaded), the
// caller-shaped outputs (downloaded; the pinned block holds the same offsets), then the kernel's
// sphere-major outputs (device only).
struct QueryMap {
    size_t q = 0, seg_link = 0, link_idx = 0, in_end = 0;
    size_t o_pos = 0, o_dist = 0, o_pot = 0, o_col = 0, o_link = 0, o_cost = 0, o_clear = 0, o_min = 0, o_in_col = 0,
           o_lim = 0, out_end = 0;
    size_t r_pos = 0, r_dist = 0, r_pot = 0, r_col = 0, r_link = 0, total = 0;
    QueryMap(const Want& w, size_t C, int J, int S, int L, int nseg)
    {
        size_t o = 0;
        auto take = [&](size_t& at, bool on, size_t bytes) {
            at = o;
            if (on) o += align256(bytes);
        };
        take(q, true, sizeof(double) * J * C);
        take(seg_link, true, sizeof(int) * (nseg + 1));
        take(link_idx, true, sizeof(int) * std::max(L, 1));
        in_end = o;
        take(o_pos, w.pos, sizeof(double) * 3 * S * C);
        take(o_dist, w.dist, sizeof(double) * S * C);
        take(o_pot, w.pot, sizeof(double) * S * C);
        take(o_col, w.col, (size_t)S * C);
        take(o_link, w.link, sizeof(double) * L * C);
        take(o_cost, w.cost, sizeof(double) * C);
        take(o_clear, w.clear, sizeof(double) * C);
        take(o_min, w.min_s, sizeof(int32_t) * C);
        take(o_in_col, w.in_col, C);
        take(o_lim, w.lim, C);
        out_end = o;
        take(r_pos, w.pos, sizeof(double) * 3 * S * C);
        take(r_dist, w.dist, sizeof(double) * S * C);
        take(r_pot, w.pot, sizeof(double) * S * C);
        take(r_col, w.col, (size_t)S * C);
        take(r_link, w.link, sizeof(double) * L * C);
        total = o;
    }
};

// states per chunk: STOMP_DEBUG_QUERY_CHUNK (read per call), else the most (a multiple of 64 once
// there are 64) whose staging stays inside the budget
long long chunk_states(const Want& w, long long M, int J, int S, int L, int nseg)
{
    if (const char* dbg = std::getenv("STOMP_DEBUG_QUERY_CHUNK")) {
        const long long v = std::atoll(dbg);
        if (v >= 1) return std::min(v, kQueryChunkMax);
    }
    long long c = std::min(M, kQueryChunkMax);
    while (c > 1 && QueryMap(w, (size_t)c, J, S, L, nseg).total > kQueryStageBudget) c = (c + 1) / 2;
    if (c < M && c >= 64) c -= c % 64;   // whole waves, when the call has more than one chunk
    return c;
}

int query_validate(const stomp_engine* e, const stomp_state_query* q)
{
    if (q->num_states < 1) return fail(nullptr, STOMP_E_INVALID, "query: num_states %d is below 1", q->num_states);
    if (q->num_links < 0) return fail(nullptr, STOMP_E_INVALID, "query: num_links %d is negative", q->num_links);
    if (q->num_links >= 1 && !q->links)
        return fail(nullptr, STOMP_E_INVALID, "query: %d links and no link array", q->num_links);
    if (q->link_costs && q->num_links == 0) return fail(nullptr, STOMP_E_INVALID, "query: link_costs without links");
    for (int l = 0; l < q->num_links; ++l)
        if (q->links[l] < 0 || q->links[l] >= e->nseg)
            return fail(nullptr, STOMP_E_INVALID, "query: link %d names segment %d, the tree has %d", l, q->links[l],
                        e->nseg);
    const size_t n = (size_t)q->num_states * e->J;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(q->states[i]))
            return fail(nullptr, STOMP_E_INVALID, "query: state %zu, joint %zu is not finite", i / e->J, i % e->J);
    if (e->tracking) return fail(nullptr, STOMP_E_INVALID, "query: the engine is inside its optimize loop");
    return 0;
}

int query_run(stomp_engine* e, const stomp_state_query* q)
{
    const Want w(*q);
    const int J = e->J, S = e->model.S, L = q->num_links, nseg = e->nseg;
    const long long M = q->num_states;
    const long long C = chunk_states(w, M, J, S, L, nseg);
    const QueryMap at(w, (size_t)C, J, S, L, nseg);
    e->q_chunks = 0;
    e->q_launches = 0;
    e->q_chunk_states = C;
    e->q_kernel_ms = 0.0;
    const size_t cap = e->qs_cap;
    if (!reserve_stage(&e->h_qs, &e->d_qs, &e->qs_cap, at.total))
        return fail(e, STOMP_E_DEVICE, "query staging allocation of %zu bytes failed", at.total);
    if (e->qs_cap != cap) e->q_allocs += 2;
    for (hipEvent_t& ev : e->q_ev)
        if (!ev) HIP_TRY(e, hipEventCreate(&ev));
    unsigned char *h = e->h_qs, *d = e->d_qs;
    hipStream_t s = e->stream;

    // the links by segment (the same for every chunk): link_idx ordered by segment, a segment's
    // entries in list order
    int* seg_link = (int*)(h + at.seg_link);
    int* link_idx = (int*)(h + at.link_idx);
    std::fill(seg_link, seg_link + nseg + 1, 0);
    for (int l = 0; l < L; ++l) ++seg_link[q->links[l] + 1];
    for (int g = 0; g < nseg; ++g) seg_link[g + 1] += seg_link[g];
    {
        std::vector<int> next(seg_link, seg_link + nseg);
        for (int l = 0; l < L; ++l) link_idx[next[q->links[l]]++] = l;
    }
    const RolloutLds lay = model_image_layout(e, e->model);
    const unsigned char* img = (const unsigned char*)e->model.img;

    for (long long m0 = 0; m0 < M; m0 += C) {
        const int mc = (int)std::min(C, M - m0);
        double* hq = (double*)(h + at.q);
        for (int i = 0; i < mc; ++i) {
            const double* row = q->states + (size_t)(m0 + i) * J;
            for (int j = 0; j < J; ++j) hq[(size_t)j * mc + i] = row[j];
        }
        HIP_TRY(e, hipMemcpyAsync(d, h, at.in_end, hipMemcpyHostToDevice, s));
        QueryArgs a{};
        a.M = mc; a.L = L;
        a.q = (const double*)(d + at.q);
        a.hl = (const int*)(img + (lay.hl - lay.sph));
        a.jlim = (const double*)(img + (lay.jlim - lay.sph));
        a.seg_link = (const int*)(d + at.seg_link);
        a.link_idx = (const int*)(d + at.link_idx);
        if (w.pos) a.pos = (double*)(d + at.r_pos);
        if (w.dist) a.dist = (double*)(d + at.r_dist);
        if (w.pot) a.pot = (double*)(d + at.r_pot);
        if (w.col) a.col = d + at.r_col;
        if (w.link) {
            a.link = (double*)(d + at.r_link);
            HIP_TRY(e, hipMemsetAsync(a.link, 0, sizeof(double) * L * mc, s));
        }
        if (w.cost) a.cost = (double*)(d + at.o_cost);
        if (w.clear) a.clear = (double*)(d + at.o_clear);
        if (w.min_s) a.min_s = (int*)(d + at.o_min);
        if (w.in_col) a.in_col = d + at.o_in_col;
        if (w.lim) a.lim = d + at.o_lim;
        HIP_TRY(e, hipEventRecord(e->q_ev[0], s));
        launch_query_states(e->model, a, s);
        ++e->q_launches;
        if (w.pos) { launch_query_transpose(a.pos, (double*)(d + at.o_pos), 3 * S, mc, s); ++e->q_launches; }
        if (w.dist) { launch_query_transpose(a.dist, (double*)(d + at.o_dist), S, mc, s); ++e->q_launches; }
        if (w.pot) { launch_query_transpose(a.pot, (double*)(d + at.o_pot), S, mc, s); ++e->q_launches; }
        if (w.col) { launch_query_transpose(a.col, d + at.o_col, S, mc, s); ++e->q_launches; }
        if (w.link) { launch_query_transpose(a.link, (double*)(d + at.o_link), L, mc, s); ++e->q_launches; }
        HIP_TRY(e, hipGetLastError());
        HIP_TRY(e, hipEventRecord(e->q_ev[1], s));
        if (at.out_end > at.in_end)
            HIP_TRY(e, hipMemcpyAsync(h + at.in_end, d + at.in_end, at.out_end - at.in_end, hipMemcpyDeviceToHost, s));
        SYNC_TRY(e);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e->q_ev[0], e->q_ev[1]) == hipSuccess) e->q_kernel_ms += ms;
        ++e->q_chunks;
        const size_t n = (size_t)mc, o = (size_t)m0;
        if (w.pos) std::memcpy(q->positions + o * 3 * S, h + at.o_pos, sizeof(double) * 3 * S * n);
        if (w.dist) std::memcpy(q->distances + o * S, h + at.o_dist, sizeof(double) * S * n);
        if (w.pot) std::memcpy(q->potentials + o * S, h + at.o_pot, sizeof(double) * S * n);
        if (w.col) std::memcpy(q->sphere_collides + o * S, h + at.o_col, (size_t)S * n);
        if (w.link) std::memcpy(q->link_costs + o * L, h + at.o_link, sizeof(double) * L * n);
        if (w.cost) std::memcpy(q->state_cost + o, h + at.o_cost, sizeof(double) * n);
        if (w.clear) std::memcpy(q->min_clearance + o, h + at.o_clear, sizeof(double) * n);
        if (w.min_s) std::memcpy(q->min_sphere + o, h + at.o_min, sizeof(int32_t) * n);
        if (w.in_col) std::memcpy(q->in_collision + o, h + at.o_in_col, n);
        if (w.lim) std::memcpy(q->limits_violated + o, h + at.o_lim, n);
    }
    return 0;
}

}  // namespace

extern "C" int stomp_engine_query_states(stomp_engine* e, const stomp_state_query* q)
{
    // (up to here e is not touched)
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    if (!q) return fail(nullptr, STOMP_E_INVALID, "query: null query");
    if (q->struct_size != (int32_t)sizeof(stomp_state_query))
        return fail(nullptr, STOMP_E_INVALID, "query: struct_size is not sizeof(stomp_state_query)");
    if (!q->states) return fail(nullptr, STOMP_E_INVALID, "query: null states");
    if (int rc = query_validate(e, q)) return rc;   // host only: no device is touched yet
    DeviceGuard dg(e->device);
    return query_run(e, q);
}

extern "C" int stomp_engine_query_info(stomp_engine* e, int64_t info[4])
{
    if (!e || !info) return fail(nullptr, STOMP_E_INVALID, "null argument");
    info[0] = e->q_chunks;
    info[1] = e->q_launches;
    info[2] = e->q_allocs;
    info[3] = e->q_chunk_states;
    return 0;
}

extern "C" int stomp_engine_query_time(stomp_engine* e, double* kernel_ms)
{
    if (!e || !kernel_ms) return fail(nullptr, STOMP_E_INVALID, "null argument");
    *kernel_ms = e->q_kernel_ms;
    return 0;
}
