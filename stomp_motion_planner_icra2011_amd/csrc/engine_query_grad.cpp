// engine_query_grad.cpp -- stomp_engine_query_gradients: a batch of joint states against the model
// and the field the engine holds now (k_query_grad.hip).  As the state query (engine_query.cpp): the
// call validates on the host, then works through the states in chunks on the query's own staging:
// one upload, one launch on the engine's stream, one download and one wait per chunk, and the
// caller's arrays are filled from the pinned block.  Nothing the engine's iterations read or write
// is touched.
#include "engine_internal.h"
#include "query_grad.h"
#include "query_grad_host.h"

#include <cstdlib>

using namespace stomp;

namespace {

constexpr size_t kQueryStageBudget = (size_t)48 << 20;   // device staging of one chunk, as the state query's
constexpr long long kQueryChunkMax = 65536;

struct Want {
    bool fg, pg, link_cost, link_grad, cost, grad, in_col;
    explicit Want(const stomp_gradient_query& q)
        : fg(q.field_gradients), pg(q.potential_gradients), link_cost(q.link_costs && q.num_links > 0),
          link_grad(q.link_gradients && q.num_links > 0), cost(q.state_cost), grad(q.state_gradient),
          in_col(q.in_collision)
    {
    }
};

// Where one chunk's staging of capacity C states holds what (bytes): the inputs (uploaded), then
// the outputs in the caller's shape (downloaded; the pinned block holds the same offsets)
struct GradMap {
    size_t q = 0, sph_seg = 0, seg_mask = 0, joint_seg = 0, links = 0, in_end = 0;
    size_t o_fg = 0, o_pg = 0, o_link_cost = 0, o_link_grad = 0, o_cost = 0, o_grad = 0, o_in_col = 0, total = 0;
    GradMap(const Want& w, size_t C, int J, int S, int L, int nseg)
    {
        size_t o = 0;
        auto take = [&](size_t& at, bool on, size_t bytes) {
            at = o;
            if (on) o += align256(bytes);
        };
        take(q, true, sizeof(double) * J * C);
        take(sph_seg, true, sizeof(int) * std::max(S, 1));
        take(seg_mask, true, sizeof(unsigned) * nseg);
        take(joint_seg, true, sizeof(int) * J);
        take(links, true, sizeof(int) * std::max(L, 1));
        in_end = o;
        take(o_fg, w.fg, sizeof(double) * 3 * S * C);
        take(o_pg, w.pg, sizeof(double) * 3 * S * C);
        take(o_link_cost, w.link_cost, sizeof(double) * L * C);
        take(o_link_grad, w.link_grad, sizeof(double) * L * J * C);
        take(o_cost, w.cost, sizeof(double) * C);
        take(o_grad, w.grad, sizeof(double) * J * C);
        take(o_in_col, w.in_col, C);
        total = o;
    }
};

// states per chunk, by the state query's rule: STOMP_DEBUG_QUERY_CHUNK (read per call), else the
// most (a multiple of 64 once there are 64) whose staging stays inside the budget
long long chunk_states(const Want& w, long long M, int J, int S, int L, int nseg)
{
    if (const char* dbg = std::getenv("STOMP_DEBUG_QUERY_CHUNK")) {
        const long long v = std::atoll(dbg);
        if (v >= 1) return std::min(v, kQueryChunkMax);
    }
    long long c = std::min(M, kQueryChunkMax);
    while (c > 1 && GradMap(w, (size_t)c, J, S, L, nseg).total > kQueryStageBudget) c = (c + 1) / 2;
    if (c < M && c >= 64) c -= c % 64;
    return c;
}

int grad_run(stomp_engine* e, const stomp_gradient_query* q)
{
    const Want w(*q);
    const int J = e->J, S = e->model.S, L = q->num_links, nseg = e->nseg;
    const long long M = q->num_states;
    const long long C = chunk_states(w, M, J, S, L, nseg);
    const GradMap at(w, (size_t)C, J, S, L, nseg);
    e->q_chunks = 0;
    e->q_launches = 0;
    e->q_chunk_states = C;
    e->q_kernel_ms = 0.0;
    const size_t cap = e->qs_cap;
    if (!reserve_stage(&e->h_qs, &e->d_qs, &e->qs_cap, at.total))
        return fail(e, STOMP_E_DEVICE, "gradient query staging allocation of %zu bytes failed", at.total);
    if (e->qs_cap != cap) e->q_allocs += 2;
    for (hipEvent_t& ev : e->q_ev)
        if (!ev) HIP_TRY(e, hipEventCreate(&ev));
    unsigned char *h = e->h_qs, *d = e->d_qs;
    hipStream_t s = e->stream;

    // the model's tables (the same for every chunk)
    grad_query_sphere_segments(e->mt.ops.data(), (int)e->mt.ops.size(), (int*)(h + at.sph_seg));
    grad_query_joint_paths(e->h_segs.data(), nseg, J, (unsigned*)(h + at.seg_mask), (int*)(h + at.joint_seg));
    for (int l = 0; l < L; ++l) ((int*)(h + at.links))[l] = q->links[l];

    for (long long m0 = 0; m0 < M; m0 += C) {
        const int mc = (int)std::min(C, M - m0);
        std::memcpy(h + at.q, q->states + (size_t)m0 * J, sizeof(double) * J * mc);
        HIP_TRY(e, hipMemcpyAsync(d, h, at.in_end, hipMemcpyHostToDevice, s));
        GradQueryArgs a{};
        a.M = mc; a.L = L; a.J = J; a.S = S; a.nseg = nseg;
        for (int k = 0; k < 3; ++k) a.bias[k] = q->field_bias[k];
        a.q = (const double*)(d + at.q);
        a.sph_seg = (const int*)(d + at.sph_seg);
        a.seg_mask = (const unsigned*)(d + at.seg_mask);
        a.joint_seg = (const int*)(d + at.joint_seg);
        a.links = (const int*)(d + at.links);
        if (w.fg) a.fgrad = (double*)(d + at.o_fg);
        if (w.pg) a.pgrad = (double*)(d + at.o_pg);
        if (w.link_cost) a.link_cost = (double*)(d + at.o_link_cost);
        if (w.link_grad) a.link_grad = (double*)(d + at.o_link_grad);
        if (w.cost) a.cost = (double*)(d + at.o_cost);
        if (w.grad) a.grad = (double*)(d + at.o_grad);
        if (w.in_col) a.in_col = d + at.o_in_col;
        HIP_TRY(e, hipEventRecord(e->q_ev[0], s));
        launch_query_gradients(e->model, a, s);
        ++e->q_launches;
        HIP_TRY(e, hipGetLastError());
        HIP_TRY(e, hipEventRecord(e->q_ev[1], s));
        if (at.total > at.in_end)
            HIP_TRY(e, hipMemcpyAsync(h + at.in_end, d + at.in_end, at.total - at.in_end, hipMemcpyDeviceToHost, s));
        SYNC_TRY(e);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e->q_ev[0], e->q_ev[1]) == hipSuccess) e->q_kernel_ms += ms;
        ++e->q_chunks;
        const size_t n = (size_t)mc, o = (size_t)m0;
        if (w.fg) std::memcpy(q->field_gradients + o * 3 * S, h + at.o_fg, sizeof(double) * 3 * S * n);
        if (w.pg) std::memcpy(q->potential_gradients + o * 3 * S, h + at.o_pg, sizeof(double) * 3 * S * n);
        if (w.link_cost) std::memcpy(q->link_costs + o * L, h + at.o_link_cost, sizeof(double) * L * n);
        if (w.link_grad) std::memcpy(q->link_gradients + o * L * J, h + at.o_link_grad, sizeof(double) * L * J * n);
        if (w.cost) std::memcpy(q->state_cost + o, h + at.o_cost, sizeof(double) * n);
        if (w.grad) std::memcpy(q->state_gradient + o * J, h + at.o_grad, sizeof(double) * J * n);
        if (w.in_col) std::memcpy(q->in_collision + o, h + at.o_in_col, n);
    }
    return 0;
}

}  // namespace

extern "C" int stomp_engine_query_gradients(stomp_engine* e, const stomp_gradient_query* q)
{
    // (up to here e is not touched)
    if (!e) return fail(nullptr, STOMP_E_INVALID, "null engine");
    if (!q) return fail(nullptr, STOMP_E_INVALID, "gradient query: null query");
    if (q->struct_size != (int32_t)sizeof(stomp_gradient_query))
        return fail(nullptr, STOMP_E_INVALID, "gradient query: struct_size is not sizeof(stomp_gradient_query)");
    if (!q->states) return fail(nullptr, STOMP_E_INVALID, "gradient query: null states");
    // host only: no device is touched yet
    char why[160];
    if (int rc = grad_query_check(q, e->J, e->nseg, why, sizeof why)) return fail(nullptr, rc, "%s", why);
    if (e->tracking) return fail(nullptr, STOMP_E_INVALID, "gradient query: the engine is inside its optimize loop");
    if (e->grid_n[0] < 3 || e->grid_n[1] < 3 || e->grid_n[2] < 3)
        return fail(nullptr, STOMP_E_UNSUPPORTED, "gradient query: the field has fewer than 3 cells on an axis");
    const size_t lds = grad_query_lds(e->J, e->model.S, e->nseg);
    if (lds > kGradQueryLdsMax)
        return fail(nullptr, STOMP_E_UNSUPPORTED, "gradient query: the kernel needs %zu B of LDS, above %zu", lds,
                    kGradQueryLdsMax);
    DeviceGuard dg(e->device);
    return grad_run(e, q);
}
