// Stand-alone host program (built by tests/test_gradient_query_abi.py with -fsanitize=address,undefined):
// the host-only part of stomp_engine_query_gradients -- the request's validation and the model's
// tables (csrc/query_grad_host.h) -- on arrays allocated at their exact sizes, so that a read or a
// write past an end is caught.  No device, no engine library.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "query_grad_host.h"

namespace {

struct Seg { int parent, q_index; };
struct Op { int seg, base, save, sph_begin, sph_end, slot; };

int failures = 0;

void expect(bool ok, const char* what)
{
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

}  // namespace

int main()
{
    using namespace stomp;
    // a tree of 6 segments and 4 joints: base(fixed) - a(q0) - b(q2) - c(fixed) and a - d(q3); joint 1 drives nothing
    const std::vector<Seg> segs = {{-1, -1}, {0, 0}, {1, 2}, {2, -1}, {1, 3}, {4, -1}};
    const int nseg = (int)segs.size(), J = 4;
    std::vector<unsigned> mask(nseg);
    std::vector<int> joint_seg(J);
    grad_query_joint_paths(segs.data(), nseg, J, mask.data(), joint_seg.data());
    expect(mask[0] == 0u && mask[1] == 1u && mask[2] == 5u && mask[3] == 5u && mask[4] == 9u && mask[5] == 9u, "masks");
    expect(joint_seg[0] == 1 && joint_seg[1] == -1 && joint_seg[2] == 2 && joint_seg[3] == 4, "joint segments");

    // the FK program: a segment's spheres in two runs (the second step emits only), a segment without spheres
    const std::vector<Op> ops = {{0, -1, -1, 0, 0, -1}, {1, -2, 0, 0, 2, 0}, {-1, -2, -1, 2, 3, 0}, {2, -2, -1, 3, 3, -1},
                                 {3, -2, -1, 3, 4, 1}, {4, 0, -1, 4, 6, 2}};
    std::vector<int> sph_seg(6, -7);
    grad_query_sphere_segments(ops.data(), (int)ops.size(), sph_seg.data());
    const int want_seg[6] = {1, 1, 1, 3, 4, 4};
    expect(std::memcmp(sph_seg.data(), want_seg, sizeof want_seg) == 0, "sphere segments");

    // the request's checks
    const int M = 3;
    std::vector<double> states((size_t)M * J, 0.25);
    std::vector<int32_t> links = {0, 5, 1, 1};
    std::vector<double> lg((size_t)M * links.size() * J, -1.0);
    char why[160];
    auto make = [&]() {
        stomp_gradient_query q;
        std::memset(&q, 0, sizeof q);
        q.struct_size = (int32_t)sizeof q;
        q.num_states = M;
        q.states = states.data();
        q.num_links = (int32_t)links.size();
        q.links = links.data();
        q.link_gradients = lg.data();
        return q;
    };
    stomp_gradient_query q = make();
    expect(grad_query_check(&q, J, nseg, why, sizeof why) == 0, "a good request");
    q = make(); q.num_states = 0;
    expect(grad_query_check(&q, J, nseg, why, sizeof why) == STOMP_E_INVALID && std::strstr(why, "num_states"), "M = 0");
    q = make(); q.num_links = -1;
    expect(grad_query_check(&q, J, nseg, why, sizeof why) == STOMP_E_INVALID && std::strstr(why, "negative"), "L < 0");
    q = make(); q.links = nullptr;
    expect(grad_query_check(&q, J, nseg, why, sizeof why) == STOMP_E_INVALID && std::strstr(why, "no link array"), "no links");
    q = make(); q.num_links = 0; q.links = nullptr;
    expect(grad_query_check(&q, J, nseg, why, sizeof why) == STOMP_E_INVALID && std::strstr(why, "link_gradients without links"),
           "link_gradients without links");
    q = make(); q.num_links = 0; q.links = nullptr; q.link_gradients = nullptr;
    expect(grad_query_check(&q, J, nseg, why, sizeof why) == 0, "no links, no link outputs");
    links[3] = nseg;
    q = make();
    expect(grad_query_check(&q, J, nseg, why, sizeof why) == STOMP_E_INVALID && std::strstr(why, "names segment"), "link at nseg");
    links[3] = -1;
    q = make();
    expect(grad_query_check(&q, J, nseg, why, sizeof why) == STOMP_E_INVALID && std::strstr(why, "names segment"), "link below 0");
    links[3] = 1;
    q = make(); q.field_bias[1] = std::numeric_limits<double>::infinity();
    expect(grad_query_check(&q, J, nseg, why, sizeof why) == STOMP_E_INVALID && std::strstr(why, "field_bias[1]"), "infinite bias");
    q = make(); q.field_bias[2] = std::nan("");
    expect(grad_query_check(&q, J, nseg, why, sizeof why) == STOMP_E_INVALID && std::strstr(why, "field_bias[2]"), "NaN bias");
    states.back() = std::nan("");                       // the last value read
    q = make();
    expect(grad_query_check(&q, J, nseg, why, sizeof why) == STOMP_E_INVALID && std::strstr(why, "state 2, joint 3"), "NaN state");
    char tiny[8];                                       // a short message buffer is not overrun
    expect(grad_query_check(&q, J, nseg, tiny, sizeof tiny) == STOMP_E_INVALID && std::strlen(tiny) == 7, "short buffer");
    for (double v : lg) expect(v == -1.0, "an output was written");
    if (failures) return 1;
    std::printf("host check passed\n");
    return 0;
}
