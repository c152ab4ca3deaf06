// facade_collision_cost_driver.cpp -- StompOptimizer::getChompCollisionCost (the reference's
// GetChompCollisionCost.srv shape) on one problem: the states and the link segments come from files,
// every state's response goes to the output.
//
// usage: facade_collision_cost_driver <out.txt> <dir> [bias_x bias_y bias_z]
// The directory holds the problem.txt and sdf.bin that tests/facade_util.py writes, states.txt (M and
// J, then M x J values) and links.txt (L, then L segment indices).  Output: per state one line
// "valid in_collision", then its L costs, then its L x J gradient values, one value per line.  Exit
// code 9: a refusal that should have happened did not, or changed the output vector.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "stomp_motion_planner/stomp_facade.h"

using namespace stomp_motion_planner;

namespace {

struct Problem {
    StompParameters params;
    StompRobotModel robot;
    StompTrajectory traj;
    StompCollisionSpace space;
    std::vector<uint16_t> sdf;   // d2 per voxel
};

// the whitespace-separated text of tests/facade_util.py (as facade_driver.cpp reads it)
bool load(const std::string& dir, Problem& p)
{
    std::ifstream f(dir + "/problem.txt");
    if (!f) return false;
    int J, N, nseg, nsph, n;
    f >> J >> N >> nseg >> nsph >> n;
    p.traj.num_joints = J;
    p.traj.num_points = N;
    p.robot.segments.resize(nseg);
    for (auto& s : p.robot.segments) {
        f >> s.parent >> s.q_index;
        for (double& v : s.rot) f >> v;
        for (double& v : s.trans) f >> v;
        for (double& v : s.axis) f >> v;
    }
    p.robot.collision_points.resize(nsph);
    for (auto& s : p.robot.collision_points) {
        f >> s.segment >> s.radius >> s.clearance;
        for (double& v : s.pos) f >> v;
    }
    p.robot.joints.resize(J);
    for (auto& j : p.robot.joints) f >> j.has_limits >> j.min >> j.max >> j.joint_cost;
    p.traj.start.resize(J);
    p.traj.goal.resize(J);
    for (double& v : p.traj.start) f >> v;
    for (double& v : p.traj.goal) f >> v;
    StompParameters& q = p.params;
    q.noise_stddev.resize(J);
    q.noise_decay.resize(J);
    for (double& v : q.noise_stddev) f >> v;
    for (double& v : q.noise_decay) f >> v;
    int cum;
    f >> q.trajectory_discretization >> q.max_iterations >> q.max_iterations_after_collision_free >>
        q.smoothness_cost_weight >> q.obstacle_cost_weight >> q.smoothness_cost_velocity >>
        q.smoothness_cost_acceleration >> q.smoothness_cost_jerk >> q.ridge_factor >> cum >> q.num_rollouts >>
        q.num_reused_rollouts >> q.seed;
    q.use_cumulative_costs = cum != 0;
    stomp_grid& g = p.space.grid;
    g.nx = g.ny = g.nz = n;
    f >> g.origin[0] >> g.origin[1] >> g.origin[2] >> g.resolution;
    f >> p.robot.torque_root >> p.robot.torque_tip >> p.robot.gravity[0] >> p.robot.gravity[1] >> p.robot.gravity[2];
    p.robot.inertias.resize(nseg);
    for (auto& in : p.robot.inertias) {
        f >> in.mass;
        for (double& v : in.com) f >> v;
        for (double& v : in.inertia) f >> v;
    }
    if (!f) return false;
    p.sdf.resize((size_t)n * n * n);
    std::ifstream b(dir + "/sdf.bin", std::ios::binary);
    b.read(reinterpret_cast<char*>(p.sdf.data()), p.sdf.size() * sizeof(uint16_t));
    if (!b) return false;
    g.data = p.sdf.data();
    g.data_on_device = 0;
    return true;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3 && argc != 6) {
        std::cerr << "usage: facade_collision_cost_driver out.txt dir [bias_x bias_y bias_z]\n";
        return 2;
    }
    const std::string dir = argv[2];
    double bias[3] = {0.0, 0.0, 0.0};
    for (int k = 0; argc == 6 && k < 3; ++k) bias[k] = std::strtod(argv[3 + k], nullptr);
    Problem p;
    if (!load(dir, p)) {
        std::cerr << "cannot read problem " << dir << "\n";
        return 2;
    }
    std::vector<std::vector<double>> states;
    std::vector<int> links;
    {
        std::ifstream f(dir + "/states.txt");
        int M = 0, J = 0;
        f >> M >> J;
        states.assign(M, std::vector<double>(J));
        for (auto& s : states)
            for (double& v : s) f >> v;
        std::ifstream l(dir + "/links.txt");
        int L = -1;
        l >> L;
        if (L >= 0) links.resize(L);
        for (int& v : links) l >> v;
        if (!f || !l || M < 1 || L < 0) {
            std::cerr << "cannot read the states or the links of " << dir << "\n";
            return 2;
        }
    }
    StompOptimizer opt(&p.traj, &p.robot, &p.params, &p.space, Constraints(), 0, nullptr);
    if (!opt.ok()) {
        std::cerr << opt.lastError() << "\n";
        return 6;
    }
    std::vector<ChompCollisionCost> out;
    if (!opt.getChompCollisionCost(states, links, out, argc == 6 ? bias : nullptr)) {
        std::cerr << opt.lastError() << "\n";
        return 7;
    }
    // refusals: a state that is not finite, a link outside the tree, a bias that is not finite, no
    // states; out stays as it is
    {
        std::vector<ChompCollisionCost> kept = out;
        auto bad = states;
        bad[0][0] = std::numeric_limits<double>::quiet_NaN();
        std::vector<int> far = links;
        far.push_back((int)p.robot.segments.size());
        const double inf_bias[3] = {0.0, std::numeric_limits<double>::infinity(), 0.0};
        const bool refused = !opt.getChompCollisionCost(bad, links, kept) && !opt.lastError().empty() &&
                             !opt.getChompCollisionCost(states, far, kept) &&
                             !opt.getChompCollisionCost(states, links, kept, inf_bias) &&
                             opt.lastError().find("field_bias") != std::string::npos &&
                             !opt.getChompCollisionCost({}, links, kept);
        bool same = kept.size() == out.size();
        for (size_t m = 0; same && m < out.size(); ++m)
            same = kept[m].costs == out[m].costs && kept[m].gradient == out[m].gradient;
        if (!refused || !same) return 9;
    }
    FILE* o = std::fopen(argv[1], "w");
    if (!o) return 2;
    for (const ChompCollisionCost& c : out) {
        std::fprintf(o, "%d %d\n", c.valid ? 1 : 0, c.in_collision ? 1 : 0);
        for (double v : c.costs) std::fprintf(o, "%.17g\n", v);
        for (const auto& g : c.gradient)
            for (double v : g) std::fprintf(o, "%.17g\n", v);
    }
    std::fclose(o);
    return 0;
}
