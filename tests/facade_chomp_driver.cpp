// facade_chomp_driver.cpp -- StompOptimizer::optimize() with use_chomp (the reference's CHOMP mode,
// stomp_optimizer.cpp:289-299) on one problem, and the refusal of use_hamiltonian_monte_carlo.
//
// usage: facade_chomp_driver <out.txt> <dir>
// The directory holds the problem.txt and sdf.bin that tests/facade_util.py writes and chomp.txt:
// learning_rate, smoothness_cost_weight, use_pseudo_inverse, pseudo_inverse_ridge_factor, then J
// joint update limits.  Output: "iterations success success_iteration collision_success_iteration
// last_improvement_iteration best_cost last_cost last_collision_free", the cost history (one value per
// line), the best trajectory (J x N values, one per line), then the lastError() of an optimize()
// with use_hamiltonian_monte_carlo set on one line.  Exit code 9: that optimize() did not fail.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
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
    if (argc != 3) {
        std::cerr << "usage: facade_chomp_driver out.txt dir\n";
        return 2;
    }
    const std::string dir = argv[2];
    Problem p;
    if (!load(dir, p)) {
        std::cerr << "cannot read problem " << dir << "\n";
        return 2;
    }
    {
        std::ifstream f(dir + "/chomp.txt");
        int pinv = 0;
        f >> p.params.learning_rate >> p.params.smoothness_cost_weight >> pinv >> p.params.pseudo_inverse_ridge_factor;
        p.params.use_pseudo_inverse = pinv != 0;
        p.robot.joint_update_limits.resize(p.traj.num_joints);
        for (double& v : p.robot.joint_update_limits) f >> v;
        if (!f) {
            std::cerr << "cannot read chomp.txt of " << dir << "\n";
            return 2;
        }
    }
    p.params.use_chomp = true;
    StompOptimizer opt(&p.traj, &p.robot, &p.params, &p.space, Constraints(), 0, nullptr);
    if (!opt.ok()) {
        std::cerr << opt.lastError() << "\n";
        return 6;
    }
    if (!opt.optimize()) {
        std::cerr << opt.lastError() << "\n";
        return 7;
    }
    const STOMPStatistics& st = opt.getStatistics();
    FILE* o = std::fopen(argv[1], "w");
    if (!o) return 2;
    std::fprintf(o, "%d %d %d %d %d %.17g %.17g %d\n", st.iterations, st.success ? 1 : 0, st.success_iteration,
                 st.collision_success_iteration, st.last_improvement_iteration, st.best_cost, opt.lastTrajectoryCost(),
                 opt.lastTrajectoryCollisionFree() ? 1 : 0);
    for (double v : st.costs) std::fprintf(o, "%.17g\n", v);
    for (const auto& row : p.traj.free)
        for (size_t t = 0; t < row.size(); ++t) std::fprintf(o, "%.17g\n", row[t]);
    // Hamiltonian Monte Carlo is not built: optimize() fails and says so; the trajectory stays
    StompParameters hmc = p.params;
    hmc.use_hamiltonian_monte_carlo = true;
    StompTrajectory t2 = p.traj;
    StompOptimizer opt2(&t2, &p.robot, &hmc, &p.space, Constraints(), 0, nullptr);
    if (!opt2.ok()) return 6;
    const bool failed = !opt2.optimize();
    std::fprintf(o, "%s\n", opt2.lastError().c_str());
    std::fclose(o);
    return failed ? 0 : 9;
}
