// facade_batch_terms_driver.cpp -- StompOptimizer::optimizeBatch over problems with state-cost
// terms: one optimizer per problem, each with its own torque_cost_weight, constraint_cost_weight
// and orientation path constraints, all constructed on one shared stream and optimized as one
// engine group.
//
// usage: facade_batch_terms_driver <out.txt> <dir> [<dir> ...]
// Each directory holds the problem.txt and sdf.bin that tests/facade_util.py writes (read as
// facade_batch_driver.cpp reads them) and the terms.txt of tests/test_facade_batch_terms.py:
//   constraint_cost_weight torque_cost_weight num_constraints
//   per constraint: segment qx qy qz qw body_fixed roll_tol pitch_tol yaw_tol weight
// The output is facade_batch_driver's: per optimizer one line of statistics, then the cost history,
// the torques and the best trajectory, one value per line.
#include <cstdio>
#include <fstream>
#include <iostream>
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
    Constraints constraints;
    std::vector<uint16_t> sdf;   // d2 per voxel
};

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
    std::ifstream t(dir + "/terms.txt");
    int noc = 0;
    t >> q.constraint_cost_weight >> q.torque_cost_weight >> noc;
    if (!t || noc < 0) return false;
    p.constraints.orientation_constraints.resize(noc);
    for (auto& c : p.constraints.orientation_constraints) {
        t >> c.segment;
        for (double& v : c.orientation) t >> v;
        t >> c.body_fixed >> c.absolute_roll_tolerance >> c.absolute_pitch_tolerance >> c.absolute_yaw_tolerance >>
            c.weight;
    }
    if (!t) return false;
    p.sdf.resize((size_t)n * n * n);
    std::ifstream b(dir + "/sdf.bin", std::ios::binary);
    b.read(reinterpret_cast<char*>(p.sdf.data()), p.sdf.size() * sizeof(uint16_t));
    if (!b) return false;
    g.data = p.sdf.data();
    g.data_on_device = 0;
    return true;
}

void write_vec(FILE* out, const std::vector<double>& v)
{
    for (double x : v) std::fprintf(out, "%.17g\n", x);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) {
        std::cerr << "usage: facade_batch_terms_driver out.txt dir [dir ...]\n";
        return 2;
    }
    std::vector<std::unique_ptr<Problem>> ps;
    for (int i = 2; i < argc; ++i) {
        ps.emplace_back(new Problem());
        if (!load(argv[i], *ps.back())) {
            std::cerr << "cannot read problem " << argv[i] << "\n";
            return 2;
        }
    }
    void* stream = nullptr;
    if (stomp_stream_create(0, &stream) != 0) {
        std::cerr << stomp_last_error() << "\n";
        return 3;
    }
    int rc = 0;
    {
        std::vector<std::unique_ptr<StompOptimizer>> opts;
        std::vector<StompOptimizer*> batch;
        for (auto& p : ps) {
            opts.emplace_back(new StompOptimizer(&p->traj, &p->robot, &p->params, &p->space, p->constraints, 0, stream));
            if (!opts.back()->ok()) {
                std::cerr << opts.back()->lastError() << "\n";
                return 6;
            }
            batch.push_back(opts.back().get());
        }
        if (!StompOptimizer::optimizeBatch(batch)) {
            std::cerr << batch[0]->lastError() << "\n";
            rc = 7;
        } else {
            FILE* out = std::fopen(argv[1], "w");
            if (!out) return 2;
            for (size_t i = 0; i < opts.size(); ++i) {
                const STOMPStatistics& st = opts[i]->getStatistics();
                std::fprintf(out, "%d %d %d %d %d %.17g %.17g %.17g %zu\n", st.iterations, st.success ? 1 : 0,
                             st.success_iteration, st.collision_success_iteration, st.last_improvement_iteration,
                             st.best_cost, st.success_duration, st.collision_success_duration, st.torques.size());
                write_vec(out, st.costs);
                write_vec(out, st.torques);
                for (const auto& row : ps[i]->traj.free) write_vec(out, row);
            }
            std::fclose(out);
        }
    }
    stomp_stream_destroy(stream);
    return rc;
}
