// facade_serve_driver.cpp -- StompOptimizer::serveBatch: one optimizer per slot problem on one
// shared stream, a queue of requests (the start, goal and seed of the request problems) served by
// them as slots.
//
// usage: facade_serve_driver <out.txt> <P> <n> <slot dir> x P <request dir> x n
// Each directory holds the problem.txt and sdf.bin that tests/facade_util.py writes.  The output
// holds, per request, one line "slot start_step" and the statistics, then the cost history and the
// best trajectory, one value per line; then per optimizer what facade_batch_driver writes of a plan:
// one line of statistics, the cost history, the torques and the caller's trajectory.  Exit code 8:
// a result carries torques, or an optimizer that planned nothing was changed; 9: a refusal that
// should have happened did not, or changed something.
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

void write_vec(FILE* out, const std::vector<double>& v)
{
    for (double x : v) std::fprintf(out, "%.17g\n", x);
}

}  // namespace

int main(int argc, char** argv)
{
    const int P = argc >= 4 ? std::atoi(argv[2]) : 0, n = argc >= 4 ? std::atoi(argv[3]) : 0;
    if (P <= 0 || n <= 0 || argc != 4 + P + n) {
        std::cerr << "usage: facade_serve_driver out.txt P n dir x P dir x n\n";
        return 2;
    }
    std::vector<std::unique_ptr<Problem>> ps, qs;
    for (int i = 0; i < P + n; ++i) {
        auto& list = i < P ? ps : qs;
        list.emplace_back(new Problem());
        if (!load(argv[4 + i], *list.back())) {
            std::cerr << "cannot read problem " << argv[4 + i] << "\n";
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
            opts.emplace_back(new StompOptimizer(&p->traj, &p->robot, &p->params, &p->space, Constraints(), 0, stream));
            if (!opts.back()->ok()) {
                std::cerr << opts.back()->lastError() << "\n";
                return 6;
            }
            batch.push_back(opts.back().get());
        }
        std::vector<std::vector<double>> starts, goals;
        std::vector<uint64_t> seeds;
        for (auto& q : qs) {
            starts.push_back(q->traj.start);
            goals.push_back(q->traj.goal);
            seeds.push_back(q->params.seed);
        }
        std::vector<StompOptimizer::ServeResult> results;
        {
            // a refused queue changes nothing: a NaN in the last request's goal, a request too few seeds
            std::vector<std::vector<double>> bad = goals;
            bad.back()[0] = std::nan("");
            const std::vector<double> start0 = ps[0]->traj.start;
            if (StompOptimizer::serveBatch(batch, starts, bad, seeds, results) || batch[0]->lastError().empty() ||
                !results.empty() || opts[0]->getStatistics().iterations != 0 || ps[0]->traj.start != start0)
                rc = 9;
            std::vector<uint64_t> few(seeds.begin(), seeds.end() - 1);
            if (!rc && (StompOptimizer::serveBatch(batch, starts, goals, few, results) || !results.empty())) rc = 9;
        }
        if (!rc && !StompOptimizer::serveBatch(batch, starts, goals, seeds, results)) {
            std::cerr << batch[0]->lastError() << "\n";
            rc = 7;
        }
        if (!rc) {
            std::vector<int> planned(P, 0);
            for (const auto& r : results) {
                if (r.slot < 0 || r.slot >= P || !r.stats.torques.empty()) rc = 8;
                else planned[r.slot] = 1;
            }
            for (int i = 0; !rc && i < P; ++i)
                if (!planned[i] && opts[i]->getStatistics().iterations != 0) rc = 8;
        }
        if (!rc) {
            FILE* out = std::fopen(argv[1], "w");
            if (!out) return 2;
            for (const auto& r : results) {
                const STOMPStatistics& st = r.stats;
                std::fprintf(out, "%d %d %d %d %d %d %d %.17g\n", r.slot, r.start_step, st.iterations, st.success ? 1 : 0,
                             st.success_iteration, st.collision_success_iteration, st.last_improvement_iteration,
                             st.best_cost);
                write_vec(out, st.costs);
                for (const auto& row : r.best_trajectory) write_vec(out, row);
            }
            for (size_t i = 0; i < opts.size(); ++i) {
                const STOMPStatistics& st = opts[i]->getStatistics();
                std::fprintf(out, "%d %d %d %d %d %.17g %.17g %.17g %zu\n", st.iterations, st.success ? 1 : 0,
                             st.success_iteration, st.collision_success_iteration, st.last_improvement_iteration,
                             st.best_cost, st.success_duration, st.collision_success_duration, st.torques.size());
                write_vec(out, st.costs);
                write_vec(out, st.torques);
                write_vec(out, ps[i]->traj.start);
                for (const auto& row : ps[i]->traj.free) write_vec(out, row);
            }
            std::fclose(out);
        }
    }
    stomp_stream_destroy(stream);
    return rc;
}
