// facade_request_driver.cpp -- StompOptimizer::retargetBatch and retarget with a request's collision
// points and path constraints, between optimize calls: one optimizer per problem on one shared stream
// plans its first problem, the batch is retargeted onto the second problems (their start, goal, seed,
// collision points and orientation constraints; the robot's tree, the field and the parameters
// stay), and plans again; then optimizer 0 alone is put onto its second problem once more with the
// single-optimizer overload and plans a third time.
//
// usage: facade_request_driver <out.txt> <P> <first dir> x P <second dir> x P
// Each directory holds the problem.txt and sdf.bin that tests/facade_util.py writes; a second
// directory also holds constraints.txt: the count and constraint_cost_weight (a parameter: the first
// directories' is the optimizers'), then per constraint the segment, the quaternion, body_fixed, the
// three tolerances and the weight.  The output holds the second plan per optimizer
// and then optimizer 0's third, as facade_batch_driver writes them: one line of statistics, then
// the cost history, the torques and the best trajectory, one value per line.  Exit code 8: an
// optimizer was not in the freshly constructed state after retargetBatch; 9: a refusal that should
// have happened did not, or changed something.
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

bool load_constraints(const std::string& dir, Constraints& c, double* cost_weight)
{
    std::ifstream f(dir + "/constraints.txt");
    int n = -1;
    f >> n >> *cost_weight;
    if (!f || n < 0) return false;
    c.orientation_constraints.resize(n);
    for (auto& o : c.orientation_constraints) {
        f >> o.segment;
        for (double& v : o.orientation) f >> v;
        f >> o.body_fixed >> o.absolute_roll_tolerance >> o.absolute_pitch_tolerance >> o.absolute_yaw_tolerance >>
            o.weight;
    }
    return (bool)f;
}

void write_vec(FILE* out, const std::vector<double>& v)
{
    for (double x : v) std::fprintf(out, "%.17g\n", x);
}

void write_plan(FILE* out, const StompOptimizer& o, const StompTrajectory& traj)
{
    const STOMPStatistics& st = o.getStatistics();
    std::fprintf(out, "%d %d %d %d %d %.17g %.17g %.17g %zu\n", st.iterations, st.success ? 1 : 0,
                 st.success_iteration, st.collision_success_iteration, st.last_improvement_iteration,
                 st.best_cost, st.success_duration, st.collision_success_duration, st.torques.size());
    write_vec(out, st.costs);
    write_vec(out, st.torques);
    for (const auto& row : traj.free) write_vec(out, row);
}

}  // namespace

int main(int argc, char** argv)
{
    const int P = argc >= 3 ? std::atoi(argv[2]) : 0;
    if (P <= 0 || argc != 3 + 2 * P) {
        std::cerr << "usage: facade_request_driver out.txt P dir x P dir x P\n";
        return 2;
    }
    std::vector<std::unique_ptr<Problem>> ps, qs;
    for (int i = 0; i < 2 * P; ++i) {
        auto& list = i < P ? ps : qs;
        list.emplace_back(new Problem());
        Constraints none;
        if (!load(argv[3 + i], *list.back()) ||
            !load_constraints(argv[3 + i], none, &list.back()->params.constraint_cost_weight)) {
            std::cerr << "cannot read problem " << argv[3 + i] << "\n";
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
        std::vector<Constraints> cons(qs.size());
        std::vector<const std::vector<stomp_sphere>*> points;
        std::vector<const Constraints*> constraints;
        for (size_t i = 0; i < qs.size(); ++i) {
            auto& q = qs[i];
            starts.push_back(q->traj.start);
            goals.push_back(q->traj.goal);
            seeds.push_back(q->params.seed);
            double weight = 0.0;
            if (!load_constraints(argv[3 + P + i], cons[i], &weight)) {
                std::cerr << "cannot read the constraints of " << argv[3 + P + i] << "\n";
                return 2;
            }
            points.push_back(&q->robot.collision_points);
            constraints.push_back(&cons[i]);
        }
        if (!StompOptimizer::optimizeBatch(batch)) {
            std::cerr << batch[0]->lastError() << "\n";
            rc = 7;
        }
        if (!rc) {
            // a refused batch changes nothing: a NaN in the last optimizer's goal
            std::vector<std::vector<double>> bad = goals;
            bad.back()[0] = std::nan("");
            const int its = opts[0]->getStatistics().iterations;
            if (StompOptimizer::retargetBatch(batch, starts, bad, seeds, points, constraints) ||
                batch[0]->lastError().empty() ||
                opts[0]->getStatistics().iterations != its || ps[0]->traj.start == starts[0])
                rc = 9;
        }
        if (!rc && !StompOptimizer::retargetBatch(batch, starts, goals, seeds, points, constraints)) {
            std::cerr << batch[0]->lastError() << "\n";
            rc = 7;
        }
        for (size_t i = 0; !rc && i < opts.size(); ++i) {
            const STOMPStatistics& st = opts[i]->getStatistics();
            if (st.iterations != 0 || st.success || !st.costs.empty() || !st.torques.empty() || st.best_cost != 0.0 ||
                opts[i]->lastTrajectoryCost() != 0.0 || opts[i]->lastTrajectoryCollisionFree() ||
                !opts[i]->lastTrajectoryConstraintsSatisfied() || ps[i]->traj.start != starts[i] ||
                ps[i]->traj.goal != goals[i])
                rc = 8;
        }
        if (!rc && !StompOptimizer::optimizeBatch(batch)) {
            std::cerr << batch[0]->lastError() << "\n";
            rc = 7;
        }
        FILE* out = rc ? nullptr : std::fopen(argv[1], "w");
        if (!rc && !out) return 2;
        for (size_t i = 0; !rc && i < opts.size(); ++i) write_plan(out, *opts[i], ps[i]->traj);
        // optimizer 0 alone, the same request again: the single-optimizer overload
        if (!rc && !opts[0]->retarget(starts[0], goals[0], seeds[0], points[0], constraints[0])) {
            std::cerr << opts[0]->lastError() << "\n";
            rc = 7;
        }
        if (!rc && opts[0]->getStatistics().iterations != 0) rc = 8;
        if (!rc && !opts[0]->optimize()) {
            std::cerr << opts[0]->lastError() << "\n";
            rc = 7;
        }
        if (!rc) write_plan(out, *opts[0], ps[0]->traj);
        if (out) std::fclose(out);
    }
    stomp_stream_destroy(stream);
    return rc;
}
