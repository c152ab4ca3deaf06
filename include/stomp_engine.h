/*
 * stomp_engine.h -- C ABI of the MI355X STOMP noisy-rollout cost engine.
 *
 * Drop-in boundary for the hot path of kalakris/stomp_motion_planner_icra2011
 * (paths relative to /root/reference/stomp_motion_planner/):
 *
 *   stomp_engine_create      replaces StompOptimizer::StompOptimizer + initialize()
 *                            (stomp_optimizer.cpp:50-202) together with
 *                            PolicyImprovementLoop::initialize (policy_improvement_loop.cpp:88-110),
 *                            PolicyImprovement::initialize (policy_improvement.cpp:64-94) and
 *                            CovariantTrajectoryPolicy::initialize/setToMinControlCost
 *                            (covariant_trajectory_policy.cpp:70-148)
 *   stomp_engine_iterate     replaces PolicyImprovementLoop::runSingleIteration
 *                            (policy_improvement_loop.cpp:143-202)
 *   stomp_engine_run         the same iteration, enqueued `count` times with no host sync
 *   stomp_engine_eval        replaces StompOptimizer::execute (stomp_optimizer.cpp:1063-1165),
 *                            batched over rollouts (Task::execute, task.h:70)
 *   stomp_engine_optimize    replaces StompOptimizer::optimize (stomp_optimizer.cpp:249-401)
 *   stomp_engine_get_theta / set_theta
 *                            replace CovariantTrajectoryPolicy::getParameters/setParameters
 *                            (covariant_trajectory_policy.h:200-227)
 *   stomp_engine_retarget / stomp_engine_retarget_request
 *                            replace the new StompOptimizer the planner node constructs per
 *                            request (stomp_planner_node.cpp:228-230, 421-423) on a live engine:
 *                            start, goal and seed; with a stomp_request also the request's collision
 *                            points and path constraints
 *   stomp_attached_collision_points
 *                            replaces generateAttachedObjectCollisionPoints +
 *                            populatePlanningGroupCollisionPoints (stomp_robot_model.cpp:377-496)
 *   stomp_sdf_build          builds the distance field that
 *                            StompCollisionSpace::setStartState + PropagationDistanceField
 *                            produce (stomp_collision_space.cpp:154-197), for box and
 *                            z-cylinder obstacles, directly in device memory
 *   stomp_sdf_build_objects  the same fill by the reference's own rules: posed boxes and
 *                            cylinders sampled on its lattice, robot bodies, collision-map
 *                            points (stomp_collision_space.cpp:199-297, 564-650)
 *   stomp_scene_*            that field kept in two layers between requests: a static layer built
 *                            once, the robot bodies and sensor points replaced per request over
 *                            the window around their marks (the reference refills the whole
 *                            field in every setStartState)
 *
 * Conventions: plain pointers and sizes only; host buffers are caller-owned and
 * read/written during the call; device buffers are engine-owned.  Trajectories
 * and parameters are row-major [joint][time step] doubles (J x N).  Every call
 * returns 0 on success (the reference's `true`) or a negative STOMP_E_* code;
 * stomp_engine_last_error() / stomp_last_error() give the message.  Calls on one
 * engine must be serialised by the caller (the reference is single-threaded,
 * stomp_planner_node.cpp:547); distinct engines may run concurrently.
 */
#ifndef STOMP_ENGINE_H
#define STOMP_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STOMP_ENGINE_ABI_VERSION 4

#define STOMP_OK 0
#define STOMP_E_INVALID (-1)   /* bad sizes / arguments */
#define STOMP_E_DEVICE (-2)    /* HIP runtime failure */
#define STOMP_E_UNSUPPORTED (-3)
#define STOMP_E_COMM (-4)      /* RCCL failure */

/* One kinematic-tree segment, DFS order (parent < own index).  Frame of the
 * segment tip: frame[s] = frame[parent] * Frame(rot, trans) * Frame(Rot2(axis, q), 0)
 * with q = joint vector[q_index] (q_index = -1: fixed segment).  Replaces the KDL
 * tree of stomp_robot_model.cpp:81-86 as consumed by
 * treefksolverjointposaxis_partial.cpp:108-178. */
typedef struct stomp_segment {
    int32_t parent;
    int32_t q_index;
    double rot[9];
    double trans[3];
    double axis[3];
} stomp_segment;

/* StompCollisionPoint (stomp_collision_point.h:76-82): sphere in a segment frame */
typedef struct stomp_sphere {
    int32_t segment;
    double radius;
    double clearance;
    double pos[3];
} stomp_sphere;

/* StompJoint limits and joint_costs/<name> (stomp_robot_model.h, stomp_optimizer.cpp:107-109) */
typedef struct stomp_joint {
    int32_t has_limits;
    double min;
    double max;
    double joint_cost;
} stomp_joint;

/* Distance field as PropagationDistanceField holds it (third party; read at
 * stomp_collision_space.h:187-191): data[(x*ny + y)*nz + z] = d2, the integer squared cell
 * distance to the nearest obstacle cell, already capped (<= ceil(max_expansion/res)^2); the
 * distance of a cell is sqrt((double)d2) * resolution, in double, as its sqrt_table_.  A
 * position maps to the cell round((p - origin)/resolution); cells with any index < 1 or
 * >= n-1 read distance 0 (distance_field::getDistanceGradient semantics). */
typedef struct stomp_grid {
    int32_t nx, ny, nz;
    double origin[3];
    double resolution;
    const uint16_t* data;       /* host pointer, or device pointer if data_on_device */
    int32_t data_on_device;     /* 1: engine reads the buffer (caller keeps it alive): in place
                                 * for a field of at most 64 MiB; a larger one (e.g. 512^3) is
                                 * copied once at creation into the engine's 4^3-brick layout
                                 * (STOMP_SDF_LAYOUT=brick|linear overrides the size rule), so a
                                 * caller that rebuilds the field in the same buffer (e.g. with
                                 * stomp_sdf_build_objects between plans) calls
                                 * stomp_engine_refresh_field afterwards */
} stomp_grid;

/* KDL::RigidBodyInertia(m, cog, Ic) of a segment, in the segment frame; Ic about the
 * centre of mass as (Ixx, Iyy, Izz, Ixy, Ixz, Iyz).  Replaces the URDF <inertial> data
 * KDL's ChainIdSolver_RNE reads (stomp_robot_model.cpp:185-189). */
typedef struct stomp_inertia {
    double mass;
    double com[3];
    double inertia[6];
} stomp_inertia;

/* motion_planning_msgs::OrientationConstraint as OrientationConstraintEvaluator stores it
 * (constraint_evaluator.cpp:50-73) */
typedef struct stomp_orientation_constraint {
    int32_t segment;            /* frame_number_ = segmentNameToIndex(link_name) */
    double orientation[4];      /* nominal orientation quaternion (x, y, z, w) */
    int32_t body_fixed;         /* 0: type == HEADER_FRAME, 1: body-fixed */
    double absolute_roll_tolerance;
    double absolute_pitch_tolerance;
    double absolute_yaw_tolerance;
    double weight;
} stomp_orientation_constraint;

typedef struct stomp_engine_desc {
    int32_t abi_version;        /* STOMP_ENGINE_ABI_VERSION */
    int32_t num_joints;         /* J (planning group joints) */
    int32_t num_time_steps;     /* N free waypoints (params.yaml num_time_steps), at most 256; the
                                 * lower bound comes from the discretization: the reference's integer
                                 * movement duration int((N + 11) * discretization) must be >= 1
                                 * (N >= 9 at 0.05), else the control cost matrix is not positive
                                 * definite and creation is refused */
    int32_t num_rollouts;       /* K (params.yaml num_rollouts), whole job */
    int32_t num_reused_rollouts;/* K_r (params.yaml num_reused_rollouts) */
    int32_t num_segments;
    const stomp_segment* segments;
    int32_t num_spheres;
    const stomp_sphere* spheres;
    const stomp_joint* joints;  /* J */
    stomp_grid grid;
    double discretization;      /* trajectory_discretization */
    double smoothness_costs[3]; /* smoothness_cost_{velocity,acceleration,jerk} */
    double ridge_factor;
    double smoothness_cost_weight;
    double obstacle_cost_weight;
    double constraint_cost_weight;
    double torque_cost_weight;  /* > 1e-9: torque term (stomp_optimizer.cpp:1117-1142) */
    const double* noise_stddev; /* J */
    const double* noise_decay;  /* J */
    int32_t use_cumulative_costs;
    const double* start;        /* J */
    const double* goal;         /* J */
    uint64_t seed;              /* Philox key of the noise stream */
    int32_t max_iterations;
    int32_t max_iterations_after_collision_free;
    int32_t device;             /* HIP device ordinal */
    void* stream;               /* hipStream_t to launch on; NULL -> engine-owned stream */
    int32_t rank;               /* rollout shard of this process (0 if world_size == 1) */
    int32_t world_size;         /* processes sharing the K rollouts (1 = no collectives) */
    const void* comm_id;        /* 128-byte RCCL unique id from stomp_comm_unique_id (rank 0) */
    /* torque term: inverse dynamics over the chain torque_root (exclusive) -> torque_tip
     * (inclusive), whose joints must be the group's joints in order (the reference's
     * kdl_tree_.getChain("torso_lift_link", "r_gripper_tool_frame"), stomp_robot_model.cpp:185-189) */
    const stomp_inertia* inertias;  /* num_segments; may be NULL while the torque term is off */
    int32_t torque_root;
    int32_t torque_tip;
    double gravity[3];              /* in the torque_root frame (the reference: 0, 0, -9.8) */
    /* orientation path constraints (stomp_optimizer.cpp:195-201, 1107-1115) */
    int32_t num_orientation_constraints;
    const stomp_orientation_constraint* orientation_constraints;
} stomp_engine_desc;

typedef struct stomp_engine stomp_engine;

typedef struct stomp_iter_out {
    double cost;                /* last_trajectory_cost_ of the noiseless rollout */
    int32_t collision_free;     /* last_trajectory_collision_free_ */
    int32_t constraints_satisfied; /* last_trajectory_constraints_satisfied_ */
} stomp_iter_out;

/* STOMPStatistics (msg/STOMPStatistics.msg): the per-iteration costs go to the
 * costs_per_iteration argument of stomp_engine_optimize, the torques to
 * stomp_engine_get_best_torques.  Durations are seconds from the loop's start to the end of
 * the noiseless rollout of (collision_)success_iteration, on the device wall clock
 * (stomp_optimizer.cpp:251, 306-319); 0 when that iteration never came. */
typedef struct stomp_stats {
    int32_t iterations;
    int32_t success;
    int32_t success_iteration;
    int32_t collision_success_iteration;
    int32_t last_improvement_iteration;
    double best_cost;
    double success_duration;
    double collision_success_duration;
} stomp_stats;

int stomp_engine_create(const stomp_engine_desc* desc, stomp_engine** out);
void stomp_engine_destroy(stomp_engine* e);
const char* stomp_engine_last_error(const stomp_engine* e);
const char* stomp_last_error(void);
/* The 16-hex-digit hash of the sources (and compile flags) this library was built from
 * (stomp_motion_planner_icra2011_amd/_build.py source_hash): the Python binding refuses a library
 * whose hash is not the checkout's, and bench.py reports the hash of the library it timed. */
const char* stomp_engine_source_hash(void);

/* Re-reads the caller's device field (data_on_device = 1) after the caller rebuilt it in place:
 * with the engine's bricked copy the copy is remade (ordered on the engine stream after the work
 * already enqueued there; the caller orders its own rebuild before this call); with the field used
 * in place, nothing to do.  A host field (data_on_device = 0) was uploaded at creation:
 * STOMP_E_UNSUPPORTED. */
int stomp_engine_refresh_field(stomp_engine* e);

/* Puts a live engine onto a new planning request: start and goal (J doubles each) and the noise
 * seed (to keep the seed, pass the old one).  Afterwards the engine is observably the engine
 * stomp_engine_create would return for the same descriptor with start, goal and seed replaced (and,
 * after the caller rebuilt its device field in place and called stomp_engine_refresh_field, with
 * that field): theta, last_trajectory and best_trajectory are theta_0 (setToMinControlCost, the
 * bits creation computes), get_pad_positions and the padding-collision flag of iteration_member 0
 * are the new poses', and every later iterate / run / optimize / eval / stomp_pi_* call gives
 * what it gives on the fresh engine, bit for bit.  Whatever iteration state the engine held is
 * dropped: a pending noiseless rollout, rows made ahead, the reuse state (the next iteration
 * generates every rollout) and the step API's state as stomp_pi_reset drops it.  The matrices, the
 * model, the field, the timing accumulators, the stream and group membership are not changed.
 * The device work is one launch on the engine's stream, ordered after everything enqueued before
 * (an earlier refresh_field included), and one read-back of the padding-collision flag: the call
 * waits for the stream.  NULL engine, start or goal, or a value that is not finite:
 * STOMP_E_INVALID, checked before any engine or device is touched (a machine without a GPU can make
 * these calls).  A sharded engine (world_size > 1): STOMP_E_UNSUPPORTED, its ranks would have to
 * retarget in lockstep.  A refused call leaves the engine untouched.
 * stomp_group_retarget (declared with the groups below) does the same for every engine of a group. */
int stomp_engine_retarget(stomp_engine* e, const double* start, const double* goal, uint64_t seed);

/* A whole planning request for a live engine: stomp_engine_retarget's start, goal and seed, and the
 * two things the reference's node also sets per request -- the collision points
 * (generateAttachedObjectCollisionPoints + populatePlanningGroupCollisionPoints after setStartState,
 * stomp_planner_node.cpp:194-199, 386-392: a robot that has grasped something plans with extra
 * spheres on the gripper link; stomp_attached_collision_points below makes the list) and the path
 * constraints (motion_plan_request.path_constraints, handed to every request's StompOptimizer,
 * stomp_planner_node.cpp:229-230, 421-423).
 * Post-condition: the engine is bit for bit the engine stomp_engine_create returns for its
 * descriptor with start, goal, seed, spheres and orientation constraints replaced -- retarget's
 * post-condition extended: theta, last and best trajectory are theta_0; get_pad_positions has
 * 12 x num_spheres x 3 entries of the new list; the padding-collision flag is the new model's; every
 * later iterate / run / optimize / eval / stomp_pi_* / get_best_torques call gives what it gives on
 * the fresh engine.  Iteration state is dropped exactly as retarget drops it.  Kept: the matrices,
 * the segments, the joints, the torque chain, the field and its bricked copy, the timers, the stream.
 * With both counts -1 the call is stomp_engine_retarget.
 * The call plans the new model on the host (the FK program, the rollout kernel's layout for it --
 * the layout a fresh engine of this process would get, environment overrides included -- and the
 * terms model), then commits: one upload of one pinned staging block, one launch and one read-back
 * of the flag on the engine's stream, after everything enqueued before (iterations still in flight
 * read the old model); it waits for the stream.  Device memory that depends on the model is held
 * with a capacity and reallocated only when a request needs more than every earlier one; a
 * repeated request allocates nothing (stomp_engine_model_info, info[11]).
 * Refusals leave the engine as it was, with creation's own messages where creation has one; a
 * refusal writes nothing of the engine, not even its last-error text (stomp_last_error() has the
 * message).  The NULL and struct_size refusals come before the engine is read (a machine without a
 * GPU can make these calls); the others are made while the model is planned on the host, which reads
 * the engine and asks the engine's device for the rollout kernels' attributes, and enqueues nothing.
 * The "inside its optimize loop" refusal may be made from another host thread than the one running
 * stomp_engine_optimize (it reads an atomic flag); every other use of one engine from two threads
 * stays the caller's to serialise.  A STOMP_E_DEVICE failure during the commit (an allocation, the
 * copy, the launch, the wait) frees what the call allocated and leaves every engine's host side as
 * it was; what the device holds is then as after any device failure.
 * STOMP_E_INVALID: NULL engine, request, start or goal; a struct_size other than
 * sizeof(stomp_request); a count below -1, or >= 1 without its array; a value that is not finite;
 * a sphere or constraint segment outside the tree; a radius or clearance creation would refuse; an
 * engine inside its optimize loop.  STOMP_E_UNSUPPORTED: a sphere list not ordered by segment; a
 * tree that then needs more saved frames than the FK program has; a rollout or state-terms kernel
 * over its LDS limit; more than 65535 pair ids; a constraint segment deeper than the terms kernel's
 * path; a sharded engine. */
typedef struct stomp_request {
    int32_t struct_size;                 /* sizeof(stomp_request) */
    const double* start;                 /* J */
    const double* goal;                  /* J */
    uint64_t seed;
    int32_t num_spheres;                 /* -1: keep the engine's collision points */
    const stomp_sphere* spheres;         /* ordered by segment, as at creation */
    int32_t num_orientation_constraints; /* -1: keep the engine's path constraints; 0: none */
    const stomp_orientation_constraint* orientation_constraints;
} stomp_request;
int stomp_engine_retarget_request(stomp_engine* e, const stomp_request* r);
/* What the engine's current model is, for tests and tables: info[0] spheres S, [1] FK program
 * steps, [2] published frame slots, [3] saved branch-point frames, [4] most spheres of one run,
 * [5] padding positions in LDS, [6] the LDS-lean layout (0, 1, 2), [7] the sincos pre-pass,
 * [8] orientation constraints, [9] state-cost terms on, [10] model changes so far (retarget-request
 * calls that replaced the collision points or the constraints), [11] device or pinned allocations
 * made inside retarget calls of either kind so far (a call's staging included; a repeated call
 * allocates nothing).  Host only. */
int stomp_engine_model_info(stomp_engine* e, int64_t info[12]);

/* The state query: per-sphere clearance and per-link costs of a batch of M joint states -- what a
 * node asks before and after every plan (is this state in collision, which link, by how much).  The
 * reference declares the capability and never built it: srv/GetStateCost.srv (link names and a robot
 * state in, per-link costs out) and srv/GetChompCollisionCost.srv (per-link costs and in_collision).
 * For sphere s of state m (S spheres, the engine's current collision points, in their order):
 *   positions        the sphere centre, the planner's own forward kinematics of the state;
 *   distances        the field distance at the centre, sqrt(d2) * resolution, metres; a centre whose
 *                    cell is outside the valid cells [1, n - 2] reads 0, as in the planner's lookup;
 *   potentials       the collision potential (stomp_collision_space.h:193-228) of that distance;
 *   sphere_collides  distance <= radius (the planner's collision test).
 * Per state, every sum sequential in ascending sphere index from 0.0:
 *   state_cost       the sum of the potentials;
 *   link_costs       [l]: the sum over the spheres on segment links[l] (0.0 for a segment without
 *                    spheres; a segment may be listed more than once);
 *   min_clearance    the least distance - radius, and min_sphere the first sphere that attains it
 *                    (with no spheres: +infinity and -1);
 *   in_collision     some sphere collides;
 *   limits_violated  some joint with limits is outside [min, max].  The state is never clipped: this
 *                    is a query, not handleJointLimits.
 * There is no velocity factor (a robot standing still has a cost here, unlike stomp_engine_eval's
 * waypoint costs) and no gradient: getDistanceGradient's gradient belongs to the third-party
 * distance_field package, which the reference tree does not hold, and only the CHOMP path reads it.
 * (Since CHOMP mode that gradient has a stated definition here, and stomp_engine_query_gradients
 * below answers with it; this call stays as it is.)
 * An output pointer that is NULL is not computed.
 * Model and field: the model the engine holds now (after a retarget request with other collision
 * points S is the new S, stomp_engine_model_info info[0]) and the field it reads now (after
 * stomp_engine_refresh_field or a scene update; the bricked copy where the engine has one).
 * The work is enqueued on the engine's stream behind everything already there, and the call waits
 * for it.  The arrays are the caller's, in host memory.  The staging, device and pinned, is the
 * engine's and held with a capacity: a repeated call of the same size allocates nothing.  A large M
 * goes through in chunks of at most 48 MiB of device staging; STOMP_DEBUG_QUERY_CHUNK (read per call)
 * sets the states per chunk instead; the results do not depend on the chunks.
 * Nothing else of the engine changes: theta, the rollout rows, the reuse state, a pending noiseless
 * rollout (not flushed), rows made ahead, the step API's state, the timers, the model-change counter
 * and group membership are as before, and a group's next call is unaffected.  A sharded engine
 * (world_size > 1) may be asked: every rank holds the whole model and field, no collective runs.
 * STOMP_E_INVALID, before any device is touched and with no output written: NULL engine, query or
 * states; a struct_size other than sizeof(stomp_state_query); num_states < 1; num_links < 0, or
 * >= 1 without links; link_costs with num_links 0; a link outside the tree; a state value that is
 * not finite; an engine inside its optimize loop (read from the loop's atomic flag, so another host
 * thread may ask).  The NULL and struct_size refusals come before the engine is read (a machine
 * without a GPU can make these calls).  A refusal writes nothing of the engine; stomp_last_error()
 * has the message. */
typedef struct stomp_state_query {
    int32_t struct_size;            /* sizeof(stomp_state_query) */
    int32_t num_states;             /* M >= 1 */
    const double* states;           /* [M][J] */
    int32_t num_links;              /* L >= 0 */
    const int32_t* links;           /* [L] segment indices (GetStateCost.srv link_names) */
    /* outputs; each may be NULL (not computed) */
    double*  positions;             /* [M][S][3] */
    double*  distances;             /* [M][S] field distance at the sphere centre, metres */
    double*  potentials;            /* [M][S] */
    uint8_t* sphere_collides;       /* [M][S] */
    double*  link_costs;            /* [M][L] */
    double*  state_cost;            /* [M] */
    double*  min_clearance;         /* [M] */
    int32_t* min_sphere;            /* [M] */
    uint8_t* in_collision;          /* [M] */
    uint8_t* limits_violated;       /* [M] */
} stomp_state_query;
int stomp_engine_query_states(stomp_engine* e, const stomp_state_query* q);
/* The last query call, for tests and tables: info[0] its chunks, [1] its kernel launches (the query
 * and the transposes of its per-sphere outputs), [2] device or pinned allocations made inside query
 * calls so far, [3] its states per chunk.  Host only. */
int stomp_engine_query_info(stomp_engine* e, int64_t info[4]);
/* Device time of the last query call's launches, milliseconds (events around each chunk's launches,
 * summed; the copies are outside).  Host only. */
int stomp_engine_query_time(stomp_engine* e, double* kernel_ms);

/* The gradient query: srv/GetChompCollisionCost.srv whole -- per link the cost and "the joint velocity
 * that will move the link away from collisions" (msg/JointVelocityArray.msg), and in_collision -- for a
 * batch of M joint states against the engine's current model and field.  Every sum is sequential from
 * 0.0 in the stated order, everything fp64 with one rounding per operation (tests/CHOMP.md's rules).
 * For state m and sphere s (the engine's current collision points, in their order):
 *   the centre p is stomp_engine_query_states' positions;
 *   (dist, fg) is the field gradient of the CHOMP section below: the nearest-cell rule, then the
 *     central differences of sqrt(d2) * resolution over the six neighbours times 1 / (2 resolution); a
 *     cell outside [1, n - 2] on any axis reads distance 0 and gradient (0, 0, 0);
 *   fgb = fg + field_bias per component (StompCollisionSpace::field_bias_*, CHOMP's parameter);
 *   the potential and its gradient pg are stomp_collision_space.h:206-227 with d = dist - radius:
 *     d >= clearance: 0 and (0, 0, 0); 0 <= d < clearance: diff = d - clearance, gm = diff *
 *     inv_clearance, 0.5 * gm * diff and gm * fgb; d < 0: -d + 0.5 * clearance and fgb.  The sphere
 *     collides when dist <= radius.  The bias does not enter the potential;
 *   the Jacobian column of joint k is axis x (p - origin) with the joint's world-frame origin and axis
 *     (CHOMP section; tests/CHOMP.md "Joint origin and axis", "Jacobian column") for a joint on the path
 *     from the root to the sphere's segment, three zeros otherwise (a joint that drives no segment
 *     included);
 *   the sphere's joint term is t_k = 0; t_k += J(r, k) * pg_r for r = 0, 1, 2.
 * Outputs:
 *   field_gradients      fg, before the bias;       potential_gradients  pg;
 *   link_gradients       [l][k]: a = 0; a -= t_k(s) over the spheres on segment links[l] in ascending
 *                        s (0.0 for a segment without spheres; a segment may be listed more than once).
 *                        The sign is CHOMP's collision_increments -= J^T g: a joint velocity that
 *                        lowers the potential;
 *   state_gradient       [k]: the same fold over all spheres;
 *   link_costs, state_cost, in_collision   stomp_engine_query_states' values, with the same bits.
 * Every sphere takes part in the folds: the descent's skip of a sphere with potential <= 1e-10 and its
 * break after the first colliding sphere (stomp_optimizer.cpp:430-431, :451-460) are rules of CHOMP's
 * fold, not of this service.  States are never clipped.  An output pointer that is NULL is not computed.
 * The sign inside an obstacle: in the clearance band (0 <= d < clearance) gm < 0 turns the field
 * gradient round and the velocity leads away from the obstacle; for d < 0 the reference takes the field
 * gradient as it is (stomp_collision_space.h:222-226) although the potential there falls along it, so
 * the velocity leads further in.  The call keeps the reference's sign, as CHOMP mode does; a caller
 * that wants the way out of a penetration negates the gradient of a link whose spheres penetrate.
 * Around the call everything is as stomp_engine_query_states: the engine's current model and field
 * (the bricked copy where there is one), the engine's stream and a wait, host arrays, the same staging
 * held with a capacity (a repeated call of the same size allocates nothing), the same 48 MiB chunks and
 * STOMP_DEBUG_QUERY_CHUNK; stomp_engine_query_info / _time report the last query call of either kind
 * (one launch per chunk here: the outputs leave the kernel in the caller's shape).  Nothing else of
 * the engine changes, and a sharded engine may be asked.
 * STOMP_E_INVALID, before any device is touched and with no output written: the refusals of
 * stomp_engine_query_states (link_gradients without links as link_costs) and a field_bias that is not
 * finite; the NULL and struct_size refusals come before the engine is read.  STOMP_E_UNSUPPORTED: a
 * field with fewer than 3 cells on an axis (as CHOMP mode), a model whose frames and terms need more
 * than 64 KiB of LDS. */
typedef struct stomp_gradient_query {
    int32_t struct_size;            /* sizeof(stomp_gradient_query) */
    int32_t num_states;             /* M >= 1 */
    const double* states;           /* [M][J] */
    int32_t num_links;              /* L >= 0 */
    const int32_t* links;           /* [L] segment indices */
    double field_bias[3];           /* 0 */
    /* outputs; each may be NULL (not computed) */
    double*  field_gradients;       /* [M][S][3] */
    double*  potential_gradients;   /* [M][S][3] */
    double*  link_costs;            /* [M][L] */
    double*  link_gradients;        /* [M][L][J] */
    double*  state_cost;            /* [M] */
    double*  state_gradient;        /* [M][J] */
    uint8_t* in_collision;          /* [M] */
} stomp_gradient_query;
int stomp_engine_query_gradients(stomp_engine* e, const stomp_gradient_query* q);

int stomp_engine_get_theta(stomp_engine* e, double* theta);
int stomp_engine_set_theta(stomp_engine* e, const double* theta);

int stomp_engine_iterate(stomp_engine* e, int32_t iteration_number, stomp_iter_out* out);
/* run: count iterations enqueued with no host sync.  The last one's noiseless rollout is left
 * pending (it rides in the next rollout launch); synchronize, iterate, set_theta and the
 * trajectory reads evaluate it first. */
int stomp_engine_run(stomp_engine* e, int32_t first_iteration, int32_t count);
/* synchronize, and every other call that waits for the engine's stream: with an RCCL communicator
 * (world_size > 1) the wait is bounded.  An RCCL error, or no completion within
 * STOMP_COMM_TIMEOUT_S seconds (default 300), aborts the communicator (ncclCommAbort) and returns
 * STOMP_E_COMM with a message naming the first collective not complete and the last one posted
 * (kind, iteration and ordinal of each); every later call on the engine returns the same. */
int stomp_engine_synchronize(stomp_engine* e);

/* Batched Task::execute: params E x J x N, costs E x N, collision_free E,
 * traj_out E x J x N (joint-limit-corrected free block, may be NULL).
 * iteration_member is StompOptimizer::iteration_ (0: padding points count for the flag).
 * constraints_satisfied E (last_trajectory_constraints_satisfied_, may be NULL). */
int stomp_engine_eval(stomp_engine* e, const double* params, int32_t num, double* costs,
                      uint8_t* collision_free, double* traj_out, int32_t iteration_member,
                      uint8_t* constraints_satisfied);

int stomp_engine_optimize(stomp_engine* e, stomp_stats* stats, double* costs_per_iteration);
/* STOMPStatistics.torques after optimize (stomp_optimizer.cpp:384-398): per free waypoint,
 * sum_j |tau_j| of the best trajectory by inverse dynamics over the torque chain (N doubles).
 * Needs the segment inertias in the descriptor (also with the torque term off);
 * STOMP_E_UNSUPPORTED without them, and with the term off also when the chain's kernel needs more
 * than 160 KiB of LDS (the message says which of the two). */
int stomp_engine_get_best_torques(stomp_engine* e, double* torques);

/* PolicyImprovement (policy_improvement.h:86-126) step by step, for a caller that executes the
 * rollouts with its own Task between the steps (single rank):
 *   get_rollouts        generateRollouts(noise_stddev) + computeProjectedNoise (:158-260): reuse
 *                       ranking, new noise for the generated rows keyed by `iteration` (the
 *                       Philox stream of runSingleIteration(iteration)); the K_gen generated
 *                       parameter sets (K_gen x J x N) and K_gen out
 *   set_rollout_costs   setRolloutCosts (:262-281): state costs of the generated rows (K x N,
 *                       rows >= K_gen ignored), control costs of all K with 0.5 * weight,
 *                       Rollout::getCost of every row (K) out
 *   improve_policy      improvePolicy (:385-401): probabilities and the update M (sum eps P)
 *                       (J x N; row 0 of the reference's per-joint update matrices), theta untouched
 *   add_extra_rollouts  addExtraRollouts (:443-462) of num = 1 rollout: parameters J x N and its
 *                       state costs N; noise against the current theta
 *   reset               setNumRollouts (:96-147) with the engine's own counts: the reuse state
 *                       starts over (the next iteration generates every rollout, a pending extra
 *                       rollout is dropped from the next ranking)
 * Applying the update is Policy::updateParameters: stomp_engine_get_theta / set_theta. */
int stomp_pi_get_rollouts(stomp_engine* e, int32_t iteration, const double* noise_stddev, double* rollouts,
                          int32_t* num_generated);
int stomp_pi_set_rollout_costs(stomp_engine* e, const double* costs, double control_cost_weight, double* totals);
int stomp_pi_improve_policy(stomp_engine* e, double* updates);
int stomp_pi_add_extra_rollouts(stomp_engine* e, int32_t num, const double* params, const double* costs);
int stomp_pi_reset(stomp_engine* e);
int stomp_engine_get_best_trajectory(stomp_engine* e, double* traj);
int stomp_engine_get_last_trajectory(stomp_engine* e, double* traj);

/* Inspection for parity tests.  which: "params","noise","control_costs","probabilities"
 * -> K_local x J x N; "state_costs" -> K_local x N; the extra (noiseless) rollout of
 * addExtraRollouts (policy_improvement.cpp:443-462): "x_params","x_noise","x_control_costs"
 * -> J x N (kept with K_r > 0 only), "x_state_costs" -> N; "cumulative_costs" -> K_local x J x N,
 * the rows the last weights launch read (computeRolloutCumulativeCosts, policy_improvement.cpp:
 * 301-320), STOMP_E_INVALID on an engine created without use_cumulative_costs. */
int stomp_engine_get_rollouts(stomp_engine* e, const char* which, double* out);
/* which: "Rinv","L","M","Qinv" (N x N, joint selects Qinv), "R" (free block of the
 * control-cost matrix, CovariantTrajectoryPolicy::getControlCosts,
 * covariant_trajectory_policy.h:235-239), "D0","D1","D2" (the policy's differentiation
 * matrices, (N+12) x (N+12), covariant_trajectory_policy.cpp:204-226).  Host only. */
int stomp_engine_get_matrix(stomp_engine* e, const char* which, int32_t joint, double* out);
/* sphere world positions at the 12 padding points (12 x S x 3) */
int stomp_engine_get_pad_positions(stomp_engine* e, double* out);

/* Per-kernel device time (HIP events on the engine stream), accumulated while enabled.
 * name: "noise", "rollout_cost", "weights", "update", "noiseless", "all". */
int stomp_engine_set_timing(stomp_engine* e, int32_t enable);
int stomp_engine_get_timing(stomp_engine* e, const char* name, double* total_ms, int32_t* launches);
int stomp_engine_local_rollouts(stomp_engine* e, int32_t* first, int32_t* count);
/* The K-sharded decomposition the engine chose: STOMP_SHARD_NONE (one rank),
 * STOMP_SHARD_PARTIALS (all-reduce + two all-gathers of 64-rollout block partials per iteration) or
 * STOMP_SHARD_GATHER (one all-gather of the state-cost rows; every rank weights all K). */
#define STOMP_SHARD_NONE 0
#define STOMP_SHARD_PARTIALS 1
#define STOMP_SHARD_GATHER 2
int stomp_engine_shard_mode(stomp_engine* e, int32_t* mode);
/* How the decomposition was chosen.  info[0] = the mode; when both were possible and none was
 * requested (STOMP_SHARD_MODE unset, world > 1) the engine measured at creation, maxima over the
 * ranks, in microseconds: info[1] = one iteration's compute in gather mode, info[2] = in partials mode
 * (no exchanges), info[3] = the all-reduce(max) of 2 J N doubles, info[4] = the all-gather of the
 * state-cost rows, info[5] = the all-gather of the block partials; zeros otherwise. */
int stomp_engine_shard_info(stomp_engine* e, double* info);
/* The rule applied to those measurements (host only): gather when info[1] + info[4] <=
 * info[2] + info[3] + 2 info[5] (one all-gather against three dependent collectives).
 * measured = info + 1. */
int stomp_shard_decide(const double* measured, int32_t* mode);

/* Distance-field builder (capped exact EDT, stomp_grid's representation):
 *   value = min(d2, ceil(max_expansion/res)^2)   (the cap must be <= 255 cells)
 * d2 = integer squared cell distance to the nearest cell whose centre
 * origin + i*res lies in an obstacle.  boxes: n_boxes x (cx,cy,cz,dx,dy,dz),
 * axis-aligned; cylinders: n_cyl x (cx,cy,cz,radius,length), z-aligned.
 * out_device: device buffer of nx*ny*nz uint16 (z fastest). */
int stomp_sdf_build(int32_t nx, int32_t ny, int32_t nz, const double* origin, double resolution,
                    double max_expansion, const double* boxes, int32_t n_boxes, const double* cylinders,
                    int32_t n_cylinders, uint16_t* out_device, void* stream);

/* An object of the collision space.  Environment objects are sampled as
 * StompCollisionSpace::addCollisionObjectsToPoints does (stomp_collision_space.cpp:199-297):
 *   STOMP_SHAPE_BOX       dims = (dx, dy, dz)
 *   STOMP_SHAPE_CYLINDER  dims = (radius, length, -), axis = the pose's z
 * on the running-sum lattice xlow, xlow + res, ... (x <= xlow + dim + res), each point p
 * mapped through Frame(Rotation::Quaternion(orientation), position) as position - p.
 * Robot bodies (getVoxelsInBody, :592-650; the links addAllBodiesButExcludeLinksToPoints keeps,
 * :564-590, with the caller's padding/scale folded into dims):
 *   STOMP_BODY_SPHERE     dims = (radius, -, -)
 *   STOMP_BODY_BOX        dims = (dx, dy, dz)
 *   STOMP_BODY_CYLINDER   dims = (radius, length, -)
 *   STOMP_BODY_MESH       vertices (num_vertices x 3, the body frame, scale applied), dims =
 *                         (padding, -, -): a robot link's mesh or an environment object of type
 *                         MESH (:216-223 take it through getVoxelsInBody too), as
 *                         bodies::ConvexMesh: the convex hull of the vertices
 * on the lattice position + g * res around the bounding sphere (a mesh's: around its vertices'
 * bounding-box centre), kept where the body contains the point (the reference's ray-crossing
 * parity for these convex bodies). */
#define STOMP_SHAPE_BOX 0
#define STOMP_SHAPE_CYLINDER 1
#define STOMP_BODY_SPHERE 2
#define STOMP_BODY_BOX 3
#define STOMP_BODY_CYLINDER 4
#define STOMP_BODY_MESH 5
typedef struct stomp_shape {
    int32_t type;
    double position[3];
    double orientation[4];      /* quaternion (x, y, z, w), geometry_msgs::Pose order */
    double dims[3];
    const double* vertices;     /* STOMP_BODY_MESH only (host memory), else NULL */
    int32_t num_vertices;
} stomp_shape;

/* The reference's distance-field fill (StompCollisionSpace::setStartState,
 * stomp_collision_space.cpp:154-197) on the device: every object's points and the
 * collision-map points (points: n_points x 3, the "points" namespace, :205-211) mark the cell
 * round((p - origin) * (1/res)) when it lies in the grid (PropagationDistanceField::
 * addPointsToField); value = min(d2, cap^2) with cap = ceil(max_expansion/res) (<= 255) and
 * d2 the integer squared cell distance to the nearest marked cell (stomp_grid's
 * representation).  marked (may be NULL): points that landed inside the grid. */
int stomp_sdf_build_objects(int32_t nx, int32_t ny, int32_t nz, const double* origin, double resolution,
                            double max_expansion, const stomp_shape* shapes, int32_t n_shapes,
                            const double* points, int64_t n_points, uint16_t* out_device, int64_t* marked,
                            void* stream);

/* The collision points of a robot holding attached bodies (generateAttachedObjectCollisionPoints +
 * populatePlanningGroupCollisionPoints, stomp_robot_model.cpp:377-496), host only, no device.  An
 * attached body is a STOMP_BODY_* shape posed in the frame of its owner segment (padding folded
 * into dims, as for robot bodies); it becomes one sphere at its bounding sphere's centre, with that
 * radius (bodies::*::computeBoundingSphere, the rule the robot bodies' lattices use) and the given
 * clearance (collision_clearance_default_).  Each new sphere is placed after the base list's last
 * sphere of a segment <= its own, bodies of one segment in input order, so the output is ordered by
 * segment whenever the base list is.  out: capacity entries; *n_out: n_base + n_bodies.  A
 * capacity that is too small: STOMP_E_INVALID with *n_out set to the size needed and out untouched.
 * NULL out, n_out or a count without its array, a negative count, a shape that is no STOMP_BODY_*,
 * a mesh without four vertices, a clearance that is not positive and finite: STOMP_E_INVALID. */
typedef struct stomp_attached_body {
    int32_t segment;
    stomp_shape shape;
} stomp_attached_body;
int stomp_attached_collision_points(const stomp_sphere* base, int32_t n_base, const stomp_attached_body* bodies,
                                    int32_t n_bodies, double clearance, stomp_sphere* out, int32_t capacity,
                                    int32_t* n_out);

/* Scene layers: the field of stomp_sdf_build_objects kept in two layers over the caller's device
 * buffer field_device (nx*ny*nz uint16, stomp_grid's layout and representation), for a caller
 * whose scene is mostly the same from request to request.  The field is a capped squared
 * distance, so for two sets of marks min(d2(A u B), cap^2) = min(min(d2(A), cap^2),
 * min(d2(B), cap^2)) holds exactly: the static layer (A) is built once and kept, and a request's
 * dynamic set (B: the robot's own bodies at the start state, the collision-map points) costs a
 * transform over the bounding window of its marks grown by cap cells and a min merge there.
 *   stomp_scene_create       records the grid and the buffer; touches no device.  stream NULL: a
 *                            stream the scene owns, made with the first stomp_scene_set_static.
 *   stomp_scene_set_static   the static layer from its objects and points, by the rules of
 *                            stomp_sdf_build_objects; written to field_device, any dynamic set
 *                            dropped: the field is then stomp_sdf_build_objects of these inputs.
 *   stomp_scene_set_dynamic  replaces the dynamic set (it does not add to it): the field is then bit
 *                            for bit what stomp_sdf_build_objects writes for the static objects and
 *                            points followed by these; cells of the previous dynamic window the new
 *                            one does not cover are back at the static layer's value; an empty set
 *                            gives the static field.  Before any set_static: STOMP_E_INVALID.  The
 *                            marking, the three passes, the merge and the restore run over the
 *                            window only (one window per call around all dynamic inputs: a dynamic
 *                            set scattered over the grid degenerates to the whole grid).
 * All work goes on the scene's stream, after everything enqueued there before.  With marked NULL a
 * set_* call does not wait for the device: the host inputs are copied into pinned staging of the
 * scene before it returns.  With marked non-NULL it waits and returns the points that landed
 * inside the grid, counted as stomp_sdf_build_objects counts (the static and the dynamic count add
 * up to the full build's).  A call allocates only when its window or its input lists are larger
 * than every earlier one (geometric growth); set_static's window is the grid.
 *   stomp_scene_window       host only, no device: the window set_dynamic would use, inclusive cell
 *                            bounds; empty (lo[0] > hi[0]) when nothing can land in the grid.
 *   stomp_scene_info         waits for the stream.  info[0..2], info[3..5]: the last call's window
 *                            (lo, hi); [6] its cells; [7] cells restored from the static layer in
 *                            the last call; [8] dynamic marks so far that landed inside the grid but
 *                            outside the window (a check on the bound: always 0); [9] allocations
 *                            made inside set_dynamic so far.
 * Errors, all checked before any device is touched (a machine without a GPU can make these calls)
 * and leaving the scene and the field untouched: NULL scene, field, origin or out, sizes <= 0, a
 * resolution that is not positive, negative counts, a count without its array, an unknown shape
 * type, a degenerate mesh, a lattice too large: STOMP_E_INVALID; ceil(max_expansion / resolution)
 * > 255: STOMP_E_UNSUPPORTED.  stomp_last_error() has the message.  Calls on one scene are
 * serialised by the caller.  Engines reading field_device in place: the ordering contract is
 * stomp_engine_refresh_field's (simplest: the scene on the engines' stream); engines with a bricked
 * copy call stomp_engine_refresh_field after a set_* call, as after any in-place rebuild. */
typedef struct stomp_scene stomp_scene;
int stomp_scene_create(int32_t device, int32_t nx, int32_t ny, int32_t nz, const double* origin,
                       double resolution, double max_expansion, uint16_t* field_device, void* stream,
                       stomp_scene** out);
int stomp_scene_set_static(stomp_scene* s, const stomp_shape* shapes, int32_t n_shapes, const double* points,
                           int64_t n_points, int64_t* marked);
int stomp_scene_set_dynamic(stomp_scene* s, const stomp_shape* shapes, int32_t n_shapes, const double* points,
                            int64_t n_points, int64_t* marked);
int stomp_scene_window(int32_t nx, int32_t ny, int32_t nz, const double* origin, double resolution,
                       double max_expansion, const stomp_shape* shapes, int32_t n_shapes, const double* points,
                       int64_t n_points, int32_t lo[3], int32_t hi[3]);
int stomp_scene_info(stomp_scene* s, int64_t info[10]);
void stomp_scene_destroy(stomp_scene* s);

/* The differentiation stencils the engine is built on (DIFF_RULES of stomp_utils.h:49-56:
 * velocity, acceleration, jerk; 3 x 7 doubles, row-major).  Host only, no device needed. */
int stomp_diff_rules(double* out);

/* Groups: several engines of one shape (same J, N, K, K_r, spheres and model layout; single
 * device, at most 16 joints, no state-cost terms, no cumulative costs), created on ONE shared
 * stream, advanced in lockstep by shared launches -- one rollout, one weights and one update launch
 * per iteration for the whole group instead of three per engine (a batch of independent planning
 * problems, BASELINE cfg5).  With reused rollouts (K_r > 0, the same for every engine; engines of
 * different K_r are STOMP_E_INVALID) the iterations that reuse add one launch for the reused rows
 * of every engine; such a group takes K <= 1023 rollouts and shapes whose reused row fits the
 * reuse kernel's LDS (otherwise STOMP_E_UNSUPPORTED).  Each engine ends in exactly the state its
 * own stomp_engine_run(first, count) leaves: its θ, rollouts (both row sets, the extra rollout's
 * rows) and pending noiseless rollout; the engines' own calls keep working between group runs.
 * The engines enter a run at one iteration state (STOMP_E_INVALID with no engine touched
 * otherwise).  stomp_group_synchronize flushes every engine's pending noiseless rollout and
 * waits.
 * stomp_group_create_with takes options; stomp_group_create(e, n, out) is exactly
 * stomp_group_create_with(e, n, {state_terms 0, compact -1}, out).  With state_terms = 1 the group
 * also accepts engines with state-cost terms (the torque term, torque_cost_weight > 1e-9, and / or
 * orientation path constraints), at K_r = 0 and K_r > 0.  Such a group may be mixed: the engines
 * share J, N, K, K_r, the spheres and the rollout layout as above, and each keeps its own terms
 * model -- the torque term only, constraints only, both, or neither (for an engine with neither
 * nothing changes: no terms launch writes any of its rows).  Every grouped rollout launch and every
 * grouped noiseless flush is then followed by one more launch, the state-cost terms of all its
 * engines, before anything reads the state costs, the noiseless rollout's total or its
 * constraints-satisfied flag; stomp_group_run, stomp_group_synchronize and stomp_group_optimize
 * keep their post-conditions (each engine bit for bit where its own calls leave it, the optimize
 * loop's stop rule counting only iterations whose noiseless trajectory satisfies the constraints).
 * Cumulative costs, more than 16 joints, sharded engines and the other conditions above stay
 * STOMP_E_UNSUPPORTED with state_terms = 1; a refused creation leaves every engine untouched.
 * compact: -1 leaves the choice to STOMP_DEBUG_GROUP_COMPACT as in stomp_group_create, 0 / 1
 * turn the compaction of stomp_group_optimize off / on.  NULL options or a struct_size other than
 * sizeof(stomp_group_options): STOMP_E_INVALID.
 * stomp_group_create_flags takes plain arguments: accept, a mask of STOMP_GROUP_ACCEPT_*, and
 * compact as above (-1 / 0 / 1).  stomp_group_create_with(e, n, {state_terms s, compact c}, out) is
 * exactly stomp_group_create_flags(e, n, s ? STOMP_GROUP_ACCEPT_STATE_TERMS : 0, c, out).  With
 * STOMP_GROUP_ACCEPT_CUMULATIVE the group also accepts engines with use_cumulative_costs (the
 * reference's default), mixed freely with engines without, at K_r = 0 and K_r > 0, with or
 * without state-cost terms (both bits): every grouped weights launch of stomp_group_run and
 * stomp_group_optimize is then preceded by one more launch, the cumulative rows of all its
 * engines (computeRolloutCumulativeCosts' suffix sums, policy_improvement.cpp:308-316; an engine
 * without cumulative costs has no workgroup that writes), after the state-cost terms and the
 * reused rows' launch; the post-conditions stay the ones above, the rows of
 * stomp_engine_get_rollouts("cumulative_costs") included.  Such a group takes N <= 256; every
 * other condition is unchanged.  Unknown bits in accept, a compact outside -1 / 0 / 1, NULL
 * engines or out, num_engines <= 0: STOMP_E_INVALID, checked before any engine or device is
 * touched (a machine without a GPU can make these calls). */
#define STOMP_GROUP_ACCEPT_STATE_TERMS 1u
#define STOMP_GROUP_ACCEPT_CUMULATIVE 2u
typedef struct stomp_group stomp_group;
typedef struct stomp_group_options {
    int32_t struct_size;   /* sizeof(stomp_group_options) */
    int32_t state_terms;   /* 1: engines with the torque term and / or path constraints are accepted */
    int32_t compact;       /* -1: STOMP_DEBUG_GROUP_COMPACT decides, as in stomp_group_create; 0 / 1: off / on */
} stomp_group_options;
int stomp_stream_create(int32_t device, void** out_stream);
int stomp_stream_destroy(void* stream);
int stomp_group_create(stomp_engine* const* engines, int32_t num_engines, stomp_group** out);
int stomp_group_create_with(stomp_engine* const* engines, int32_t num_engines,
                            const stomp_group_options* options, stomp_group** out);
int stomp_group_create_flags(stomp_engine* const* engines, int32_t num_engines, uint32_t accept, int32_t compact,
                             stomp_group** out);
int stomp_group_run(stomp_group* g, int32_t first_iteration, int32_t count);
int stomp_group_synchronize(stomp_group* g);
/* StompOptimizer::optimize (stomp_optimizer.cpp:249-401) for every engine of the group at once.
   stats: [P]; costs_per_iteration: NULL or [P][costs_stride], row p holding engine p's
   last_trajectory_cost_ per iteration; costs_stride >= every engine's max_iterations.
   The engines run in lockstep through the grouped launches; the loop's bookkeeping is one more
   launch per iteration for the whole group, and each engine stops on its own (its collision-free
   streak reaching its max_iterations_after_collision_free, or its own max_iterations).  The host
   reads every engine's stop flag once per chunk of STOMP_GROUP_OPTIMIZE_CHUNK iterations, one
   chunk behind the one it enqueues, and returns once every engine has stopped.  A stopped engine
   stays in the later launches as a no-op, or, with STOMP_DEBUG_GROUP_COMPACT=1 at
   stomp_group_create, is left out of every chunk staged after the host has seen it stopped
   (=0: it stays; the results are the same bit for bit; DESIGN.md 7 has the measurement).
   Post-conditions, per engine p: exactly the state its own stomp_engine_optimize leaves --
   stats[p] (durations: device wall clock from the group's start), the cost history,
   best_trajectory, last_trajectory, theta and the rollout rows (with K_r > 0 also the extra
   rollout's rows and the reuse state of the iteration it stopped at); it is not gated and not tracking,
   holds no pending noiseless rollout and no pregen rows, so its own iterate / run and
   stomp_group_run with any first iteration continue from there.  Engines may enter in any state
   stomp_engine_optimize accepts.  NULL stats or a costs_stride below an engine's max_iterations:
   STOMP_E_INVALID with no engine touched. */
#define STOMP_GROUP_OPTIMIZE_CHUNK 8
int stomp_group_optimize(stomp_group* g, stomp_stats* stats, double* costs_per_iteration, int32_t costs_stride);
int32_t stomp_group_optimize_chunk(void);
/* stomp_engine_retarget for every engine of the group at once: starts and goals are P x J (row p
 * for engine p), seeds P values.  One launch retargets the whole group and one read-back fetches
 * the P padding-collision flags; the group's own copy of every engine's model carries the new flag
 * before the next grouped launch.  Each engine is then the freshly created engine of its new
 * problem, so engines that left stomp_group_optimize at different iterations are in one iteration
 * state again: stomp_group_run and stomp_group_optimize accept them with any first iteration.
 * (An engine of a group may also be retargeted on its own with stomp_engine_retarget; the group
 * picks its new flag up at its next call.)  NULL group or array, or a value that is not finite:
 * STOMP_E_INVALID before any engine or device is touched; a refused call leaves every engine
 * untouched. */
int stomp_group_retarget(stomp_group* g, const double* starts, const double* goals, const uint64_t* seeds);
/* stomp_engine_retarget_request for every engine of the group at once: requests[p] is engine p's.
 * All P models are planned first; the planned engines must again be of one shape (the same number
 * of spheres, the same rollout LDS size and layout: STOMP_E_INVALID otherwise), and a request that
 * gives an engine path constraints in a group created without STOMP_GROUP_ACCEPT_STATE_TERMS is
 * STOMP_E_UNSUPPORTED.  Only then is anything committed: one upload, one launch and one read-back for
 * the whole group, which also rewrite the group's own copies of the engines' models.  Requests may
 * differ per engine in the spheres' values and in the constraints.  Every refusal of
 * stomp_engine_retarget_request applies, before any engine or device is touched; a refused call
 * leaves every engine untouched.
 * An engine of a group whose model was changed on its own with stomp_engine_retarget_request leaves
 * the group's copies stale: the next stomp_group_run / synchronize / optimize / retarget returns
 * STOMP_E_INVALID naming the engine and touches nothing, until stomp_group_retarget_requests has
 * brought the group back in step. */
int stomp_group_retarget_requests(stomp_group* g, const stomp_request* requests /* P */);
/* A queue of requests served by the group's P engines as slots: a slot whose request has stopped
 * takes the next waiting request instead of idling until the slowest problem of a batch ends.
 * A request is a plain retarget: a start, a goal and a seed (row r of starts / goals, seeds[r]).
 * The model, the field and every parameter are the slot's own as they stand.  A request that
 * replaces collision points or constraints, or a scene update between requests, stays with
 * stomp_group_retarget_requests + stomp_group_optimize.
 * Assignment: requests are handed out in index order.  Requests 0 .. min(P, n) - 1 go to slots
 * 0, 1, .. in one retarget launch and run their iteration 1 in group step 1.  The host reads the
 * slots' stop flags once per chunk of STOMP_GROUP_OPTIMIZE_CHUNK steps, one chunk behind the one it
 * enqueues (as stomp_group_optimize does); each time it learns that slots have stopped, the free
 * slots take the next waiting requests in ascending slot order, and the requests' iteration 1 runs
 * in the first step of the next chunk staged.  While requests wait every chunk has
 * STOMP_GROUP_OPTIMIZE_CHUNK steps (a step in which no slot has work launches nothing).  These
 * decisions depend on P, the chunk size and the requests' iteration counts alone, never on
 * timing: stomp_serve_schedule is the same decision procedure as a host-only function and returns,
 * for given iteration counts, the slots and start steps the loop produces (total_steps: the step in
 * which the last request stops, start_step + iterations at most).  With n < P the slots >= n are
 * neither retargeted nor launched.
 * Results, for request r planned by slot s: results[r].stats but for the two durations (which
 * count from the slot's own start stamp), best_trajectories[r] and
 * costs_per_iteration[r][0 .. iterations) are bit for bit what stomp_engine_retarget(e_s, start_r,
 * goal_r, seed_r) followed by stomp_engine_optimize(e_s, ..) gives.  Afterwards every used engine is
 * where the retarget to the last request it planned followed by its own stomp_engine_optimize
 * leaves it (stomp_group_optimize's post-conditions).  Per-request torque statistics are not
 * available: the engine's best-trajectory buffer has moved on when a later request runs.
 * Refused before any engine or device is touched: a NULL group, starts, goals, seeds, results or
 * best_trajectories, num_requests <= 0, a value that is not finite (the message names the
 * request), a costs_stride below the largest max_iterations when costs_per_iteration is given, an
 * engine inside its own optimize loop, an engine without iterations to run (max_iterations <= 0),
 * a stale model epoch (STOMP_E_INVALID each); sharded engines (STOMP_E_UNSUPPORTED).
 * stomp_group_serve_info, about the last call: [0] group steps run (up to the one in which the last
 * request stopped), [1] the requests' iterations summed (occupied slot-steps), [2] turnovers
 * (requests that did not start in step 1), [3] steps in which two live slots ran different
 * iteration numbers, [4] the largest idle gap in steps between a slot's stop and its next
 * request's iteration 1, [5] kernel launches enqueued, [6] device bytes held for results,
 * [7] allocations made by the call. */
typedef struct stomp_serve_result {
    int32_t slot;        /* index in the group of the engine that planned the request */
    int32_t start_step;  /* 1-based group step whose rollout launch ran the request's iteration 1 */
    stomp_stats stats;   /* durations from the slot's own start stamp, device wall clock */
} stomp_serve_result;
int stomp_group_serve(stomp_group* g, const double* starts /* [n][J] */, const double* goals /* [n][J] */,
                      const uint64_t* seeds /* [n] */, int32_t num_requests,
                      stomp_serve_result* results /* [n] */, double* best_trajectories /* [n][J][N] */,
                      double* costs_per_iteration /* NULL or [n][costs_stride] */, int32_t costs_stride);
int stomp_group_serve_info(stomp_group* g, int64_t info[8]);
/* iterations: [n], each >= 1; slot, start_step: [n] out; total_steps: out or NULL */
int stomp_serve_schedule(int32_t num_slots, int32_t num_requests, const int32_t* iterations /* [n] */,
                         int32_t* slot /* [n] */, int32_t* start_step /* [n] */, int32_t* total_steps);
const char* stomp_group_last_error(const stomp_group* g);
void stomp_group_destroy(stomp_group* g);

/* CHOMP mode: the reference's covariant gradient descent (use_chomp; StompOptimizer::
 * doChompOptimization, stomp_optimizer.cpp:208-247, in the loop of optimize(), :249-382) on the
 * model, field and cost of a live engine.  A stomp_chomp borrows the engine (which must outlive it)
 * and holds B independent descents between the engine's start and goal, from B initial trajectories
 * (multi-start); every kernel works on (descent, waypoint) or (descent, joint), so the batch is what
 * fills the device.
 * One step is, per descent: the smoothness increments -(quad_cost_full_i (2 x_i)) over the free
 * block (:403-411), the collision increments (:413-470: per free waypoint the spheres in ascending
 * order, a sphere with potential <= 1e-10 skipped, the fold ended after the first colliding sphere,
 * whose own term is included; J^T g, or J^T (J J^T + ridge I)^-1 g with use_pseudo_inverse, the 3 x 3
 * inverse by cofactors over the determinant), learning_rate Qinv_i (smoothness_cost_weight s_i +
 * obstacle_cost_weight c_i) (:472-486), the per-joint scale min(1, limit / |max|, limit / |min|) of
 * addIncrementsToTrajectory (:488-506), handleJointLimits, the forward kinematics and the cost
 * (:233-246: per waypoint a prefix sum of prefix sums of potential * vel_mag over the spheres, times
 * obstacle_cost_weight).  A zero vel_mag divides as IEEE 754 says, as in the reference; nothing guards it.
 * The field gradient is the third-party distance_field package's getDistanceGradient, which the
 * reference tree does not hold; this definition follows that package as its maintainers know it and
 * is stated from knowledge, not from a file: at the nearest cell g, component a is
 * (dist(g + e_a) - dist(g - e_a)) * (1 / (2 resolution)) with dist = sqrt(double(d2)) * resolution; a
 * centre whose cell is outside [1, n - 2] on any axis reads distance 0 and gradient 0 (the window of
 * the distance lookup, so the neighbours at 0 and n - 1 are always readable).  field_bias is added to
 * it before the potential's gradient is formed (stomp_collision_space.h:202-204).
 * Joint origins and axes are world-frame quantities of the same FK: the frame's translation of the
 * segment the joint drives, and that frame's rotation times the stored axis; a joint that drives no
 * segment reads zeros and has a zero Jacobian column, as has every joint off the path from the root
 * to the sphere's segment (fixed segments and branches included).
 * Taken from the engine: obstacle_cost_weight, max_iterations, max_iterations_after_collision_free,
 * the discretization, the joints' limits, start, goal, the model and the field (the bricked copy where
 * the engine has one), all as the engine holds them at the last stomp_chomp_reset.
 * reset: the descents' trajectories (NULL: every descent starts at the engine's policy parameters as
 *   they are on its stream, copyPolicyToGroupTrajectory of :268 -- theta_0 on an engine that has not
 *   iterated since its creation or last retarget), then optimize()'s pass before its loop (:267-271, iteration_ = 0): joint
 *   limits and FK.  The buffers are held with a capacity: a reset of a B not above an earlier one
 *   allocates nothing.
 * step: `count` iterations enqueued on the engine's stream behind what is there, no host wait; the
 *   first step after a reset runs with iteration_ = 0 (the padding's collisions count), the others with
 *   their own index.  optimize: the loop of :284-359 with its bookkeeping on the device, from a fresh
 *   reset; each descent stops on its own (its rows stay as they were when it stopped, later steps leave
 *   it out); the host reads the stop flags once per chunk of STOMP_GROUP_OPTIMIZE_CHUNK iterations, one
 *   chunk behind, and returns when all descents have stopped.  stats[b].success_duration and
 *   collision_success_duration are 0 (no clock is read).
 * get: one of "trajectory", "smoothness_increments", "collision_increments", "final_increments"
 *   ([B][J][N]), "scales" ([B][J]), "sphere_positions" ([B][N + 12][S][3], padding waypoints included),
 *   "distances", "potentials", "vel_mags" ([B][N][S]), "field_gradients" (without the bias),
 *   "potential_gradients", "velocities", "accelerations" ([B][N][S][3]), "joint_origins", "joint_axes"
 *   ([B][N][J][3]), "costs" ([B][N]), "cost", "collision_free" ([B]); waits for the stream.
 * info: [0] B, [1] iterations stepped since the reset, [2] kernel launches of the last reset / step /
 *   optimize call, [3] device and pinned allocations so far, [4..7] LDS bytes per workgroup of the FK,
 *   gradient (increments and velocities), update and bookkeeping kernels.
 * The CHOMP object changes nothing of the engine: theta, the rollout rows, the reuse state, a pending
 * noiseless rollout, the step API's state, the timers and group membership are untouched.
 * After stomp_engine_retarget (either kind, through a group too) or stomp_engine_refresh_field the next
 * step / optimize / get returns STOMP_E_INVALID naming the reason, until reset is called again (a field
 * read in place that a scene update rewrites without a refresh call cannot be noticed).
 * STOMP_E_INVALID, before any device is touched: NULL arguments; a struct_size other than
 * sizeof(stomp_chomp_params); num_trajectories < 1; a parameter or trajectory value that is not
 * finite; an update limit that is not positive; costs_stride below max_iterations (with costs); an
 * engine inside its optimize loop; optimize without a fresh reset.  STOMP_E_UNSUPPORTED: a sharded
 * engine (world_size > 1), use_hamiltonian_monte_carlo (the reference's HMC updates, :219-226, are not
 * built), N > 256, a kernel over its LDS limit.  The NULL and struct_size refusals come before the
 * engine is read (a machine without a GPU can make these calls). */
typedef struct stomp_chomp_params {
    int32_t struct_size;                  /* sizeof(stomp_chomp_params) */
    double learning_rate;                 /* 0.01 (stomp_parameters.cpp:60) */
    double smoothness_cost_weight;        /* 0.1  (:56) */
    int32_t use_pseudo_inverse;           /* 0    (:71) */
    double pseudo_inverse_ridge_factor;   /* 1e-4 (:72) */
    double field_bias[3];                 /* 0 */
    const double* joint_update_limits;    /* J; stomp_joints_[i].joint_update_limit_, 0.05 (stomp_robot_model.cpp:78) */
    int32_t use_hamiltonian_monte_carlo;  /* must be 0 */
} stomp_chomp_params;
typedef struct stomp_chomp stomp_chomp;
int stomp_chomp_create(stomp_engine* e, const stomp_chomp_params* p, stomp_chomp** out);
int stomp_chomp_reset(stomp_chomp* c, int32_t num_trajectories /* B >= 1 */,
                      const double* trajectories /* [B][J][N] or NULL: theta_0 */);
int stomp_chomp_step(stomp_chomp* c, int32_t count);      /* enqueue, no host sync */
int stomp_chomp_synchronize(stomp_chomp* c);
int stomp_chomp_optimize(stomp_chomp* c, stomp_stats* stats /* [B] */, double* costs /* [B][stride] or NULL */,
                         int32_t costs_stride, double* best_trajectories /* [B][J][N] or NULL */);
int stomp_chomp_get(stomp_chomp* c, const char* which, double* out);
int stomp_chomp_info(stomp_chomp* c, int64_t info[8]);
const char* stomp_chomp_last_error(const stomp_chomp* c);
void stomp_chomp_destroy(stomp_chomp* c);

/* Device buffers for callers without a HIP runtime of their own (bench, tests). */
int stomp_device_alloc(int32_t device, uint64_t bytes, void** out);
int stomp_device_free(void* p);
int stomp_device_copy_to_host(void* dst, const void* src, uint64_t bytes);
int stomp_device_count(int32_t* count);

/* RCCL unique id for world_size > 1 (call on rank 0, broadcast the 128 bytes). */
int stomp_comm_unique_id(void* out128);
/* Id of an in-process exchange group of world_size ranks: the ranks are engines of THIS
 * process (on one device or several), each created with this id, its rank and world_size and
 * each driven by a host thread of its own; the per-iteration exchanges are device-to-device
 * copies ordered by HIP events instead of RCCL (same results bit for bit). */
int stomp_comm_local_id(int32_t world_size, void* out128);

/* deterministic math + RNG primitives evaluated on the device (parity tests) */
int stomp_device_selftest(const double* x, int32_t n, double* out_exp, double* out_log, double* out_sin,
                          double* out_cos, double* out_sqrt);
/* atan2(y[i], x[i]) and asin(y[i]) as the orientation-constraint term evaluates them on the device */
int stomp_device_selftest_trig(const double* y, const double* x, int32_t n, double* out_atan2, double* out_asin);
int stomp_device_normals(uint64_t seed, int32_t iteration, int32_t joint, int32_t rollout, int32_t n, double* z);

#ifdef __cplusplus
}
#endif
#endif
