/*
 * trajopt_host.h — C entry points of the C++ host front door
 * (trajopt-1_amd/lib/libtrajopt_host.so, sources in trajopt-1_amd/host/).
 *
 * The C++ API (trajopt-1_amd/host/include/trajopt_amd/ headers) mirrors the
 * reference's problem-construction surface: ProblemConstructionInfo::fromJson,
 * the TermInfo registry and hatch(), ConstructProblem
 * (trajopt/src/problem_description.cpp:36-598) and a batch
 * BasicTrustRegionSQP (trajopt_sco/src/optimizers.cpp:699-991).  These C
 * wrappers expose it to ctypes / FFI callers: JSON problem text in the
 * reference's TrajOptRequest format (trajopt_common/data/config/ JSON files) on the
 * built-in environment of the reference's test robots (thost_lower_json).  Return 0 on success, -1 on failure
 * with the message (the reference's std::runtime_error text) in err.
 */
#ifndef TRAJOPT_HOST_H
#define TRAJOPT_HOST_H

#include "trajopt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Parse + ConstructProblem for one JSON problem; `scene` holds primitives added
 * to the built-in environment's own ([n_prims][16], THIP_PRIM_* records, may be
 * NULL when n_prims == 0).  The environment is the reference test robot of
 * basic_info.manip: the PR2 (right_arm, left_arm, both_arms; empty scene) or
 * spherebot ("manipulator"; its three static spheres first).  Outputs
 * (caller-sized to the maxima: THIP_EVAL_MAX_STEPS waypoints, THIP_MAX_CART,
 * THIP_MAX_JPOS terms, THIP_EVAL_MAX_PRIMS primitives):
 *   desc          the batch-shared structure (per-problem JointPos targets zeroed)
 *   init          [n_steps][n_dof]                initial trajectory
 *   cart_targets  [n_cart][12]                    CartPose target offsets in the chain root
 *   jpos_targets  [n_jpos][n_dof]                 JointPos targets
 *   scene_out     [desc.n_prims][16]              the scene the collision terms see
 * Any output pointer may be NULL. */
int thost_lower_json(const char* json_text, const double* scene, int n_prims, thip_problem_desc* desc,
                     double* init, double* cart_targets, double* jpos_targets, double* scene_out, char* err,
                     int err_len);

/* ConstructProblem for each of `batch` JSON problems (scenes [batch][n_prims][16])
 * and one BatchTrustRegionSQP on HIP device `device`:
 *   x        [batch][n_steps][n_dof]   final trajectories
 *   results  [batch]                   status and counters (may be NULL) */
int thost_solve_json_batch(const char* const* json_texts, int batch, const double* scenes, int n_prims, int device,
                           double* x, thip_result* results, char* err, int err_len);

/* A batch with problems the fused kernel does not lower runs the problems' host
 * SQP loops on a bounded pool of worker threads (each worker takes the next
 * unsolved problem when its current one ends), every QP round in one launch per
 * sparsity pattern (trajopt::BatchTrustRegionSQP's host-loop mode, sco::GpuQPBatcher);
 * x then holds [batch][n_steps][n_dof (+ 1 with use_time)].  This reports the QP
 * launches and QPs of the calling thread's last batch solve (0 for a fused-kernel batch). */
void thost_last_batch_qp_stats(long long* launches, long long* qps);
/* Worker threads of such host-loop batches (process-wide; n <= 0 restores the
 * default, 64; never more than the batch). */
void thost_set_host_loop_workers(int n);

/* A prepared batch: ConstructProblem for each of `batch` JSON problems
 * (scenes [batch][n_prims][16]) and the trajopt::BatchTrustRegionSQP over them
 * on HIP device `device`, without solving -- so a caller (the bench) times the
 * solve alone.  thost_batch_solve runs it once: x [batch][n_steps][n_dof (+1
 * with use_time)], results [batch] (may be NULL); a host-loop batch's models
 * keep their warm starts, so it is solved at most once (a second call fails).
 * thost_batch_stats: host_loops (1 when the problems run the host loops with
 * batched QPs, 0 for the fused kernel), and for host loops the QP launches, QPs,
 * their algorithmic HBM bytes (sco::GpuQPBatcher::bytes) and the wall seconds
 * spent in the launches.  Every problem's host loop runs at once (one worker
 * per problem), so each QP round of the batch is one launch per pattern. */
typedef struct thost_batch thost_batch;
int thost_batch_create(const char* const* json_texts, int batch, const double* scenes, int n_prims, int device,
                       thost_batch** out, char* err, int err_len);
int thost_batch_solve(thost_batch* b, double* x, thip_result* results, char* err, int err_len);
int thost_batch_stats(const thost_batch* b, int* host_loops, long long* qp_launches, long long* qps, double* qp_bytes,
                      double* qp_seconds);
/* Host-loop batches (diagnostic): out[0] ADMM iterations of all QPs, then the
 * largest KKT's thip_qp_shape (6 entries). */
int thost_batch_qp_shape(const thost_batch* b, long long* out);
void thost_batch_destroy(thost_batch* b);

/* thost_solve_json_batch sharded over n_devices HIP devices of this process
 * (trajopt::MultiDeviceBatchSQP: contiguous shards, sizes differing by at most
 * one, all shards running concurrently; a device may be listed more than once). */
int thost_solve_json_batch_multi(const char* const* json_texts, int batch, const double* scenes, int n_prims,
                                 const int* devices, int n_devices, double* x, thip_result* results, char* err,
                                 int err_len);

/* A stream of n_batches batches of `batch` JSON problems each (json_texts
 * [n_batches * batch], scenes [n_batches * batch][n_prims][16]), every batch
 * sharded over the device entries as thost_solve_json_batch_multi does, with
 * `inflight` batches in flight per device entry
 * (trajopt::MultiDeviceBatchSQP::optimizeStream: the next batches fill the CUs
 * the current batch's tail leaves idle).  x [n_batches * batch][n_steps][n_dof],
 * results [n_batches * batch] (may be NULL), in input order. */
int thost_solve_json_stream(const char* const* json_texts, int n_batches, int batch, const double* scenes, int n_prims,
                            const int* devices, int n_devices, int inflight, double* x, thip_result* results, char* err,
                            int err_len);

/* ConstructProblem for one JSON problem and trajopt::BasicTrustRegionSQP
 * (sco::BasicTrustRegionSQP with the problem's opt_info) on HIP device
 * `device`, as the reference's planning code runs one problem
 * (optimizers.cpp:699-991): a problem whose every term lowered into the
 * batched kernel runs it as a batch of one (*native = 1); one with terms the
 * kernel does not lower (JointAcc / JointJerk, JointVel equality constraints,
 * time-parameterised JointVel, TotalTime, fixed dofs) runs the SQP loop on the
 * host with every QP on the GPU (GpuModel, *native = 0).
 * x: [n_steps][n_dof (+ 1: the dt column with basic_info.use_time)];
 * result and native may be NULL. */
int thost_solve_json(const char* json_text, const double* scene, int n_prims, int device, double* x,
                     thip_result* result, int* native, char* err, int err_len);

/* trajopt::checkTrajectory (trajopt_amd/check_trajectory.hpp; thip_check_* in
 * trajopt_hip.h) for `batch` JSON problems of one group, horizon and scene size:
 * is each trajectory (trajectories [batch][n_steps][n_dof], joint values only)
 * within config->margin of its scene (scenes [batch][n_prims][16] after the
 * built-in environment's own) or of itself, and its clearance.  A problem needs
 * no collision term.  results [batch]; `found` is the reference's
 * checkTrajectory return value (planning_unit.cpp:92-101, 143-148). */
int thost_check_json_batch(const char* const* json_texts, int batch, const double* scenes, int n_prims,
                           const double* trajectories, const thip_check_config* config, int device,
                           thip_check_result* results, char* err, int err_len);

/* trajopt::TermEvaluator (trajopt_amd/term_evaluator.hpp; thip_terms_* in
 * trajopt_hip.h) for `batch` lowerable JSON problems of one structure: the value
 * of every cost and the violation of every constraint of each problem at its
 * trajectory (trajectories [batch][n_steps][n_dof]), in prob->getCosts() /
 * getConstraints() order (equality constraints first).
 *   route THOST_EVAL_DEVICE   the batched term-value kernels (one evaluator)
 *         THOST_EVAL_OBJECTS  the host term objects, Cost::value /
 *                             Constraint::violation per problem (the device
 *                             evaluators of the host loop)
 *         THOST_EVAL_NAMES    counts, names and the slot map only: no device call
 * n_costs / n_cnts: the counts.  cost_vals [batch][n_costs], cnt_viols
 * [batch][n_cnts] (may be NULL with THOST_EVAL_NAMES).  names: problem 0's cost
 * names, then its constraint names, each followed by '\n' (may be NULL).
 * slot_map [n_costs + n_cnts] (may be NULL): the getCosts() position of every
 * kernel cost slot, then the getConstraints() position of every constraint slot. */
#define THOST_EVAL_DEVICE 0
#define THOST_EVAL_OBJECTS 1
#define THOST_EVAL_NAMES 2
int thost_eval_json_batch(const char* const* json_texts, int batch, const double* scenes, int n_prims,
                          const double* trajectories, int route, int device, int* n_costs, int* n_cnts,
                          double* cost_vals, double* cnt_viols, char* names, int names_len, int* slot_map, char* err,
                          int err_len);

/* Solve `batch` JSON problems of one structure and return OptResults::cost_vals /
 * cnt_viols with the usual results: through trajopt::BatchTrustRegionSQP
 * (drop_in = 0) or problem by problem through the trajopt::BasicTrustRegionSQP
 * drop-in (drop_in = 1: initialize, optimize, results()).  sizes[0] / sizes[1]:
 * the lengths of problem 0's cost_vals / cnt_viols; cost_vals
 * [batch][cap_costs] and cnt_viols [batch][cap_cnts] take each problem's
 * vectors (an error when one is longer than its cap). */
int thost_solve_json_batch_terms(const char* const* json_texts, int batch, const double* scenes, int n_prims,
                                 int device, int drop_in, double* x, thip_result* results, int* sizes,
                                 double* cost_vals, int cap_costs, double* cnt_viols, int cap_cnts, char* err,
                                 int err_len);

/* ---------------------------------------------------------- trajopt_sqp
 * The second SQP front end (the ifopt stack):
 * trajopt_sqp::TrustRegionSQPSolver over a trajopt_sqp::TrajOptQPProblem whose
 * QP keeps one sparsity pattern and is updated in place on the GPU
 * (trajopt_sqp::GpuQPSolver over thip_qp's resident workspace).  The C++ API is
 * trajopt-1_amd/host/include/trajopt_sqp/ and trajopt_ifopt/; this flat spec
 * drives it from FFI callers and the tests: a joint trajectory of n_nodes
 * nodes (one trajopt_ifopt::Var of n_dof positions each) with joint
 * position / velocity / acceleration / jerk terms as constraints or costs. */
#define TSQP_MAX_NODES 64
#define TSQP_MAX_TERMS 16
enum { TSQP_JOINT_POS = 0, TSQP_JOINT_VEL = 1, TSQP_JOINT_ACC = 2, TSQP_JOINT_JERK = 3 };
/* addConstraintSet, or addCostSet with CostPenaltyType kSquared / kAbsolute / kHinge */
enum { TSQP_CONSTRAINT = 0, TSQP_SQUARED = 1, TSQP_ABSOLUTE = 2, TSQP_HINGE = 3 };
/* trajopt_sqp::SQPStatus (types.h) */
enum {
  TSQP_STATUS_RUNNING = 0,
  TSQP_STATUS_CONVERGED = 1,
  TSQP_STATUS_ITERATION_LIMIT = 2,
  TSQP_STATUS_PENALTY_ITERATION_LIMIT = 3,
  TSQP_STATUS_TIME_LIMIT = 4,
  TSQP_STATUS_QP_SOLVE_FAILED = 5,
  TSQP_STATUS_STOPPED_BY_CALLBACK = 6
};
typedef struct tsqp_term {
  int kind;        /* TSQP_JOINT_* */
  int penalty;     /* TSQP_CONSTRAINT / SQUARED / ABSOLUTE / HINGE */
  int first, last; /* nodes first..last (JointPos: the node `first`) */
  int n_coeffs;    /* 0, 1 or n_dof coefficients */
  double coeffs[THIP_MAX_DOF];
  /* JointPos: per-dof bounds (lower == upper: a target; a range splits into two
   * inequalities, RangeBoundHandling::kSplitToTwoInequalities); JointVel / Acc /
   * Jerk: per-dof targets in `lower` */
  double lower[THIP_MAX_DOF], upper[THIP_MAX_DOF];
} tsqp_term;
typedef struct tsqp_spec {
  int n_nodes, n_dof;
  double init[TSQP_MAX_NODES * THIP_MAX_DOF]; /* [n_nodes][n_dof] */
  double var_lower[THIP_MAX_DOF], var_upper[THIP_MAX_DOF]; /* variable bounds (+-inf allowed) */
  int n_terms;
  tsqp_term terms[TSQP_MAX_TERMS];
  /* trajopt_sqp::SQPParameters (types.h) */
  double improve_ratio_threshold, min_trust_box_size, min_approx_improve, min_approx_improve_frac;
  int max_iterations;
  double trust_shrink_ratio, trust_expand_ratio, cnt_tolerance, max_merit_coeff_increases;
  int max_qp_solver_failures;
  double merit_coeff_increase_ratio, max_time, initial_merit_error_coeff;
  int inflate_constraints_individually;
  double initial_trust_box_size;
  thip_osqp_settings osqp; /* OSQPEigenSolver::setDefaultOSQPSettings + the test's overrides */
} tsqp_spec;
typedef struct tsqp_result {
  int status;             /* TSQP_STATUS_* */
  int overall_iteration;  /* QP solves of the trust-region loop (SQPResults::overall_iteration) */
  int penalty_iteration;
  int qp_setups;          /* full QP setups (first solve, pattern or size change) */
  int qp_updates;         /* convexifications applied in place (update_data_mat / _vec) */
  int qp_solves;
  long long admm_iters;
  double best_exact_merit;
} tsqp_result;
/* SQPParameters / OSQP settings defaults into a spec (terms untouched) */
void thost_tsqp_defaults(tsqp_spec* spec);
/* solve on HIP device `device`: x [n_nodes][n_dof] (the best variables) */
int thost_tsqp_solve(const tsqp_spec* spec, int device, double* x, tsqp_result* result, char* err, int err_len);
/* sizeof(tsqp_spec) / sizeof(tsqp_result) as compiled into the library (FFI layout check) */
int thost_tsqp_sizeof_spec(void);
int thost_tsqp_sizeof_result(void);

/* The kinematic sets of the same front end (trajopt_ifopt::CartPosConstraint and
 * the fixed-size trajopt_ifopt::DiscreteCollisionConstraint over a
 * SingleTimestepCollisionEvaluator, trajopt-1_amd/host/include/trajopt_ifopt/
 * constraints/), their values and jacobians from the device: a tsqp_kin_spec
 * adds them to the joint terms of a tsqp_spec, on the built-in environment of
 * `manip` (Environment::builtin: the PR2 groups, or spherebot's "manipulator")
 * with `n_prims` more scene primitives.  spec->n_dof must be the group's. */
#define TSQP_KIN_MAX_CART 16
#define TSQP_KIN_MAX_COLL 4
#define TSQP_KIN_MAX_PRIMS 32
#define TSQP_KIN_NAME_LEN 64
typedef struct tsqp_cart_term {
  int node;
  int penalty;                        /* TSQP_CONSTRAINT / SQUARED / ABSOLUTE / HINGE */
  int analytic_jacobian;              /* 1: use_numeric_differentiation = false, which the set refuses at update() */
  int pad_;
  char source_frame[TSQP_KIN_NAME_LEN], target_frame[TSQP_KIN_NAME_LEN];
  double source_offset[12], target_offset[12]; /* 3x4 row-major [R | t] */
  double coeffs[6];                   /* a zero coefficient drops the component's row */
  double lower[6], upper[6];          /* bounds of the six error components (a range splits into two rows) */
} tsqp_cart_term;
typedef struct tsqp_coll_term {
  int first, last;                    /* one DiscreteCollisionConstraint per node of first..last, one evaluator */
  int penalty;
  int max_num_cnt, fixed_sparsity;
  double margin, coeff, buffer;       /* TrajOptCollisionConfig(margin, coeff), collision_margin_buffer */
} tsqp_coll_term;
typedef struct tsqp_ccoll_term {
  int first, last;                    /* one ContinuousCollisionConstraint per segment (n, n + 1), first <= n < last,
                                         all on one evaluator */
  int penalty;
  int max_num_cnt, fixed_sparsity;
  int evaluator_type;                 /* tesseract's CollisionEvaluatorType: DISCRETE 1 / LVS_DISCRETE 2 go to an
                                         LVSDiscreteCollisionEvaluator, every other value to an
                                         LVSContinuousCollisionEvaluator (CONTINUOUS 3, LVS_CONTINUOUS 4); each
                                         refuses the types it does not take */
  int fixed_first, fixed_last;        /* vars0_fixed of the first segment, vars1_fixed of the last */
  double margin, coeff, buffer;       /* TrajOptCollisionConfig(margin, coeff), collision_margin_buffer */
  double lvs_length;                  /* collision_check_config.longest_valid_segment_length */
} tsqp_ccoll_term;
typedef struct tsqp_kin_spec {
  char manip[TSQP_KIN_NAME_LEN];
  int n_prims;
  double prims[TSQP_KIN_MAX_PRIMS][16]; /* THIP_PRIM_* records appended to the environment's scene */
  int n_cart;
  tsqp_cart_term cart[TSQP_KIN_MAX_CART];
  int n_coll;
  tsqp_coll_term coll[TSQP_KIN_MAX_COLL];
  int n_ccoll;
  tsqp_ccoll_term ccoll[TSQP_KIN_MAX_COLL];
} tsqp_kin_spec;
/* thost_tsqp_solve with the kinematic sets added after the joint terms (the
 * CartPos sets, then each collision term's nodes, then each continuous collision
 * term's segments) */
int thost_tsqp_solve_kin(const tsqp_spec* spec, const tsqp_kin_spec* kin, int device, double* x, tsqp_result* result,
                         char* err, int err_len);
/* The same sets without a solve: for each of the n_x variable vectors xs
 * [n_x][n_nodes][n_dof], set in turn with TrajOptQPProblem::setVariables, every
 * set's getValues, dense getJacobian and getCoefficients, rows concatenated in
 * set order (joint terms, CartPos sets, collision nodes, continuous collision segments):
 *   n_sets, set_rows [cap_sets]          the sets and their row counts
 *   values, coeffs [n_x][cap_rows]       jac [n_x][cap_rows][n_nodes * n_dof]
 *   lower, upper [cap_rows]              getBounds (+-inf as +-HUGE_VAL)
 *   probe_q [n_dof] (may be NULL) -> probe_values [cap_rows]: after the last x,
 *     every CartPos set's calcValues(probe_q) in its rows (other rows untouched),
 *     asked while the variables still hold the last x
 *   launches [2]                         device launches of the CartPos evaluator and of the collision
 *                                        evaluators over the whole call (the probe's included)
 * Any output may be NULL; more than cap_sets sets or cap_rows rows is an error.
 * With n_x = 0 the sets are only constructed (their validation, rows and bounds):
 * no device call is made. */
int thost_tsqp_eval_kin(const tsqp_spec* spec, const tsqp_kin_spec* kin, int device, const double* xs, int n_x,
                        int* n_sets, int* set_rows, int cap_sets, double* values, double* jac, double* coeffs,
                        double* lower, double* upper, int cap_rows, const double* probe_q, double* probe_values,
                        long long* launches, char* err, int err_len);
int thost_tsqp_sizeof_kin_spec(void);
int thost_tsqp_sizeof_cart_term(void);
int thost_tsqp_sizeof_coll_term(void);
int thost_tsqp_sizeof_ccoll_term(void);

/* A batch of trajopt_sqp problems in lock step on one device
 * (trajopt_sqp::BatchTrustRegionSQPSolver): every problem runs the
 * TrustRegionSQPSolver of thost_tsqp_solve / thost_tsqp_solve_kin on a host
 * thread of its own, and the QPs of a round run as one thip_qp_step per group
 * of problems that share a QP pattern, sizes and OSQP settings.  Every
 * problem's x and result are bit for bit those of its solve alone.
 *   specs [batch], kins [batch] (NULL: joint terms only)
 *   x [batch][TSQP_MAX_NODES * THIP_MAX_DOF]: problem b's [n_nodes][n_dof] at x + b * that stride
 *   results [batch]; qp_rounds [batch] (may be NULL): the rounds problem b took part in
 *   stats (may be NULL)
 * batch < 1 or a NULL specs / x / results is an error before any device call.
 * When problems fail, the others still finish: the return value is -1, err
 * holds "problem <b>: <message>" of each failed problem (one per line), and a
 * failed problem's result has status -1. */
typedef struct tsqp_batch_stats {
  long long rounds;          /* rendezvous rounds */
  long long step_launches;   /* thip_qp_step launches: one per group with a waiting problem, per round */
  long long groups;          /* thip_qp objects created: one symbolic KKT analysis each */
  long long max_group;       /* the largest batch of one */
  long long set_launches[2]; /* launches of the problems' CartPos evaluators and collision evaluators (each problem's
                                sets launch for their own problem), as thost_tsqp_eval_kin counts them */
} tsqp_batch_stats;
int thost_tsqp_solve_batch(const tsqp_spec* specs, const tsqp_kin_spec* kins /* NULL: joint terms only */, int batch,
                           int device, double* x /* [batch][TSQP_MAX_NODES*THIP_MAX_DOF] stride */,
                           tsqp_result* results, int* qp_rounds /*[batch]*/, tsqp_batch_stats* stats, char* err,
                           int err_len);
int thost_tsqp_sizeof_batch_stats(void);

#ifdef __cplusplus
}
#endif

#endif /* TRAJOPT_HOST_H */
