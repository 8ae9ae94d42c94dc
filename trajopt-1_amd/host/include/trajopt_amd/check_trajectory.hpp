// checkTrajectory: tesseract's trajectory collision check as the reference's
// tests run it around every solve (trajopt/test/planning_unit.cpp:92-101,
// 143-148: the initial trajectory is in collision, the optimised one is not),
// for a batch, on the device (include/trajopt_hip.h thip_check_*).
//
//   tesseract_collision::CollisionCheckConfig config;      reference
//   config.type = CollisionEvaluatorType::CONTINUOUS;
//   config.longest_valid_segment_length = ...;
//   config.contact_manager_config.default_margin = 0;      (margin_data)
//   found = checkTrajectory(contacts, *manager, *state_solver, joint_names, traj, config);
//
//   trajopt::CollisionCheckConfig config;                   here
//   config.type = trajopt::CollisionEvaluatorType::CONTINUOUS;
//   found = trajopt::checkTrajectory(prob, traj, config).found;
//
// The robot is the environment's sphere model and the scene its primitives, as
// in the collision terms: verdicts are not pinned against Bullet.
#pragma once
#include <vector>

#include "trajopt_amd/problem_description.hpp"

namespace trajopt
{
// rows of joint values, one per waypoint (a dt column after the joints is ignored)
using TrajArray = std::vector<DblVec>;

// tesseract_collision::CollisionEvaluatorType (the JSON evaluator_type values)
enum class CollisionEvaluatorType : int
{
  DISCRETE = 1,
  LVS_DISCRETE = 2,
  CONTINUOUS = 3,
  LVS_CONTINUOUS = 4
};

// The fields of tesseract_collision::CollisionCheckConfig the reference's tests set
struct CollisionCheckConfig
{
  CollisionEvaluatorType type = CollisionEvaluatorType::CONTINUOUS;
  double longest_valid_segment_length = 0.005;  // LVS kinds
  double contact_margin = 0.0;                  // contact_manager_config's default margin: a contact is dist < margin
  int first_step = 0, last_step = -1;           // -1: the last waypoint
};

struct TrajectoryCheckReport
{
  bool found = false;  // the reference's return value
  int n_contacts = 0;
  int first_step = -1;  // waypoint of the first unit (waypoint or step pair) with a contact
  long long n_candidates = 0;
  // the smallest signed distance on the trajectory and where: the unit's waypoint,
  // robot link (chain index), scene primitive or -1 - robot sphere, robot sphere,
  // LVS sub-state, and the time within the step pair
  double min_distance = 0.0;
  int min_step = -1, min_link = -1, min_other = -1, min_sphere = -1, min_substate = -1;
  double min_cc_time = 0.0;
};

// The C-ABI form of a config (CONTINUOUS: LVS_CONTINUOUS with lvs = +inf)
thip_check_config toCheckConfig(const CollisionCheckConfig& config);

// One report per problem.  The problems share one group, horizon and scene size
// (a batch's structure); a problem without a collision term is checked with its
// environment's collision model all the same.
std::vector<TrajectoryCheckReport> checkTrajectory(const std::vector<TrajOptProb::Ptr>& probs,
                                                   const std::vector<TrajArray>& trajs,
                                                   const CollisionCheckConfig& config = CollisionCheckConfig(),
                                                   int device = 0);
TrajectoryCheckReport checkTrajectory(const TrajOptProb::Ptr& prob, const TrajArray& traj,
                                      const CollisionCheckConfig& config = CollisionCheckConfig(), int device = 0);

// The shared implementation: `batch` problems of descriptor d (its chain, robot
// spheres, self pairs, n_prims, n_steps), scenes [batch][n_prims][16],
// trajectories [batch][n_steps][n_dof] on the host (x) or on the device (d_x).
std::vector<TrajectoryCheckReport> checkTrajectories(const thip_problem_desc& d, int batch,
                                                     const std::vector<double>& scenes, const thip_check_config& cfg,
                                                     int device, const double* x, const double* d_x);
}  // namespace trajopt
