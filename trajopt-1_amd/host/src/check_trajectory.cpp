#include "trajopt_amd/check_trajectory.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>

namespace trajopt
{
thip_check_config toCheckConfig(const CollisionCheckConfig& config)
{
  thip_check_config c;
  thip_default_check_config(&c);
  switch (config.type)
  {
    case CollisionEvaluatorType::DISCRETE:
      c.type = 2;
      break;
    case CollisionEvaluatorType::LVS_DISCRETE:
      c.type = 0;
      break;
    case CollisionEvaluatorType::CONTINUOUS:
    case CollisionEvaluatorType::LVS_CONTINUOUS:
      c.type = 1;
      break;
    default:
      throw std::runtime_error("checkTrajectory: CollisionEvaluatorType " +
                               std::to_string(static_cast<int>(config.type)) + " is not supported");
  }
  // CONTINUOUS casts each step pair once (problem_description.cpp:1742-1744)
  c.lvs = config.type == CollisionEvaluatorType::CONTINUOUS ? std::numeric_limits<double>::infinity()
                                                            : config.longest_valid_segment_length;
  c.margin = config.contact_margin;
  c.first_step = config.first_step;
  c.last_step = config.last_step;
  return c;
}

std::vector<TrajectoryCheckReport> checkTrajectories(const thip_problem_desc& d, int batch,
                                                     const std::vector<double>& scenes, const thip_check_config& cfg,
                                                     int device, const double* x, const double* d_x)
{
  if (batch <= 0 || (!x && !d_x))
    throw std::runtime_error("checkTrajectory: empty batch or no trajectories");
  if (scenes.size() != static_cast<std::size_t>(batch) * static_cast<std::size_t>(std::max(d.n_prims, 0)) * 16)
    throw std::runtime_error("checkTrajectory: scenes do not hold [batch][n_prims][16] values");
  thip_check* chk = nullptr;
  if (thip_check_create(device, &d, &cfg, batch, &chk) != THIP_OK)
    throw std::runtime_error(thip_check_last_error(nullptr));
  std::vector<thip_check_result> res(static_cast<std::size_t>(batch));
  int rc = thip_check_upload(chk, scenes.empty() ? nullptr : scenes.data());
  if (rc == THIP_OK)
    rc = x ? thip_check_run(chk, x, res.data(), nullptr) : thip_check_run_device(chk, d_x, res.data(), nullptr);
  if (rc != THIP_OK)
  {
    const std::string why = thip_check_last_error(chk);
    thip_check_destroy(chk);
    throw std::runtime_error("checkTrajectory: " + why);
  }
  thip_check_destroy(chk);
  std::vector<TrajectoryCheckReport> out(res.size());
  for (std::size_t b = 0; b < res.size(); ++b)
  {
    const thip_check_result& r = res[b];
    TrajectoryCheckReport& o = out[b];
    o.found = r.found != 0;
    o.n_contacts = r.n_contacts;
    o.first_step = r.first_unit;
    o.n_candidates = r.n_candidates;
    o.min_distance = r.min_distance;
    o.min_step = r.min_t;
    o.min_link = r.min_link;
    o.min_other = r.min_other;
    o.min_sphere = r.min_sphere;
    o.min_substate = r.min_substate;
    o.min_cc_time = r.min_cc_time;
  }
  return out;
}

namespace
{
// the fields a check reads: equal across a batch
bool sameModel(const thip_problem_desc& a, const thip_problem_desc& b)
{
  return a.n_steps == b.n_steps && std::memcmp(&a.chain, &b.chain, sizeof(a.chain)) == 0 &&
         a.n_spheres == b.n_spheres && std::memcmp(a.sphere_link, b.sphere_link, sizeof(a.sphere_link)) == 0 &&
         std::memcmp(a.sphere_center, b.sphere_center, sizeof(a.sphere_center)) == 0 &&
         std::memcmp(a.sphere_radius, b.sphere_radius, sizeof(a.sphere_radius)) == 0 && a.n_prims == b.n_prims &&
         a.n_self_pairs == b.n_self_pairs && std::memcmp(a.self_pair, b.self_pair, sizeof(a.self_pair)) == 0;
}
}  // namespace

std::vector<TrajectoryCheckReport> checkTrajectory(const std::vector<TrajOptProb::Ptr>& probs,
                                                   const std::vector<TrajArray>& trajs,
                                                   const CollisionCheckConfig& config, int device)
{
  if (probs.empty() || probs.size() != trajs.size())
    throw std::runtime_error("checkTrajectory: " + std::to_string(probs.size()) + " problems and " +
                             std::to_string(trajs.size()) + " trajectories");
  thip_problem_desc d0{};
  std::vector<double> scenes, x;
  for (std::size_t b = 0; b < probs.size(); ++b)
  {
    if (!probs[b])
      throw std::runtime_error("checkTrajectory: null problem");
    thip_problem_desc d = probs[b]->desc();
    std::vector<double> scene = probs[b]->scene;
    // a problem without a collision term has no collision model in its descriptor yet
    if (!d.coll_enabled && d.n_coll_extra == 0)
    {
      scene.clear();
      lowerCollisionModel(*probs[b]->GetKin(), *probs[b]->GetEnv(), d, scene);
    }
    if (b == 0)
      d0 = d;
    else if (!sameModel(d0, d))
      throw std::runtime_error("checkTrajectory: problem " + std::to_string(b) +
                               " does not share problem 0's group, horizon, collision model or scene size");
    scenes.insert(scenes.end(), scene.begin(), scene.end());
    const std::size_t N = static_cast<std::size_t>(d.n_steps), D = static_cast<std::size_t>(d.chain.n_dof);
    if (trajs[b].size() != N)
      throw std::runtime_error("checkTrajectory: trajectory " + std::to_string(b) + " has " +
                               std::to_string(trajs[b].size()) + " waypoints, the problem " + std::to_string(N));
    for (const DblVec& row : trajs[b])
    {
      if (row.size() < D)
        throw std::runtime_error("checkTrajectory: a waypoint of trajectory " + std::to_string(b) + " has " +
                                 std::to_string(row.size()) + " values, the group " + std::to_string(D) + " joints");
      x.insert(x.end(), row.begin(), row.begin() + static_cast<long>(D));
    }
  }
  return checkTrajectories(d0, static_cast<int>(probs.size()), scenes, toCheckConfig(config), device, x.data(),
                           nullptr);
}

TrajectoryCheckReport checkTrajectory(const TrajOptProb::Ptr& prob, const TrajArray& traj,
                                      const CollisionCheckConfig& config, int device)
{
  return checkTrajectory(std::vector<TrajOptProb::Ptr>{ prob }, std::vector<TrajArray>{ traj }, config, device)[0];
}
}  // namespace trajopt
