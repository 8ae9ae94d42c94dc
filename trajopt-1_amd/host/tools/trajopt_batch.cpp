// trajopt_batch: solve JSON problems (the reference's TrajOptRequest format)
// as one batch on one MI355X through the C++ front door.
//   trajopt_batch [--device D] [--repeat R] [--check] [--terms] problem.json [problem.json ...]
// Every file is one problem (all must share one structure); --repeat R
// replicates the list R times.  Prints one line per problem.  --check: after
// the solve, each problem's checkTrajectory verdict (a CONTINUOUS check with
// margin 0, as planning_unit.cpp runs it) and clearance, from the trajectories
// on the device.  --terms: one line per problem and term with its name and its
// cost value or constraint violation at the returned trajectory
// (OptResults::cost_vals / cnt_viols).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "trajopt_amd/batch_sqp.hpp"

int main(int argc, char** argv)
{
  int device = 0, repeat = 1;
  bool do_check = false, do_terms = false;
  std::vector<std::string> files;
  for (int i = 1; i < argc; ++i)
  {
    if (!std::strcmp(argv[i], "--device") && i + 1 < argc)
      device = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--repeat") && i + 1 < argc)
      repeat = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--check"))
      do_check = true;
    else if (!std::strcmp(argv[i], "--terms"))
      do_terms = true;
    else
      files.emplace_back(argv[i]);
  }
  if (files.empty() || repeat < 1)
  {
    std::fprintf(stderr, "usage: %s [--device D] [--repeat R] [--check] [--terms] problem.json [...]\n", argv[0]);
    return 2;
  }
  try
  {
    auto env = trajopt::Environment::makePR2();
    std::vector<trajopt::TrajOptProb::Ptr> probs;
    for (int r = 0; r < repeat; ++r)
      for (const auto& f : files)
        probs.push_back(trajopt::ConstructProblem(Json::parseFile(f), env));
    trajopt::BatchTrustRegionSQP opt(probs, device);
    const auto res = opt.optimize();
    for (std::size_t b = 0; b < res.size(); ++b)
      std::printf("problem %zu: %s sqp_iters %d qp_solves %d cost %.9g max_viol %.3g\n", b,
                  sco::toString(res[b].status).c_str(), res[b].n_sqp_iters, res[b].n_qp_solves, res[b].total_cost,
                  res[b].max_cnt_viol);
    std::printf("kernel %.3f ms for %zu problems\n", opt.lastKernelMs(), res.size());
    if (do_terms)
      for (std::size_t b = 0; b < res.size(); ++b)
      {
        const auto& costs = probs[b]->getCosts();
        const auto cnts = probs[b]->getConstraints();
        for (std::size_t i = 0; i < res[b].cost_vals.size() && i < costs.size(); ++i)
          std::printf("problem %zu: cost %s %.12g\n", b, costs[i]->name().c_str(), res[b].cost_vals[i]);
        for (std::size_t i = 0; i < res[b].cnt_viols.size() && i < cnts.size(); ++i)
          std::printf("problem %zu: constraint %s %.12g\n", b, cnts[i]->name().c_str(), res[b].cnt_viols[i]);
      }
    if (do_check)
    {
      // a host-loop batch keeps its trajectories on the host
      std::vector<trajopt::TrajectoryCheckReport> rep;
      if (opt.hostLoops())
      {
        std::vector<trajopt::TrajArray> trajs;
        for (std::size_t b = 0; b < res.size(); ++b)
        {
          const std::size_t N = static_cast<std::size_t>(probs[b]->GetNumSteps()), W = res[b].x.size() / N;
          trajopt::TrajArray t;
          for (std::size_t i = 0; i < N; ++i)
            t.emplace_back(res[b].x.begin() + static_cast<long>(i * W), res[b].x.begin() + static_cast<long>((i + 1) * W));
          trajs.push_back(std::move(t));
        }
        rep = trajopt::checkTrajectory(probs, trajs, trajopt::CollisionCheckConfig(), device);
      }
      else
        rep = opt.checkResults();
      for (std::size_t b = 0; b < rep.size(); ++b)
        std::printf("problem %zu: check %s contacts %d clearance %.9g at step %d link %d other %d\n", b,
                    rep[b].found ? "IN_COLLISION" : "collision_free", rep[b].n_contacts, rep[b].min_distance,
                    rep[b].min_step, rep[b].min_link, rep[b].min_other);
    }
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "trajopt_batch: %s\n", e.what());
    return 1;
  }
  return 0;
}
