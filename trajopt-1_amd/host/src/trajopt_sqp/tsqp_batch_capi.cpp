// thost_tsqp_solve_batch (include/trajopt_host.h): the problems of
// thost_tsqp_solve / thost_tsqp_solve_kin, built by the same builders
// (tsqp_build.h), solved in lock step by trajopt_sqp::BatchTrustRegionSQPSolver.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "trajopt_host.h"
#include "trajopt_sqp/batch_trust_region_sqp_solver.h"
#include "tsqp_build.h"

extern "C" {

int thost_tsqp_solve_batch(const tsqp_spec* specs, const tsqp_kin_spec* kins, int batch, int device, double* x,
                           tsqp_result* results, int* qp_rounds, tsqp_batch_stats* stats, char* err, int err_len)
{
  using namespace trajopt_sqp;
  const char* who = "thost_tsqp_solve_batch";
  std::string failed;
  try
  {
    if (batch < 1)
      throw std::runtime_error(std::string(who) + ": batch must be at least 1");
    if (!specs || !x || !results)
      throw std::runtime_error(std::string(who) + ": null argument (specs, x and results are required)");
    const std::size_t B = static_cast<std::size_t>(batch);
    if (stats)
      std::memset(stats, 0, sizeof(*stats));
    std::memset(results, 0, sizeof(*results) * B);
    if (qp_rounds)
      std::fill(qp_rounds, qp_rounds + B, 0);
    std::vector<capi::KinProblem> built(B);
    std::vector<std::string> errors(B);
    std::vector<QPProblem::Ptr> problems;
    std::vector<SQPParameters> params;
    std::vector<thip_osqp_settings> osqp;
    std::vector<std::size_t> index;  // problems[k] is problem index[k] of the call
    for (std::size_t b = 0; b < B; ++b)
    {
      try
      {
        if (kins)
          built[b] = capi::buildKinProblem(&specs[b], &kins[b], device, who);
        else
          built[b].joint = capi::buildJointProblem(&specs[b], who);
        problems.push_back(built[b].joint.problem);
        params.push_back(capi::paramsOf(&specs[b]));
        osqp.push_back(specs[b].osqp);
        index.push_back(b);
      }
      catch (const std::exception& e)
      {
        errors[b] = e.what();
      }
    }
    BatchTrustRegionSQPSolver solver(device);
    solver.setup_problems = true;  // a set that refuses its configuration does so there, for its problem alone
    std::vector<BatchTrustRegionSQPSolver::Outcome> out;
    if (!problems.empty())
      out = solver.solve(problems, params, osqp);
    const std::size_t stride = static_cast<std::size_t>(TSQP_MAX_NODES) * THIP_MAX_DOF;
    for (std::size_t k = 0; k < out.size(); ++k)
    {
      const std::size_t b = index[k];
      const BatchTrustRegionSQPSolver::Outcome& o = out[k];
      tsqp_result& r = results[b];
      r.qp_setups = o.qp_setups;
      r.qp_updates = o.qp_updates;
      r.qp_solves = o.qp_solves;
      r.admm_iters = o.admm_iters;
      if (qp_rounds)
        qp_rounds[b] = o.qp_rounds;
      if (!o.error.empty())
      {
        errors[b] = o.error;
        continue;
      }
      const trajopt_ifopt::VectorXd xv = problems[k]->getVariableValues();
      std::memcpy(x + b * stride, xv.data(), sizeof(double) * xv.size());
      r.status = static_cast<int>(o.status);
      r.overall_iteration = o.results.overall_iteration;
      r.penalty_iteration = o.results.penalty_iteration;
      r.best_exact_merit = o.results.best_exact_merit;
    }
    if (stats)
    {
      const GpuQPBatch::Stats& s = solver.stats();
      stats->rounds = s.rounds;
      stats->step_launches = s.step_launches;
      stats->groups = s.groups;
      stats->max_group = s.max_group;
      for (std::size_t b = 0; b < B; ++b)
        if (built[b].set_launches)
        {
          long long l[2] = { 0, 0 };
          built[b].set_launches(l);
          stats->set_launches[0] += l[0];
          stats->set_launches[1] += l[1];
        }
    }
    for (std::size_t b = 0; b < B; ++b)
      if (!errors[b].empty())
      {
        results[b].status = -1;
        failed += (failed.empty() ? "" : "\n") + std::string("problem ") + std::to_string(b) + ": " + errors[b];
      }
  }
  catch (const std::exception& e)
  {
    failed = e.what();
  }
  if (failed.empty())
    return 0;
  if (err && err_len > 0)
    std::snprintf(err, static_cast<std::size_t>(err_len), "%s", failed.c_str());
  return -1;
}

int thost_tsqp_sizeof_batch_stats(void) { return static_cast<int>(sizeof(tsqp_batch_stats)); }
}  // extern "C"
