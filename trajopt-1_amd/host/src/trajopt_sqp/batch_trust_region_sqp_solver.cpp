// trajopt_sqp::BatchTrustRegionSQPSolver (batch_trust_region_sqp_solver.h).
#include "trajopt_sqp/batch_trust_region_sqp_solver.h"

#include <algorithm>
#include <atomic>
#include <stdexcept>
#include <thread>

#include "trajopt_sqp/trust_region_sqp_solver.h"

namespace trajopt_sqp
{
BatchTrustRegionSQPSolver::BatchTrustRegionSQPSolver(int device) : device_(device) {}

int BatchTrustRegionSQPSolver::hostWorkers(std::size_t batch) const
{
  const int want = workers > 0 ? workers : 64;
  return std::max(1, std::min(want, static_cast<int>(batch)));
}

std::vector<BatchTrustRegionSQPSolver::Outcome>
BatchTrustRegionSQPSolver::solve(const std::vector<QPProblem::Ptr>& problems, const std::vector<SQPParameters>& params,
                                 const std::vector<thip_osqp_settings>& osqp)
{
  const std::size_t B = problems.size();
  if (B == 0)
    throw std::runtime_error("BatchTrustRegionSQPSolver: empty batch");
  if (params.size() != 1 && params.size() != B)
    throw std::runtime_error("BatchTrustRegionSQPSolver: one SQPParameters per problem, or one for all");
  if (!osqp.empty() && osqp.size() != 1 && osqp.size() != B)
    throw std::runtime_error("BatchTrustRegionSQPSolver: one thip_osqp_settings per problem, one for all, or none");
  for (std::size_t b = 0; b < B; ++b)
    if (!problems[b])
      throw std::runtime_error("BatchTrustRegionSQPSolver: problem " + std::to_string(b) + " is null");
  const std::size_t W = static_cast<std::size_t>(hostWorkers(B));
  auto batch = std::make_shared<GpuQPBatch>(device_);
  std::vector<Outcome> out(B);
  // every worker is a client of the rendezvous before any thread starts, so the
  // first round holds every worker's QP; a worker leaves when no problem is left
  for (std::size_t w = 0; w < W; ++w)
    batch->enter();
  std::atomic<std::size_t> next{ 0 };
  std::vector<std::thread> threads;
  threads.reserve(W);
  for (std::size_t w = 0; w < W; ++w)
    threads.emplace_back([&]() {
      for (std::size_t b = next++; b < B; b = next++)
      {
        Outcome& o = out[b];
        std::shared_ptr<GpuQPBatch::Slot> slot;
        try
        {
          slot = batch->makeSlot();
          if (!osqp.empty())
            slot->settings = osqp[osqp.size() == 1 ? 0 : b];
          if (setup_problems)
            problems[b]->setup();
          TrustRegionSQPSolver solver(slot);
          solver.params = params[params.size() == 1 ? 0 : b];
          solver.solve(problems[b]);
          o.status = solver.getStatus();
          o.results = solver.getResults();
        }
        catch (const std::exception& e)
        {
          o.error = e.what();
          if (o.error.empty())
            o.error = "unknown error";
        }
        if (slot)
        {
          o.qp_setups = slot->n_setups;
          o.qp_updates = slot->n_updates;
          o.qp_solves = slot->n_solves;
          o.qp_rounds = slot->n_rounds;
          o.admm_iters = slot->admm_iters;
        }
      }
      batch->leave();  // the others' rounds no longer wait for this worker
    });
  for (auto& t : threads)
    t.join();
  stats_ = batch->stats();
  return out;
}
}  // namespace trajopt_sqp
