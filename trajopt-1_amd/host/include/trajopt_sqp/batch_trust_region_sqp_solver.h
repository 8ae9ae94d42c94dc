// trajopt_sqp::BatchTrustRegionSQPSolver: B TrustRegionSQPSolvers in lock step
// on one device.  Each problem runs an unmodified TrustRegionSQPSolver on a host
// thread over a GpuQPBatch::Slot, so every accept / shrink / penalty decision is
// the single solver's own code and every problem's result is the one it has
// alone; the QPs of a round run as one thip_qp_step per group of problems that
// share a QP pattern (gpu_qp_batch.h).  The sets of a problem (CartPos,
// collision) launch for their own problem from its thread, as they do alone.
#pragma once
#include <string>
#include <vector>

#include "trajopt_hip.h"
#include "trajopt_sqp/gpu_qp_batch.h"
#include "trajopt_sqp/qp_problem.h"
#include "trajopt_sqp/types.h"

namespace trajopt_sqp
{
class BatchTrustRegionSQPSolver
{
public:
  struct Outcome
  {
    SQPStatus status = SQPStatus::kRunning;
    SQPResults results;
    // the slot's counters (GpuQPSolver's) and the rounds it took part in
    int qp_setups = 0, qp_updates = 0, qp_solves = 0, qp_rounds = 0;
    long long admm_iters = 0;
    std::string error;  // not empty: this problem's thread threw; the others finished
  };

  explicit BatchTrustRegionSQPSolver(int device = 0);

  // One SQPParameters per problem, or one for all.  osqp: the slots' OSQP settings,
  // one per problem, one for all, or none (GpuQPSolver::setDefaultOSQPSettings).
  std::vector<Outcome> solve(const std::vector<QPProblem::Ptr>& problems, const std::vector<SQPParameters>& params,
                             const std::vector<thip_osqp_settings>& osqp = {});

  // Host threads of a solve: `workers` when positive, else 64, and never more
  // than the problems (BatchTrustRegionSQP::hostLoopWorkers' cap; not sized by
  // the machine).  A thread takes the next unsolved problem when it finishes one.
  int workers = 0;
  int hostWorkers(std::size_t batch) const;
  // call QPProblem::setup() on the problem's thread before its solve (a set that
  // refuses its configuration there fails that problem alone)
  bool setup_problems = false;

  const GpuQPBatch::Stats& stats() const { return stats_; }

private:
  int device_;
  GpuQPBatch::Stats stats_;
};
}  // namespace trajopt_sqp
