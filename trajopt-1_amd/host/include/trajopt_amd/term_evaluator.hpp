// Per-term cost values and constraint violations of lowerable problems, for a
// batch, on the device (include/trajopt_hip.h thip_terms_*): what the
// reference's optimizer returns with every result (OptResults::cost_vals /
// cnt_viols, optimizers.cpp:908-909, 976) and TrajOptResult pairs with the
// terms' names (problem_description.hpp:108-125), at any trajectories.
//
//   TrajOptResult r(results, *prob);              reference
//   r.cost_names[i], r.cost_vals[i], r.cnt_names[i], r.cnt_viols[i]
//
//   trajopt::TermEvaluator ev(probs);              here
//   std::vector<trajopt::TrajOptResult> r = ev.evaluate(trajs);
//
// Values are in prob->getCosts() / prob->getConstraints() order (equality
// constraints first), names the term objects' name().
#pragma once
#include <string>
#include <vector>

#include "trajopt_amd/check_trajectory.hpp"
#include "trajopt_amd/problem_description.hpp"

struct thip_terms;

namespace trajopt
{
// problem_description.hpp:108-125
struct TrajOptResult
{
  std::vector<std::string> cost_names, cnt_names;
  DblVec cost_vals, cnt_viols;
  TrajArray traj;
  sco::OptStatus status = sco::INVALID;
};

// Kernel slots -> positions in prob.getCosts() / prob.getConstraints(): built from
// the evaluator's slot table and the record every built-in hatch() leaves with
// its lowered term objects (TrajOptProb::loweredRecords).  A permutation that
// covers every term exactly once, or it throws.
struct TermSlotMap
{
  std::vector<int> cost_pos, cnt_pos;  // slot -> position
  std::vector<std::string> cost_names, cnt_names;  // in position order
};
TermSlotMap termSlotMap(const TrajOptProb& prob, const std::vector<thip_term_slot>& table, int n_costs, int n_cnts);
// The slot table a descriptor gets, without a device (thip_create's numbering
// restated on the host; the evaluator's own table is checked against it)
std::vector<thip_term_slot> termSlotTable(const thip_problem_desc& d, int& n_costs, int& n_cnts);

// Why the batched kernels do not take a problem (empty for a lowerable one): its
// horizon, scene size, time parameterisation, JointAcc form, further collision
// terms, or the names of the terms the fused kernel does not run.
std::string whyNotLowerable(const TrajOptProb& prob);

class TermEvaluator
{
public:
  // The problems share one structure (as a BatchTrustRegionSQP batch) and are
  // lowerable; anything else throws with a message naming the host loop, where
  // Cost::value / Constraint::violation answer.
  explicit TermEvaluator(const std::vector<TrajOptProb::Ptr>& probs, int device = 0);
  // Without term objects: values in slot order, names from the slot table
  explicit TermEvaluator(const std::vector<LoweredProblem>& probs, int device = 0);
  ~TermEvaluator();
  TermEvaluator(const TermEvaluator&) = delete;
  TermEvaluator& operator=(const TermEvaluator&) = delete;

  int batch() const { return batch_; }
  int numCosts() const { return n_costs_; }
  int numConstraints() const { return n_cnts_; }
  const std::vector<thip_term_slot>& slots() const { return table_; }
  // per-problem data of another batch of the same structure
  void upload(const std::vector<LoweredProblem>& probs);
  // one result per problem (status stays INVALID: nothing was optimised)
  std::vector<TrajOptResult> evaluate(const std::vector<TrajArray>& trajs);
  // trajectories [batch][n_steps][n_dof] already on the device (thip_device_x)
  std::vector<TrajOptResult> evaluateDevice(const double* d_x);
  double lastKernelMs() const;

private:
  void create(const thip_problem_desc& d, int device);
  std::vector<TrajOptResult> collect(const std::vector<double>& costs, const std::vector<double>& viols) const;
  thip_terms* t_ = nullptr;
  int batch_ = 0, n_costs_ = 0, n_cnts_ = 0, n_steps_ = 0, n_dof_ = 0;
  std::vector<thip_term_slot> table_;
  std::vector<TermSlotMap> maps_;  // per problem (empty without term objects)
};
}  // namespace trajopt
