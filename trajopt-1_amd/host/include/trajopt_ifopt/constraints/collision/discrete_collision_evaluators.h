// trajopt_ifopt::SingleTimestepCollisionEvaluator (trajopt_ifopt/src/constraints/
// collision/discrete_collision_evaluators.cpp:36-190) on the device: the contact
// test, the filter, the gradient sets and their order are thip_csets_*'s
// (include/trajopt_hip.h, coll_sets.hip) on the primitive collision model of
// the environment.  One evaluator serves the DiscreteCollisionConstraints of
// every node that names it: they register their Var at construction, and the
// first update() or getValues() at new variable values launches once over all
// those nodes; each constraint reads its node's rows.
// tesseract's JointGroup / Environment are trajopt::KinematicGroup /
// trajopt::Environment.  The LVS and continuous evaluators are in
// continuous_collision_evaluators.h.
#pragma once
#include <memory>
#include <vector>

#include "trajopt_amd/problem_description.hpp"
#include "trajopt_common/collision_types.h"
#include "trajopt_ifopt/variable_sets/nodes_variables.h"

namespace trajopt_ifopt
{
// The descriptor fields thip_csets_create / thip_ccsets_create read, lowered from the
// group, the environment and the config's pair entries (no device call): the
// lowering of every collision evaluator.
void lowerCollisionSets(const trajopt::KinematicGroup& manip, const trajopt::Environment& env,
                        const trajopt_common::TrajOptCollisionConfig& config, int n_steps, thip_problem_desc& desc,
                        std::vector<double>& scene);

class DiscreteCollisionEvaluator
{
public:
  using Ptr = std::shared_ptr<DiscreteCollisionEvaluator>;
  virtual ~DiscreteCollisionEvaluator() = default;
  // one node's rows at the current variables, max_num_cnt of them (thip_csets_run's layout)
  struct NodeRows
  {
    const double* values = nullptr;  // [rows]
    const double* jac = nullptr;     // [rows][n_dof]
    const double* coeffs = nullptr;  // [rows]
    int count = 0;                   // sets before truncation
  };
  // a constraint over `var` with `max_num_cnt` rows will ask for rows(var)
  virtual void registerVar(const std::shared_ptr<const Var>& var, int max_num_cnt) = 0;
  virtual NodeRows rows(const Var& var) = 0;
  virtual double getCollisionMarginBuffer() const = 0;
  // device launches so far
  virtual long long launches() const = 0;
};

class SingleTimestepCollisionEvaluator : public DiscreteCollisionEvaluator
{
public:
  // the HIP device is trajopt_ifopt::defaultDevice() at construction
  SingleTimestepCollisionEvaluator(std::shared_ptr<const trajopt::KinematicGroup> manip,
                                   std::shared_ptr<const trajopt::Environment> env,
                                   const trajopt_common::TrajOptCollisionConfig& collision_config);
  ~SingleTimestepCollisionEvaluator() override;
  SingleTimestepCollisionEvaluator(const SingleTimestepCollisionEvaluator&) = delete;
  SingleTimestepCollisionEvaluator& operator=(const SingleTimestepCollisionEvaluator&) = delete;

  void registerVar(const std::shared_ptr<const Var>& var, int max_num_cnt) override;
  NodeRows rows(const Var& var) override;
  double getCollisionMarginBuffer() const override { return config_.collision_margin_buffer; }
  long long launches() const override { return launches_; }
  // the descriptor fields thip_csets_create reads, lowered from the group, the
  // environment and the config's pair entries (no device call)
  void lower(thip_problem_desc& desc, std::vector<double>& scene) const;

private:
  void ensure();
  std::shared_ptr<const trajopt::KinematicGroup> manip_;
  std::shared_ptr<const trajopt::Environment> env_;
  trajopt_common::TrajOptCollisionConfig config_;
  int device_;
  std::vector<std::shared_ptr<const Var>> nodes_;  // registered Vars
  std::vector<std::shared_ptr<Var>> vars_;         // every Var of their NodesVariables
  int rows_ = 0, first_ = 0, last_ = -1;
  thip_csets* cs_ = nullptr;
  bool rebuild_ = true, valid_ = false;
  VectorXd x_;  // the variables of the kept rows
  std::vector<double> values_, jac_, coeffs_;
  std::vector<int> counts_;
  long long launches_ = 0;
};
}  // namespace trajopt_ifopt
