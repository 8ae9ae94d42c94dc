// trajopt_ifopt::ContinuousCollisionConstraint, the fixed-size set (trajopt_ifopt/
// src/constraints/collision/continuous_collision_constraint.cpp:43-248):
// max_num_cnt rows with BoundSmallerZero on the segment between two nodes, row i
// the i-th gradient set of the evaluator (value = its maximum error at the free
// ends, jacobian = minus its weighted average gradients at var0 and at var1, a
// fixed end's columns left out), unused rows at -margin_buffer with a zero
// jacobian.  update() overwrites only the first min(max_num_cnt, sets)
// coefficients (:99-101).  With fixed_sparsity getJacobian holds all
// 2 x max_num_cnt x n_dof entries, zeros included: the QP's pattern never
// changes.  ContinuousCollisionConstraintD and the numerical variants are not
// built: a changing row count would change the resident QP's pattern.
#pragma once
#include <array>
#include <memory>
#include <string>
#include <vector>

#include "trajopt_ifopt/constraints/collision/continuous_collision_evaluators.h"
#include "trajopt_ifopt/core/constraint_set.h"

namespace trajopt_ifopt
{
class ContinuousCollisionConstraint : public ConstraintSet
{
public:
  ContinuousCollisionConstraint(std::shared_ptr<ContinuousCollisionEvaluator> collision_evaluator,
                                std::array<std::shared_ptr<const Var>, 2> position_vars, bool vars0_fixed,
                                bool vars1_fixed, int max_num_cnt = 1, bool fixed_sparsity = false,
                                std::string name = "LVSCollision");
  int update() override;
  VectorXd getValues() const override;
  Jacobian getJacobian() const override;
  VectorXd getCoefficients() const override { return coeffs_; }
  std::vector<Bounds> getBounds() const override { return bounds_; }
  void setBounds(const std::vector<Bounds>& bounds);
  std::shared_ptr<ContinuousCollisionEvaluator> getCollisionEvaluator() const { return collision_evaluator_; }

private:
  Index n_dof_ = 0;
  std::array<std::shared_ptr<const Var>, 2> position_vars_;
  bool vars0_fixed_, vars1_fixed_;
  std::shared_ptr<ContinuousCollisionEvaluator> collision_evaluator_;
  bool fixed_sparsity_;
  VectorXd coeffs_;
  std::vector<Bounds> bounds_;
};
}  // namespace trajopt_ifopt
