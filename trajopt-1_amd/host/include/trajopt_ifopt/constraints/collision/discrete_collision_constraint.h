// trajopt_ifopt::DiscreteCollisionConstraint, the fixed-size set (trajopt_ifopt/
// src/constraints/collision/discrete_collision_constraint.cpp:45-158):
// max_num_cnt rows with BoundSmallerZero at one node, row i the i-th gradient
// set of the evaluator (value = its error, jacobian = minus its weighted average
// gradient), unused rows at -margin_buffer with a zero jacobian.  update()
// overwrites only the first min(max_num_cnt, sets) coefficients (:82-84), so a
// row that falls out of use keeps the coefficient it last had, as in the
// reference.  With fixed_sparsity getJacobian holds all max_num_cnt x n_dof
// entries, zeros included: the QP's pattern never changes.
// DiscreteCollisionConstraintD is not built.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "trajopt_ifopt/constraints/collision/discrete_collision_evaluators.h"
#include "trajopt_ifopt/core/constraint_set.h"

namespace trajopt_ifopt
{
class DiscreteCollisionConstraint : public ConstraintSet
{
public:
  DiscreteCollisionConstraint(std::shared_ptr<DiscreteCollisionEvaluator> collision_evaluator,
                              std::shared_ptr<const Var> position_var, int max_num_cnt = 1, bool fixed_sparsity = false,
                              std::string name = "DiscreteCollision");
  int update() override;
  VectorXd getValues() const override;
  Jacobian getJacobian() const override;
  VectorXd getCoefficients() const override { return coeffs_; }
  std::vector<Bounds> getBounds() const override { return bounds_; }
  void setBounds(const std::vector<Bounds>& bounds);
  std::shared_ptr<DiscreteCollisionEvaluator> getCollisionEvaluator() const { return collision_evaluator_; }

private:
  Index n_dof_ = 0;
  std::shared_ptr<const Var> position_var_;
  std::shared_ptr<DiscreteCollisionEvaluator> collision_evaluator_;
  bool fixed_sparsity_;
  VectorXd coeffs_;
  std::vector<Bounds> bounds_;
};
}  // namespace trajopt_ifopt
