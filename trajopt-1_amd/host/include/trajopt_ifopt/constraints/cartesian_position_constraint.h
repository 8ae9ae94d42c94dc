// trajopt_ifopt::CartPosConstraint (trajopt_ifopt/src/constraints/
// cartesian_position_constraint.cpp): the pose error between a source and a
// target frame of a kinematic group at one node, in its default numeric mode
// (forward differences, eps 1e-5, calcJacobianTransformErrorDiff: :142-169,
// :263-311), evaluated on the device through the CartPose evaluator
// (thip_eval_cart_pose_all) by the DeviceSetEvaluator of the variable set.
//   source active: calcTransformError(target_tf, source_tf)
//   target active: calcTransformError(source_tf, target_tf), the active frame
//                  perturbed either way
// tesseract's JointGroup and LinkId are trajopt::KinematicGroup and link names;
// poses are 3x4 row-major blocks of 12 doubles.  Refused, not dropped:
// use_numeric_differentiation = false (getJacobian throws) and two active
// frames (the constructor throws).
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "trajopt_ifopt/core/constraint_set.h"
#include "trajopt_ifopt/utils/device_set_evaluator.h"

namespace trajopt_ifopt
{
class CartPosConstraint : public ConstraintSet
{
public:
  enum class Type
  {
    kTargetActive,
    kSourceActive,
    kBothActive
  };
  // coefficients of ones and BoundZero on the six components
  CartPosConstraint(std::shared_ptr<const Var> position_var, std::shared_ptr<const trajopt::KinematicGroup> manip,
                    std::string source_frame, std::string target_frame, const Pose12& source_frame_offset = poseIdentity(),
                    const Pose12& target_frame_offset = poseIdentity(), std::string name = "CartPos",
                    RangeBoundHandling range_bound_handling = RangeBoundHandling::kSplitToTwoInequalities);
  // six coefficients and six bounds; a component whose coefficient is zero
  // (almostEqualRelativeAndAbs) has no row, a range bound splits into two
  // inequality rows with kSplitToTwoInequalities (:91-136)
  CartPosConstraint(std::shared_ptr<const Var> position_var, const VectorXd& coeffs, const std::vector<Bounds>& bounds,
                    std::shared_ptr<const trajopt::KinematicGroup> manip, std::string source_frame,
                    std::string target_frame, const Pose12& source_frame_offset = poseIdentity(),
                    const Pose12& target_frame_offset = poseIdentity(), std::string name = "CartPos",
                    RangeBoundHandling range_bound_handling = RangeBoundHandling::kSplitToTwoInequalities);

  int update() override;
  VectorXd getValues() const override;
  Jacobian getJacobian() const override;
  VectorXd getCoefficients() const override { return coeffs_; }
  std::vector<Bounds> getBounds() const override { return bounds_; }

  VectorXd calcValues(const VectorXd& joint_vals) const;
  void calcJacobianBlock(Jacobian& jac_block, const VectorXd& joint_vals) const;
  // the target frame's offset (setTargetPose of the reference); the kept device results are dropped
  void setTargetPose(const Pose12& target_frame_offset);
  Pose12 getTargetPose() const { return target_frame_offset_; }
  // the source frame's world pose at the current variables (numpy-grade host FK)
  Pose12 getCurrentPose() const;
  Type getType() const { return type_; }
  const std::vector<int>& getIndices() const { return indices_; }

  // the analytic path of the reference is not built: update(), getJacobian and calcJacobianBlock throw when false
  bool use_numeric_differentiation{ true };

private:
  Pose12 staticInRoot() const;
  Index n_dof_ = 0;
  std::shared_ptr<const Var> position_var_;
  std::shared_ptr<const trajopt::KinematicGroup> manip_;
  std::string source_frame_, target_frame_;
  Pose12 source_frame_offset_, target_frame_offset_;
  Type type_ = Type::kSourceActive;
  VectorXd coeffs_;
  std::vector<Bounds> bounds_;
  std::vector<int> indices_;  // error component of each row
  std::shared_ptr<DeviceSetEvaluator> evaluator_;
  int slot_ = -1;
};
}  // namespace trajopt_ifopt
