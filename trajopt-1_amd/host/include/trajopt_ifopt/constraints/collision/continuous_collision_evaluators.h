// trajopt_ifopt::LVSContinuousCollisionEvaluator and LVSDiscreteCollisionEvaluator
// (trajopt_ifopt/src/constraints/collision/continuous_collision_evaluators.cpp:
// 36-458) on the device: the sub-states, the contact test, the filter, the
// gradient sets, their per-end maxima and their order are thip_ccsets_*'s
// (include/trajopt_hip.h, coll_sets_cont.hip) on the primitive collision model
// of the environment.  As with SingleTimestepCollisionEvaluator one evaluator
// may serve the ContinuousCollisionConstraints of many segments: they register
// their two Vars at construction, and the first update() or getValues() at new
// variable values launches once over all those segments.  One evaluator per
// segment, as the reference's tests build them, works too and costs one launch
// per segment.
#pragma once
#include <memory>
#include <vector>

#include "trajopt_ifopt/constraints/collision/discrete_collision_evaluators.h"

namespace trajopt_ifopt
{
class ContinuousCollisionEvaluator
{
public:
  using Ptr = std::shared_ptr<ContinuousCollisionEvaluator>;
  virtual ~ContinuousCollisionEvaluator() = default;
  // one segment's rows at the current variables, max_num_cnt of them (thip_ccsets_run's layout)
  struct SegmentRows
  {
    const double* values = nullptr;  // [rows]
    const double* jac = nullptr;     // [rows][2][n_dof]: end 0 = var0, end 1 = var1
    const double* coeffs = nullptr;  // [rows]
    int count = 0;                   // sets before truncation
  };
  // a constraint over the segment (var0, var1) with `max_num_cnt` rows will ask for rows(var0, var1);
  // var1 is the node after var0 in their NodesVariables
  virtual void registerSegment(const std::shared_ptr<const Var>& var0, const std::shared_ptr<const Var>& var1,
                               bool vars0_fixed, bool vars1_fixed, int max_num_cnt) = 0;
  virtual SegmentRows rows(const Var& var0, const Var& var1) = 0;
  virtual double getCollisionMarginBuffer() const = 0;
  // device launches so far
  virtual long long launches() const = 0;
};

// the device evaluator behind both classes below: they differ in the evaluator types they accept
class DeviceContinuousCollisionEvaluator : public ContinuousCollisionEvaluator
{
public:
  ~DeviceContinuousCollisionEvaluator() override;
  DeviceContinuousCollisionEvaluator(const DeviceContinuousCollisionEvaluator&) = delete;
  DeviceContinuousCollisionEvaluator& operator=(const DeviceContinuousCollisionEvaluator&) = delete;

  void registerSegment(const std::shared_ptr<const Var>& var0, const std::shared_ptr<const Var>& var1,
                       bool vars0_fixed, bool vars1_fixed, int max_num_cnt) override;
  SegmentRows rows(const Var& var0, const Var& var1) override;
  double getCollisionMarginBuffer() const override { return config_.collision_margin_buffer; }
  long long launches() const override { return launches_; }
  // the descriptor fields thip_ccsets_create reads (lowerCollisionSets; no device call)
  void lower(thip_problem_desc& desc, std::vector<double>& scene) const;

protected:
  // the HIP device is trajopt_ifopt::defaultDevice() at construction
  DeviceContinuousCollisionEvaluator(std::shared_ptr<const trajopt::KinematicGroup> manip,
                                     std::shared_ptr<const trajopt::Environment> env,
                                     const trajopt_common::TrajOptCollisionConfig& collision_config, const char* who);

private:
  void ensure();
  std::shared_ptr<const trajopt::KinematicGroup> manip_;
  std::shared_ptr<const trajopt::Environment> env_;
  trajopt_common::TrajOptCollisionConfig config_;
  int device_;
  struct Segment
  {
    std::shared_ptr<const Var> var0, var1;
    int t = 0, fixed = 0;  // var0's node; bit 0 vars0 fixed, bit 1 vars1 fixed
  };
  std::vector<Segment> segments_;
  std::vector<std::shared_ptr<Var>> vars_;  // every Var of their NodesVariables
  int rows_ = 0, first_ = 0, last_ = 0;     // nodes first_ .. last_: segments first_ .. last_ - 1
  thip_ccsets* cs_ = nullptr;
  bool rebuild_ = true, valid_ = false;
  VectorXd x_;  // the variables of the kept rows
  std::vector<double> values_, jac_, coeffs_;
  std::vector<int> counts_;
  long long launches_ = 0;
};

class LVSContinuousCollisionEvaluator : public DeviceContinuousCollisionEvaluator
{
public:
  // CONTINUOUS (one cast per segment) or LVS_CONTINUOUS
  LVSContinuousCollisionEvaluator(std::shared_ptr<const trajopt::KinematicGroup> manip,
                                  std::shared_ptr<const trajopt::Environment> env,
                                  const trajopt_common::TrajOptCollisionConfig& collision_config);
};

class LVSDiscreteCollisionEvaluator : public DeviceContinuousCollisionEvaluator
{
public:
  // LVS_DISCRETE
  LVSDiscreteCollisionEvaluator(std::shared_ptr<const trajopt::KinematicGroup> manip,
                                std::shared_ptr<const trajopt::Environment> env,
                                const trajopt_common::TrajOptCollisionConfig& collision_config);
};
}  // namespace trajopt_ifopt
