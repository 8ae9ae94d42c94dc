// The continuous collision sets of the trajopt_sqp front end on the device:
// LVSContinuousCollisionEvaluator / LVSDiscreteCollisionEvaluator and the
// fixed-size ContinuousCollisionConstraint (trajopt_ifopt/src/constraints/
// collision/continuous_collision_evaluators.cpp, continuous_collision_constraint.cpp)
// over thip_ccsets_* (csrc/coll_sets_cont.hip).
#include <algorithm>
#include <stdexcept>

#include "trajopt_ifopt/constraints/collision/continuous_collision_constraint.h"
#include "trajopt_ifopt/constraints/collision/continuous_collision_evaluators.h"
#include "trajopt_ifopt/utils/device_set_evaluator.h"

namespace trajopt_ifopt
{
namespace
{
const NodesVariables& variablesOf(const Var& var)
{
  const Node* node = var.getParent();
  const NodesVariables* nv = node ? node->getParent() : nullptr;
  if (!nv)
    throw std::runtime_error("the position Var '" + var.getName() +
                             "' is in no NodesVariables yet: construct the variable set before its constraint sets");
  return *nv;
}

int evaluatorCode(trajopt_common::CollisionEvaluatorType type)
{
  switch (type)
  {
    case trajopt_common::CollisionEvaluatorType::LVS_DISCRETE:
      return THIP_EVALUATOR_LVS_DISCRETE;
    case trajopt_common::CollisionEvaluatorType::CONTINUOUS:
      return THIP_EVALUATOR_CONTINUOUS;
    case trajopt_common::CollisionEvaluatorType::LVS_CONTINUOUS:
      return THIP_EVALUATOR_LVS_CONTINUOUS;
    default:
      return -1;
  }
}
}  // namespace

// ------------------------------------------------------------------ evaluators
DeviceContinuousCollisionEvaluator::DeviceContinuousCollisionEvaluator(
    std::shared_ptr<const trajopt::KinematicGroup> manip, std::shared_ptr<const trajopt::Environment> env,
    const trajopt_common::TrajOptCollisionConfig& collision_config, const char* who)
  : manip_(std::move(manip)), env_(std::move(env)), config_(collision_config), device_(defaultDevice())
{
  if (!manip_ || !env_)
    throw std::runtime_error(std::string(who) + ": null kinematic group or environment");
  int n_spheres = 0;
  for (const auto& cs : env_->collision_spheres)
    n_spheres += manip_->linkIndex(cs.link) > 0 ? 1 : 0;
  if (n_spheres == 0)
    throw std::runtime_error(std::string(who) + ": the environment has no collision spheres on the links of group '" +
                             manip_->name + "': the robot's sphere model is missing");
}

LVSContinuousCollisionEvaluator::LVSContinuousCollisionEvaluator(
    std::shared_ptr<const trajopt::KinematicGroup> manip, std::shared_ptr<const trajopt::Environment> env,
    const trajopt_common::TrajOptCollisionConfig& collision_config)
  : DeviceContinuousCollisionEvaluator(std::move(manip), std::move(env), collision_config,
                                       "LVSContinuousCollisionEvaluator")
{
  if (collision_config.type != trajopt_common::CollisionEvaluatorType::CONTINUOUS &&
      collision_config.type != trajopt_common::CollisionEvaluatorType::LVS_CONTINUOUS)
    throw std::runtime_error("LVSContinuousCollisionEvaluator, should be configured with CONTINUOUS or LVS_CONTINUOUS");
}

LVSDiscreteCollisionEvaluator::LVSDiscreteCollisionEvaluator(std::shared_ptr<const trajopt::KinematicGroup> manip,
                                                             std::shared_ptr<const trajopt::Environment> env,
                                                             const trajopt_common::TrajOptCollisionConfig& collision_config)
  : DeviceContinuousCollisionEvaluator(std::move(manip), std::move(env), collision_config,
                                       "LVSDiscreteCollisionEvaluator")
{
  if (collision_config.type != trajopt_common::CollisionEvaluatorType::LVS_DISCRETE)
    throw std::runtime_error("LVSDiscreteCollisionEvaluator, should be configured with LVS_DISCRETE");
}

DeviceContinuousCollisionEvaluator::~DeviceContinuousCollisionEvaluator()
{
  if (cs_)
    thip_ccsets_destroy(cs_);
}

void DeviceContinuousCollisionEvaluator::lower(thip_problem_desc& d, std::vector<double>& scene) const
{
  lowerCollisionSets(*manip_, *env_, config_, std::max<int>(2, static_cast<int>(vars_.size())), d, scene);
}

void DeviceContinuousCollisionEvaluator::registerSegment(const std::shared_ptr<const Var>& var0,
                                                         const std::shared_ptr<const Var>& var1, bool vars0_fixed,
                                                         bool vars1_fixed, int max_num_cnt)
{
  if (!var0 || !var1)
    throw std::runtime_error("ContinuousCollisionEvaluator: null position variable");
  for (const auto& v : { var0, var1 })
    if (v->size() != manip_->numJoints())
      throw std::runtime_error("ContinuousCollisionConstraint: the position Var has " + std::to_string(v->size()) +
                               " values, the group " + std::to_string(manip_->numJoints()) + " joints");
  if (vars0_fixed && vars1_fixed)
    throw std::runtime_error("ContinuousCollisionConstraint: both ends cannot be fixed!");
  if (max_num_cnt > THIP_CSETS_MAX_ROWS)
    throw std::runtime_error("max_num_cnt " + std::to_string(max_num_cnt) + " exceeds the device's " +
                             std::to_string(THIP_CSETS_MAX_ROWS) + " rows per segment");
  const auto& all = variablesOf(*var0).getVars();
  if (&variablesOf(*var1) != &variablesOf(*var0))
    throw std::runtime_error("ContinuousCollisionConstraint: all vars must belong to the same variable set");
  if (vars_.empty())
    vars_ = all;
  else if (vars_ != all)
    throw std::runtime_error("ContinuousCollisionEvaluator: the constraints of one evaluator must share one "
                             "NodesVariables");
  const int t = varOrdinal(*var0);
  if (varOrdinal(*var1) != t + 1)
    throw std::runtime_error("ContinuousCollisionConstraint: the position Vars '" + var0->getName() + "' and '" +
                             var1->getName() + "' are not consecutive nodes of their NodesVariables");
  for (const auto& s : segments_)
    if (s.t == t && s.fixed != ((vars0_fixed ? 1 : 0) | (vars1_fixed ? 2 : 0)))
      throw std::runtime_error("ContinuousCollisionEvaluator: the segment after '" + var0->getName() +
                               "' is registered twice with different fixed ends");
  if (segments_.empty())
  {
    first_ = t;
    last_ = t + 1;
  }
  first_ = std::min(first_, t);
  last_ = std::max(last_, t + 1);
  Segment s;
  s.var0 = var0;
  s.var1 = var1;
  s.t = t;
  s.fixed = (vars0_fixed ? 1 : 0) | (vars1_fixed ? 2 : 0);
  segments_.push_back(s);
  rows_ = std::max(rows_, max_num_cnt);
  rebuild_ = true;
  valid_ = false;
}

void DeviceContinuousCollisionEvaluator::ensure()
{
  if (!rebuild_)
    return;
  if (cs_)
    thip_ccsets_destroy(cs_);
  cs_ = nullptr;
  auto desc = std::make_unique<thip_problem_desc>();
  std::vector<double> scene;
  lower(*desc, scene);
  thip_ccsets_config cfg{};
  cfg.margin = config_.collision_margin;
  cfg.coeff = config_.collision_coeff;
  cfg.margin_buffer = config_.collision_margin_buffer;
  cfg.max_num_cnt = rows_;
  cfg.first_step = first_;
  cfg.last_step = last_;
  cfg.evaluator_type = evaluatorCode(config_.type);
  cfg.longest_valid_segment_length = config_.longest_valid_segment_length;
  // a segment between registered ones that no constraint asked for runs unfixed: its rows are not read
  std::vector<int> fixed(static_cast<std::size_t>(last_ - first_), 0);
  for (const auto& s : segments_)
    fixed[static_cast<std::size_t>(s.t - first_)] = s.fixed;
  if (thip_ccsets_create(device_, desc.get(), &cfg, fixed.data(), 1, &cs_) != THIP_OK)
    throw std::runtime_error(thip_ccsets_last_error(nullptr));
  if (thip_ccsets_upload(cs_, scene.empty() ? nullptr : scene.data()) != THIP_OK)
    throw std::runtime_error(std::string("thip_ccsets_upload: ") + thip_ccsets_last_error(cs_));
  rebuild_ = false;
  valid_ = false;
}

ContinuousCollisionEvaluator::SegmentRows DeviceContinuousCollisionEvaluator::rows(const Var& var0, const Var& var1)
{
  int t = -1;
  for (const auto& s : segments_)
    if (s.var0.get() == &var0 && s.var1.get() == &var1)
      t = s.t;
  if (t < 0)
    throw std::runtime_error("ContinuousCollisionEvaluator: the segment '" + var0.getName() + "' -> '" +
                             var1.getName() + "' was not registered");
  ensure();
  const std::size_t D = static_cast<std::size_t>(manip_->numJoints()), R = static_cast<std::size_t>(rows_);
  VectorXd x(vars_.size() * D, 0.0);
  for (std::size_t i = 0; i < vars_.size(); ++i)
    if (vars_[i]->value().size() == D)
      std::copy(vars_[i]->value().begin(), vars_[i]->value().end(), x.begin() + static_cast<long>(i * D));
  if (!valid_ || x != x_)
  {
    const std::size_t n = static_cast<std::size_t>(last_ - first_);
    values_.assign(n * R, 0.0);
    jac_.assign(n * R * 2 * D, 0.0);
    coeffs_.assign(n * R, 0.0);
    counts_.assign(n, 0);
    valid_ = false;
    if (thip_ccsets_run(cs_, x.data(), values_.data(), jac_.data(), coeffs_.data(), counts_.data(), nullptr) != THIP_OK)
      throw std::runtime_error(std::string("thip_ccsets_run: ") + thip_ccsets_last_error(cs_));
    ++launches_;
    x_ = std::move(x);
    valid_ = true;
  }
  const std::size_t u = static_cast<std::size_t>(t - first_);
  SegmentRows r;
  r.values = values_.data() + u * R;
  r.jac = jac_.data() + u * R * 2 * D;
  r.coeffs = coeffs_.data() + u * R;
  r.count = counts_[u];
  return r;
}

// ------------------------------------------------------------------ constraint
ContinuousCollisionConstraint::ContinuousCollisionConstraint(
    std::shared_ptr<ContinuousCollisionEvaluator> collision_evaluator,
    std::array<std::shared_ptr<const Var>, 2> position_vars, bool vars0_fixed, bool vars1_fixed, int max_num_cnt,
    bool fixed_sparsity, std::string name)
  : ConstraintSet(std::move(name), max_num_cnt)
  , position_vars_(std::move(position_vars))
  , vars0_fixed_(vars0_fixed)
  , vars1_fixed_(vars1_fixed)
  , collision_evaluator_(std::move(collision_evaluator))
  , fixed_sparsity_(fixed_sparsity)
{
  if (!collision_evaluator_)
    throw std::runtime_error("ContinuousCollisionConstraint: null evaluator");
  // the reference tests `[0] == nullptr && [1] == nullptr` and then reads [0]: either one is refused here
  if (position_vars_[0] == nullptr || position_vars_[1] == nullptr)
    throw std::runtime_error("ContinuousCollisionConstraint: position_vars contains a nullptr!");
  n_dof_ = position_vars_.front()->size();
  if (n_dof_ <= 0)
    throw std::runtime_error("ContinuousCollisionConstraint: first position var is empty!");
  if (position_vars_[0]->size() != position_vars_[1]->size())
    throw std::runtime_error("ContinuousCollisionConstraint: all position_vars must have same size!");
  if (vars0_fixed_ && vars1_fixed_)
    throw std::runtime_error("ContinuousCollisionConstraint: both ends cannot be fixed!");
  if (max_num_cnt < 1)
    throw std::runtime_error("ContinuousCollisionConstraint: max_num_cnt must be greater than zero!");
  // refuses a count beyond the device's rows, Vars of two variable sets or of another joint count
  collision_evaluator_->registerSegment(position_vars_[0], position_vars_[1], vars0_fixed_, vars1_fixed_, max_num_cnt);
  coeffs_.assign(static_cast<std::size_t>(max_num_cnt), 1.0);
  bounds_.assign(static_cast<std::size_t>(max_num_cnt), BoundSmallerZero);
  non_zeros_ = 2 * static_cast<Index>(rows_) * n_dof_;
}

int ContinuousCollisionConstraint::update()
{
  const auto r = collision_evaluator_->rows(*position_vars_[0], *position_vars_[1]);
  // only the rows in use: a row past them keeps its last coefficient (continuous_collision_constraint.cpp:99-101)
  const int cnt = std::min(rows_, r.count);
  for (int i = 0; i < cnt; ++i)
    coeffs_[static_cast<std::size_t>(i)] = r.coeffs[i];
  return rows_;
}

VectorXd ContinuousCollisionConstraint::getValues() const
{
  const auto r = collision_evaluator_->rows(*position_vars_[0], *position_vars_[1]);
  const int cnt = std::min(rows_, r.count);
  VectorXd v(static_cast<std::size_t>(rows_), -collision_evaluator_->getCollisionMarginBuffer());
  for (int i = 0; i < cnt; ++i)
    v[static_cast<std::size_t>(i)] = r.values[i];  // a set without an error at the free end reads -margin_buffer
  return v;
}

Jacobian ContinuousCollisionConstraint::getJacobian() const
{
  Jacobian jac(rows_, variables_ ? variables_->getRows() : variablesOf(*position_vars_[0]).getRows());
  jac.reserve(non_zeros_);
  const auto r = collision_evaluator_->rows(*position_vars_[0], *position_vars_[1]);
  const int cnt = std::min(rows_, r.count);
  // var1 is the node after var0: its columns follow var0's
  for (int i = 0; i < rows_; ++i)
  {
    if (i >= cnt && !fixed_sparsity_)
      break;
    jac.startVec(i);
    for (int e = 0; e < 2; ++e)
    {
      // a fixed end's columns hold no entry of a used row (:196, :216); with fixed_sparsity they hold zeros
      if ((e == 0 ? vars0_fixed_ : vars1_fixed_) && !fixed_sparsity_)
        continue;
      for (Index j = 0; j < n_dof_; ++j)
        jac.insertBack(i, position_vars_[static_cast<std::size_t>(e)]->getIndex() + j) =
            i < cnt ? r.jac[(static_cast<Index>(i) * 2 + e) * n_dof_ + j] : 0.0;
    }
  }
  jac.finalize();
  return jac;
}

void ContinuousCollisionConstraint::setBounds(const std::vector<Bounds>& bounds)
{
  if (bounds.size() != static_cast<std::size_t>(rows_))
    throw std::runtime_error("ContinuousCollisionConstraint::setBounds: " + std::to_string(bounds.size()) +
                             " bounds for " + std::to_string(rows_) + " rows");
  bounds_ = bounds;
}
}  // namespace trajopt_ifopt
