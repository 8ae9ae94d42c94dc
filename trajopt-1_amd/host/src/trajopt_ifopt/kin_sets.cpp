// The kinematic sets of the trajopt_sqp front end on the device: the shared
// evaluator of a variable set (device_set_evaluator.h), CartPosConstraint
// (trajopt_ifopt/src/constraints/cartesian_position_constraint.cpp),
// SingleTimestepCollisionEvaluator and the fixed-size
// DiscreteCollisionConstraint (src/constraints/collision/
// discrete_collision_evaluators.cpp, discrete_collision_constraint.cpp).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>

#include "trajopt_ifopt/constraints/cartesian_position_constraint.h"
#include "trajopt_ifopt/constraints/collision/discrete_collision_constraint.h"
#include "trajopt_ifopt/constraints/collision/discrete_collision_evaluators.h"
#include "trajopt_ifopt/utils/device_set_evaluator.h"

namespace trajopt_ifopt
{
// ------------------------------------------------------------------ poses
Pose12 poseIdentity() { return Pose12{ { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 } }; }

Pose12 poseMul(const Pose12& a, const Pose12& b)
{
  Pose12 o{};
  for (std::size_t r = 0; r < 3; ++r)
  {
    for (std::size_t c = 0; c < 3; ++c)
      o[r * 4 + c] = a[r * 4 + 0] * b[0 * 4 + c] + a[r * 4 + 1] * b[1 * 4 + c] + a[r * 4 + 2] * b[2 * 4 + c];
    o[r * 4 + 3] = a[r * 4 + 0] * b[3] + a[r * 4 + 1] * b[7] + a[r * 4 + 2] * b[11] + a[r * 4 + 3];
  }
  return o;
}

Pose12 poseInv(const Pose12& a)
{
  Pose12 o{};
  for (std::size_t r = 0; r < 3; ++r)
    for (std::size_t c = 0; c < 3; ++c)
      o[r * 4 + c] = a[c * 4 + r];
  for (std::size_t r = 0; r < 3; ++r)
    o[r * 4 + 3] = -(o[r * 4 + 0] * a[3] + o[r * 4 + 1] * a[7] + o[r * 4 + 2] * a[11]);
  return o;
}

namespace
{
std::atomic<int> g_default_device{ 0 };

Pose12 poseOf(const double* p)
{
  Pose12 o;
  std::copy(p, p + 12, o.begin());
  return o;
}

// world pose of chain link `link` at joint values q (the arithmetic of kin_device.hpp's chain_fk)
Pose12 hostFk(const thip_chain& ch, const VectorXd& q, int link)
{
  std::vector<int> path;
  for (int k = link; k > 0; k = ch.is_tree ? ch.parent[k] : k - 1)
    path.insert(path.begin(), k);
  Pose12 T = poseOf(ch.base_pose);
  for (const int k : path)
  {
    T = poseMul(T, poseOf(ch.joint_origin[k]));
    const int type = ch.joint_type[k];
    if (type == THIP_JOINT_FIXED)
      continue;
    const double v = q[static_cast<std::size_t>(ch.joint_dof[k])];
    const double* ax = ch.joint_axis[k];
    Pose12 M = poseIdentity();
    if (type == THIP_JOINT_PRISMATIC)
    {
      M[3] = ax[0] * v;
      M[7] = ax[1] * v;
      M[11] = ax[2] * v;
    }
    else
    {
      // Eigen AngleAxis::toRotationMatrix
      const double s = std::sin(v), c = std::cos(v);
      const double sa0 = s * ax[0], sa1 = s * ax[1], sa2 = s * ax[2];
      const double ca0 = (1 - c) * ax[0], ca1 = (1 - c) * ax[1], ca2 = (1 - c) * ax[2];
      double tmp = ca0 * ax[1];
      M[1] = tmp - sa2;
      M[4] = tmp + sa2;
      tmp = ca0 * ax[2];
      M[2] = tmp + sa1;
      M[8] = tmp - sa1;
      tmp = ca1 * ax[2];
      M[6] = tmp - sa0;
      M[9] = tmp + sa0;
      M[0] = ca0 * ax[0] + c;
      M[5] = ca1 * ax[1] + c;
      M[10] = ca2 * ax[2] + c;
    }
    T = poseMul(T, M);
  }
  return T;
}

const NodesVariables& variablesOf(const Var& var)
{
  const Node* node = var.getParent();
  const NodesVariables* nv = node ? node->getParent() : nullptr;
  if (!nv)
    throw std::runtime_error("the position Var '" + var.getName() +
                             "' is in no NodesVariables yet: construct the variable set before its constraint sets");
  return *nv;
}

// tesseract::common::almostEqualRelativeAndAbs(a, b) with its defaults (max_diff 1e-6, max_rel_diff epsilon)
bool almostEqualRelativeAndAbs(double a, double b)
{
  const double diff = std::fabs(a - b);
  if (diff <= 1e-6)
    return true;
  return diff <= std::max(std::fabs(a), std::fabs(b)) * std::numeric_limits<double>::epsilon();
}
}  // namespace

void setDefaultDevice(int device) { g_default_device.store(device); }
int defaultDevice() { return g_default_device.load(); }

int varOrdinal(const Var& var)
{
  const auto& vars = variablesOf(var).getVars();
  for (std::size_t k = 0; k < vars.size(); ++k)
    if (vars[k].get() == &var)
      return static_cast<int>(k);
  throw std::runtime_error("the position Var '" + var.getName() + "' is not in its NodesVariables");
}

// ------------------------------------------------------------------ shared evaluator
std::shared_ptr<DeviceSetEvaluator> DeviceSetEvaluator::of(const Var& var,
                                                           const trajopt::KinematicGroup::ConstPtr& manip, int device)
{
  const NodesVariables& nv = variablesOf(var);
  std::shared_ptr<void>& slot = nv.attachment(device, manip.get());
  if (!slot)
    slot = std::shared_ptr<DeviceSetEvaluator>(new DeviceSetEvaluator(nv.getVars(), manip, device));
  return std::static_pointer_cast<DeviceSetEvaluator>(slot);
}

DeviceSetEvaluator::DeviceSetEvaluator(std::vector<std::shared_ptr<Var>> vars, trajopt::KinematicGroup::ConstPtr manip,
                                       int device)
  : vars_(std::move(vars)), manip_(std::move(manip)), device_(device)
{
  if (vars_.size() > static_cast<std::size_t>(THIP_EVAL_MAX_STEPS))
    throw std::runtime_error("DeviceSetEvaluator: more than " + std::to_string(THIP_EVAL_MAX_STEPS) + " Vars");
}

DeviceSetEvaluator::~DeviceSetEvaluator()
{
  if (ev_)
    thip_eval_destroy(ev_);
}

int DeviceSetEvaluator::addCartPos(const Var& var, int active_link, const Pose12& active_offset,
                                   const Pose12& static_in_root)
{
  if (terms_.size() >= static_cast<std::size_t>(THIP_MAX_CART))
    throw std::runtime_error("more than " + std::to_string(THIP_MAX_CART) + " CartPos sets over one NodesVariables");
  if (var.size() != manip_->numJoints())
    throw std::runtime_error("CartPosConstraint: the position Var has " + std::to_string(var.size()) +
                             " values, the group " + std::to_string(manip_->numJoints()) + " joints");
  int step = -1;
  for (std::size_t k = 0; k < vars_.size(); ++k)
    if (vars_[k].get() == &var)
      step = static_cast<int>(k);
  if (step < 0)
    throw std::runtime_error("CartPosConstraint: the position Var is not in the evaluator's NodesVariables");
  terms_.push_back({ step, active_link, active_offset, static_in_root });
  rebuild_ = true;
  valid_ = false;
  return static_cast<int>(terms_.size()) - 1;
}

void DeviceSetEvaluator::updateCartPos(int slot, const Pose12& active_offset, const Pose12& static_in_root)
{
  Term& t = terms_.at(static_cast<std::size_t>(slot));
  if (t.offset != active_offset)
    rebuild_ = true;
  t.offset = active_offset;
  t.target = static_in_root;
  reupload_ = true;
  valid_ = false;
}

void DeviceSetEvaluator::ensure()
{
  if (rebuild_)
  {
    if (ev_)
      thip_eval_destroy(ev_);
    ev_ = nullptr;
    auto desc = std::make_unique<thip_problem_desc>();
    std::memset(desc.get(), 0, sizeof(thip_problem_desc));
    desc->abi_version = THIP_ABI_VERSION;
    desc->n_steps = static_cast<int>(vars_.size());
    desc->chain = manip_->chain;
    desc->n_cart = static_cast<int>(terms_.size());
    for (std::size_t k = 0; k < terms_.size(); ++k)
    {
      desc->cart_step[k] = terms_[k].step;
      desc->cart_is_cnt[k] = 1;
      desc->cart_source_link[k] = terms_[k].link;
      std::copy(terms_[k].offset.begin(), terms_[k].offset.end(), desc->cart_source_offset[k]);
      for (int i = 0; i < 3; ++i)
        desc->cart_pos_coeffs[k][i] = desc->cart_rot_coeffs[k][i] = 1.0;
    }
    if (thip_eval_create(device_, desc.get(), 1, &ev_) != THIP_OK)
      throw std::runtime_error(std::string("thip_eval_create: ") + thip_eval_last_error(nullptr));
    rebuild_ = false;
    reupload_ = true;
  }
  if (reupload_)
  {
    std::vector<double> tg;
    for (const Term& t : terms_)
      tg.insert(tg.end(), t.target.begin(), t.target.end());
    if (thip_eval_upload(ev_, tg.data(), nullptr) != THIP_OK)
      throw std::runtime_error(std::string("thip_eval_upload: ") + thip_eval_last_error(ev_));
    reupload_ = false;
    valid_ = false;
  }
}

VectorXd DeviceSetEvaluator::gather() const
{
  // [n_vars][n_dof]; a Var of another size (not a joint position) reads as zeros
  const std::size_t D = static_cast<std::size_t>(manip_->numJoints());
  VectorXd x(vars_.size() * D, 0.0);
  for (std::size_t k = 0; k < vars_.size(); ++k)
    if (vars_[k]->value().size() == D)
      std::copy(vars_[k]->value().begin(), vars_[k]->value().end(), x.begin() + static_cast<long>(k * D));
  return x;
}

void DeviceSetEvaluator::prefetch()
{
  if (terms_.empty())
    return;
  ensure();
  VectorXd x = gather();
  if (valid_ && x == x_)
    return;
  const std::size_t n = terms_.size(), D = static_cast<std::size_t>(manip_->numJoints());
  err_.assign(n * 6, 0.0);
  jac_.assign(n * 6 * D, 0.0);
  if (thip_eval_cart_pose_all(ev_, x.data(), err_.data(), jac_.data()) != THIP_OK)
    throw std::runtime_error(std::string("thip_eval_cart_pose_all: ") + thip_eval_last_error(ev_));
  ++launches_;
  x_ = std::move(x);
  valid_ = true;
}

void DeviceSetEvaluator::cartPos(int slot, const VectorXd& q, double* err, double* jac)
{
  const Term& t = terms_.at(static_cast<std::size_t>(slot));
  const std::size_t D = static_cast<std::size_t>(manip_->numJoints()), s = static_cast<std::size_t>(slot);
  if (q.size() != D)
    throw std::runtime_error("CartPosConstraint: " + std::to_string(q.size()) + " joint values for " +
                             std::to_string(D) + " joints");
  if (q == vars_[static_cast<std::size_t>(t.step)]->value())
  {
    prefetch();
    std::copy(err_.begin() + static_cast<long>(s * 6), err_.begin() + static_cast<long>(s * 6 + 6), err);
    if (jac)
      std::copy(jac_.begin() + static_cast<long>(s * 6 * D), jac_.begin() + static_cast<long>((s + 1) * 6 * D), jac);
    return;
  }
  // not the variables' values: a launch for this set alone; the kept results stay the variables'
  ensure();
  if (thip_eval_cart_pose(ev_, slot, q.data(), err, jac) != THIP_OK)
    throw std::runtime_error(std::string("thip_eval_cart_pose: ") + thip_eval_last_error(ev_));
  ++launches_;
}

// ------------------------------------------------------------------ CartPos
CartPosConstraint::CartPosConstraint(std::shared_ptr<const Var> position_var,
                                     std::shared_ptr<const trajopt::KinematicGroup> manip, std::string source_frame,
                                     std::string target_frame, const Pose12& source_frame_offset,
                                     const Pose12& target_frame_offset, std::string name,
                                     RangeBoundHandling range_bound_handling)
  : CartPosConstraint(std::move(position_var), VectorXd(6, 1.0), std::vector<Bounds>(6, BoundZero), std::move(manip),
                      std::move(source_frame), std::move(target_frame), source_frame_offset, target_frame_offset,
                      std::move(name), range_bound_handling)
{
}

CartPosConstraint::CartPosConstraint(std::shared_ptr<const Var> position_var, const VectorXd& coeffs,
                                     const std::vector<Bounds>& bounds,
                                     std::shared_ptr<const trajopt::KinematicGroup> manip, std::string source_frame,
                                     std::string target_frame, const Pose12& source_frame_offset,
                                     const Pose12& target_frame_offset, std::string name,
                                     RangeBoundHandling range_bound_handling)
  : ConstraintSet(std::move(name), 6)
  , position_var_(std::move(position_var))
  , manip_(std::move(manip))
  , source_frame_(std::move(source_frame))
  , target_frame_(std::move(target_frame))
  , source_frame_offset_(source_frame_offset)
  , target_frame_offset_(target_frame_offset)
{
  if (!position_var_ || !manip_)
    throw std::runtime_error("CartPosConstraint: null position variable or kinematic group");
  n_dof_ = manip_->numJoints();
  if (!manip_->hasLinkId(source_frame_))
    throw std::runtime_error("Source Link name '" + source_frame_ + "' provided does not exist.");
  if (!manip_->hasLinkId(target_frame_))
    throw std::runtime_error("Target Link name '" + target_frame_ + "' provided does not exist.");
  if (bounds.size() != 6)
    throw std::runtime_error("The number of bounds should be six.");
  if (coeffs.size() != 6)
    throw std::runtime_error("The number of coeffs should be six.");
  const bool target_active = manip_->isActiveLinkId(target_frame_);
  const bool source_active = manip_->isActiveLinkId(source_frame_);
  if (target_active && source_active)
    // kBothActive differences the error with calcJacobianTransformErrorDiff's four-argument form
    // (cartesian_position_constraint.cpp:223, "different from legacy kinematic_terms"), which the
    // CartPose device evaluator's dynamic term is not
    throw std::runtime_error("CartPosConstraint: source '" + source_frame_ + "' and target '" + target_frame_ +
                             "' are both active links (kBothActive); its error difference differs from the "
                             "dynamic CartPose term the device evaluates, so it is not supported on the HIP path");
  if (target_active)
    type_ = Type::kTargetActive;
  else if (source_active)
    type_ = Type::kSourceActive;
  else
    throw std::runtime_error("CartPosInfo: Target and Source are both static links.");

  const double inf = std::numeric_limits<double>::infinity();
  for (int i = 0; i < 6; ++i)
  {
    const auto u = static_cast<std::size_t>(i);
    if (almostEqualRelativeAndAbs(coeffs[u], 0))
      continue;
    const Bounds& b = bounds[u];
    if (range_bound_handling == RangeBoundHandling::kSplitToTwoInequalities && b.getType() == BoundsType::kRangeBound)
    {
      bounds_.emplace_back(b.getLower(), inf);
      bounds_.emplace_back(-inf, b.getUpper());
      indices_.insert(indices_.end(), { i, i });
      coeffs_.insert(coeffs_.end(), { coeffs[u], coeffs[u] });
    }
    else
    {
      bounds_.push_back(b);
      indices_.push_back(i);
      coeffs_.push_back(coeffs[u]);
    }
  }
  rows_ = static_cast<int>(indices_.size());
  non_zeros_ = n_dof_ * static_cast<Index>(indices_.size());

  evaluator_ = DeviceSetEvaluator::of(*position_var_, manip_, defaultDevice());
  const bool ta = type_ == Type::kTargetActive;
  slot_ = evaluator_->addCartPos(*position_var_, manip_->linkIndex(ta ? target_frame_ : source_frame_),
                                 ta ? target_frame_offset_ : source_frame_offset_, staticInRoot());
}

// the static frame's pose in the chain root: the evaluator forms base_pose * this
Pose12 CartPosConstraint::staticInRoot() const
{
  const bool ta = type_ == Type::kTargetActive;
  const std::string& frame = ta ? source_frame_ : target_frame_;
  const Pose12& off = ta ? source_frame_offset_ : target_frame_offset_;
  if (manip_->linkIndex(frame) == 0)
    return off;
  return poseMul(poseInv(poseOf(manip_->chain.base_pose)), poseMul(manip_->staticWorldPose(frame), off));
}

namespace
{
const char* const kAnalyticRefused =
    "CartPosConstraint: use_numeric_differentiation = false is not supported on the HIP path (the reference's "
    "analytic jacobian is not built); leave the flag true";
}

int CartPosConstraint::update()
{
  // refused where the problem first touches the set, not at the first convexification
  if (!use_numeric_differentiation)
    throw std::runtime_error(kAnalyticRefused);
  evaluator_->prefetch();
  return rows_;
}

VectorXd CartPosConstraint::calcValues(const VectorXd& joint_vals) const
{
  double err[6];
  evaluator_->cartPos(slot_, joint_vals, err, nullptr);
  VectorXd v;
  for (const int i : indices_)
    v.push_back(err[i]);
  return v;
}

VectorXd CartPosConstraint::getValues() const { return calcValues(position_var_->value()); }

void CartPosConstraint::calcJacobianBlock(Jacobian& jac_block, const VectorXd& joint_vals) const
{
  if (!use_numeric_differentiation)
    throw std::runtime_error(kAnalyticRefused);
  const std::size_t D = static_cast<std::size_t>(n_dof_);
  double err[6];
  std::vector<double> jac(6 * D);
  evaluator_->cartPos(slot_, joint_vals, err, jac.data());
  for (std::size_t r = 0; r < indices_.size(); ++r)
  {
    jac_block.startVec(static_cast<Index>(r));
    for (std::size_t j = 0; j < D; ++j)
      jac_block.insertBack(static_cast<Index>(r), position_var_->getIndex() + static_cast<Index>(j)) =
          jac[static_cast<std::size_t>(indices_[r]) * D + j];
  }
  jac_block.finalize();
}

Jacobian CartPosConstraint::getJacobian() const
{
  Jacobian jac(rows_, variables_ ? variables_->getRows() : variablesOf(*position_var_).getRows());
  jac.reserve(non_zeros_);
  calcJacobianBlock(jac, position_var_->value());
  return jac;
}

void CartPosConstraint::setTargetPose(const Pose12& target_frame_offset)
{
  target_frame_offset_ = target_frame_offset;
  const bool ta = type_ == Type::kTargetActive;
  evaluator_->updateCartPos(slot_, ta ? target_frame_offset_ : source_frame_offset_, staticInRoot());
}

Pose12 CartPosConstraint::getCurrentPose() const
{
  const int link = manip_->linkIndex(source_frame_);
  const Pose12 T = link >= 0 && manip_->isActiveLinkId(source_frame_) ? hostFk(manip_->chain, position_var_->value(), link)
                                                                      : manip_->staticWorldPose(source_frame_);
  return poseMul(T, source_frame_offset_);
}

// ------------------------------------------------------------------ collision evaluator
SingleTimestepCollisionEvaluator::SingleTimestepCollisionEvaluator(
    std::shared_ptr<const trajopt::KinematicGroup> manip, std::shared_ptr<const trajopt::Environment> env,
    const trajopt_common::TrajOptCollisionConfig& collision_config)
  : manip_(std::move(manip)), env_(std::move(env)), config_(collision_config), device_(defaultDevice())
{
  if (!manip_ || !env_)
    throw std::runtime_error("SingleTimestepCollisionEvaluator: null kinematic group or environment");
  if (config_.type != trajopt_common::CollisionEvaluatorType::DISCRETE)
    throw std::runtime_error("SingleTimestepCollisionEvaluator, should be configured with DISCRETE");
  int n_spheres = 0;
  for (const auto& cs : env_->collision_spheres)
    n_spheres += manip_->linkIndex(cs.link) > 0 ? 1 : 0;
  if (n_spheres == 0)
    throw std::runtime_error("SingleTimestepCollisionEvaluator: the environment has no collision spheres on the links "
                             "of group '" + manip_->name + "': the robot's sphere model is missing");
}

SingleTimestepCollisionEvaluator::~SingleTimestepCollisionEvaluator()
{
  if (cs_)
    thip_csets_destroy(cs_);
}

void SingleTimestepCollisionEvaluator::lower(thip_problem_desc& d, std::vector<double>& scene) const
{
  lowerCollisionSets(*manip_, *env_, config_, std::max<int>(1, static_cast<int>(vars_.size())), d, scene);
}

void lowerCollisionSets(const trajopt::KinematicGroup& manip, const trajopt::Environment& env,
                        const trajopt_common::TrajOptCollisionConfig& config, int n_steps, thip_problem_desc& d,
                        std::vector<double>& scene)
{
  const trajopt::KinematicGroup* manip_ = &manip;
  const trajopt::Environment* env_ = &env;
  const trajopt_common::TrajOptCollisionConfig& config_ = config;
  std::memset(&d, 0, sizeof(d));
  d.abi_version = THIP_ABI_VERSION;
  d.n_steps = n_steps;
  d.chain = manip_->chain;
  scene.clear();
  trajopt::lowerCollisionModel(*manip_, *env_, d, scene);
  // the pair entries as CollisionTermInfo::hatch lowers them (term 0): a robot link
  // against a scene object or another robot link; a later entry replaces an earlier one
  for (const auto& pd : config_.pairs)
  {
    const int ra = manip_->linkIndex(pd.link), rb = manip_->linkIndex(pd.other);
    const int sa = env_->sceneIndex(pd.link), sb = env_->sceneIndex(pd.other);
    thip_coll_pair e{};
    e.term = 0;
    if (ra > 0 && sb >= 0)
    {
      e.link = ra;
      e.other = sb;
    }
    else if (sa >= 0 && rb > 0)
    {
      e.link = rb;
      e.other = sa;
    }
    else if (ra > 0 && rb > 0)
    {
      e.link = ra;
      e.other = -1 - rb;
    }
    else
      continue;  // names no link of the group: in no contact
    e.margin = pd.dist_pen;
    e.coeff = pd.coeff;
    if (d.n_coll_pairs >= THIP_MAX_COLL_PAIRS)
      throw std::runtime_error("more than " + std::to_string(THIP_MAX_COLL_PAIRS) +
                               " collision link pairs with their own data");
    d.coll_pairs[d.n_coll_pairs++] = e;
  }
}

void SingleTimestepCollisionEvaluator::registerVar(const std::shared_ptr<const Var>& var, int max_num_cnt)
{
  if (!var)
    throw std::runtime_error("SingleTimestepCollisionEvaluator: null position variable");
  if (var->size() != manip_->numJoints())
    throw std::runtime_error("DiscreteCollisionConstraint: the position Var has " + std::to_string(var->size()) +
                             " values, the group " + std::to_string(manip_->numJoints()) + " joints");
  if (max_num_cnt > THIP_CSETS_MAX_ROWS)
    throw std::runtime_error("max_num_cnt " + std::to_string(max_num_cnt) + " exceeds the device's " +
                             std::to_string(THIP_CSETS_MAX_ROWS) + " rows per node");
  const auto& all = variablesOf(*var).getVars();
  if (vars_.empty())
    vars_ = all;
  else if (vars_ != all)
    throw std::runtime_error("SingleTimestepCollisionEvaluator: the constraints of one evaluator must share one "
                             "NodesVariables");
  const int k = varOrdinal(*var);
  if (nodes_.empty())
    first_ = last_ = k;
  first_ = std::min(first_, k);
  last_ = std::max(last_, k);
  nodes_.push_back(var);
  rows_ = std::max(rows_, max_num_cnt);
  rebuild_ = true;
  valid_ = false;
}

void SingleTimestepCollisionEvaluator::ensure()
{
  if (!rebuild_)
    return;
  if (cs_)
    thip_csets_destroy(cs_);
  cs_ = nullptr;
  auto desc = std::make_unique<thip_problem_desc>();
  std::vector<double> scene;
  lower(*desc, scene);
  thip_csets_config cfg{};
  cfg.margin = config_.collision_margin;
  cfg.coeff = config_.collision_coeff;
  cfg.margin_buffer = config_.collision_margin_buffer;
  cfg.max_num_cnt = rows_;
  cfg.first_step = first_;
  cfg.last_step = last_;
  if (thip_csets_create(device_, desc.get(), &cfg, 1, &cs_) != THIP_OK)
    throw std::runtime_error(thip_csets_last_error(nullptr));
  if (thip_csets_upload(cs_, scene.empty() ? nullptr : scene.data()) != THIP_OK)
    throw std::runtime_error(std::string("thip_csets_upload: ") + thip_csets_last_error(cs_));
  rebuild_ = false;
  valid_ = false;
}

DiscreteCollisionEvaluator::NodeRows SingleTimestepCollisionEvaluator::rows(const Var& var)
{
  int k = -1;
  for (std::size_t i = 0; i < vars_.size(); ++i)
    if (vars_[i].get() == &var)
      k = static_cast<int>(i);
  bool registered = false;
  for (const auto& n : nodes_)
    registered = registered || n.get() == &var;
  if (!registered || k < first_ || k > last_)
    throw std::runtime_error("SingleTimestepCollisionEvaluator: the Var '" + var.getName() + "' was not registered");
  ensure();
  const std::size_t D = static_cast<std::size_t>(manip_->numJoints()), R = static_cast<std::size_t>(rows_);
  VectorXd x(vars_.size() * D, 0.0);
  for (std::size_t i = 0; i < vars_.size(); ++i)
    if (vars_[i]->value().size() == D)
      std::copy(vars_[i]->value().begin(), vars_[i]->value().end(), x.begin() + static_cast<long>(i * D));
  if (!valid_ || x != x_)
  {
    const std::size_t n = static_cast<std::size_t>(last_ - first_ + 1);
    values_.assign(n * R, 0.0);
    jac_.assign(n * R * D, 0.0);
    coeffs_.assign(n * R, 0.0);
    counts_.assign(n, 0);
    if (thip_csets_run(cs_, x.data(), values_.data(), jac_.data(), coeffs_.data(), counts_.data(), nullptr) != THIP_OK)
      throw std::runtime_error(std::string("thip_csets_run: ") + thip_csets_last_error(cs_));
    ++launches_;
    x_ = std::move(x);
    valid_ = true;
  }
  const std::size_t u = static_cast<std::size_t>(k - first_);
  NodeRows r;
  r.values = values_.data() + u * R;
  r.jac = jac_.data() + u * R * D;
  r.coeffs = coeffs_.data() + u * R;
  r.count = counts_[u];
  return r;
}

// ------------------------------------------------------------------ collision constraint
DiscreteCollisionConstraint::DiscreteCollisionConstraint(std::shared_ptr<DiscreteCollisionEvaluator> collision_evaluator,
                                                         std::shared_ptr<const Var> position_var, int max_num_cnt,
                                                         bool fixed_sparsity, std::string name)
  : ConstraintSet(std::move(name), max_num_cnt)
  , position_var_(std::move(position_var))
  , collision_evaluator_(std::move(collision_evaluator))
  , fixed_sparsity_(fixed_sparsity)
{
  if (!position_var_ || !collision_evaluator_)
    throw std::runtime_error("DiscreteCollisionConstraint: null position variable or evaluator");
  n_dof_ = position_var_->size();
  if (max_num_cnt < 1)
    throw std::runtime_error("max_num_cnt must be greater than zero!");
  collision_evaluator_->registerVar(position_var_, max_num_cnt);  // refuses a count beyond the device's rows
  coeffs_.assign(static_cast<std::size_t>(max_num_cnt), 1.0);
  bounds_.assign(static_cast<std::size_t>(max_num_cnt), BoundSmallerZero);
  non_zeros_ = static_cast<Index>(rows_) * n_dof_;
}

int DiscreteCollisionConstraint::update()
{
  const auto r = collision_evaluator_->rows(*position_var_);
  // only the rows in use: a row past them keeps its last coefficient (discrete_collision_constraint.cpp:82-84)
  const int cnt = std::min(rows_, r.count);
  for (int i = 0; i < cnt; ++i)
    coeffs_[static_cast<std::size_t>(i)] = r.coeffs[i];
  return rows_;
}

VectorXd DiscreteCollisionConstraint::getValues() const
{
  const auto r = collision_evaluator_->rows(*position_var_);
  const int cnt = std::min(rows_, r.count);
  VectorXd v(static_cast<std::size_t>(rows_), -collision_evaluator_->getCollisionMarginBuffer());
  for (int i = 0; i < cnt; ++i)
    v[static_cast<std::size_t>(i)] = r.values[i];
  return v;
}

Jacobian DiscreteCollisionConstraint::getJacobian() const
{
  Jacobian jac(rows_, variables_ ? variables_->getRows() : variablesOf(*position_var_).getRows());
  jac.reserve(non_zeros_);
  const auto r = collision_evaluator_->rows(*position_var_);
  const int cnt = std::min(rows_, r.count);
  for (int i = 0; i < rows_; ++i)
  {
    if (i >= cnt && !fixed_sparsity_)
      break;
    jac.startVec(i);
    for (Index j = 0; j < n_dof_; ++j)
      jac.insertBack(i, position_var_->getIndex() + j) = i < cnt ? r.jac[static_cast<Index>(i) * n_dof_ + j] : 0.0;
  }
  jac.finalize();
  return jac;
}

void DiscreteCollisionConstraint::setBounds(const std::vector<Bounds>& bounds)
{
  if (bounds.size() != static_cast<std::size_t>(rows_))
    throw std::runtime_error("DiscreteCollisionConstraint::setBounds: " + std::to_string(bounds.size()) +
                             " bounds for " + std::to_string(rows_) + " rows");
  bounds_ = bounds;
}
}  // namespace trajopt_ifopt
