// C entry points of the trajopt_sqp front end's kinematic sets
// (include/trajopt_host.h, tsqp_kin_*): a tsqp_spec's joint terms plus
// CartPosConstraint sets and fixed-size DiscreteCollisionConstraint and
// ContinuousCollisionConstraint sets on the built-in environment of a group -- the setups of the reference's
// cart_position_optimization_unit, numerical_ik_unit and simple_collision_unit
// (trajopt_optimizers/trajopt_sqp/test/).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <limits>
#include <memory>
#include <string>

#include "trajopt_host.h"
#include "trajopt_ifopt/constraints/cartesian_position_constraint.h"
#include "trajopt_ifopt/constraints/collision/continuous_collision_constraint.h"
#include "trajopt_ifopt/constraints/collision/discrete_collision_constraint.h"
#include "tsqp_build.h"

namespace
{
using namespace trajopt_ifopt;

void setErr(char* err, int len, const std::string& msg)
{
  if (err && len > 0)
    std::snprintf(err, static_cast<std::size_t>(len), "%s", msg.c_str());
}

std::string nameOf(const char* s)
{
  return std::string(s, strnlen(s, TSQP_KIN_NAME_LEN));
}

struct KinBuilt
{
  trajopt_sqp::capi::Built joint;
  std::shared_ptr<trajopt::Environment> env;
  std::shared_ptr<DeviceSetEvaluator> cart_eval;
  std::vector<std::shared_ptr<CartPosConstraint>> cart;
  std::vector<std::shared_ptr<DiscreteCollisionEvaluator>> coll_evals;
  std::vector<std::shared_ptr<ContinuousCollisionEvaluator>> ccoll_evals;
};

void addSet(trajopt_sqp::capi::Built& b, const std::shared_ptr<ConstraintSet>& cs, int penalty, const std::string& w)
{
  switch (penalty)
  {
    case TSQP_CONSTRAINT:
      b.problem->addConstraintSet(cs);
      break;
    case TSQP_SQUARED:
      b.problem->addCostSet(cs, trajopt_sqp::CostPenaltyType::kSquared);
      break;
    case TSQP_ABSOLUTE:
      b.problem->addCostSet(cs, trajopt_sqp::CostPenaltyType::kAbsolute);
      break;
    case TSQP_HINGE:
      b.problem->addCostSet(cs, trajopt_sqp::CostPenaltyType::kHinge);
      break;
    default:
      throw std::runtime_error(w + ": unknown penalty type");
  }
  b.sets.push_back(cs);
}

KinBuilt buildKin(const tsqp_spec* s, const tsqp_kin_spec* k, int device, const char* who)
{
  const std::string w(who);
  if (k->n_prims < 0 || k->n_prims > TSQP_KIN_MAX_PRIMS || k->n_cart < 0 || k->n_cart > TSQP_KIN_MAX_CART ||
      k->n_coll < 0 || k->n_coll > TSQP_KIN_MAX_COLL || k->n_ccoll < 0 || k->n_ccoll > TSQP_KIN_MAX_COLL)
    throw std::runtime_error(w + ": kinematic spec out of range");
  KinBuilt out;
  out.joint = trajopt_sqp::capi::buildJointProblem(s, who);
  const std::string manip = nameOf(k->manip);
  out.env = trajopt::Environment::builtin(manip);
  const auto kin = out.env->getJointGroup(manip);
  if (!kin)
    throw std::runtime_error(w + ": no kinematic group '" + manip + "'");
  if (kin->numJoints() != s->n_dof)
    throw std::runtime_error(w + ": the spec has " + std::to_string(s->n_dof) + " dofs, group '" + manip + "' " +
                             std::to_string(kin->numJoints()) + " joints");
  for (int p = 0; p < k->n_prims; ++p)
  {
    std::array<double, 16> rec;
    std::copy(k->prims[p], k->prims[p] + 16, rec.begin());
    out.env->addSceneObject("", rec);
  }
  // the sets below take `device`; the caller's default is put back on every way out
  struct DeviceScope
  {
    int prev;
    explicit DeviceScope(int d) : prev(defaultDevice()) { setDefaultDevice(d); }
    ~DeviceScope() { setDefaultDevice(prev); }
  } scope(device);
  for (int i = 0; i < k->n_cart; ++i)
  {
    const tsqp_cart_term& t = k->cart[i];
    if (t.node < 0 || t.node >= s->n_nodes)
      throw std::runtime_error(w + ": CartPos term " + std::to_string(i) + ": node out of range");
    std::vector<Bounds> bounds;
    for (int c = 0; c < 6; ++c)
      bounds.emplace_back(t.lower[c], t.upper[c]);
    Pose12 so, to;
    std::copy(t.source_offset, t.source_offset + 12, so.begin());
    std::copy(t.target_offset, t.target_offset + 12, to.begin());
    auto cs = std::make_shared<CartPosConstraint>(out.joint.vars[static_cast<std::size_t>(t.node)],
                                                  VectorXd(t.coeffs, t.coeffs + 6), bounds, kin, nameOf(t.source_frame),
                                                  nameOf(t.target_frame), so, to, "CartPos_" + std::to_string(i));
    cs->use_numeric_differentiation = t.analytic_jacobian == 0;
    out.cart.push_back(cs);
    addSet(out.joint, cs, t.penalty, w);
  }
  if (!out.cart.empty())
    out.cart_eval = DeviceSetEvaluator::of(*out.joint.vars[0], kin, device);
  for (int i = 0; i < k->n_coll; ++i)
  {
    const tsqp_coll_term& t = k->coll[i];
    if (t.first < 0 || t.last < t.first || t.last >= s->n_nodes)
      throw std::runtime_error(w + ": collision term " + std::to_string(i) + ": nodes out of range");
    trajopt_common::TrajOptCollisionConfig cfg(t.margin, t.coeff);
    cfg.collision_margin_buffer = t.buffer;
    auto ev = std::make_shared<SingleTimestepCollisionEvaluator>(kin, out.env, cfg);
    out.coll_evals.push_back(ev);
    for (int n = t.first; n <= t.last; ++n)
      addSet(out.joint,
             std::make_shared<DiscreteCollisionConstraint>(ev, out.joint.vars[static_cast<std::size_t>(n)],
                                                           t.max_num_cnt, t.fixed_sparsity != 0,
                                                           "DiscreteCollision_" + std::to_string(i) + "_" +
                                                               std::to_string(n)),
             t.penalty, w);
  }
  for (int i = 0; i < k->n_ccoll; ++i)
  {
    const tsqp_ccoll_term& t = k->ccoll[i];
    if (t.first < 0 || t.last <= t.first || t.last >= s->n_nodes)
      throw std::runtime_error(w + ": continuous collision term " + std::to_string(i) + ": nodes out of range");
    using trajopt_common::CollisionEvaluatorType;
    trajopt_common::TrajOptCollisionConfig cfg(t.margin, t.coeff);
    cfg.collision_margin_buffer = t.buffer;
    cfg.longest_valid_segment_length = t.lvs_length;
    cfg.type = (t.evaluator_type >= 0 && t.evaluator_type <= 4) ? static_cast<CollisionEvaluatorType>(t.evaluator_type)
                                                                : CollisionEvaluatorType::NONE;
    std::shared_ptr<ContinuousCollisionEvaluator> ev;
    if (cfg.type == CollisionEvaluatorType::DISCRETE || cfg.type == CollisionEvaluatorType::LVS_DISCRETE)
      ev = std::make_shared<LVSDiscreteCollisionEvaluator>(kin, out.env, cfg);
    else
      ev = std::make_shared<LVSContinuousCollisionEvaluator>(kin, out.env, cfg);
    out.ccoll_evals.push_back(ev);
    for (int n = t.first; n < t.last; ++n)
      addSet(out.joint,
             std::make_shared<ContinuousCollisionConstraint>(
                 ev,
                 std::array<std::shared_ptr<const Var>, 2>{ out.joint.vars[static_cast<std::size_t>(n)],
                                                            out.joint.vars[static_cast<std::size_t>(n) + 1] },
                 n == t.first && t.fixed_first != 0, n + 1 == t.last && t.fixed_last != 0, t.max_num_cnt,
                 t.fixed_sparsity != 0, "LVSCollision_" + std::to_string(i) + "_" + std::to_string(n)),
             t.penalty, w);
  }
  return out;
}

void setLaunches(const KinBuilt& b, long long* launches)
{
  launches[0] = b.cart_eval ? b.cart_eval->launches() : 0;
  launches[1] = 0;
  for (const auto& ev : b.coll_evals)
    launches[1] += ev->launches();
  for (const auto& ev : b.ccoll_evals)
    launches[1] += ev->launches();
}
}  // namespace

namespace trajopt_sqp
{
namespace capi
{
KinProblem buildKinProblem(const tsqp_spec* spec, const tsqp_kin_spec* kin, int device, const char* who)
{
  auto kb = std::make_shared<KinBuilt>(buildKin(spec, kin, device, who));
  KinProblem out;
  out.joint = kb->joint;
  out.keep = kb;
  out.set_launches = [kb](long long* launches) { setLaunches(*kb, launches); };
  return out;
}
}  // namespace capi
}  // namespace trajopt_sqp

extern "C" {

int thost_tsqp_solve_kin(const tsqp_spec* s, const tsqp_kin_spec* k, int device, double* x, tsqp_result* result,
                         char* err, int err_len)
{
  try
  {
    if (!s || !k || !x)
      throw std::runtime_error("thost_tsqp_solve_kin: null argument");
    KinBuilt b = buildKin(s, k, device, "thost_tsqp_solve_kin");
    trajopt_sqp::capi::solveBuilt(b.joint, s, device, "thost_tsqp_solve_kin", x, result);
    return 0;
  }
  catch (const std::exception& e)
  {
    setErr(err, err_len, e.what());
    return -1;
  }
}

int thost_tsqp_eval_kin(const tsqp_spec* s, const tsqp_kin_spec* k, int device, const double* xs, int n_x, int* n_sets,
                        int* set_rows, int cap_sets, double* values, double* jac, double* coeffs, double* lower,
                        double* upper, int cap_rows, const double* probe_q, double* probe_values, long long* launches,
                        char* err, int err_len)
{
  try
  {
    const std::string w = "thost_tsqp_eval_kin";
    if (!s || !k || n_x < 0 || (n_x > 0 && !xs) || cap_sets < 0 || cap_rows < 0)
      throw std::runtime_error(w + ": null or negative argument");
    KinBuilt b = buildKin(s, k, device, w.c_str());
    const auto& sets = b.joint.sets;
    long total = 0;
    for (const auto& cs : sets)
      total += cs->getRows();
    if (n_sets)
      *n_sets = static_cast<int>(sets.size());
    if (static_cast<long>(sets.size()) > cap_sets && set_rows)
      throw std::runtime_error(w + ": " + std::to_string(sets.size()) + " sets, cap_sets " + std::to_string(cap_sets));
    if (total > cap_rows && (values || jac || coeffs || lower || upper || probe_values))
      throw std::runtime_error(w + ": " + std::to_string(total) + " rows, cap_rows " + std::to_string(cap_rows));
    for (std::size_t i = 0; set_rows && i < sets.size(); ++i)
      set_rows[i] = sets[i]->getRows();
    const long nv = static_cast<long>(s->n_nodes) * s->n_dof;
    if (n_x > 0)  // with no x the sets are only built: rows and bounds, no device call
      b.joint.problem->setup();
    for (int ix = 0; ix < n_x; ++ix)
    {
      b.joint.problem->setVariables(xs + static_cast<long>(ix) * nv);
      long row = 0;
      for (const auto& cs : sets)
      {
        const VectorXd v = cs->getValues(), c = cs->getCoefficients();
        const Jacobian J = cs->getJacobian();
        for (long r = 0; r < cs->getRows(); ++r, ++row)
        {
          const long o = static_cast<long>(ix) * cap_rows + row;
          if (values)
            values[o] = v[static_cast<std::size_t>(r)];
          if (coeffs)
            coeffs[o] = c[static_cast<std::size_t>(r)];
          if (jac)
          {
            std::fill(jac + o * nv, jac + (o + 1) * nv, 0.0);
            for (long e = J.rowBegin(r); e < J.rowEnd(r); ++e)
              jac[o * nv + J.col(e)] = J.value(e);
          }
        }
      }
    }
    long row = 0;
    for (const auto& cs : sets)
    {
      const auto bounds = cs->getBounds();
      for (long r = 0; r < cs->getRows(); ++r, ++row)
      {
        if (lower)
          lower[row] = bounds[static_cast<std::size_t>(r)].getLower();
        if (upper)
          upper[row] = bounds[static_cast<std::size_t>(r)].getUpper();
      }
    }
    if (probe_q && probe_values)
    {
      const VectorXd q(probe_q, probe_q + s->n_dof);
      row = 0;
      for (const auto& cs : sets)
      {
        if (const auto* cp = dynamic_cast<const CartPosConstraint*>(cs.get()))
        {
          const VectorXd v = cp->calcValues(q);
          std::copy(v.begin(), v.end(), probe_values + row);
        }
        row += cs->getRows();
      }
    }
    if (launches)
      setLaunches(b, launches);
    return 0;
  }
  catch (const std::exception& e)
  {
    setErr(err, err_len, e.what());
    return -1;
  }
}

int thost_tsqp_sizeof_kin_spec(void) { return static_cast<int>(sizeof(tsqp_kin_spec)); }
int thost_tsqp_sizeof_cart_term(void) { return static_cast<int>(sizeof(tsqp_cart_term)); }
int thost_tsqp_sizeof_coll_term(void) { return static_cast<int>(sizeof(tsqp_coll_term)); }
int thost_tsqp_sizeof_ccoll_term(void) { return static_cast<int>(sizeof(tsqp_ccoll_term)); }
}  // extern "C"
