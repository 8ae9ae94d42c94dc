#include "trajopt_amd/term_evaluator.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>

namespace trajopt
{
namespace
{
// the structure of a lowered problem (BatchTrustRegionSQP's rule: the descriptor
// with the per-problem default JointPos targets cleared)
thip_problem_desc structureOf(const thip_problem_desc& in)
{
  thip_problem_desc d = in;
  for (auto& row : d.jpos_targets)
    for (double& v : row)
      v = 0.0;
  return d;
}

const char* kindName(int kind)
{
  static const char* const names[] = { "joint_vel", "jvx", "jpos", "jdt", "cart", "coll" };
  return kind >= 0 && kind < 6 ? names[kind] : "?";
}

std::string slotName(const thip_term_slot& s)
{
  return std::string(kindName(s.kind)) + "_" + std::to_string(s.kind == THIP_TERM_COLL ? s.unit : s.index);
}
}  // namespace

std::string whyNotLowerable(const TrajOptProb& prob)
{
  if (prob.lowerable())
    return "";
  const thip_problem_desc& d = prob.desc();
  std::string why;
  auto note = [&](const std::string& s) { why += (why.empty() ? "" : "; ") + s; };
  if (d.n_steps < 2 || d.n_steps > THIP_MAX_STEPS)
    note("n_steps " + std::to_string(d.n_steps) + " outside [2, " + std::to_string(THIP_MAX_STEPS) + "]");
  if (d.n_prims > THIP_MAX_PRIMS)
    note("n_prims " + std::to_string(d.n_prims) + " above " + std::to_string(THIP_MAX_PRIMS));
  if (d.n_coll_extra > 0)
    note("more than one collision term (coll_extra)");
  if (d.use_time || d.n_jvt > 0 || d.n_ttt > 0 || d.n_fixed_dofs > 0)
    note("time parameterisation (use_time, time terms) or fixed dofs");
  if (d.n_cvel > 0)
    note("CartVel terms (cart_vel), which the generic path evaluates on the device");
  if (!thip_jdt_fused(&d))
    note("a JointVel constraint / JointAcc / JointJerk term that is not the fused JointAccEqCost (jdt)");
  const std::string terms = prob.unloweredTerms();
  if (!terms.empty())
    note("the terms " + terms);
  return why;
}

std::vector<thip_term_slot> termSlotTable(const thip_problem_desc& d, int& n_costs, int& n_cnts)
{
  std::vector<thip_term_slot> table(static_cast<std::size_t>(2 + THIP_MAX_CART + THIP_MAX_JPOS + THIP_MAX_JVX +
                                                             THIP_MAX_JDT + THIP_MAX_STEPS));
  if (thip_terms_slot_table(&d, table.data(), static_cast<int>(table.size()), &n_costs, &n_cnts) != THIP_OK)
    throw std::runtime_error(std::string("TermEvaluator: ") + thip_terms_last_error(nullptr));
  table.resize(static_cast<std::size_t>(n_costs + n_cnts));
  return table;
}

TermSlotMap termSlotMap(const TrajOptProb& prob, const std::vector<thip_term_slot>& table, int n_costs, int n_cnts)
{
  auto& p = const_cast<TrajOptProb&>(prob);  // getCosts() is not const
  const std::vector<sco::Cost::Ptr>& costs = p.getCosts();
  const std::vector<sco::Constraint::Ptr> cnts = prob.getConstraints();
  if (static_cast<int>(costs.size()) != n_costs || static_cast<int>(cnts.size()) != n_cnts)
    throw std::runtime_error("termSlotMap: the problem has " + std::to_string(costs.size()) + " costs and " +
                             std::to_string(cnts.size()) + " constraints, the kernel " + std::to_string(n_costs) +
                             " and " + std::to_string(n_cnts) + " slots");
  TermSlotMap m;
  m.cost_pos.assign(static_cast<std::size_t>(n_costs), -1);
  m.cnt_pos.assign(static_cast<std::size_t>(n_cnts), -1);
  for (const auto& c : costs)
    m.cost_names.push_back(c->name());
  for (const auto& c : cnts)
    m.cnt_names.push_back(c->name());
  std::vector<char> cost_used(costs.size(), 0), cnt_used(cnts.size(), 0);
  const std::vector<TrajOptProb::LoweredRecord>& recs = prob.loweredRecords();
  for (std::size_t s = 0; s < table.size(); ++s)
  {
    const thip_term_slot& e = table[s];
    const void* obj = nullptr;
    for (const auto& r : recs)
      if (r.kind == e.kind && (r.is_cnt != 0) == (e.is_cnt != 0) &&
          (e.kind == THIP_TERM_COLL ? r.unit == e.unit : r.index == e.index))
      {
        if (obj)
          throw std::runtime_error("termSlotMap: two term objects claim slot " + slotName(e));
        obj = r.obj;
      }
    if (!obj)
      throw std::runtime_error("termSlotMap: no term object for slot " + slotName(e));
    int pos = -1;
    if (e.is_cnt)
    {
      for (std::size_t i = 0; i < cnts.size(); ++i)
        if (cnts[i].get() == obj)
          pos = static_cast<int>(i);
    }
    else
      for (std::size_t i = 0; i < costs.size(); ++i)
        if (costs[i].get() == obj)
          pos = static_cast<int>(i);
    std::vector<char>& used = e.is_cnt ? cnt_used : cost_used;
    if (pos < 0 || used[static_cast<std::size_t>(pos)])
      throw std::runtime_error("termSlotMap: slot " + slotName(e) + " has no place of its own among the problem's terms");
    used[static_cast<std::size_t>(pos)] = 1;
    (e.is_cnt ? m.cnt_pos[s - static_cast<std::size_t>(n_costs)] : m.cost_pos[s]) = pos;
  }
  return m;
}

void TermEvaluator::create(const thip_problem_desc& d, int device)
{
  if (thip_terms_create(device, &d, batch_, &t_) != THIP_OK)
    throw std::runtime_error(std::string("TermEvaluator: ") + thip_terms_last_error(nullptr));
  thip_terms_counts(t_, &n_costs_, &n_cnts_);
  table_.resize(static_cast<std::size_t>(n_costs_ + n_cnts_));
  if (!table_.empty())
    thip_terms_slots(t_, table_.data());
  n_steps_ = d.n_steps;
  n_dof_ = d.chain.n_dof;
}

TermEvaluator::TermEvaluator(const std::vector<TrajOptProb::Ptr>& probs, int device)
{
  if (probs.empty())
    throw std::runtime_error("TermEvaluator: empty batch");
  std::vector<LoweredProblem> lowered;
  for (const auto& p : probs)
  {
    if (!p)
      throw std::runtime_error("TermEvaluator: null problem");
    if (!p->lowerable())
      throw std::runtime_error("TermEvaluator: the batched kernels do not take this problem (" + whyNotLowerable(*p) +
                               "): evaluate it on the host loop (Cost::value / Constraint::violation)");
    lowered.push_back(p->lowered());
  }
  batch_ = static_cast<int>(probs.size());
  create(structureOf(lowered[0].desc), device);
  try
  {
    for (const auto& p : probs)
      maps_.push_back(termSlotMap(*p, table_, n_costs_, n_cnts_));
    upload(lowered);
  }
  catch (...)
  {
    thip_terms_destroy(t_);
    t_ = nullptr;
    throw;
  }
}

TermEvaluator::TermEvaluator(const std::vector<LoweredProblem>& probs, int device)
{
  if (probs.empty())
    throw std::runtime_error("TermEvaluator: empty batch");
  batch_ = static_cast<int>(probs.size());
  create(structureOf(probs[0].desc), device);
  try
  {
    upload(probs);
  }
  catch (...)
  {
    thip_terms_destroy(t_);
    t_ = nullptr;
    throw;
  }
}

TermEvaluator::~TermEvaluator() { thip_terms_destroy(t_); }

void TermEvaluator::upload(const std::vector<LoweredProblem>& probs)
{
  if (static_cast<int>(probs.size()) != batch_)
    throw std::runtime_error("TermEvaluator::upload: " + std::to_string(probs.size()) + " problems on an evaluator of " +
                             std::to_string(batch_));
  const thip_problem_desc d0 = structureOf(probs[0].desc);
  std::vector<double> tgt, jpt, scene;
  for (std::size_t b = 0; b < probs.size(); ++b)
  {
    const thip_problem_desc db = structureOf(probs[b].desc);
    if (b > 0 && std::memcmp(&d0, &db, sizeof(d0)) != 0)
      throw std::runtime_error("TermEvaluator: problem " + std::to_string(b) + " does not share problem 0's structure");
    tgt.insert(tgt.end(), probs[b].cart_targets.begin(), probs[b].cart_targets.end());
    jpt.insert(jpt.end(), probs[b].jpos_targets.begin(), probs[b].jpos_targets.end());
    scene.insert(scene.end(), probs[b].scene.begin(), probs[b].scene.end());
  }
  const std::size_t B = probs.size();
  if (tgt.size() != B * d0.n_cart * 12 || jpt.size() != B * d0.n_jpos * d0.chain.n_dof ||
      scene.size() != B * (d0.coll_enabled ? d0.n_prims : 0) * 16)
    throw std::runtime_error("TermEvaluator: per-problem data sizes do not match the structure");
  if (thip_terms_upload(t_, tgt.empty() ? nullptr : tgt.data(), scene.empty() ? nullptr : scene.data()) != THIP_OK ||
      (d0.n_jpos > 0 && thip_terms_upload_joint_targets(t_, jpt.data()) != THIP_OK))
    throw std::runtime_error(std::string("TermEvaluator: ") + thip_terms_last_error(t_));
}

std::vector<TrajOptResult> TermEvaluator::collect(const std::vector<double>& costs,
                                                  const std::vector<double>& viols) const
{
  std::vector<TrajOptResult> out(static_cast<std::size_t>(batch_));
  for (int b = 0; b < batch_; ++b)
  {
    TrajOptResult& r = out[static_cast<std::size_t>(b)];
    r.cost_vals.assign(static_cast<std::size_t>(n_costs_), 0.0);
    r.cnt_viols.assign(static_cast<std::size_t>(n_cnts_), 0.0);
    const double* c = costs.data() + static_cast<std::size_t>(b) * n_costs_;
    const double* v = viols.data() + static_cast<std::size_t>(b) * n_cnts_;
    if (maps_.empty())
    {
      std::copy(c, c + n_costs_, r.cost_vals.begin());
      std::copy(v, v + n_cnts_, r.cnt_viols.begin());
      for (int s = 0; s < n_costs_ + n_cnts_; ++s)
        (s < n_costs_ ? r.cost_names : r.cnt_names).push_back(slotName(table_[static_cast<std::size_t>(s)]));
      continue;
    }
    const TermSlotMap& m = maps_[static_cast<std::size_t>(b)];
    for (int s = 0; s < n_costs_; ++s)
      r.cost_vals[static_cast<std::size_t>(m.cost_pos[static_cast<std::size_t>(s)])] = c[s];
    for (int s = 0; s < n_cnts_; ++s)
      r.cnt_viols[static_cast<std::size_t>(m.cnt_pos[static_cast<std::size_t>(s)])] = v[s];
    r.cost_names = m.cost_names;
    r.cnt_names = m.cnt_names;
  }
  return out;
}

std::vector<TrajOptResult> TermEvaluator::evaluate(const std::vector<TrajArray>& trajs)
{
  if (static_cast<int>(trajs.size()) != batch_)
    throw std::runtime_error("TermEvaluator::evaluate: " + std::to_string(trajs.size()) + " trajectories for " +
                             std::to_string(batch_) + " problems");
  std::vector<double> x;
  const std::size_t N = static_cast<std::size_t>(n_steps_), D = static_cast<std::size_t>(n_dof_);
  for (std::size_t b = 0; b < trajs.size(); ++b)
  {
    if (trajs[b].size() != N)
      throw std::runtime_error("TermEvaluator::evaluate: trajectory " + std::to_string(b) + " has " +
                               std::to_string(trajs[b].size()) + " waypoints, the problem " + std::to_string(N));
    for (const DblVec& row : trajs[b])
    {
      if (row.size() < D)
        throw std::runtime_error("TermEvaluator::evaluate: a waypoint of trajectory " + std::to_string(b) + " has " +
                                 std::to_string(row.size()) + " values, the group " + std::to_string(D) + " joints");
      x.insert(x.end(), row.begin(), row.begin() + static_cast<long>(D));
    }
  }
  std::vector<double> costs(static_cast<std::size_t>(batch_) * std::max(n_costs_, 1)),
      viols(static_cast<std::size_t>(batch_) * std::max(n_cnts_, 1));
  if (thip_terms_run(t_, x.data(), costs.data(), viols.data()) != THIP_OK)
    throw std::runtime_error(std::string("TermEvaluator::evaluate: ") + thip_terms_last_error(t_));
  std::vector<TrajOptResult> out = collect(costs, viols);
  for (std::size_t b = 0; b < out.size(); ++b)
    out[b].traj = trajs[b];
  return out;
}

std::vector<TrajOptResult> TermEvaluator::evaluateDevice(const double* d_x)
{
  std::vector<double> costs(static_cast<std::size_t>(batch_) * std::max(n_costs_, 1)),
      viols(static_cast<std::size_t>(batch_) * std::max(n_cnts_, 1));
  if (thip_terms_run_device(t_, d_x, costs.data(), viols.data()) != THIP_OK)
    throw std::runtime_error(std::string("TermEvaluator::evaluateDevice: ") + thip_terms_last_error(t_));
  return collect(costs, viols);
}

double TermEvaluator::lastKernelMs() const { return thip_terms_last_ms(t_); }
}  // namespace trajopt
