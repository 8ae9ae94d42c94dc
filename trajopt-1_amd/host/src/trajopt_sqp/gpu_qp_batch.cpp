// trajopt_sqp::GpuQPBatch and its Slot (gpu_qp_batch.h).
#include "trajopt_sqp/gpu_qp_batch.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "qp_data.h"
#include "trajopt_sqp/gpu_qp_solver.h"

namespace trajopt_sqp
{
namespace
{
constexpr int kSetup = THIP_QP_OP_SETUP, kMatP = THIP_QP_OP_MAT_P, kVecQ = THIP_QP_OP_VEC_Q, kMatA = THIP_QP_OP_MAT_A,
              kBounds = THIP_QP_OP_VEC_BOUNDS, kWarm = THIP_QP_OP_WARM, kSolve = THIP_QP_OP_SOLVE;

template <class T>
void append(std::string& k, const T& v)
{
  k.append(reinterpret_cast<const char*>(&v), sizeof(T));
}
void appendInts(std::string& k, const std::vector<int>& v)
{
  append(k, static_cast<int>(v.size()));
  if (!v.empty())
    k.append(reinterpret_cast<const char*>(v.data()), v.size() * sizeof(int));
}
}  // namespace

GpuQPBatch::Device GpuQPBatch::Device::hip()
{
  Device d;
  d.create = thip_qp_create;
  d.step = thip_qp_step;
  d.destroy = thip_qp_destroy;
  d.last_error = [](thip_qp* q) { return std::string(thip_qp_last_error(q)); };
  return d;
}

GpuQPBatch::GpuQPBatch(int device, Device dev) : device_(device), dev_(std::move(dev)) {}

GpuQPBatch::~GpuQPBatch()
{
  for (auto& kv : groups_)
    dev_.destroy(kv.second->qp);
}

void GpuQPBatch::enter()
{
  std::lock_guard<std::mutex> lk(mu_);
  ++active_;
}

void GpuQPBatch::leave()
{
  std::unique_lock<std::mutex> lk(mu_);
  --active_;
  // the clients still running may all be waiting now
  if (!pending_.empty() && static_cast<int>(pending_.size()) >= active_)
    flushLocked();
}

std::shared_ptr<GpuQPBatch::Slot> GpuQPBatch::makeSlot() { return std::shared_ptr<Slot>(new Slot(shared_from_this())); }

GpuQPBatch::Stats GpuQPBatch::stats() const
{
  std::lock_guard<std::mutex> lk(mu_);
  return stats_;
}

// the group a slot's QP belongs to: sizes, both patterns, every OSQP setting
std::string GpuQPBatch::keyOf(const Slot& s)
{
  std::string k;
  append(k, static_cast<int>(s.nv_));
  append(k, static_cast<int>(s.nc_));
  const thip_osqp_settings& o = s.settings;
  append(k, o.rho), append(k, o.sigma), append(k, o.alpha), append(k, o.scaling), append(k, o.adaptive_rho);
  append(k, o.adaptive_rho_interval), append(k, o.adaptive_rho_tolerance), append(k, o.max_iter), append(k, o.eps_abs);
  append(k, o.eps_rel), append(k, o.eps_prim_inf), append(k, o.eps_dual_inf), append(k, o.check_termination);
  append(k, o.warm_starting), append(k, o.polishing), append(k, o.delta), append(k, o.polish_refine_iter);
  appendInts(k, s.P_.p), appendInts(k, s.P_.i), appendInts(k, s.A_.p), appendInts(k, s.A_.i);
  return k;
}

void GpuQPBatch::release(Slot& s)
{
  if (s.group_)
    s.group_->owner[static_cast<std::size_t>(s.index_)] = nullptr;
  s.group_ = nullptr;
  s.index_ = -1;
}

void GpuQPBatch::submit(Slot& s, int bits)
{
  const std::size_t n = static_cast<std::size_t>(s.nv_), m = static_cast<std::size_t>(s.nc_);
  if (((bits & (kSetup | kVecQ)) && s.q_.size() != n) ||
      ((bits & (kSetup | kBounds)) && (s.lo_.size() != m || s.up_.size() != m)) ||
      ((bits & kWarm) && (!s.wx_ || !s.wy_ || s.wx_->size() != n || s.wy_->size() != m)) ||
      ((bits & kSetup) && (s.P_.p.size() != n + 1 || s.A_.p.size() != n + 1)))
    throw std::runtime_error("GpuQPBatch: the QP data do not have the sizes given to init()");
  std::unique_lock<std::mutex> lk(mu_);
  s.submitted_ = bits;
  s.done_ = false;
  s.error_.clear();
  pending_.push_back(&s);
  if (static_cast<int>(pending_.size()) >= active_)
    flushLocked();  // the last client of the round runs it
  else
    cv_.wait(lk, [&] { return s.done_; });
  if (!s.error_.empty())
    throw std::runtime_error(s.error_);
}

// Called with the lock held by the thread that completed the round: every other
// running client is blocked in submit(), so the pending set cannot change.
void GpuQPBatch::flushLocked()
{
  std::vector<Slot*> reqs;
  reqs.swap(pending_);
  ++stats_.rounds;
  // a place for every slot that sets up: its own when the key is unchanged, else a
  // free index of a group of its key, else a new group as large as the slots still
  // asking for that key in this round
  std::map<std::string, std::vector<Slot*>> asking;
  for (Slot* s : reqs)
  {
    ++s->n_rounds;
    if (!(s->submitted_ & kSetup))
      continue;
    std::string key = keyOf(*s);
    if (s->group_ && s->group_->key == key)
      continue;
    release(*s);
    asking[std::move(key)].push_back(s);
  }
  for (auto& kv : asking)
  {
    std::vector<Slot*>& v = kv.second;
    std::size_t k = 0;
    auto place = [&](Group& g) {
      for (std::size_t i = 0; i < g.owner.size() && k < v.size(); ++i)
        if (!g.owner[i])
        {
          g.owner[i] = v[k];
          v[k]->group_ = &g;
          v[k]->index_ = static_cast<int>(i);
          ++k;
        }
    };
    const auto range = groups_.equal_range(kv.first);
    for (auto it = range.first; it != range.second; ++it)
      place(*it->second);
    if (k == v.size())
      continue;
    const Slot& s0 = *v[k];
    const int count = static_cast<int>(v.size() - k);
    auto g = std::make_unique<Group>();
    if (dev_.create(device_, static_cast<int>(s0.nv_), static_cast<int>(s0.nc_), s0.P_.p.data(), s0.P_.i.data(),
                    s0.A_.p.data(), s0.A_.i.data(), count, &g->qp) != THIP_OK)
    {
      const std::string msg = "GpuQPBatch: thip_qp_create: " + dev_.last_error(nullptr);
      for (; k < v.size(); ++k)
        v[k]->error_ = msg;
      continue;
    }
    g->key = kv.first;
    g->n = static_cast<int>(s0.nv_);
    g->m = static_cast<int>(s0.nc_);
    g->capacity = count;
    g->np = s0.P_.x.size();
    g->na = s0.A_.x.size();
    g->settings = s0.settings;
    const std::size_t B = static_cast<std::size_t>(count), n = static_cast<std::size_t>(g->n),
                      m = static_cast<std::size_t>(g->m);
    g->owner.assign(B, nullptr);
    g->P.resize(B * g->np), g->A.resize(B * g->na), g->q.resize(B * n), g->l.resize(B * m), g->u.resize(B * m);
    g->wx.resize(B * n), g->wy.resize(B * m), g->x.resize(B * n), g->y.resize(B * std::max<std::size_t>(m, 1));
    g->info.resize(B);
    ++stats_.groups;
    stats_.max_group = std::max<long long>(stats_.max_group, count);
    place(*g);
    groups_.emplace(kv.first, std::move(g));
  }
  // one thip_qp_step per group with a waiting slot
  std::map<Group*, std::vector<Slot*>> by_group;
  for (Slot* s : reqs)
    if (s->error_.empty())
    {
      if (s->group_)
        by_group[s->group_].push_back(s);
      else
        s->error_ = "GpuQPBatch: a slot without a workspace submitted operations without a setup";
    }
  for (auto& kv : by_group)
  {
    Group& g = *kv.first;
    const std::size_t n = static_cast<std::size_t>(g.n), m = static_cast<std::size_t>(g.m);
    g.ops.assign(static_cast<std::size_t>(g.capacity), 0);
    int all = 0;
    for (Slot* s : kv.second)
    {
      const std::size_t i = static_cast<std::size_t>(s->index_);
      const int bits = s->submitted_;
      g.ops[i] = bits;
      all |= bits;
      if (bits & (kSetup | kMatP))
        std::copy(s->P_.x.begin(), s->P_.x.end(), g.P.begin() + static_cast<long>(i * g.np));
      if (bits & (kSetup | kMatA))
        std::copy(s->A_.x.begin(), s->A_.x.end(), g.A.begin() + static_cast<long>(i * g.na));
      if (bits & (kSetup | kVecQ))
        std::copy(s->q_.begin(), s->q_.end(), g.q.begin() + static_cast<long>(i * n));
      if (bits & (kSetup | kBounds))
      {
        std::copy(s->lo_.begin(), s->lo_.end(), g.l.begin() + static_cast<long>(i * m));
        std::copy(s->up_.begin(), s->up_.end(), g.u.begin() + static_cast<long>(i * m));
      }
      if (bits & kWarm)
      {
        std::copy(s->wx_->begin(), s->wx_->end(), g.wx.begin() + static_cast<long>(i * n));
        std::copy(s->wy_->begin(), s->wy_->end(), g.wy.begin() + static_cast<long>(i * m));
      }
    }
    ++stats_.step_launches;
    const bool warm = (all & kWarm) != 0;
    if (dev_.step(g.qp, g.ops.data(), g.P.data(), g.q.data(), g.A.data(), g.l.data(), g.u.data(), &g.settings,
                  warm ? g.wx.data() : nullptr, warm ? g.wy.data() : nullptr, g.x.data(), g.y.data(),
                  g.info.data()) != THIP_OK)
    {
      const std::string msg = "GpuQPBatch: thip_qp_step: " + dev_.last_error(g.qp);
      for (Slot* s : kv.second)
        s->error_ = msg;
      continue;
    }
    for (Slot* s : kv.second)
    {
      const std::size_t i = static_cast<std::size_t>(s->index_);
      if (s->submitted_ & ~kWarm)
        s->info_ = g.info[i];
      if (s->submitted_ & kSolve)
      {
        s->x_.assign(g.x.begin() + static_cast<long>(i * n), g.x.begin() + static_cast<long>((i + 1) * n));
        s->y_.assign(g.y.begin() + static_cast<long>(i * m), g.y.begin() + static_cast<long>((i + 1) * m));
      }
    }
  }
  for (Slot* s : reqs)
    s->done_ = true;
  cv_.notify_all();
}

// ---- Slot ------------------------------------------------------------------
namespace
{
template <class C>
void toCsc(const trajopt_ifopt::Jacobian& J, bool upper, double scale, C& out)
{
  qp_data::Csc c;
  qp_data::toCsc(J, upper, scale, c);
  out.p = std::move(c.p);
  out.i = std::move(c.i);
  out.x = std::move(c.x);
}
}  // namespace

GpuQPBatch::Slot::Slot(std::shared_ptr<GpuQPBatch> batch) : batch_(std::move(batch))
{
  GpuQPSolver::setDefaultOSQPSettings(settings);
}

GpuQPBatch::Slot::~Slot() { dropWorkspace(); }

void GpuQPBatch::Slot::dropWorkspace()
{
  std::lock_guard<std::mutex> lk(batch_->mu_);
  batch_->release(*this);
  live_ = false;
}

bool GpuQPBatch::Slot::init(long num_vars, long num_cnts)
{
  nv_ = num_vars;
  nc_ = num_cnts;
  x0_.assign(static_cast<std::size_t>(nv_), 0.0);
  y0_.assign(static_cast<std::size_t>(nc_), 0.0);
  status_ = QPSolverStatus::kInitialized;
  return true;
}

bool GpuQPBatch::Slot::clear()
{
  dropWorkspace();
  bits_ = 0;
  have_solution_ = false;
  nv_ = nc_ = 0;
  P_ = Csc{};
  A_ = Csc{};
  q_.clear();
  lo_.clear();
  up_.clear();
  x0_.clear();
  y0_.clear();
  status_ = QPSolverStatus::kUninitialized;
  return true;
}

// the pattern changed under a live workspace: a setup with the data of this
// moment, warm started from the last solution, as a round of its own
bool GpuQPBatch::Slot::reinitKeepingSolution()
{
  const std::vector<double> xs = x_, ys = y_;
  const bool warm = have_solution_ && static_cast<long>(xs.size()) == nv_ && static_cast<long>(ys.size()) == nc_;
  bits_ = 0;  // what was recorded for the old workspace goes with it
  ++n_setups;
  wx_ = &xs;
  wy_ = &ys;
  batch_->submit(*this, kSetup | (warm ? kWarm : 0));
  wx_ = wy_ = nullptr;
  live_ = info_.status != -1;
  if (!live_)
    dropWorkspace();
  return live_;
}

bool GpuQPBatch::Slot::updateHessianMatrix(const trajopt_ifopt::Jacobian& hessian)
{
  Csc n;
  toCsc(hessian, true, 2.0, n);  // OSQP halves the quadratic term
  const bool same = n.p == P_.p && n.i == P_.i;
  P_ = std::move(n);
  if (!live_)
    return true;  // collected for the setup
  if (!same)
    return reinitKeepingSolution();
  bits_ |= kMatP;
  return true;
}

bool GpuQPBatch::Slot::updateGradient(const trajopt_ifopt::VectorXd& gradient)
{
  qp_data::cleanGradient(gradient, q_);
  if (live_)
    bits_ |= kVecQ;
  return true;
}

bool GpuQPBatch::Slot::updateLowerBound(const trajopt_ifopt::VectorXd& lowerBound)
{
  return updateBounds(lowerBound, up_.size() == lowerBound.size() ?
                                      up_ :
                                      trajopt_ifopt::VectorXd(lowerBound.size(), qp_data::kOsqpInfty));
}

bool GpuQPBatch::Slot::updateUpperBound(const trajopt_ifopt::VectorXd& upperBound)
{
  return updateBounds(lo_.size() == upperBound.size() ? lo_ :
                                                        trajopt_ifopt::VectorXd(upperBound.size(), -qp_data::kOsqpInfty),
                      upperBound);
}

bool GpuQPBatch::Slot::updateBounds(const trajopt_ifopt::VectorXd& lowerBound, const trajopt_ifopt::VectorXd& upperBound)
{
  std::vector<double> lo, up;
  qp_data::clampBounds(lowerBound, upperBound, lo, up);
  if (!live_)
  {
    lo_.swap(lo);
    up_.swap(up);
    return true;
  }
  bool ok = lo.size() == up.size();
  for (std::size_t r = 0; ok && r < lo.size(); ++r)
    ok = lo[r] <= up[r];
  if (!ok)
  {
    // osqp_update_data_vec refuses them and the workspace keeps its bounds: those
    // recorded before must have reached it, so they go as a round of their own
    if (bits_ & kBounds)
    {
      const int bits = bits_;
      bits_ = 0;
      batch_->submit(*this, bits);
      if (info_.status == -1)
        dropWorkspace();
    }
    lo_.swap(lo);
    up_.swap(up);
    info_ = thip_qp_info{};
    info_.status = -1;
    info_.setup_error = 1;
    return false;
  }
  lo_.swap(lo);
  up_.swap(up);
  bits_ |= kBounds;
  return true;
}

bool GpuQPBatch::Slot::updateLinearConstraintsMatrix(const trajopt_ifopt::Jacobian& linearConstraintsMatrix)
{
  if (linearConstraintsMatrix.rows() != nc_ || linearConstraintsMatrix.cols() != nv_)
    throw std::runtime_error("GpuQPBatch::Slot::updateLinearConstraintsMatrix: size mismatch");
  Csc n;
  toCsc(linearConstraintsMatrix, false, 1.0, n);
  const bool same = n.p == A_.p && n.i == A_.i;
  A_ = std::move(n);
  if (!live_)
    return true;
  if (!same)
    return reinitKeepingSolution();
  ++n_updates;  // one per convexification applied in place
  bits_ |= kMatA;
  return true;
}

bool GpuQPBatch::Slot::setWarmStart(const QPProblem& qp_problem)
{
  if (settings.warm_starting != 1)
    return true;
  qp_data::warmStartPoint(qp_problem, nv_, nc_, x0_, y0_);
  return true;
}

bool GpuQPBatch::Slot::solve()
{
  int bits = bits_ | kSolve;
  const bool setup = !live_;
  if (setup)
  {
    // OsqpEigen initSolver right before the first solve, then the stored warm start
    if (nv_ + nc_ > THIP_QP_MAX_KKT)  // the KKT capacity bounds the problem size: a limit, not a QP failure
      throw std::runtime_error("GpuQPBatch: the QP has " + std::to_string(nv_) + " variables and " +
                               std::to_string(nc_) + " constraints; the GPU QP solver takes n + m <= THIP_QP_MAX_KKT (" +
                               std::to_string(THIP_QP_MAX_KKT) + ")");
    ++n_setups;
    bits = kSetup | (settings.warm_starting == 1 ? kWarm : 0) | kSolve;
    wx_ = &x0_;
    wy_ = &y0_;
  }
  bits_ = 0;
  x_.assign(static_cast<std::size_t>(nv_), 0.0);
  y_.assign(static_cast<std::size_t>(nc_), 0.0);
  batch_->submit(*this, bits);
  wx_ = wy_ = nullptr;
  if (setup && info_.status == -1)
  {
    dropWorkspace();
    status_ = QPSolverStatus::kFailed;
    return false;
  }
  live_ = true;
  ++n_solves;
  admm_iters += info_.iter;
  have_solution_ = true;
  if (info_.status == 1 || info_.status == 2)
    return true;
  if (info_.status == -1)
    dropWorkspace();  // a refactorisation failed inside the step: set up again at the next solve
  status_ = QPSolverStatus::kFailed;
  return false;
}

trajopt_ifopt::VectorXd GpuQPBatch::Slot::getSolution() { return x_; }
}  // namespace trajopt_sqp
