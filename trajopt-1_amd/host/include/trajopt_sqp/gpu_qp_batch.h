// trajopt_sqp::GpuQPBatch: the QPs of many TrustRegionSQPSolvers that run in
// lock step, one resident thip_qp workspace per pattern instead of one per
// problem.  Each solver gets a GpuQPBatch::Slot, a QPSolver that behaves like
// GpuQPSolver (the same conversions, warm start and counters) except that its
// update calls only record data and set THIP_QP_OP_* bits: solve() submits the
// bits and blocks, and when every running client is waiting the round runs as
// one thip_qp_step per group -- the slots that share P and A pattern, sizes and
// OSQP settings.  The rendezvous is sco::GpuQPBatcher's: enter / leave, the
// arrival that completes a round flushes it.
//
// Where deferring differs from GpuQPSolver's eager calls:
//  - updateBounds checks l <= u on the host at once and returns false, so the
//    solver's rebuild() runs as with GpuQPSolver;
//  - an operation recorded twice before a solve keeps the later data (the bounds
//    pushed after an accepted step, then again by the next convexification);
//  - a refactorisation that fails inside a step surfaces at solve(): false,
//    kFailed, and the slot is set up again at its next solve (GpuQPSolver would
//    have returned false from the update call and been rebuilt immediately);
//  - a pattern change under a live slot is a round of its own (SETUP | WARM, no
//    SOLVE) with the data of that moment, as GpuQPSolver::reinitKeepingSolution
//    sets up before the remaining updates arrive.
#pragma once
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "trajopt_hip.h"
#include "trajopt_sqp/qp_solver.h"

namespace trajopt_sqp
{
class GpuQPBatch : public std::enable_shared_from_this<GpuQPBatch>
{
public:
  // The device calls a batch makes; the defaults are thip_qp_create / thip_qp_step /
  // thip_qp_destroy / thip_qp_last_error.  A test injects its own.
  struct Device
  {
    std::function<int(int device, int n, int m, const int* Pp, const int* Pi, const int* Ap, const int* Ai, int batch,
                      thip_qp** out)>
        create;
    std::function<int(thip_qp* qp, const int* ops, const double* P, const double* q, const double* A, const double* l,
                      const double* u, const thip_osqp_settings* s, const double* wx, const double* wy, double* x,
                      double* y, thip_qp_info* info)>
        step;
    std::function<void(thip_qp*)> destroy;
    std::function<std::string(thip_qp*)> last_error;
    static Device hip();
  };
  struct Stats
  {
    long long rounds = 0;         // rendezvous rounds flushed
    long long step_launches = 0;  // thip_qp_step calls (one per group with a waiting slot, per round)
    long long groups = 0;         // thip_qp objects created (one symbolic analysis each)
    long long max_group = 0;      // the largest batch of one
  };

  class Slot;

  explicit GpuQPBatch(int device = 0, Device dev = Device::hip());
  ~GpuQPBatch();
  GpuQPBatch(const GpuQPBatch&) = delete;
  GpuQPBatch& operator=(const GpuQPBatch&) = delete;

  // A client is a thread that will submit: a round waits for every client that
  // has entered and not left.  All clients enter before any of them submits.
  void enter();
  void leave();
  // a QPSolver for one problem, owned by the caller, used from one client thread
  std::shared_ptr<Slot> makeSlot();
  Stats stats() const;

private:
  friend class Slot;
  struct Group
  {
    thip_qp* qp = nullptr;
    std::string key;
    int n = 0, m = 0, capacity = 0;
    std::size_t np = 0, na = 0;
    thip_osqp_settings settings{};
    std::vector<Slot*> owner;  // per index; null = free
    std::vector<int> ops;
    std::vector<double> P, q, A, l, u, wx, wy, x, y;
    std::vector<thip_qp_info> info;
  };
  // submit `bits` of a slot and block until its round has run; throws what the round reported for the slot
  void submit(Slot& s, int bits);
  void release(Slot& s);  // a slot gives its index back (under the lock)
  void flushLocked();
  static std::string keyOf(const Slot& s);

  const int device_;
  Device dev_;
  mutable std::mutex mu_;
  std::condition_variable cv_;
  int active_ = 0;
  std::vector<Slot*> pending_;
  std::multimap<std::string, std::unique_ptr<Group>> groups_;
  Stats stats_;
};

class GpuQPBatch::Slot : public QPSolver
{
public:
  ~Slot() override;
  Slot(const Slot&) = delete;
  Slot& operator=(const Slot&) = delete;
  bool init(long num_vars, long num_cnts) override;
  bool clear() override;
  bool solve() override;
  trajopt_ifopt::VectorXd getSolution() override;
  bool updateHessianMatrix(const trajopt_ifopt::Jacobian& hessian) override;
  bool updateGradient(const trajopt_ifopt::VectorXd& gradient) override;
  bool updateLowerBound(const trajopt_ifopt::VectorXd& lowerBound) override;
  bool updateUpperBound(const trajopt_ifopt::VectorXd& upperBound) override;
  bool updateBounds(const trajopt_ifopt::VectorXd& lowerBound, const trajopt_ifopt::VectorXd& upperBound) override;
  bool updateLinearConstraintsMatrix(const trajopt_ifopt::Jacobian& linearConstraintsMatrix) override;
  bool setWarmStart(const QPProblem& qp_problem) override;
  QPSolverStatus getSolverStatus() const override { return status_; }

  thip_osqp_settings settings;  // applied at the next setup (GpuQPSolver::setDefaultOSQPSettings at first)
  // GpuQPSolver's counters, and the rounds this slot took part in
  int n_setups = 0, n_updates = 0, n_solves = 0, n_rounds = 0;
  long long admm_iters = 0;
  const thip_qp_info& lastInfo() const { return info_; }

private:
  friend class GpuQPBatch;
  explicit Slot(std::shared_ptr<GpuQPBatch> batch);
  struct Csc
  {
    std::vector<int> p, i;
    std::vector<double> x;
  };
  bool reinitKeepingSolution();
  void dropWorkspace();
  std::shared_ptr<GpuQPBatch> batch_;
  QPSolverStatus status_ = QPSolverStatus::kUninitialized;
  long nv_ = 0, nc_ = 0;
  bool live_ = false;  // the slot owns a live workspace of a group
  Csc P_, A_;
  std::vector<double> q_, lo_, up_, x0_, y0_, x_, y_;
  thip_qp_info info_{};
  bool have_solution_ = false;
  int bits_ = 0;  // operations recorded since the last round
  // the round's side (GpuQPBatch, under its lock)
  GpuQPBatch::Group* group_ = nullptr;
  int index_ = -1;
  int submitted_ = 0;
  const std::vector<double>*wx_ = nullptr, *wy_ = nullptr;  // the warm start of a submitted WARM
  bool done_ = false;
  std::string error_;
};
}  // namespace trajopt_sqp
