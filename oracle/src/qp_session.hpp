// ORACLE — test infrastructure only (see sco_expr.hpp header).
//
// One OsqpSolver kept alive behind the calls of the OSQP 1.0 update-in-place
// API (osqp_setup, osqp_update_data_vec, osqp_update_data_mat, osqp_warm_start,
// osqp_solve), and the one-shot solve with OSQPModel's warm start: the
// reference of the direct tests of the device's generic QP kernel
// (tests/test_gpu_qp_direct.py).  thip_qp_info's conventions: status -1 with
// setup_error set when the solver object could not be built or was lost.
#pragma once
#include <memory>

#include "../../include/trajopt_hip.h"
#include "jitter.hpp"
#include "osqp_restated.hpp"

namespace orc
{
// thip_qp_info and what the oracle knows beyond it
struct QpInfoEx
{
  thip_qp_info info;
  int rho_updates;       // rho refactorisations of the last solve
  double polish_margin;  // smallest margin of the last polish's active-set comparisons
};

inline OsqpSettings osqpSettingsFrom(const thip_osqp_settings& s)
{
  OsqpSettings st;
  st.rho = s.rho;
  st.sigma = s.sigma;
  st.alpha = s.alpha;
  st.scaling = s.scaling;
  st.adaptive_rho = s.adaptive_rho;
  st.adaptive_rho_interval = s.adaptive_rho_interval;
  st.adaptive_rho_tolerance = s.adaptive_rho_tolerance;
  st.max_iter = s.max_iter;
  st.eps_abs = s.eps_abs;
  st.eps_rel = s.eps_rel;
  st.eps_prim_inf = s.eps_prim_inf;
  st.eps_dual_inf = s.eps_dual_inf;
  st.check_termination = s.check_termination;
  st.warm_starting = s.warm_starting;
  st.polishing = s.polishing;
  st.delta = s.delta;
  st.polish_refine_iter = s.polish_refine_iter;
  return st;
}

inline Csc cscFromArrays(int rows, int cols, const int* p, const int* i, const double* x)
{
  Csc M;
  M.m = rows;
  M.n = cols;
  M.p.assign(p, p + cols + 1);
  M.i.assign(i, i + p[cols]);
  M.x.assign(x, x + p[cols]);
  return M;
}

class QpSession
{
public:
  // osqp_setup on a fresh solver object (the old one is dropped): 0 or the OSQP error code
  int setup(int n, int m, const int* Pp, const int* Pi, const double* Px, const double* q, const int* Ap,
            const int* Ai, const double* Ax, const double* l, const double* u, const thip_osqp_settings& s)
  {
    jitterSeed(0);
    n_ = n;
    m_ = m;
    solver_ = std::make_unique<OsqpSolver>();
    const Csc P = cscFromArrays(n, n, Pp, Pi, Px), A = cscFromArrays(m, n, Ap, Ai, Ax);
    error_ = solver_->setup(P, q, A, l, u, m, n, osqpSettingsFrom(s));
    if (error_)
      solver_.reset();
    return error_;
  }
  // 1: l > u, the update is rejected and the solver object stays
  int update_vec(const double* q, const double* l, const double* u)
  {
    if (!solver_)
      return -1;
    return solver_->update_data_vec(q, l, u);
  }
  // 4 / 5: the refactorisation failed, the solver object is gone
  int update_mat(const double* Px, const double* Ax)
  {
    if (!solver_)
      return -1;
    const int e = solver_->update_data_mat(Px, Ax);
    if (e == 4 || e == 5)
    {
      error_ = e;
      solver_.reset();
    }
    return e;
  }
  int warm_start(const double* x, const double* y)
  {
    if (!solver_)
      return -1;
    return solver_->warm_start(x, y);
  }
  // x [n], y [m] (either may be NULL)
  void solve(double* x, double* y, QpInfoEx* out)
  {
    *out = QpInfoEx{};
    if (!solver_)
    {
      out->info.status = -1;
      out->info.setup_error = error_;
      return;
    }
    solver_->solve();
    fill(*solver_, n_, m_, x, y, out);
  }
  bool alive() const { return solver_ != nullptr; }

  static void fill(const OsqpSolver& s, int n, int m, double* x, double* y, QpInfoEx* out)
  {
    if (x)
      for (int j = 0; j < n; ++j)
        x[j] = s.sol_x[static_cast<std::size_t>(j)];
    if (y)
      for (int r = 0; r < m; ++r)
        y[r] = s.sol_y[static_cast<std::size_t>(r)];
    out->info.status = s.status_val;
    out->info.setup_error = 0;
    out->info.polish_status = s.status_polish;
    out->info.iter = static_cast<int>(s.iter);
    out->info.rho = s.settings().rho;
    out->info.prim_res = s.prim_res;
    out->info.dual_res = s.dual_res;
    out->rho_updates = s.rho_updates;
    out->polish_margin = s.polish_margin;
  }

private:
  std::unique_ptr<OsqpSolver> solver_;
  int n_ = 0, m_ = 0, error_ = 0;
};

// One QP from a fresh solver object, warm started as OSQPModel::createOrUpdateSolver
// does it (trajopt_sco/src/osqp_interface.cpp:283-370): warm_rho (> 0) into
// the settings before osqp_setup, then osqp_warm_start(warm_x, warm_y) when
// both are given.
inline void qpSolveInfo(int n, int m, const int* Pp, const int* Pi, const double* Px, const double* q,
                        const int* Ap, const int* Ai, const double* Ax, const double* l, const double* u,
                        const thip_osqp_settings& s, const double* warm_x, const double* warm_y, double warm_rho,
                        double* x, double* y, QpInfoEx* out)
{
  thip_osqp_settings st = s;
  if (warm_rho > 0)
    st.rho = warm_rho;
  QpSession session;
  if (session.setup(n, m, Pp, Pi, Px, q, Ap, Ai, Ax, l, u, st) == 0 && warm_x && warm_y)
    session.warm_start(warm_x, warm_y);
  session.solve(x, y, out);
}

}  // namespace orc
