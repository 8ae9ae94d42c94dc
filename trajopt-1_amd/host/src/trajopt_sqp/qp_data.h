// What GpuQPSolver and GpuQPBatch::Slot share: how a QPSolver's update calls
// become the arrays a thip_qp takes (OSQPEigenSolver's conversions,
// trajopt_optimizers/trajopt_sqp/src/osqp_eigen_solver.cpp:160-324).
#pragma once
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "trajopt_ifopt/core/eigen_types.h"
#include "trajopt_sqp/qp_problem.h"

namespace trajopt_sqp
{
namespace qp_data
{
constexpr double kOsqpInfty = 1e30;  // OSQP_INFTY

struct Csc
{
  std::vector<int> p, i;
  std::vector<double> x;
  bool samePattern(const Csc& o) const { return p == o.p && i == o.i; }
};

// CSC of a row-major matrix (all stored entries, zeros included), optionally the
// upper triangle only, scaled
inline void toCsc(const trajopt_ifopt::Jacobian& J, bool upper, double scale, Csc& out)
{
  const long n = J.cols();
  std::vector<std::vector<std::pair<int, double>>> col(static_cast<std::size_t>(n));
  for (long r = 0; r < J.rows(); ++r)
    for (long e = J.rowBegin(r); e < J.rowEnd(r); ++e)
      if (!upper || r <= J.col(e))
        col[static_cast<std::size_t>(J.col(e))].emplace_back(static_cast<int>(r), J.value(e) * scale);
  out.p.assign(static_cast<std::size_t>(n) + 1, 0);
  out.i.clear();
  out.x.clear();
  for (long j = 0; j < n; ++j)
  {
    for (const auto& e : col[static_cast<std::size_t>(j)])  // rows ascending: row-major scan order
    {
      out.i.push_back(e.first);
      out.x.push_back(e.second);
    }
    out.p[static_cast<std::size_t>(j) + 1] = static_cast<int>(out.i.size());
  }
}

// the gradient with its entries below 1e-7 cleaned to zero
inline void cleanGradient(const trajopt_ifopt::VectorXd& gradient, std::vector<double>& q)
{
  q.resize(gradient.size());
  for (std::size_t j = 0; j < gradient.size(); ++j)
    q[j] = (std::abs(gradient[j]) < 1e-7) ? 0.0 : gradient[j];
}

// the bounds clamped to +-OSQP_INFTY
inline void clampBounds(const trajopt_ifopt::VectorXd& lower, const trajopt_ifopt::VectorXd& upper,
                        std::vector<double>& lo, std::vector<double>& up)
{
  lo.resize(lower.size());
  up.resize(upper.size());
  for (std::size_t r = 0; r < lower.size(); ++r)
    lo[r] = std::max(lower[r], -kOsqpInfty);
  for (std::size_t r = 0; r < upper.size(); ++r)
    up[r] = std::min(upper[r], kOsqpInfty);
}

// osqp_eigen_solver.cpp:267-324: primal start = [NLP values; slacks], the slack
// of constraint-matrix row k from convex violation k (the reference pairs the
// k-th merit violation with the k-th matrix row), dual start 0
inline void warmStartPoint(const QPProblem& qp_problem, long nv, long nc, std::vector<double>& x0,
                           std::vector<double>& y0)
{
  const long nn = qp_problem.getNumNLPVars();
  x0.assign(static_cast<std::size_t>(nv), 0.0);
  const trajopt_ifopt::VectorXd vars = qp_problem.getVariableValues();
  std::copy(vars.begin(), vars.begin() + nn, x0.begin());
  if (nv > nn)
  {
    const trajopt_ifopt::VectorXd viol = qp_problem.evaluateConvexConstraintViolations(vars);
    const trajopt_ifopt::Jacobian& A = qp_problem.getConstraintMatrix();
    for (long k = 0; k < static_cast<long>(viol.size()) && k < A.rows(); ++k)
      for (long e = A.rowBegin(k); e < A.rowEnd(k); ++e)
        if (A.col(e) >= nn && std::abs(A.value(e)) > 1e-14)
          x0[static_cast<std::size_t>(A.col(e))] = std::max(0.0, viol[static_cast<std::size_t>(k)] / A.value(e));
  }
  y0.assign(static_cast<std::size_t>(nc), 0.0);
}
}  // namespace qp_data
}  // namespace trajopt_sqp
