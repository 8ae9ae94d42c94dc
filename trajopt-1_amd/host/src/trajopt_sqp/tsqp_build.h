// Shared by the C entry points of the trajopt_sqp front end (tsqp_capi.cpp,
// tsqp_kin_capi.cpp): a tsqp_spec as NodesVariables + joint constraint sets in a
// TrajOptQPProblem, and the solve of a built problem.
#pragma once
#include <memory>
#include <vector>

#include "trajopt_host.h"
#include "trajopt_ifopt/core/constraint_set.h"
#include "trajopt_sqp/trajopt_qp_problem.h"

namespace trajopt_sqp
{
namespace capi
{
struct Built
{
  std::shared_ptr<trajopt_ifopt::NodesVariables> variables;
  std::vector<std::shared_ptr<const trajopt_ifopt::Var>> vars;  // one per node
  std::shared_ptr<TrajOptQPProblem> problem;
  std::vector<std::shared_ptr<trajopt_ifopt::ConstraintSet>> sets;  // in the order they were added
};
// the spec's variables and joint terms (`who` prefixes the error messages)
Built buildJointProblem(const tsqp_spec* spec, const char* who);
// setup + TrustRegionSQPSolver over a GpuQPSolver with the spec's parameters: x [n_nodes][n_dof], result may be null
void solveBuilt(Built& b, const tsqp_spec* spec, int device, const char* who, double* x, tsqp_result* result);
}  // namespace capi
}  // namespace trajopt_sqp
