// Shared by the C entry points of the trajopt_sqp front end (tsqp_capi.cpp,
// tsqp_kin_capi.cpp): a tsqp_spec as NodesVariables + joint constraint sets in a
// TrajOptQPProblem, and the solve of a built problem.
#pragma once
#include <functional>
#include <memory>
#include <vector>

#include "trajopt_host.h"
#include "trajopt_ifopt/core/constraint_set.h"
#include "trajopt_sqp/trajopt_qp_problem.h"
#include "trajopt_sqp/types.h"

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
// the spec's SQPParameters
SQPParameters paramsOf(const tsqp_spec* spec);
// the spec with the kinematic sets of `kin` added after its joint terms (tsqp_kin_capi.cpp).  `keep` owns the
// environment and the device evaluators of the sets; set_launches: the launches of the CartPos evaluator [0] and of
// the collision evaluators [1] so far, as thost_tsqp_eval_kin counts them.
struct KinProblem
{
  Built joint;
  std::shared_ptr<void> keep;
  std::function<void(long long* out)> set_launches;
};
KinProblem buildKinProblem(const tsqp_spec* spec, const tsqp_kin_spec* kin, int device, const char* who);
// setup + TrustRegionSQPSolver over a GpuQPSolver with the spec's parameters: x [n_nodes][n_dof], result may be null
void solveBuilt(Built& b, const tsqp_spec* spec, int device, const char* who, double* x, tsqp_result* result);
}  // namespace capi
}  // namespace trajopt_sqp
