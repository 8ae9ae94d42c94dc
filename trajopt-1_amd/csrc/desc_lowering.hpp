// Host side: where a problem descriptor (include/trajopt_hip.h) is lowered.
//
//   validate()      the fused kernel's domain: the descriptors thip_create,
//                   thip_terms_create and thip_terms_slot_table accept, one list
//                   of tests in one order, the first finding returned.
//   plan_terms()    a validated descriptor's term plan: hatch-clamped step
//                   ranges, kept CartPose components, collision units, and the
//                   cost / constraint slot of every term.  thip_create builds
//                   its rows and tables from it; the term-value evaluator copies
//                   it into its kernels' slot struct and the public slot table.
//   small pieces every evaluator's create repeats: the serial chain's parent
//                   table, the robot spheres grouped by link, the chain checks
//                   and the abi_version sentence of the generic evaluators.
//
// Plain C++ (no device code, no HIP types): host/tests/desc_lowering_san.cpp
// compiles it alone, with the sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "pair_data.hpp"
#include "self_pairs.hpp"

namespace thip
{
namespace lowering
{
// ---------------------------------------------------------------- small pieces

// a serial chain's parent[] is not read from the caller
inline void fill_serial_parents(thip_chain& ch)
{
  if (!ch.is_tree)
    for (int k = 0; k < THIP_MAX_LINKS; ++k)
      ch.parent[k] = k > 0 ? k - 1 : 0;
}

// The robot spheres grouped by link, ascending (the contact scan's order, the
// ContactResultMap key order): order = sphere indices sorted by (link, index);
// group g is link grp_link[g], entries [grp_s0[g], grp_s0[g] + grp_ns[g]) of order.
struct SphereGroups
{
  std::vector<int> order, grp_link, grp_s0, grp_ns;
};

inline SphereGroups group_spheres_by_link(const thip_problem_desc& d)
{
  SphereGroups g;
  for (int s = 0; s < d.n_spheres; ++s)
    g.order.push_back(s);
  std::stable_sort(g.order.begin(), g.order.end(), [&](int a, int b) { return d.sphere_link[a] < d.sphere_link[b]; });
  for (size_t k = 0; k < g.order.size(); ++k)
  {
    const int link = d.sphere_link[g.order[k]];
    if (g.grp_link.empty() || g.grp_link.back() != link)
    {
      g.grp_link.push_back(link);
      g.grp_s0.push_back(static_cast<int>(k));
      g.grp_ns.push_back(0);
    }
    g.grp_ns.back()++;
  }
  return g;
}

// ... into a device model's arrays (n_groups, grp_link, grp_s0, grp_ns, sph_order: THIP_MAX_SPHERES each)
template <class DeviceModel>
inline void store_sphere_groups(const SphereGroups& g, DeviceModel& m)
{
  m.n_groups = static_cast<int>(g.grp_link.size());
  std::copy(g.grp_link.begin(), g.grp_link.end(), m.grp_link);
  std::copy(g.grp_s0.begin(), g.grp_s0.end(), m.grp_s0);
  std::copy(g.grp_ns.begin(), g.grp_ns.end(), m.grp_ns);
  std::copy(g.order.begin(), g.order.end(), m.sph_order);
}

// What the device models of the robot's spheres share: n_sph, center, radius
// and the self-collision sphere pairs (ssa, ssb: self_sphere_pairs).  A model's
// own fields (link, where it has one) stay with its create.
template <class DeviceModel>
inline void fill_sphere_model(const thip_problem_desc& d, const std::vector<int>& ssa, const std::vector<int>& ssb,
                              DeviceModel& m)
{
  m.n_sph = d.n_spheres;
  m.n_self_sph = static_cast<int>(ssa.size());
  std::copy(ssa.begin(), ssa.end(), m.self_sa);
  std::copy(ssb.begin(), ssb.end(), m.self_sb);
  for (int s = 0; s < d.n_spheres; ++s)
  {
    m.radius[s] = d.sphere_radius[s];
    for (int i = 0; i < 3; ++i)
      m.center[s][i] = d.sphere_center[s][i];
  }
}

// "" or the generic evaluators' sentence for a descriptor of another header
inline std::string abi_mismatch(const thip_problem_desc& d)
{
  if (d.abi_version == THIP_ABI_VERSION)
    return "";
  return "descriptor abi_version " + std::to_string(d.abi_version) + " != THIP_ABI_VERSION " +
         std::to_string(THIP_ABI_VERSION);
}

// the generic evaluators' chain checks: null or the finding
inline const char* chain_range_finding(const thip_chain& ch)
{
  if (ch.n_dof <= 0 || ch.n_dof > THIP_MAX_DOF || ch.n_links < 1 || ch.n_links > THIP_MAX_LINKS)
    return "chain out of range";
  return nullptr;
}

inline const char* chain_table_finding(const thip_chain& ch)
{
  for (int k = 1; k < ch.n_links; ++k)
    if ((ch.joint_type[k] < 0 || ch.joint_type[k] > 3) ||
        (ch.joint_type[k] != THIP_JOINT_FIXED && (ch.joint_dof[k] < 0 || ch.joint_dof[k] >= ch.n_dof)) ||
        (ch.is_tree && (ch.parent[k] < 0 || ch.parent[k] >= k)))
      return "bad chain joint / parent table";
  return nullptr;
}

// thip_jdt_fused (trajopt_hip.h)
inline bool jdt_fused(const thip_problem_desc& d)
{
  if (d.n_jdt == 0)
    return true;
  if (d.n_jdt < 0 || d.n_jdt > THIP_MAX_JDT || d.n_steps % 2 != 0 || 2 * d.chain.n_dof > THIP_MAX_DOF || d.use_time)
    return false;
  for (int k = 0; k < d.n_jdt; ++k)
  {
    if (d.jdt_order[k] != 2 || d.jdt_is_cnt[k])
      return false;
    for (int j = 0; j < d.chain.n_dof; ++j)
      if (d.jdt_upper_tols[k][j] >= 1e-5 || d.jdt_upper_tols[k][j] <= -1e-5 || d.jdt_lower_tols[k][j] >= 1e-5 ||
          d.jdt_lower_tols[k][j] <= -1e-5)
        return false;
  }
  return true;
}

// ------------------------------------------------------------------ validation

// What validate() found.  kRefused: `why` is the whole reason, the same words
// for every caller.  The findings after it are worded per caller: each entry
// point keeps a sentence per enumerator and appends it to `why` (which holds
// what the wordings share: the versions, the n_steps range; else nothing).
enum Finding : int
{
  kAccepted = 0,
  kRefused,
  kAbiVersion,        // why: "descriptor abi_version A != THIP_ABI_VERSION B"
  kStepsRange,        // why: "n_steps must be in [2, THIP_MAX_STEPS]"
  kJvxZeroTols,       // a jvx term with zero tolerances
  kJdtNotFused,       // !thip_jdt_fused
  kTimeOrFixedDofs,   // use_time, n_jvt, n_ttt, n_fixed_dofs
  kCartVel,           // n_cvel
  kCollExtra,         // n_coll_extra
  kPrimsRange,        // n_prims outside [0, THIP_MAX_PRIMS]
  kFindingCount
};

inline Finding validate(const thip_problem_desc& d, std::string& why)
{
  const auto refuse = [&why](const std::string& m) { return why = m, kRefused; };
  why = abi_mismatch(d);
  if (!why.empty())
    return kAbiVersion;
  const thip_chain& ch = d.chain;
  if (ch.n_dof <= 0 || ch.n_dof > THIP_MAX_DOF)
    return refuse("n_dof out of range");
  if (ch.n_links < 1 || ch.n_links > THIP_MAX_LINKS)
    return refuse("n_links out of range");
  if (d.n_steps < 2 || d.n_steps > THIP_MAX_STEPS)
    return why = "n_steps must be in [2, " + std::to_string(THIP_MAX_STEPS) + "]", kStepsRange;
  for (int k = 1; k < ch.n_links; ++k)
  {
    const int ty = ch.joint_type[k];
    if (ty < 0 || ty > 3)
      return refuse("bad joint type");
    if (ty != THIP_JOINT_FIXED && (ch.joint_dof[k] < 0 || ch.joint_dof[k] >= ch.n_dof))
      return refuse("bad joint dof index");
    if (ch.is_tree && (ch.parent[k] < 0 || ch.parent[k] >= k))
      return refuse("bad parent link (links must be in tree order, 0 <= parent[k] < k)");
  }
  if (d.n_fixed < 0 || d.n_fixed > THIP_MAX_STEPS)
    return refuse("n_fixed out of range");
  {
    bool seen[THIP_MAX_STEPS] = {};
    for (int f = 0; f < d.n_fixed; ++f)
    {
      const int t = d.fixed_steps[f];
      if (t < 0 || t >= d.n_steps)
        return refuse("Fixed timestep index is outside the bounds of the initial trajectory.");
      if (seen[t])
        return refuse("duplicate fixed timestep");
      seen[t] = true;
    }
  }
  if (d.n_cart < 0 || d.n_cart > THIP_MAX_CART)
    return refuse("n_cart out of range");
  for (int k = 0; k < d.n_cart; ++k)
  {
    if (d.cart_step[k] < 0 || d.cart_step[k] >= d.n_steps)
      return refuse("CartPose timestep out of range");
    if (d.cart_source_link[k] <= 0 || d.cart_source_link[k] >= ch.n_links)
      return refuse("CartPose source frame must be an active chain link");
    if (d.cart_target_link[k] < 0 || d.cart_target_link[k] >= ch.n_links)
      return refuse("CartPose target link out of range (0: the static chain root)");
  }
  // JointVelTermInfo::hatch clamps a first step from above only and asserts first_step >= 0
  // (problem_description.cpp:1227-1251); the kernels index x with the clamped steps
  if (d.jv_enabled && d.jv_first_step < 0)
    return refuse("jv_first_step must be >= 0");
  if (d.n_jvx < 0 || d.n_jvx > THIP_MAX_JVX)
    return refuse("n_jvx out of range");
  for (int x = 0; x < d.n_jvx; ++x)
  {
    if (d.jvx_first_step[x] < 0)
      return refuse("jvx term " + std::to_string(x) + ": jvx_first_step must be >= 0");
    bool tol = false;
    for (int j = 0; j < ch.n_dof; ++j)
      tol = tol || std::fabs(d.jvx_upper_tols[x][j]) >= 1e-5 || std::fabs(d.jvx_lower_tols[x][j]) >= 1e-5;
    if (!tol)
      return kJvxZeroTols;
  }
  if (!jdt_fused(d))
    return kJdtNotFused;
  // the kernels index x with a JointAccEqCost term's steps as given (jacc_value,
  // build_and_scale, term_values.hip): the range JointAccTermInfo::hatch clamps to
  for (int k = 0; k < d.n_jdt; ++k)
    if (d.jdt_first_step[k] < 0 || d.jdt_last_step[k] > d.n_steps - 1 || d.jdt_last_step[k] < 2 ||
        d.jdt_first_step[k] > d.jdt_last_step[k] - 2)  // (first + 2 > last, without the overflow)
      return refuse("jdt term " + std::to_string(k) + ": need 0 <= jdt_first_step and jdt_first_step + 2 <= "
                    "jdt_last_step <= n_steps - 1 (got " + std::to_string(d.jdt_first_step[k]) + ", " +
                    std::to_string(d.jdt_last_step[k]) + " on " + std::to_string(d.n_steps) + " waypoints)");
  if (d.use_time != 0 || d.n_jvt != 0 || d.n_ttt != 0 || d.n_fixed_dofs != 0)
    return kTimeOrFixedDofs;
  if (d.n_cvel != 0)
    return kCartVel;
  if (d.coll_enabled && d.coll_contact_test != THIP_CONTACT_ALL && d.coll_contact_test != THIP_CONTACT_FIRST &&
      d.coll_contact_test != THIP_CONTACT_CLOSEST)
    return refuse("coll_contact_test is not a THIP_CONTACT_* value");
  if (d.n_coll_extra != 0)
    return kCollExtra;
  if (d.n_jpos < 0 || d.n_jpos > THIP_MAX_JPOS)
    return refuse("n_jpos out of range");
  for (int k = 0; k < d.n_jpos; ++k)
    for (int j = 0; j < ch.n_dof; ++j)
      if (!std::isfinite(d.jpos_coeffs[k][j]) || !std::isfinite(d.jpos_targets[k][j]) ||
          !std::isfinite(d.jpos_upper_tols[k][j]) || !std::isfinite(d.jpos_lower_tols[k][j]))
        return refuse("JointPos coeffs / targets / tolerances must be finite");
  if (d.coll_enabled)
  {
    if (d.n_spheres < 1 || d.n_spheres > THIP_MAX_SPHERES)
      return refuse("collision: n_spheres out of range");
    for (int s = 0; s < d.n_spheres; ++s)
      if (d.sphere_link[s] < 1 || d.sphere_link[s] >= ch.n_links || !(d.sphere_radius[s] >= 0))
        return refuse("collision: bad robot sphere");
    if (d.n_prims < 0 || d.n_prims > THIP_MAX_PRIMS)
      return kPrimsRange;
    const int last = d.coll_last_step < 0 ? d.n_steps - 1 : d.coll_last_step;
    if (d.coll_first_step < 0 || d.coll_first_step >= d.n_steps || last < d.coll_first_step || last >= d.n_steps)
      return refuse("collision: bad first/last step");
    if (d.coll_continuous < 0 || d.coll_continuous > 2)
      return refuse("collision: coll_continuous must be 0 (LVS_DISCRETE), 1 (LVS_CONTINUOUS) or 2 (DISCRETE)");
    const bool single = d.coll_continuous == 2;
    if ((!single && !(d.coll_lvs > 0)) || !(d.coll_buffer >= 0))
      return refuse("collision: bad longest_valid_segment_length / buffer");
    if (d.coll_n_fixed < 0 || d.coll_n_fixed > THIP_MAX_STEPS)
      return refuse("collision: coll_n_fixed out of range");
    // (single-timestep terms skip fixed waypoints; only the step-pair evaluators reject
    // adjacent fixed steps, problem_description.cpp:1765-1767 vs :1785-1795)
    for (int t = d.coll_first_step; !single && t < last; ++t)
    {
      bool a = false, b = false;
      for (int k = 0; k < d.coll_n_fixed; ++k)
      {
        a |= d.coll_fixed_steps[k] == t;
        b |= d.coll_fixed_steps[k] == t + 1;
      }
      if (a && b)
        return refuse("Currently two adjacent fixed steps are not supported in collision term.");
    }
  }
  for (int k = 0; k < d.n_cart; ++k)
    if (d.cart_has_tol[k])
      for (int i = 0; i < 6; ++i)
        if (!(d.cart_lower_tol[k][i] <= d.cart_upper_tol[k][i]))
          return refuse("CartPoseErrCalculator: Inverted tolerance band - lower > upper at one or more indices");
  if (d.coll_enabled && (d.coll_max_contacts < 0 || d.coll_max_contacts > THIP_MAX_CONTACTS))
    return refuse("collision: coll_max_contacts out of range");
  if (d.coll_enabled)
  {
    std::vector<int> sa, sb, kp;
    const std::string w = self_sphere_pairs(d, sa, sb, kp);
    if (!w.empty())
      return refuse(w);
  }
  {
    const std::string w = validate_coll_pairs(d);
    if (!w.empty())
      return refuse(w);
  }
  // (the term-value evaluator reads neither, but its domain is thip_create's)
  if (!(d.sqp.max_time >= 0))
    return refuse("sqp.max_time must be >= 0 (DBL_MAX: no limit)");
  if (!(d.sqp.trust_shrink_ratio > 0 && d.sqp.trust_shrink_ratio < 1) || !(d.sqp.min_trust_box_size > 0) ||
      !(d.sqp.trust_box_size > 0))
    return refuse("sqp: need 0 < trust_shrink_ratio < 1, min_trust_box_size > 0 and trust_box_size > 0");
  if (d.osqp.check_termination < 0 || d.osqp.max_iter < 1 || d.osqp.scaling < 0)
    return refuse("bad OSQP settings");
  return kAccepted;
}

// ------------------------------------------------------------------- term plan

// Slots: costs and constraints are numbered apart, each from 0, in the order
// the reference's OptProb holds them (ConstructProblem's cost_infos, then
// cnt_infos): JointVel (cost slot 0), CartPose costs, JointPos costs, jvx costs,
// JointAccEqCost terms, [collision units]; CartPose constraints, JointPos
// constraints, jvx constraints, [collision units].  The tests pin the numbering
// against the solver's A_COST / A_VIOL.
struct TermPlan
{
  int N, D;
  // JointVelTermInfo::hatch-clamped steps; jv_ineq: the tolerance (hinge) form
  int jv_first, jv_last, jv_ineq;
  int jvx_first[THIP_MAX_JVX], jvx_last[THIP_MAX_JVX], jvx_slot[THIP_MAX_JVX];
  // JointPosTermInfo::hatch-clamped steps; jpos_ineq: the tolerance (hinge) form
  int jpos_first[THIP_MAX_JPOS], jpos_last[THIP_MAX_JPOS], jpos_slot[THIP_MAX_JPOS], jpos_ineq[THIP_MAX_JPOS];
  int jacc_slot[THIP_MAX_JDT];  // -1 past n_jdt
  // CartPose term k: its kept components (|coefficient| > 1e-5) with their weights, its slot
  int cart_nrow[THIP_MAX_CART], cart_comp[THIP_MAX_CART][6], cart_slot[THIP_MAX_CART];
  double cart_w[THIP_MAX_CART][6];
  int cart_order[THIP_MAX_CART];  // the terms in emission order: cost terms (convexifyCosts), then constraint terms
  // collision units [coll_first, coll_last): step pairs, or with coll_single (DISCRETE) the
  // waypoints that are not fixed steps; unit u starts at waypoint unit_t[u], slot coll_cost0 + u
  int coll, coll_first, coll_last, coll_single, coll_cnt, coll_cost0;
  int coll_fixed[THIP_MAX_STEPS];  // per waypoint: 1 if a collision fixed step
  int n_units, unit_t[THIP_MAX_STEPS];
  int n_costs, n_cnts;
  std::vector<thip_term_slot> table;  // thip_terms_slots: the cost slots, then the constraint slots
};

// d: accepted by validate()
inline void plan_terms(const thip_problem_desc& d, TermPlan& P)
{
  P = TermPlan();
  const int N = P.N = d.n_steps, D = P.D = d.chain.n_dof;
  // JointVelTermInfo::hatch step clamping (problem_description.cpp:1228-1245)
  auto jv_clamp = [N](int first, int last, int& f_out, int& l_out) {
    if (last <= -1)
      last = N - 1;
    if ((N - 2) <= first)
      first = N - 2;
    if ((N - 1) <= last)
      last = N - 1;
    if (last == first)
      last += 1;
    if (last < first)
      std::swap(first, last);
    f_out = first;
    l_out = last;
  };
  jv_clamp(d.jv_first_step, d.jv_last_step, P.jv_first, P.jv_last);
  for (int x = 0; x < d.n_jvx; ++x)
    jv_clamp(d.jvx_first_step[x], d.jvx_last_step[x], P.jvx_first[x], P.jvx_last[x]);
  // zero tolerances: trajopt_common::doubleEquals(tol, 0.) (problem_description.cpp:1135-1138,1249-1252)
  auto zero_tol = [](double v) { return std::fabs(v) < 1e-5; };
  if (d.jv_enabled)
    for (int j = 0; j < D; ++j)
      if (!zero_tol(d.jv_upper_tols[j]) || !zero_tol(d.jv_lower_tols[j]))
        P.jv_ineq = 1;
  for (int k = 0; k < d.n_jpos; ++k)
    for (int j = 0; j < D; ++j)
      if (!zero_tol(d.jpos_upper_tols[k][j]) || !zero_tol(d.jpos_lower_tols[k][j]))
        P.jpos_ineq[k] = 1;
  std::vector<thip_term_slot> cnt_tab;
  // the term's slot, entered in its table
  auto take = [&](int kind, int index, int unit, int is_cnt) {
    thip_term_slot e;
    e.kind = kind;
    e.index = index;
    e.unit = unit;
    e.is_cnt = is_cnt;
    (is_cnt ? cnt_tab : P.table).push_back(e);
    return is_cnt ? P.n_cnts++ : P.n_costs++;
  };
  if (d.jv_enabled)
    take(THIP_TERM_JOINT_VEL, 0, -1, 0);
  // CartPose terms: cost terms first, then constraint terms (cntsToCosts), each in descriptor order
  int n_emitted = 0;
  for (int pass = 0; pass < 2; ++pass)
    for (int k = 0; k < d.n_cart; ++k)
    {
      if ((pass == 0) != (d.cart_is_cnt[k] == 0))
        continue;
      for (int i = 0; i < 6; ++i)
      {
        const double cf = (i < 3) ? d.cart_pos_coeffs[k][i] : d.cart_rot_coeffs[k][i - 3];
        if (std::fabs(cf) > 1e-5)
        {
          P.cart_comp[k][P.cart_nrow[k]] = i;
          P.cart_w[k][P.cart_nrow[k]] = cf;
          P.cart_nrow[k]++;
        }
      }
      P.cart_slot[k] = take(THIP_TERM_CART, k, -1, pass);
      P.cart_order[n_emitted++] = k;
    }
  // JointPosTermInfo::hatch step clamping (problem_description.cpp:1097-1196)
  for (int k = 0; k < d.n_jpos; ++k)
  {
    int f = d.jpos_first_step[k], l = d.jpos_last_step[k];
    if (l <= -1)
      l = N - 1;
    if ((N - 1) <= f)
      f = N - 1;
    if ((N - 1) <= l)
      l = N - 1;
    if (l < f)
      std::swap(f, l);
    f = std::max(f, 0);
    P.jpos_first[k] = f;
    P.jpos_last[k] = l;
    if (!d.jpos_is_cnt[k])
      P.jpos_slot[k] = take(THIP_TERM_JPOS, k, -1, 0);
  }
  for (int x = 0; x < d.n_jvx; ++x)
    if (!d.jvx_is_cnt[x])
      P.jvx_slot[x] = take(THIP_TERM_JVX, x, -1, 0);
  // JointAccEqCost terms (thip_jdt_fused): cost slots after the JointVel
  // tolerance costs (the oracle's / ConstructProblem's cost order)
  for (int k = 0; k < THIP_MAX_JDT; ++k)
    P.jacc_slot[k] = (k < d.n_jdt) ? take(THIP_TERM_JDT, k, -1, 0) : -1;
  for (int k = 0; k < d.n_jpos; ++k)
    if (d.jpos_is_cnt[k])
      P.jpos_slot[k] = take(THIP_TERM_JPOS, k, -1, 1);
  for (int x = 0; x < d.n_jvx; ++x)
    if (d.jvx_is_cnt[x])
      P.jvx_slot[x] = take(THIP_TERM_JVX, x, -1, 1);
  // collision: one term per unit after the other costs (cost_infos order; CollisionTermInfo::hatch,
  // problem_description.cpp:1747) or, in the constraint form, after the other constraints
  // (problem_description.cpp:1797-1840 / OptProb eq-then-ineq order)
  P.coll = d.coll_enabled ? 1 : 0;
  P.coll_first = d.coll_first_step;
  P.coll_last = (d.coll_last_step < 0) ? N - 1 : d.coll_last_step;
  // DISCRETE: one SingleTimestepCollisionEvaluator term per waypoint of [first, last] that is
  // not a fixed step (problem_description.cpp:1782-1796)
  P.coll_single = (P.coll && d.coll_continuous == 2) ? 1 : 0;
  if (P.coll_single)
    P.coll_last += 1;
  P.coll_cnt = (P.coll && d.coll_is_cnt) ? 1 : 0;
  P.coll_cost0 = P.coll_cnt ? P.n_cnts : P.n_costs;
  for (int k = 0; P.coll && k < d.coll_n_fixed; ++k)
    if (d.coll_fixed_steps[k] >= 0 && d.coll_fixed_steps[k] < N)
      P.coll_fixed[d.coll_fixed_steps[k]] = 1;
  for (int t = P.coll_first; P.coll && t < P.coll_last; ++t)
    if (!(P.coll_single && P.coll_fixed[t]))
    {
      take(THIP_TERM_COLL, P.n_units, t, P.coll_cnt);
      P.unit_t[P.n_units++] = t;
    }
  P.table.insert(P.table.end(), cnt_tab.begin(), cnt_tab.end());
}
}  // namespace lowering
}  // namespace thip
