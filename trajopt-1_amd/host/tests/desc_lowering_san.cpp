// The descriptor lowering (csrc/desc_lowering.hpp: validate, plan_terms and the
// small shared pieces) under AddressSanitizer + UBSan, on its own: every count
// field of a small valid descriptor set in turn to -1, its maximum + 1 and
// INT_MAX, every step field to -1, n_steps and INT_MAX; the validator runs on
// each, and whenever it accepts, the plan is made and its invariants hold:
//   * the cost slots are exactly 0 .. n_costs - 1, each used once, and the
//     constraint slots 0 .. n_cnts - 1;
//   * every collision unit starts at a waypoint of [0, n_steps);
//   * every clamped step range lies within [0, n_steps - 1];
//   * the slot table has n_costs + n_cnts entries, costs first.
// Own main, header only: no library, no GPU call; built by `make san`.
#include <climits>
#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../csrc/desc_lowering.hpp"

namespace
{
using thip::lowering::TermPlan;
using Desc = thip_problem_desc;
using Field = std::function<int&(Desc&)>;

int g_fail = 0, g_accepted = 0, g_refused = 0;

#define CHECK(cond, what)                                                          \
  do                                                                               \
  {                                                                                \
    if (!(cond))                                                                   \
    {                                                                              \
      std::printf("FAIL %s: %s (%s)\n", (what).c_str(), #cond, __func__);          \
      g_fail++;                                                                    \
    }                                                                              \
  } while (0)

// a 3-dof serial chain on 6 waypoints: one CartPose cost, one JointPos constraint with
// tolerances, one jvx cost, collision with two spheres on different links and one primitive
std::unique_ptr<Desc> base_desc()
{
  std::unique_ptr<Desc> p(new Desc());
  Desc& d = *p;
  d.abi_version = THIP_ABI_VERSION;
  d.n_steps = 6;
  d.chain.n_links = 4;
  d.chain.n_dof = 3;
  for (int k = 1; k < 4; ++k)
  {
    d.chain.joint_type[k] = THIP_JOINT_REVOLUTE;
    d.chain.joint_dof[k] = k - 1;
    d.chain.joint_axis[k][2] = 1.0;
    d.chain.joint_origin[k][0] = d.chain.joint_origin[k][5] = d.chain.joint_origin[k][10] = 1.0;
    d.chain.joint_origin[k][3] = 0.3;
  }
  d.chain.base_pose[0] = d.chain.base_pose[5] = d.chain.base_pose[10] = 1.0;
  for (int j = 0; j < 3; ++j)
  {
    d.chain.lower[j] = -3.0;
    d.chain.upper[j] = 3.0;
  }
  d.n_fixed = 1;
  d.fixed_steps[0] = 0;
  d.jv_enabled = 1;
  d.jv_first_step = 0;
  d.jv_last_step = -1;
  d.n_cart = 1;
  d.cart_step[0] = 5;
  d.cart_source_link[0] = 3;
  for (int i = 0; i < 3; ++i)
    d.cart_pos_coeffs[0][i] = d.cart_rot_coeffs[0][i] = 1.0;
  d.n_jpos = 1;
  d.jpos_is_cnt[0] = 1;
  d.jpos_first_step[0] = 2;
  d.jpos_last_step[0] = 4;
  d.n_jvx = 1;
  d.jvx_first_step[0] = 1;
  d.jvx_last_step[0] = 4;
  for (int j = 0; j < 3; ++j)
  {
    d.jv_coeffs[j] = d.jpos_coeffs[0][j] = d.jvx_coeffs[0][j] = 1.0;
    d.jpos_lower_tols[0][j] = d.jvx_lower_tols[0][j] = -0.1;
    d.jpos_upper_tols[0][j] = d.jvx_upper_tols[0][j] = 0.2;
  }
  d.coll_enabled = 1;
  d.coll_first_step = 0;
  d.coll_last_step = -1;
  d.coll_margin = 0.025;
  d.coll_coeff = 20.0;
  d.coll_buffer = 0.01;
  d.coll_lvs = 0.05;
  d.n_spheres = 2;
  d.sphere_link[0] = 3;
  d.sphere_link[1] = 2;
  d.sphere_radius[0] = d.sphere_radius[1] = 0.05;
  d.n_prims = 1;
  // (thip_default_sqp_params / thip_default_osqp_settings live in the library: the fields the validator reads)
  d.sqp.improve_ratio_threshold = 0.25;
  d.sqp.min_trust_box_size = 1e-4;
  d.sqp.min_approx_improve = 1e-4;
  d.sqp.max_iter = 50;
  d.sqp.trust_shrink_ratio = 0.1;
  d.sqp.trust_expand_ratio = 1.5;
  d.sqp.cnt_tolerance = 1e-4;
  d.sqp.trust_box_size = 0.1;
  d.sqp.max_time = 1e300;
  d.osqp.max_iter = 8192;
  d.osqp.check_termination = 25;
  d.osqp.scaling = 10;
  return p;
}

// the same with a DISCRETE collision constraint that has one fixed step, and a JointAccEqCost
std::unique_ptr<Desc> second_desc()
{
  std::unique_ptr<Desc> p = base_desc();
  Desc& d = *p;
  d.coll_continuous = 2;
  d.coll_is_cnt = 1;
  d.coll_n_fixed = 1;
  d.coll_fixed_steps[0] = 3;
  d.cart_is_cnt[0] = 1;
  d.jpos_is_cnt[0] = 0;
  d.jvx_is_cnt[0] = 1;
  d.n_jdt = 1;
  d.jdt_order[0] = 2;
  d.jdt_first_step[0] = 0;
  d.jdt_last_step[0] = 5;
  for (int j = 0; j < 3; ++j)
    d.jdt_coeffs[0][j] = 1.0;
  return p;
}

struct Named
{
  const char* name;
  Field at;
  int max;  // counts only
};

const std::vector<Named> kCounts = {
  { "chain.n_dof", [](Desc& d) -> int& { return d.chain.n_dof; }, THIP_MAX_DOF },
  { "chain.n_links", [](Desc& d) -> int& { return d.chain.n_links; }, THIP_MAX_LINKS },
  { "n_steps", [](Desc& d) -> int& { return d.n_steps; }, THIP_MAX_STEPS },
  { "n_fixed", [](Desc& d) -> int& { return d.n_fixed; }, THIP_MAX_STEPS },
  { "n_cart", [](Desc& d) -> int& { return d.n_cart; }, THIP_MAX_CART },
  { "n_jpos", [](Desc& d) -> int& { return d.n_jpos; }, THIP_MAX_JPOS },
  { "n_jvx", [](Desc& d) -> int& { return d.n_jvx; }, THIP_MAX_JVX },
  { "n_jdt", [](Desc& d) -> int& { return d.n_jdt; }, THIP_MAX_JDT },
  { "n_jvt", [](Desc& d) -> int& { return d.n_jvt; }, THIP_MAX_JVT },
  { "n_ttt", [](Desc& d) -> int& { return d.n_ttt; }, THIP_MAX_TTT },
  { "n_fixed_dofs", [](Desc& d) -> int& { return d.n_fixed_dofs; }, THIP_MAX_DOF },
  { "n_cvel", [](Desc& d) -> int& { return d.n_cvel; }, THIP_MAX_CVEL },
  { "coll_n_fixed", [](Desc& d) -> int& { return d.coll_n_fixed; }, THIP_MAX_STEPS },
  { "n_spheres", [](Desc& d) -> int& { return d.n_spheres; }, THIP_MAX_SPHERES },
  { "n_prims", [](Desc& d) -> int& { return d.n_prims; }, THIP_MAX_PRIMS },
  { "n_self_pairs", [](Desc& d) -> int& { return d.n_self_pairs; }, THIP_MAX_SELF_PAIRS },
  { "coll_max_contacts", [](Desc& d) -> int& { return d.coll_max_contacts; }, THIP_MAX_CONTACTS },
  { "n_coll_extra", [](Desc& d) -> int& { return d.n_coll_extra; }, THIP_MAX_COLL_EXTRA },
  { "n_coll_pairs", [](Desc& d) -> int& { return d.n_coll_pairs; }, THIP_MAX_COLL_PAIRS },
};

const std::vector<Named> kSteps = {
  { "fixed_steps[0]", [](Desc& d) -> int& { return d.fixed_steps[0]; }, 0 },
  { "jv_first_step", [](Desc& d) -> int& { return d.jv_first_step; }, 0 },
  { "jv_last_step", [](Desc& d) -> int& { return d.jv_last_step; }, 0 },
  { "cart_step[0]", [](Desc& d) -> int& { return d.cart_step[0]; }, 0 },
  { "jpos_first_step[0]", [](Desc& d) -> int& { return d.jpos_first_step[0]; }, 0 },
  { "jpos_last_step[0]", [](Desc& d) -> int& { return d.jpos_last_step[0]; }, 0 },
  { "jvx_first_step[0]", [](Desc& d) -> int& { return d.jvx_first_step[0]; }, 0 },
  { "jvx_last_step[0]", [](Desc& d) -> int& { return d.jvx_last_step[0]; }, 0 },
  { "jdt_first_step[0]", [](Desc& d) -> int& { return d.jdt_first_step[0]; }, 0 },
  { "jdt_last_step[0]", [](Desc& d) -> int& { return d.jdt_last_step[0]; }, 0 },
  { "coll_first_step", [](Desc& d) -> int& { return d.coll_first_step; }, 0 },
  { "coll_last_step", [](Desc& d) -> int& { return d.coll_last_step; }, 0 },
  { "coll_fixed_steps[0]", [](Desc& d) -> int& { return d.coll_fixed_steps[0]; }, 0 },
};

void check_plan(const Desc& d, const TermPlan& P, const std::string& what)
{
  const int N = d.n_steps;
  CHECK(P.N == N && P.D == d.chain.n_dof, what);
  CHECK(P.n_costs >= 0 && P.n_cnts >= 0, what);
  CHECK(static_cast<int>(P.table.size()) == P.n_costs + P.n_cnts, what);
  for (size_t k = 0; k < P.table.size(); ++k)
    CHECK(P.table[k].is_cnt == (static_cast<int>(k) >= P.n_costs ? 1 : 0), what);
  // every term's slot, costs and constraints apart: an exact cover of 0 .. n - 1
  std::vector<int> used[2] = { std::vector<int>(static_cast<size_t>(P.n_costs), 0),
                               std::vector<int>(static_cast<size_t>(P.n_cnts), 0) };
  auto use = [&](int is_cnt, int slot) {
    std::vector<int>& u = used[is_cnt ? 1 : 0];
    CHECK(slot >= 0 && slot < static_cast<int>(u.size()), what);
    if (slot >= 0 && slot < static_cast<int>(u.size()))
      u[static_cast<size_t>(slot)]++;
  };
  if (d.jv_enabled)
    use(0, 0);
  for (int k = 0; k < d.n_cart; ++k)
    use(d.cart_is_cnt[k], P.cart_slot[k]);
  for (int k = 0; k < d.n_jpos; ++k)
    use(d.jpos_is_cnt[k], P.jpos_slot[k]);
  for (int x = 0; x < d.n_jvx; ++x)
    use(d.jvx_is_cnt[x], P.jvx_slot[x]);
  for (int k = 0; k < THIP_MAX_JDT; ++k)
    if (k < d.n_jdt)
      use(0, P.jacc_slot[k]);
    else
      CHECK(P.jacc_slot[k] == -1, what);
  for (int u = 0; u < P.n_units; ++u)
    use(P.coll_cnt, P.coll_cost0 + u);
  for (const std::vector<int>& u : used)
    for (int n : u)
      CHECK(n == 1, what);
  // collision units
  CHECK(P.n_units >= 0 && P.n_units <= THIP_MAX_STEPS, what);
  CHECK(P.coll || P.n_units == 0, what);
  for (int u = 0; u < P.n_units; ++u)
  {
    CHECK(P.unit_t[u] >= 0 && P.unit_t[u] < N, what);
    CHECK(u == 0 || P.unit_t[u] > P.unit_t[u - 1], what);
    CHECK(P.coll_single || P.unit_t[u] + 1 < N, what);  // a step pair ends on a waypoint
    CHECK(!(P.coll_single && P.coll_fixed[P.unit_t[u]]), what);
  }
  // clamped ranges of the terms the descriptor has
  if (d.jv_enabled)
    CHECK(0 <= P.jv_first && P.jv_first < P.jv_last && P.jv_last <= N - 1, what);
  for (int x = 0; x < d.n_jvx; ++x)
    CHECK(0 <= P.jvx_first[x] && P.jvx_first[x] < P.jvx_last[x] && P.jvx_last[x] <= N - 1, what);
  for (int k = 0; k < d.n_jpos; ++k)
    CHECK(0 <= P.jpos_first[k] && P.jpos_first[k] <= P.jpos_last[k] && P.jpos_last[k] <= N - 1, what);
  // CartPose terms: the emission order is a permutation, costs before constraints
  std::vector<int> seen(static_cast<size_t>(d.n_cart), 0);
  for (int e = 0; e < d.n_cart; ++e)
  {
    const int k = P.cart_order[e];
    CHECK(k >= 0 && k < d.n_cart, what);
    if (k < 0 || k >= d.n_cart)
      continue;
    seen[static_cast<size_t>(k)]++;
    CHECK(e == 0 || (d.cart_is_cnt[P.cart_order[e - 1]] != 0) <= (d.cart_is_cnt[k] != 0), what);
    CHECK(P.cart_nrow[k] >= 0 && P.cart_nrow[k] <= 6, what);
    for (int i = 0; i < P.cart_nrow[k] && i < 6; ++i)
      CHECK(P.cart_comp[k][i] >= 0 && P.cart_comp[k][i] < 6, what);
  }
  for (int n : seen)
    CHECK(n == 1, what);
}

// the validator on d, and whenever it accepts, the plan and the small pieces
void run(const Desc& d, const std::string& what)
{
  std::string why;
  const thip::lowering::Finding f = thip::lowering::validate(d, why);
  CHECK(f >= 0 && f < thip::lowering::kFindingCount, what);
  CHECK((f == thip::lowering::kRefused || f == thip::lowering::kAbiVersion || f == thip::lowering::kStepsRange) ==
            !why.empty(),
        what);
  if (f != thip::lowering::kAccepted)
  {
    g_refused++;
    return;
  }
  g_accepted++;
  TermPlan P;
  thip::lowering::plan_terms(d, P);
  check_plan(d, P, what);
  if (d.coll_enabled)
  {
    const thip::lowering::SphereGroups g = thip::lowering::group_spheres_by_link(d);
    int n = 0;
    CHECK(static_cast<int>(g.order.size()) == d.n_spheres, what);
    for (size_t k = 0; k < g.grp_link.size(); ++k)
    {
      CHECK(g.grp_s0[k] == n && g.grp_ns[k] > 0, what);
      CHECK(k == 0 || g.grp_link[k] > g.grp_link[k - 1], what);
      for (int i = 0; i < g.grp_ns[k]; ++i)
        CHECK(d.sphere_link[g.order[static_cast<size_t>(n + i)]] == g.grp_link[k], what);
      n += g.grp_ns[k];
    }
    CHECK(n == d.n_spheres, what);
  }
  thip_chain ch = d.chain;
  thip::lowering::fill_serial_parents(ch);
  for (int k = 1; k < THIP_MAX_LINKS; ++k)
    CHECK(ch.is_tree || ch.parent[k] == k - 1, what);
  CHECK(thip::lowering::chain_range_finding(ch) == nullptr && thip::lowering::chain_table_finding(ch) == nullptr, what);
}

void sweep(const Desc& base, const std::string& tag)
{
  run(base, tag);
  std::unique_ptr<Desc> w(new Desc());
  for (const Named& c : kCounts)
    for (int v : { -1, c.max + 1, INT_MAX })
    {
      *w = base;
      c.at(*w) = v;
      run(*w, tag + " " + c.name + " = " + std::to_string(v));
    }
  for (const Named& s : kSteps)
    for (int v : { -1, base.n_steps, INT_MAX })
    {
      *w = base;
      s.at(*w) = v;
      run(*w, tag + " " + s.name + " = " + std::to_string(v));
    }
}
}  // namespace

int main()
{
  const std::unique_ptr<Desc> a = base_desc(), b = second_desc();
  std::string why;
  if (thip::lowering::validate(*a, why) != thip::lowering::kAccepted ||
      thip::lowering::validate(*b, why) != thip::lowering::kAccepted)
  {
    std::printf("FAIL the base descriptors are refused: %s\n", why.c_str());
    return 1;
  }
  sweep(*a, "base");
  sweep(*b, "discrete");
  // coll_n_fixed past coll_fixed_steps: refused by the shared validator, with these words
  for (int v : { -1, THIP_MAX_STEPS + 1, 1000, INT_MAX })
  {
    std::unique_ptr<Desc> w(new Desc(*a));
    w->coll_n_fixed = v;
    const thip::lowering::Finding f = thip::lowering::validate(*w, why);
    CHECK(f == thip::lowering::kRefused && why == "collision: coll_n_fixed out of range", std::to_string(v));
  }
  // the generic evaluators' sentences
  {
    std::unique_ptr<Desc> w(new Desc(*a));
    w->abi_version = THIP_ABI_VERSION + 1;
    CHECK(thip::lowering::abi_mismatch(*a).empty() && !thip::lowering::abi_mismatch(*w).empty(), std::string("abi"));
    w->chain.n_links = THIP_MAX_LINKS + 1;
    CHECK(thip::lowering::chain_range_finding(w->chain) != nullptr, std::string("chain range"));
    *w = *a;
    w->chain.joint_dof[2] = w->chain.n_dof;
    CHECK(thip::lowering::chain_table_finding(w->chain) != nullptr, std::string("chain table"));
  }
  std::printf("accepted=%d refused=%d fail=%d\n", g_accepted, g_refused, g_fail);
  return g_fail ? 1 : 0;
}
