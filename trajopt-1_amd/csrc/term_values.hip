// Batched per-term values (include/trajopt_hip.h thip_terms_*): the exact value
// of every cost and the violation of every constraint of every problem of a
// batch at trajectories x [batch][n_steps][n_dof] -- OptResults::cost_vals /
// cnt_viols (trajopt_sco/src/optimizers.cpp:176-192, 908-909) for the problem
// structures the fused kernel lowers, at any x, outside the fused kernel.
//
//   term_values_kernel  one 256-thread workgroup per problem: the JointVel,
//                       JointAcc, CartPose / DynamicCartPose and JointPos slots,
//                       the expressions of sqp_kernel.hip's evaluate(),
//                       jpos_values(), sh_values() and jacc_value().
//   coll_values_kernel  one 256-thread workgroup per (collision unit, problem),
//                       traj_check_kernel's shape: one chain_fk per (sub-state,
//                       sphere-carrying link) into LDS, kChunk sub-states at a
//                       time, threads striding over the chunk's candidates.  A
//                       candidate within margin + buffer of its pair that passes
//                       the fixed-end filter of removeInvalidContactResults (as
//                       coll_scan_pairs / coll_eval_kernel apply it) adds
//                       coeff * max(margin - d, 0) to the unit's slot.
// Sums are reduced by shuffles inside a wave and through LDS in wave order: no
// floating-point atomics, no hand-off between workgroups, so the values are
// bitwise repeatable and do not depend on a problem's position in the batch.
// fp64; kinematics and distances are kin_device.hpp's / collision_device.hpp's.
//
// The evaluator accepts the descriptors thip_create accepts and numbers its
// slots as thip_create numbers Layout::n_costs / n_cnts, jacc_slot, coll_cost0
// and Tables::term_slot / jpos_slot / jvx_slot / coll_slot: both validate with
// desc_lowering.hpp's validate() and read one term plan (plan_terms(); tests pin
// the numbering against the solver's A_COST / A_VIOL).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "collision_device.hpp"
#include "desc_lowering.hpp"
#include "device_handle.hpp"
#include "kin_device.hpp"
#include "layout.hpp"

namespace thip
{
namespace tv
{
constexpr int kTvBlock = 256;
constexpr int kTvWaves = kTvBlock / 64;
constexpr int kChunk = THIP_CHECK_CHUNK;

// what the kernels read besides the descriptor: the slot tables
struct Slots
{
  int N, D, n_costs, n_cnts;
  int jv_eq;  // JointVelEqCost in cost slot 0
  int jv_ineq, jv_first, jv_last;
  int n_jacc, jacc_slot[THIP_MAX_JDT];
  int n_cart, term_nrow[THIP_MAX_CART], term_slot[THIP_MAX_CART], row_comp[THIP_MAX_CART][6];
  double row_w[THIP_MAX_CART][6];
  int n_jpos, jpos_first[THIP_MAX_JPOS], jpos_last[THIP_MAX_JPOS], jpos_slot[THIP_MAX_JPOS], jpos_ineq[THIP_MAX_JPOS];
  int n_jvx, jvx_first[THIP_MAX_JVX], jvx_last[THIP_MAX_JVX], jvx_slot[THIP_MAX_JVX];
  // collision units (step pairs, or free waypoints for DISCRETE) and their slots
  int coll, coll_single, coll_cnt, coll_cost0, n_units;
  int unit_t[THIP_MAX_STEPS], unit_slot[THIP_MAX_STEPS], coll_fixed[THIP_MAX_STEPS];
};

// the robot spheres grouped by link, ascending, and the self-collision sphere pairs
struct Model
{
  int n_sph, n_groups, n_prims;
  int grp_link[THIP_MAX_SPHERES];
  int grp_s0[THIP_MAX_SPHERES];
  int grp_ns[THIP_MAX_SPHERES];
  int sph_order[THIP_MAX_SPHERES];
  double center[THIP_MAX_SPHERES][3];
  double radius[THIP_MAX_SPHERES];
  int n_self_sph;
  int self_sa[THIP_MAX_SELF_SPHERE_PAIRS];
  int self_sb[THIP_MAX_SELF_SPHERE_PAIRS];
  int continuous;
  double lvs, margin, coeff, buffer;
};

__device__ __forceinline__ void stage_chain_tv(thip_chain& dst_chain, const thip_chain* chain)
{
  const int* src = reinterpret_cast<const int*>(chain);
  int* dst = reinterpret_cast<int*>(&dst_chain);
  for (int w = threadIdx.x; w < static_cast<int>(sizeof(thip_chain) / 4); w += kTvBlock)
    dst[w] = src[w];
}

// the workgroup's sum, the same bits on every thread: lanes by xor shuffles, then
// the waves' sums in wave order
__device__ __forceinline__ double block_sum_tv(double v, double* s_w)
{
  for (int off = 32; off > 0; off >>= 1)
    v += __shfl_xor(v, off);
  __syncthreads();  // the previous sum's reads of s_w
  if ((threadIdx.x & 63) == 0)
    s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = s_w[0];
  for (int w = 1; w < kTvWaves; ++w)
    s += s_w[w];
  return s;
}

__global__ __launch_bounds__(kTvBlock) void term_values_kernel(const thip_problem_desc* desc, const Slots* slots,
                                                              int batch, const double* xin, const double* tgt_all,
                                                              const double* jpt_all, double* costs_all,
                                                              double* viols_all)
{
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= batch)
    return;
  __shared__ thip_chain s_chain;
  __shared__ double s_w[kTvWaves];
  stage_chain_tv(s_chain, &desc->chain);
  __syncthreads();
  const thip_chain& ch = s_chain;
  const thip_problem_desc& d = *desc;
  const Slots& S = *slots;
  const int D = S.D;
  const double* x = xin + static_cast<long long>(b) * S.N * D;
  const double* tgt = tgt_all + static_cast<long long>(b) * (S.n_cart > 0 ? S.n_cart : 1) * 12;
  const double* jpt = jpt_all + static_cast<long long>(b) * (S.n_jpos > 0 ? S.n_jpos : 1) * D;
  double* costs = costs_all + static_cast<long long>(b) * (S.n_costs > 0 ? S.n_costs : 1);
  double* viols = viols_all + static_cast<long long>(b) * (S.n_cnts > 0 ? S.n_cnts : 1);

  // JointVelEqCost::value: sum_{t,j} c_j (x_{t+1,j} - x_{t,j} - targ_j)^2
  if (S.jv_eq)
  {
    const int nv = (S.jv_last - S.jv_first) * D;
    double jv = 0;
    for (int i = tid; i < nv; i += kTvBlock)
    {
      const int t = S.jv_first + i / D, j = i % D;
      if (t < 0 || t + 1 >= S.N)
        continue;
      const double dd = (x[(t + 1) * D + j] - x[t * D + j]) - d.jv_targets[j];
      jv += (dd * dd) * d.jv_coeffs[j];
    }
    jv = block_sum_tv(jv, s_w);
    if (tid == 0)
      costs[0] = jv;
  }
  // JointAccEqCost::value: the repeated difference as diffAxis0 forms it
  for (int k = 0; k < S.n_jacc; ++k)
  {
    const int f = d.jdt_first_step[k], n = (d.jdt_last_step[k] - 2 - f + 1) * D;
    double v = 0;
    for (int e = tid; e < n; e += kTvBlock)
    {
      const int i = f + e / D, j = e % D;
      if (i < 0 || i + 2 >= S.N)
        continue;
      const double x0 = x[i * D + j], x1 = x[(i + 1) * D + j], x2 = x[(i + 2) * D + j];
      const double dd = ((x2 - x1) - (x1 - x0)) - d.jdt_targets[k][j];
      v += (dd * dd) * d.jdt_coeffs[k][j];
    }
    v = block_sum_tv(v, s_w);
    if (tid == 0)
      costs[S.jacc_slot[k]] = v;
  }
  // CartPose / DynamicCartPose: one term per thread
  for (int k = tid; k < S.n_cart; k += kTvBlock)
  {
    const int t = d.cart_step[k];
    Pose P, So, Ss, Tb, To, Tt, Ti;
    chain_fk(ch, x + t * D, d.cart_source_link[k], P);
    pose_load(So, d.cart_source_offset[k]);
    pose_mul(P, So, Ss);
    pose_load(To, tgt + 12 * k);
    if (d.cart_target_link[k] > 0)
      chain_fk(ch, x + t * D, d.cart_target_link[k], Tb);
    else
      pose_load(Tb, ch.base_pose);
    pose_mul(Tb, To, Tt);
    pose_inv(Tt, Ti);
    double err[6];
    transform_error(Ti, Ss, err);
    if (d.cart_has_tol[k])
      apply_tolerances(err, d.cart_lower_tol[k], d.cart_upper_tol[k]);
    const int nr = S.term_nrow[k];
    double v = 0;
    if (d.cart_is_cnt[k])
    {
      for (int rr = 0; rr < nr; ++rr)
        v += fabs(err[S.row_comp[k][rr]] * S.row_w[k][rr]);
      viols[S.term_slot[k]] = v;
    }
    else
    {
      for (int rr = 0; rr < nr; ++rr)
        v += fabs(err[S.row_comp[k][rr]]) * S.row_w[k][rr];
      costs[S.term_slot[k]] = v;
    }
  }
  // JointPosEqCost::value / JointPosEqConstraint violation (sum |c_j (x - targ)^2|)
  for (int k = 0; k < S.n_jpos; ++k)
  {
    const int f = S.jpos_first[k], n = (S.jpos_last[k] - f + 1) * D;
    const bool cnt = d.jpos_is_cnt[k] != 0;
    double s1 = 0, s2 = 0;
    if (!S.jpos_ineq[k])
    {
      for (int i = tid; i < n; i += kTvBlock)
      {
        const int t = f + i / D, j = i % D;
        const double dd = x[t * D + j] - jpt[k * D + j];
        const double e = (dd * dd) * d.jpos_coeffs[k][j];
        s1 += cnt ? fabs(e) : e;
      }
      s1 = block_sum_tv(s1, s_w);
    }
    else
    {
      // tolerance forms: JointPosIneqCost::value / JointPosIneqConstraint violation
      for (int i = tid; i < n; i += kTvBlock)
      {
        const int t = f + i / D, j = i % D;
        const double cf = d.jpos_coeffs[k][j];
        const double d0 = x[t * D + j] - jpt[k * D + j];
        s1 += fmax((d0 - d.jpos_upper_tols[k][j]) * cf, 0.0);
        s2 += fmax(((d0 * -1) + d.jpos_lower_tols[k][j]) * cf, 0.0);
      }
      s1 = block_sum_tv(s1, s_w);
      s2 = block_sum_tv(s2, s_w);
      s1 = s1 + s2;
    }
    if (tid == 0)
      (cnt ? viols : costs)[S.jpos_slot[k]] = s1;
  }
  // JointVelIneqCost::value (cost slot 0) and the further JointVel tolerance terms
  for (int xo = -1; xo < S.n_jvx; ++xo)
  {
    if (xo < 0 && !S.jv_ineq)
      continue;
    const int f = (xo < 0) ? S.jv_first : S.jvx_first[xo];
    const int nv = (((xo < 0) ? S.jv_last : S.jvx_last[xo]) - f) * D;
    const double* cfs = (xo < 0) ? d.jv_coeffs : d.jvx_coeffs[xo];
    const double* tg = (xo < 0) ? d.jv_targets : d.jvx_targets[xo];
    const double* up = (xo < 0) ? d.jv_upper_tols : d.jvx_upper_tols[xo];
    const double* lo = (xo < 0) ? d.jv_lower_tols : d.jvx_lower_tols[xo];
    double s1 = 0, s2 = 0;
    for (int i = tid; i < nv; i += kTvBlock)
    {
      const int t = f + i / D, j = i % D;
      if (t < 0 || t + 1 >= S.N)
        continue;
      const double cf = cfs[j];
      const double d0 = (x[(t + 1) * D + j] - x[t * D + j]) - tg[j];
      s1 += fmax((d0 - up[j]) * cf, 0.0);
      s2 += fmax(((d0 * -1) + lo[j]) * cf, 0.0);
    }
    s1 = block_sum_tv(s1, s_w);
    s2 = block_sum_tv(s2, s_w);
    if (tid == 0)
    {
      if (xo < 0)
        costs[0] = s1 + s2;
      else
        (d.jvx_is_cnt[xo] ? viols : costs)[S.jvx_slot[xo]] = s1 + s2;
    }
  }
}

__device__ __forceinline__ void sphere_world_tv(const Pose& T, const double* cl, double* c)
{
  for (int r = 0; r < 3; ++r)
    c[r] = T.r[r * 3 + 0] * cl[0] + T.r[r * 3 + 1] * cl[1] + T.r[r * 3 + 2] * cl[2] + T.t[r];
}

__global__ __launch_bounds__(kTvBlock) void coll_values_kernel(const thip_chain* chain, const Model* model,
                                                              const Slots* slots, const double* pmc, int batch,
                                                              const double* xin, const double* scene, double* out_all,
                                                              int out_stride)
{
  const Slots& S = *slots;
  const long long item = blockIdx.x;
  if (item >= static_cast<long long>(S.n_units) * batch)
    return;
  const int b = static_cast<int>(item / S.n_units), u = static_cast<int>(item % S.n_units);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ thip_chain s_chain;
  __shared__ double s_q[2][THIP_MAX_DOF];
  __shared__ double s_ctr[kChunk + 1][THIP_MAX_SPHERES][3];
  __shared__ double s_prim[THIP_MAX_PRIMS * 16];
  __shared__ double s_w[kTvWaves];

  const Model& M = *model;
  const int n_prims = M.n_prims, D = S.D;
  const bool single = S.coll_single != 0, cont = M.continuous != 0;
  const double* gprims = scene + static_cast<long long>(b) * (n_prims > 0 ? n_prims : 1) * 16;
  stage_chain_tv(s_chain, chain);
  const int t0 = S.unit_t[u];
  if (tid < 2 * D)
  {
    const int e = tid / D, j = tid % D;
    const int t = (e == 1 && !single) ? t0 + 1 : t0;
    s_q[e][j] = xin[(static_cast<long long>(b) * S.N + t) * D + j];
  }
  for (int w = tid; w < n_prims * 16; w += kTvBlock)
    s_prim[w] = gprims[w];
  __syncthreads();
  const thip_chain& ch = s_chain;
  const double* q0 = s_q[0];
  const double* q1 = s_q[1];
  // the unit's fixed ends (step-pair evaluators only; a DISCRETE term has no fixed waypoint)
  const bool f0 = !single && S.coll_fixed[t0] != 0, f1 = !single && S.coll_fixed[t0 + 1] != 0;

  // sub-states (DiscreteCollisionEvaluator / CastCollisionEvaluator, collision_terms.cpp:846-852)
  const int cnt = single ? 1 : lvs_count(q0, q1, D, M.lvs);
  const int n_sub = single ? 1 : (cont ? cnt - 1 : cnt);
  const int last = cnt - 1;
  const int n_sph = M.n_sph, n_groups = M.n_groups, PW = n_prims + n_sph;
  const double buffer = M.buffer;

  double lsum = 0.0;
  for (int i0 = 0; i0 < n_sub; i0 += kChunk)
  {
    const int nc = min(kChunk, n_sub - i0);
    const int nst = cont ? nc + 1 : nc;
    // one FK per (state of the chunk, sphere-carrying link): world centres to LDS
    for (int it = tid; it < nst * n_groups; it += kTvBlock)
    {
      const int j = it / n_groups, g = it - j * n_groups;
      double q[THIP_MAX_DOF];
      for (int k = 0; k < D; ++k)
        q[k] = single ? q0[k] : linspaced(cnt, q0[k], q1[k], i0 + j);
      Pose T;
      chain_fk(ch, q, M.grp_link[g], T);
      const int s0 = M.grp_s0[g], ng = M.grp_ns[g];
      for (int e = 0; e < ng; ++e)
      {
        const int s = M.sph_order[s0 + e];
        sphere_world_tv(T, M.center[s], s_ctr[j][s]);
      }
    }
    __syncthreads();
    const int n_scene_loc = n_sph * n_prims * nc;
    const int n_loc = n_scene_loc + M.n_self_sph * nc;
    for (int c = tid; c < n_loc; c += kTvBlock)
    {
      double dist, n[3], margin, coeff;
      bool ok;  // the fixed-end rule keeps a contact of this candidate
      if (c < n_scene_loc)
      {
        const int s = c % n_sph, r = c / n_sph, p = r % n_prims, il = r / n_prims, i = i0 + il;
        const double* e = pmc ? pmc + 2 * (s * PW + p) : nullptr;
        margin = e ? e[0] : M.margin;
        coeff = e ? e[1] : M.coeff;
        const double* prim = s_prim + 16 * p;
        double pt[3];
        int cct;  // CCType of the robot link: 1 Time0, 2 Time1, 3 Between
        if (cont)
        {
          double ts = 0;
          swept_sphere_prim_distance(s_ctr[il][s], s_ctr[il + 1][s], M.radius[s], prim, dist, n, pt, ts);
          cct = (i == 0 && ts == 0.0) ? 1 : ((i + 1 == last && ts == 1.0) ? 2 : 3);
        }
        else
        {
          sphere_prim_distance(s_ctr[il][s], M.radius[s], prim, dist, n, pt);
          cct = (i == 0) ? 1 : ((i == last) ? 2 : 3);
        }
        ok = !(f0 || f1) || (f0 && cct != 1) || (f1 && cct != 2);
      }
      else
      {
        const int r = c - n_scene_loc, j = r % M.n_self_sph, il = r / M.n_self_sph, i = i0 + il;
        const int sa = M.self_sa[j], sb = M.self_sb[j];
        const double* e = pmc ? pmc + 2 * (sa * PW + n_prims + sb) : nullptr;
        margin = e ? e[0] : M.margin;
        coeff = e ? e[1] : M.coeff;
        const int il1 = cont ? il + 1 : il;
        double pa[3], pb[3], ta, tb;
        self_sphere_distance(s_ctr[il][sa], s_ctr[il1][sa], M.radius[sa], s_ctr[il][sb], s_ctr[il1][sb], M.radius[sb],
                             cont, dist, n, pa, pb, ta, tb);
        int cta, ctb;
        if (cont)
        {
          cta = (i == 0 && ta == 0.0) ? 1 : ((i + 1 == last && ta == 1.0) ? 2 : 3);
          ctb = (i == 0 && tb == 0.0) ? 1 : ((i + 1 == last && tb == 1.0) ? 2 : 3);
        }
        else
          cta = ctb = (i == 0) ? 1 : ((i == last) ? 2 : 3);
        ok = !(f0 || f1) || (f0 && (cta != 1 || ctb != 1)) || (f1 && (cta != 2 || ctb != 2));
      }
      // contactTest's hit within the pair's contact distance margin + buffer (a
      // zero-coefficient pair reads margin -inf), then the evaluator's filter
      const bool hit = dist < margin + buffer && ok;
      lsum += hit ? fmax(margin - dist, 0.0) * coeff : 0.0;
    }
    __syncthreads();  // the next chunk overwrites the centres
  }
  for (int off = 32; off > 0; off >>= 1)
    lsum += __shfl_xor(lsum, off);
  if (lane == 0)
    s_w[wave] = lsum;
  __syncthreads();
  if (tid == 0)
  {
    double s = s_w[0];
    for (int w = 1; w < kTvWaves; ++w)
      s += s_w[w];
    out_all[static_cast<long long>(b) * out_stride + S.coll_cost0 + S.unit_slot[u]] = s;
  }
}
// Contact test FIRST / CLOSEST: the selection is per contactTest call and order
// dependent, and coll_eval_kernel (term_eval.hip) already makes it; this kernel
// only sums its records [batch][cap][W] = [t, link, prim, sphere, substate,
// distance, ...] per unit.  One workgroup per (unit, problem), threads striding
// over the problem's records.
__global__ __launch_bounds__(kTvBlock) void coll_reduce_kernel(const Model* model, const Slots* slots, const double* pmc,
                                                              int batch, const double* recs, const int* counts,
                                                              int cap, int W, double* out_all, int out_stride)
{
  const Slots& S = *slots;
  const long long item = blockIdx.x;
  if (item >= static_cast<long long>(S.n_units) * batch)
    return;
  const int b = static_cast<int>(item / S.n_units), u = static_cast<int>(item % S.n_units);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ double s_w[kTvWaves];
  const Model& M = *model;
  const int PW = M.n_prims + M.n_sph, t0 = S.unit_t[u];
  const int n = min(counts[b], cap);
  const double* rec = recs + static_cast<long long>(b) * cap * W;
  double lsum = 0.0;
  for (int r = tid; r < n; r += kTvBlock)
  {
    const double* e = rec + static_cast<long long>(r) * W;
    if (static_cast<int>(e[0]) != t0)
      continue;
    const int p = static_cast<int>(e[2]), s = static_cast<int>(e[3]);
    const int col = p >= 0 ? p : M.n_prims + (-1 - p);
    if (s < 0 || s >= M.n_sph || col < 0 || col >= PW)
      continue;
    const double* mc = pmc ? pmc + 2 * (s * PW + col) : nullptr;
    const double margin = mc ? mc[0] : M.margin, coeff = mc ? mc[1] : M.coeff;
    lsum += fmax(margin - e[5], 0.0) * coeff;
  }
  for (int off = 32; off > 0; off >>= 1)
    lsum += __shfl_xor(lsum, off);
  if (lane == 0)
    s_w[wave] = lsum;
  __syncthreads();
  if (tid == 0)
  {
    double s = s_w[0];
    for (int w = 1; w < kTvWaves; ++w)
      s += s_w[w];
    out_all[static_cast<long long>(b) * out_stride + S.coll_cost0 + S.unit_slot[u]] = s;
  }
}
}  // namespace tv
}  // namespace thip

using namespace thip;
using namespace thip::tv;

struct thip_terms : thip::host::Handle
{
  thip_problem_desc desc{};
  Slots slots{};
  std::vector<thip_term_slot> table;
  thip_problem_desc* d_desc = nullptr;
  Slots* d_slots = nullptr;
  Model* d_model = nullptr;
  double* d_pair = nullptr;
  double* d_tgt = nullptr;
  double* d_scene = nullptr;
  double* d_jpt = nullptr;
  double* d_x = nullptr;  // staging of host trajectories
  double* d_costs = nullptr;
  double* d_viols = nullptr;
  // contact test FIRST / CLOSEST: the device evaluator whose records are summed
  // (thip_eval_collision: host trajectories in, host records out), and their staging
  thip_eval* ev = nullptr;
  std::vector<double> h_x, h_rec, h_scene;
  std::vector<int> h_cnt;
  double* d_rec = nullptr;
  int* d_cnt = nullptr;
  int rec_cap = 0;
};

static thread_local std::string g_terms_create_err;

namespace
{
const std::string kHostLoop =
    ": not lowered into the batched kernels -- evaluate such a problem on the host loop "
    "(sco::BasicTrustRegionSQP, Cost::value / Constraint::violation)";

// The descriptors thip_create accepts are refused here with the same tests
// (lowering::validate), before any device call; the evaluator's words for the
// findings each entry point words itself
const std::string kTermsWording[lowering::kFindingCount] = {
  "",  // kAccepted
  "",  // kRefused: the shared reason as it stands
  "",  // kAbiVersion
  kHostLoop,  // kStepsRange
  "jvx terms are the tolerance forms: a term with zero tolerances goes in jv_*",  // kJvxZeroTols
  "JointAcc / JointJerk terms other than the fused JointAccEqCost (non-fused jdt)" + kHostLoop,  // kJdtNotFused
  "time-parameterised problems (use_time, JointVel terms with use_time, TotalTime) and fixed dofs" +
      kHostLoop,  // kTimeOrFixedDofs
  "CartVel terms (n_cvel > 0) run the generic path, its device evaluator thip_eval_cart_vel_all" +
      kHostLoop,                                               // kCartVel
  "more than one collision term (coll_extra)" + kHostLoop,    // kCollExtra
  "collision: n_prims out of range (THIP_MAX_PRIMS)" + kHostLoop,  // kPrimsRange
};

template <class A>
void copy_array(A& dst, const A& src)
{
  std::memcpy(&dst, &src, sizeof(A));
}

// the term plan (desc_lowering.hpp) as the kernels read it
void fill_slots(const thip_problem_desc& d, const lowering::TermPlan& P, Slots& S)
{
  S = Slots{};
  S.N = P.N;
  S.D = P.D;
  S.n_costs = P.n_costs;
  S.n_cnts = P.n_cnts;
  S.jv_eq = (d.jv_enabled && !P.jv_ineq) ? 1 : 0;
  S.jv_ineq = P.jv_ineq;
  S.jv_first = P.jv_first;
  S.jv_last = P.jv_last;
  S.n_jacc = d.n_jdt;
  copy_array(S.jacc_slot, P.jacc_slot);
  S.n_cart = d.n_cart;
  copy_array(S.term_nrow, P.cart_nrow);
  copy_array(S.term_slot, P.cart_slot);
  copy_array(S.row_comp, P.cart_comp);
  copy_array(S.row_w, P.cart_w);
  S.n_jpos = d.n_jpos;
  copy_array(S.jpos_first, P.jpos_first);
  copy_array(S.jpos_last, P.jpos_last);
  copy_array(S.jpos_slot, P.jpos_slot);
  copy_array(S.jpos_ineq, P.jpos_ineq);
  S.n_jvx = d.n_jvx;
  copy_array(S.jvx_first, P.jvx_first);
  copy_array(S.jvx_last, P.jvx_last);
  copy_array(S.jvx_slot, P.jvx_slot);
  S.coll = P.coll;
  S.coll_single = P.coll_single;
  S.coll_cnt = P.coll_cnt;
  S.coll_cost0 = P.coll_cost0;
  S.n_units = P.n_units;
  copy_array(S.unit_t, P.unit_t);
  for (int u = 0; u < P.n_units; ++u)
    S.unit_slot[u] = u;
  copy_array(S.coll_fixed, P.coll_fixed);
}

// the kernels of a run, in stream order
int launch_kernels(thip_terms* t, const double* d_x)
{
  const size_t B = static_cast<size_t>(t->batch);
  const Slots& S = t->slots;
  hipError_t e;
  hipLaunchKernelGGL(term_values_kernel, dim3(t->batch), dim3(kTvBlock), 0, t->stream, t->d_desc, t->d_slots, t->batch,
                     d_x, t->d_tgt, t->d_jpt, t->d_costs, t->d_viols);
  if (const int rc = launched(t, "term_values_kernel"); rc != THIP_OK)
    return rc;
  if (S.coll && S.n_units > 0 && t->ev)
  {
    // FIRST / CLOSEST: coll_eval_kernel's records of every problem, then their per-unit sums
    const size_t nx = B * S.N * S.D;
    const int W = 8 + 2 * S.D + 1;
    t->h_x.resize(nx);
    t->h_cnt.assign(B, 0);
    if ((e = hipMemcpyAsync(t->h_x.data(), d_x, nx * sizeof(double), hipMemcpyDeviceToHost, t->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(t->stream)) != hipSuccess)
      return hipfail(t, "hipMemcpy(x)", e);
    for (int attempt = 0; attempt < 2; ++attempt)
    {
      t->h_rec.resize(B * static_cast<size_t>(t->rec_cap) * W);
      if (thip_eval_collision(t->ev, 0, t->h_x.data(), t->h_rec.data(), t->rec_cap, t->h_cnt.data()) != THIP_OK)
        return fail(t, std::string("thip_eval_collision: ") + thip_eval_last_error(t->ev));
      const int mx = *std::max_element(t->h_cnt.begin(), t->h_cnt.end());
      if (mx <= t->rec_cap)
        break;
      t->rec_cap = mx;  // a problem had more contacts than the staging holds: once more with room for all
      drop(*t, t->d_rec);
    }
    // a record names a robot sphere and a primitive or a second sphere: anything else is an
    // error here, not a contact to skip (the kernel's own range test only guards its reads)
    for (size_t b = 0; b < B; ++b)
      for (int r = 0; r < t->h_cnt[b]; ++r)
      {
        const double* e = t->h_rec.data() + (b * static_cast<size_t>(t->rec_cap) + r) * W;
        const int p = static_cast<int>(e[2]), s = static_cast<int>(e[3]);
        if (s < 0 || s >= t->desc.n_spheres || (p >= 0 ? p >= t->desc.n_prims : -1 - p >= t->desc.n_spheres))
          return fail(t, "thip_eval_collision returned a contact record with sphere " + std::to_string(s) +
                              " / other " + std::to_string(p) + " out of range");
      }
    if (!t->d_rec && (e = alloc(*t, t->d_rec, B * static_cast<size_t>(t->rec_cap) * W)) != hipSuccess)
      return hipfail(t, "hipMalloc(contact records)", e);
    if ((e = hipMemcpyAsync(t->d_rec, t->h_rec.data(), t->h_rec.size() * sizeof(double), hipMemcpyHostToDevice,
                            t->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(t->d_cnt, t->h_cnt.data(), B * sizeof(int), hipMemcpyHostToDevice, t->stream)) != hipSuccess)
      return hipfail(t, "hipMemcpy(contact records)", e);
    hipLaunchKernelGGL(coll_reduce_kernel, dim3(static_cast<unsigned>(B * S.n_units)), dim3(kTvBlock), 0, t->stream,
                       t->d_model, t->d_slots, t->d_pair, t->batch, t->d_rec, t->d_cnt, t->rec_cap, W,
                       S.coll_cnt ? t->d_viols : t->d_costs, std::max(S.coll_cnt ? S.n_cnts : S.n_costs, 1));
    return launched(t, "coll_reduce_kernel");
  }
  if (S.coll && S.n_units > 0)
  {
    hipLaunchKernelGGL(coll_values_kernel, dim3(static_cast<unsigned>(B * S.n_units)), dim3(kTvBlock), 0, t->stream,
                       &t->d_desc->chain, t->d_model, t->d_slots, t->d_pair, t->batch, d_x, t->d_scene,
                       S.coll_cnt ? t->d_viols : t->d_costs, std::max(S.coll_cnt ? S.n_cnts : S.n_costs, 1));
    return launched(t, "coll_values_kernel");
  }
  return THIP_OK;
}

// thip_terms_run (x on the host) and thip_terms_run_device
int run(thip_terms* t, bool on_host, const double* x, double* costs, double* viols)
{
  if (!t)
    return THIP_E_INVALID;
  const Slots& S = t->slots;
  const size_t B = static_cast<size_t>(t->batch);
  const double* d_x = nullptr;
  if (const int rc = stage_x(t, "thip_terms", on_host, x, (S.n_costs == 0 || costs) && (S.n_cnts == 0 || viols),
                             " / costs / viols", t->d_x, B * S.N * S.D, d_x);
      rc != THIP_OK)
    return rc;
  auto fetch = [&] {
    const hipError_t e = to_host(t, S.n_costs > 0 ? costs : nullptr, t->d_costs, B * S.n_costs * sizeof(double));
    return e != hipSuccess ? e : to_host(t, S.n_cnts > 0 ? viols : nullptr, t->d_viols, B * S.n_cnts * sizeof(double));
  };
  return timed_run(t, "term value kernels", [&] { return launch_kernels(t, d_x); }, fetch);
}

int upload_inputs(thip_terms* t, const double* tgt, const double* scene, hipMemcpyKind kind, const char* who)
{
  if (!t)
    return THIP_E_INVALID;
  const thip_problem_desc& d = t->desc;
  const bool need_scene = d.coll_enabled && d.n_prims > 0;
  if (d.n_cart > 0 && !tgt)
    return fail(t, std::string(who) + ": cart_targets required when n_cart > 0");
  if (need_scene && !scene)
    return fail(t, std::string(who) + ": scene required when the collision term has primitives");
  const size_t B = static_cast<size_t>(t->batch);
  hipError_t e;
  if ((e = hipSetDevice(t->device)) != hipSuccess)
    return hipfail(t, "hipSetDevice", e);
  if (d.n_cart > 0 && (e = hipMemcpyAsync(t->d_tgt, tgt, B * d.n_cart * 12 * sizeof(double), kind, t->stream)) != hipSuccess)
    return hipfail(t, "hipMemcpy(cart_targets)", e);
  if (need_scene &&
      (e = hipMemcpyAsync(t->d_scene, scene, B * d.n_prims * 16 * sizeof(double), kind, t->stream)) != hipSuccess)
    return hipfail(t, "hipMemcpy(scene)", e);
  if ((e = hipStreamSynchronize(t->stream)) != hipSuccess)
    return hipfail(t, "hipStreamSynchronize", e);
  if (t->ev)
  {
    // the FIRST / CLOSEST route's evaluator takes host arrays; it reads no CartPose target
    const double* hs = scene;
    if (need_scene && kind == hipMemcpyDeviceToDevice)
    {
      t->h_scene.resize(B * d.n_prims * 16);
      if ((e = hipMemcpy(t->h_scene.data(), t->d_scene, t->h_scene.size() * sizeof(double), hipMemcpyDeviceToHost)) !=
          hipSuccess)
        return hipfail(t, "hipMemcpy(scene)", e);
      hs = t->h_scene.data();
    }
    const std::vector<double> zeros(B * std::max(d.n_cart, 1) * 12, 0.0);
    if (thip_eval_upload(t->ev, zeros.data(), hs) != THIP_OK)
      return fail(t, std::string("thip_eval_upload: ") + thip_eval_last_error(t->ev));
  }
  t->uploaded = true;
  return THIP_OK;
}

int upload_jpt(thip_terms* t, const double* jpt, hipMemcpyKind kind, const char* who)
{
  if (!t)
    return THIP_E_INVALID;
  if (!jpt)
    return fail(t, std::string(who) + ": null jpos_targets");
  if (t->desc.n_jpos == 0)
    return THIP_OK;
  hipError_t e;
  if ((e = hipSetDevice(t->device)) != hipSuccess)
    return hipfail(t, "hipSetDevice", e);
  const size_t n = static_cast<size_t>(t->batch) * t->desc.n_jpos * t->desc.chain.n_dof;
  if ((e = hipMemcpyAsync(t->d_jpt, jpt, n * sizeof(double), kind, t->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(t->stream)) != hipSuccess)
    return hipfail(t, "hipMemcpy(jpos_targets)", e);
  return THIP_OK;
}
}  // namespace

extern "C" {

int thip_sizeof_term_slot(void) { return static_cast<int>(sizeof(thip_term_slot)); }

int thip_terms_create(int device, const thip_problem_desc* desc, int batch, thip_terms** out)
{
  if (out)
    *out = nullptr;
  if (!desc || !out || batch <= 0)
  {
    g_terms_create_err = "thip_terms_create: null argument or batch <= 0";
    return THIP_E_INVALID;
  }
  const host::CreateError reject{ g_terms_create_err, "thip_terms_create: " };
  {
    std::string why;
    if (const lowering::Finding f = lowering::validate(*desc, why))
      return reject(why + kTermsWording[f]);
  }
  std::unique_ptr<thip_terms, void (*)(thip_terms*)> t(new thip_terms(), thip_terms_destroy);
  t->device = device;
  t->batch = batch;
  t->desc = *desc;
  lowering::fill_serial_parents(t->desc.chain);
  const thip_problem_desc& d = t->desc;
  {
    lowering::TermPlan P;
    lowering::plan_terms(d, P);
    fill_slots(d, P, t->slots);
    t->table = P.table;
  }
  const Slots& S = t->slots;
  if (static_cast<long long>(std::max(S.n_units, 1)) * batch > INT_MAX)
    return reject("batch * collision units exceeds the grid");
  Model md{};
  std::vector<double> ptab;
  if (d.coll_enabled)
  {
    std::vector<int> ssa, ssb, skp;
    self_sphere_pairs(d, ssa, ssb, skp);
    lowering::fill_sphere_model(d, ssa, ssb, md);
    md.n_prims = d.n_prims;
    lowering::store_sphere_groups(lowering::group_spheres_by_link(d), md);
    md.continuous = d.coll_continuous == 1;
    md.lvs = d.coll_lvs;
    md.margin = d.coll_margin;
    md.coeff = d.coll_coeff;
    md.buffer = d.coll_buffer;
    coll_pair_table(d, 0, ptab);
  }
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess)
    return reject.hip("hipSetDevice", e);
  const size_t B = static_cast<size_t>(batch), D = static_cast<size_t>(S.D);
  const size_t n_tgt = B * std::max(d.n_cart, 1) * 12, n_scene = B * std::max(d.n_prims, 1) * 16;
  const size_t per_jpt = std::max(d.n_jpos, 1) * D;
  const size_t n_c = B * std::max(S.n_costs, 1), n_v = B * std::max(S.n_cnts, 1);
  if ((e = alloc(*t, t->d_desc, 1)) != hipSuccess || (e = alloc(*t, t->d_slots, 1)) != hipSuccess ||
      (e = alloc(*t, t->d_model, 1)) != hipSuccess || (e = alloc(*t, t->d_tgt, n_tgt)) != hipSuccess ||
      (e = alloc(*t, t->d_scene, n_scene)) != hipSuccess || (e = alloc(*t, t->d_jpt, B * per_jpt)) != hipSuccess ||
      (e = alloc(*t, t->d_x, B * S.N * D)) != hipSuccess || (e = alloc(*t, t->d_costs, n_c)) != hipSuccess ||
      (e = alloc(*t, t->d_viols, n_v)) != hipSuccess ||
      (!ptab.empty() && (e = alloc(*t, t->d_pair, ptab.size())) != hipSuccess))
    return reject.hip("hipMalloc", e);
  if ((e = open_stream(*t)) != hipSuccess)
    return reject.hip("hipStreamCreate", e);
  if ((e = open_events(*t)) != hipSuccess)
    return reject.hip("hipEventCreate", e);
  // every problem starts with the descriptor's JointPos targets
  std::vector<double> jpt(B * per_jpt, 0.0);
  for (size_t b = 0; b < B; ++b)
    for (int k = 0; k < d.n_jpos; ++k)
      for (size_t j = 0; j < D; ++j)
        jpt[b * per_jpt + k * D + j] = d.jpos_targets[k][j];
  if ((e = hipMemcpyAsync(t->d_desc, &t->desc, sizeof(thip_problem_desc), hipMemcpyHostToDevice, t->stream)) !=
          hipSuccess ||
      (e = hipMemcpyAsync(t->d_slots, &t->slots, sizeof(Slots), hipMemcpyHostToDevice, t->stream)) != hipSuccess ||
      (e = hipMemcpyAsync(t->d_model, &md, sizeof(Model), hipMemcpyHostToDevice, t->stream)) != hipSuccess ||
      (e = hipMemcpyAsync(t->d_jpt, jpt.data(), jpt.size() * sizeof(double), hipMemcpyHostToDevice, t->stream)) !=
          hipSuccess ||
      (!ptab.empty() && (e = hipMemcpyAsync(t->d_pair, ptab.data(), ptab.size() * sizeof(double),
                                            hipMemcpyHostToDevice, t->stream)) != hipSuccess) ||
      (e = hipMemsetAsync(t->d_tgt, 0, n_tgt * sizeof(double), t->stream)) != hipSuccess ||
      (e = hipMemsetAsync(t->d_scene, 0, n_scene * sizeof(double), t->stream)) != hipSuccess ||
      (e = hipMemsetAsync(t->d_costs, 0, n_c * sizeof(double), t->stream)) != hipSuccess ||
      (e = hipMemsetAsync(t->d_viols, 0, n_v * sizeof(double), t->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(t->stream)) != hipSuccess)
    return reject.hip("hipMemcpy", e);
  // nothing to upload: the evaluator is ready
  t->uploaded = d.n_cart == 0 && !(d.coll_enabled && d.n_prims > 0);
  if (d.coll_enabled && d.coll_contact_test != THIP_CONTACT_ALL)
  {
    if (thip_eval_create(device, &t->desc, batch, &t->ev) != THIP_OK)
    {
      g_terms_create_err = std::string("thip_terms_create: ") + thip_eval_last_error(nullptr);
      return THIP_E_HIP;
    }
    t->rec_cap = 256;
    if ((e = alloc(*t, t->d_cnt, B)) != hipSuccess)
      return reject.hip("hipMalloc", e);
    if (t->uploaded && thip_eval_upload(t->ev, nullptr, nullptr) != THIP_OK)
    {
      g_terms_create_err = std::string("thip_terms_create: ") + thip_eval_last_error(t->ev);
      return THIP_E_HIP;
    }
  }
  *out = t.release();
  return THIP_OK;
}

int thip_terms_slot_table(const thip_problem_desc* desc, thip_term_slot* out, int cap, int* n_costs, int* n_cnts)
{
  if (!desc || cap < 0 || (cap > 0 && !out))
  {
    g_terms_create_err = "thip_terms_slot_table: bad arguments";
    return THIP_E_INVALID;
  }
  std::string why;
  if (const lowering::Finding f = lowering::validate(*desc, why))
  {
    g_terms_create_err = "thip_terms_slot_table: " + why + kTermsWording[f];
    return THIP_E_INVALID;
  }
  lowering::TermPlan P;
  lowering::plan_terms(*desc, P);
  if (n_costs)
    *n_costs = P.n_costs;
  if (n_cnts)
    *n_cnts = P.n_cnts;
  for (size_t k = 0; k < P.table.size() && k < static_cast<size_t>(cap); ++k)
    out[k] = P.table[k];
  return THIP_OK;
}

int thip_terms_counts(const thip_terms* t, int* n_costs, int* n_cnts)
{
  if (!t)
    return THIP_E_INVALID;
  if (n_costs)
    *n_costs = t->slots.n_costs;
  if (n_cnts)
    *n_cnts = t->slots.n_cnts;
  return THIP_OK;
}

int thip_terms_slots(const thip_terms* t, thip_term_slot* out)
{
  if (!t || !out)
    return THIP_E_INVALID;
  for (size_t k = 0; k < t->table.size(); ++k)
    out[k] = t->table[k];
  return THIP_OK;
}

int thip_terms_upload(thip_terms* t, const double* cart_targets, const double* scene)
{
  return upload_inputs(t, cart_targets, scene, hipMemcpyHostToDevice, "thip_terms_upload");
}

int thip_terms_upload_device(thip_terms* t, const double* d_cart_targets, const double* d_scene)
{
  return upload_inputs(t, d_cart_targets, d_scene, hipMemcpyDeviceToDevice, "thip_terms_upload_device");
}

int thip_terms_upload_joint_targets(thip_terms* t, const double* jpos_targets)
{
  return upload_jpt(t, jpos_targets, hipMemcpyHostToDevice, "thip_terms_upload_joint_targets");
}

int thip_terms_upload_joint_targets_device(thip_terms* t, const double* d_jpos_targets)
{
  return upload_jpt(t, d_jpos_targets, hipMemcpyDeviceToDevice, "thip_terms_upload_joint_targets_device");
}

int thip_terms_run(thip_terms* t, const double* x, double* costs, double* viols)
{
  return run(t, true, x, costs, viols);
}

int thip_terms_run_device(thip_terms* t, const double* d_x, double* costs, double* viols)
{
  return run(t, false, d_x, costs, viols);
}

double thip_terms_last_ms(thip_terms* t) { return t ? t->last_ms : -1.0; }

void thip_terms_destroy(thip_terms* t)
{
  if (!t)
    return;
  release(*t);
  thip_eval_destroy(t->ev);
  delete t;
}

const char* thip_terms_last_error(thip_terms* t) { return t ? t->err.c_str() : g_terms_create_err.c_str(); }

}  // extern "C"
