// Fixed-size continuous collision sets (include/trajopt_hip.h thip_ccsets_*):
// the rows of trajopt_ifopt's ContinuousCollisionConstraint over an
// LVSContinuousCollisionEvaluator / LVSDiscreteCollisionEvaluator, for every
// segment (t, t + 1) of every problem of a batch in one launch --
//   calcCollisionData / calcCollisionsHelper  continuous_collision_evaluators.cpp:97-248, 317-458
//   update / getValues / getJacobian          continuous_collision_constraint.cpp:80-236
//   removeInvalidContactResults / getGradient trajopt_common/src/collision_utils.cpp:73-221
//   LinkMaxError / GradientResultsSet         collision_types.cpp:128-330
//   getWeightedAvgGradientT0 / T1             weighted_average_methods.cpp:31-107
// restated on the primitive collision model (collision_device.hpp).  The
// sub-states, candidates, distances, normals, contact points, cc_time, cc_type
// and the kept-contact rule are those of term_eval.hip's coll_eval_kernel
// (contact test ALL, the same lvs_count / linspaced arithmetic, the same strict
// distance test).
//
//   ccsets_kernel   one 256-thread workgroup per (problem, segment):
//     1. scan: the keys (robot sphere x primitive, then the self sphere pairs)
//        kBlock at a time, one key per thread.  Within a pass the workgroup
//        walks the sub-states; each sub-state's link poses and sphere centres
//        (one or two states) are staged in LDS once, a cast's end state staying
//        for the next cast's start.  A thread keeps its key's four maxima
//        (side x end; -inf: no error) in registers.  Keys with a kept contact
//        are compacted in candidate order (ballot + prefix over the waves).
//     2. select: as csets_kernel -- the running top R (LDS, double buffered)
//        and the pass's sets ranked together, E descending, ties by packed key.
//        The four maxima travel with the set.
//     3. rows: only for the min(R, count) selected sets the sub-states are
//        walked again, one thread per (row, end, dof), 256 at a time; each
//        thread recomputes its set's contact and runs one forward-kinematics
//        walk per side at that contact's own q_t (getGradient evaluates the
//        jacobian there, not at the node), keeping only its dof's joint axis
//        and origin: no per-thread jacobian array.
// The reference's weighted average divides by the summed weight after an
// assert; where that sum is zero (every qualifying contact has error + buffer
// <= 0 while the set's maximum is positive through a contact that does not
// qualify at this end) it would divide by zero: the row is zero here.
// No atomics and no hand-off between workgroups: a problem's rows do not depend
// on its place in the batch, and every run gives the same bits.  fp64.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "coll_sets_common.hpp"
#include "collision_device.hpp"

namespace thip
{
namespace ccs
{
using namespace sets;  // coll_sets_common.hpp: Model, the key packing, the row order

constexpr int kMaxStates = THIP_CCSETS_MAX_SUBSTATES;
constexpr int kCCNone = 0, kCCTime0 = 1, kCCTime1 = 2, kCCBetween = 3;

struct Params
{
  double margin, coeff, buffer, lvs;
  const double* pmc;  // pair_data.hpp table [n_sph][pw][2], or null: margin / coeff for every pair
  const int* seg_fixed;  // [n_seg] bit 0: vars0 fixed, bit 1: vars1 fixed
  int pw;
  int R, first_step, n_seg, batch, N, n_prims;
  int cast;     // CONTINUOUS / LVS_CONTINUOUS: casts between consecutive states
  int one_cast; // CONTINUOUS: two states whatever the joint distance
};

struct Contact
{
  double dist, n[3], pt[2][3], time[2];
  int type[2];
};

__device__ __forceinline__ int cast_type(int i, int last, double t)
{
  return (i == 0 && t == 0.0) ? kCCTime0 : ((i + 1 == last && t == 1.0) ? kCCTime1 : kCCBetween);
}

// The contact of robot sphere s against primitive p (sb < 0) or robot sphere sb
// at sub-state i: cA / cB the sphere centres at the sub-state's start / end state
// (coll_eval_kernel's eval_cand).  `reach`: a contact farther than this cannot be
// kept, so a cast whose lower bound exceeds it is answered with that bound.
__device__ void eval_contact(const Model& M, bool cast, int i, int last, double dt, int s, int p, int sb,
                             const double (*cA)[3], const double (*cB)[3], const double* prims, double reach,
                             Contact& c)
{
  c.type[1] = kCCNone;
  c.time[1] = 0.0;
  if (sb < 0)
  {
    const double* prim = prims + 16 * p;
    if (cast)
    {
      const double lb = swept_lower_bound(cA[s], cB[s], M.radius[s], prim);
      if (lb > reach)
      {
        c.dist = lb;
        c.type[0] = kCCBetween;
        c.time[0] = 0.0;
        return;
      }
      double ts = 0;
      swept_sphere_prim_distance(cA[s], cB[s], M.radius[s], prim, c.dist, c.n, c.pt[0], ts);
      c.time[0] = (double(i) + ts) * dt;
      c.type[0] = cast_type(i, last, ts);
    }
    else
    {
      sphere_prim_distance(cA[s], M.radius[s], prim, c.dist, c.n, c.pt[0]);
      c.time[0] = double(i) * dt;
      c.type[0] = (i == 0) ? kCCTime0 : ((i == last) ? kCCTime1 : kCCBetween);
    }
    return;
  }
  double t0, t1;
  self_sphere_distance(cA[s], cB[s], M.radius[s], cA[sb], cB[sb], M.radius[sb], cast, c.dist, c.n, c.pt[0], c.pt[1], t0,
                       t1);
  if (cast)
  {
    c.time[0] = (double(i) + t0) * dt;
    c.time[1] = (double(i) + t1) * dt;
    c.type[0] = cast_type(i, last, t0);
    c.type[1] = cast_type(i, last, t1);
  }
  else
  {
    c.time[0] = c.time[1] = double(i) * dt;
    c.type[0] = c.type[1] = (i == 0) ? kCCTime0 : ((i == last) ? kCCTime1 : kCCBetween);
  }
}

// removeInvalidContactResults on a contact the test returned (coll_eval_kernel's
// pre && keep): strictly within the contact distance, and at a fixed end one
// robot side away from that end
__device__ __forceinline__ bool kept_contact(double dist, double reach, const int* type, bool f0, bool f1)
{
  bool h = dist < reach;
  if (h && (f0 || f1))
    h = (f0 && ((type[0] != kCCNone && type[0] != kCCTime0) || (type[1] != kCCNone && type[1] != kCCTime0))) ||
        (f1 && ((type[0] != kCCNone && type[0] != kCCTime1) || (type[1] != kCCNone && type[1] != kCCTime1)));
  return h;
}

// d(distance)/d(q_j) of one side of a contact with the link's jacobian at
// q_t = q0 (Time0), q1 (Time1), else q0 + (q1 - q0) cc_time
// (collision_utils.cpp:203-216): one forward-kinematics walk down the link's
// path that keeps the axis and origin of the joint of dof j (chain_jacobian's
// column j), shifted by r = R_e p_local (jacobianChangeRefPoint) and dotted with
// the normal; sg = -1 for the first link, +1 for the second.
__device__ double side_gradient_at(const thip_chain& ch, const double* q0, const double* q1, int type, double time,
                                   int link, const double* r, const double* normal, double sg, int j)
{
  const unsigned path = chain_path(ch, link);
  Pose T;
  pose_load(T, ch.base_pose);
  double a[3] = { 0.0, 0.0, 0.0 }, pk[3] = { 0.0, 0.0, 0.0 };
  int jt = THIP_JOINT_FIXED;
  for (int k = 1; k <= link; ++k)
  {
    if (!((path >> k) & 1u))
      continue;
    Pose O, Tn;
    pose_load(O, ch.joint_origin[k]);
    pose_mul(T, O, Tn);
    const int kt = ch.joint_type[k];
    if (kt == THIP_JOINT_FIXED)
    {
      T = Tn;
      continue;
    }
    const int d = ch.joint_dof[k];
    const double qv = (type == kCCTime0) ? q0[d] : ((type == kCCTime1) ? q1[d] : q0[d] + (q1[d] - q0[d]) * time);
    Pose Mj;
    if (kt == THIP_JOINT_PRISMATIC)
    {
      Mj.r[0] = Mj.r[4] = Mj.r[8] = 1;
      Mj.r[1] = Mj.r[2] = Mj.r[3] = Mj.r[5] = Mj.r[6] = Mj.r[7] = 0;
      Mj.t[0] = ch.joint_axis[k][0] * qv;
      Mj.t[1] = ch.joint_axis[k][1] * qv;
      Mj.t[2] = ch.joint_axis[k][2] * qv;
    }
    else
    {
      rot_axis_angle(ch.joint_axis[k], qv, Mj.r);
      Mj.t[0] = Mj.t[1] = Mj.t[2] = 0;
    }
    pose_mul(Tn, Mj, T);
    if (d == j)
    {
      const double* ax = ch.joint_axis[k];
      for (int i = 0; i < 3; ++i)
      {
        a[i] = T.r[i * 3 + 0] * ax[0] + T.r[i * 3 + 1] * ax[1] + T.r[i * 3 + 2] * ax[2];
        pk[i] = T.t[i];
      }
      jt = kt;
    }
  }
  if (jt == THIP_JOINT_FIXED)
    return 0.0;  // no joint of dof j moves the link
  double l0 = a[0], l1 = a[1], l2 = a[2];
  if (jt != THIP_JOINT_PRISMATIC)
  {
    const double d[3] = { T.t[0] - pk[0], T.t[1] - pk[1], T.t[2] - pk[2] };
    l0 = (a[1] * d[2] - a[2] * d[1]) + (a[1] * r[2] - a[2] * r[1]);
    l1 = (a[2] * d[0] - a[0] * d[2]) + (a[2] * r[0] - a[0] * r[2]);
    l2 = (a[0] * d[1] - a[1] * d[0]) + (a[0] * r[1] - a[1] * r[0]);
  }
  return sg * (normal[0] * l0 + normal[1] * l1 + normal[2] * l2);
}

__global__ __launch_bounds__(kBlock) void ccsets_kernel(const thip_chain* chain, const Model* model, Params pr,
                                                       const double* x, const double* scene, double* values,
                                                       double* jac, double* coeffs, int* counts, int* keys)
{
  const long long item = blockIdx.x;
  if (item >= static_cast<long long>(pr.n_seg) * pr.batch)
    return;
  const int b = static_cast<int>(item / pr.n_seg), u = static_cast<int>(item % pr.n_seg);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ thip_chain s_chain;
  __shared__ double s_q0[THIP_MAX_DOF], s_q1[THIP_MAX_DOF];
  __shared__ double s_qs[2][THIP_MAX_DOF];  // the sub-state's start / end joint values
  __shared__ Pose s_T[2][THIP_MAX_LINKS];
  __shared__ double s_ctr[2][THIP_MAX_SPHERES][3];
  __shared__ double s_prim[kLdsPrims * 16];
  __shared__ double s_rerr[2][kMaxRows];  // the running top R, double buffered
  __shared__ unsigned s_rkey[2][kMaxRows];
  __shared__ double s_rmax[2][kMaxRows][4];  // [side * 2 + end] maximum error, -inf: none
  __shared__ double s_perr[kBlock];  // one pass's sets, candidate order
  __shared__ unsigned s_pkey[kBlock];
  __shared__ double s_pmax[kBlock][4];
  __shared__ int s_wcnt[kWaves];

  const Model& M = *model;
  const int n_prims = pr.n_prims, R = pr.R;
  // the prologue (chain and scene to LDS): the same text as csets_kernel's, coll_sets.hip
  const double* gprims = scene + static_cast<long long>(b) * (n_prims > 0 ? n_prims : 1) * 16;
  const bool lds_prims = n_prims <= kLdsPrims;
  {
    const int* src = reinterpret_cast<const int*>(chain);
    int* dst = reinterpret_cast<int*>(&s_chain);
    for (int w = tid; w < static_cast<int>(sizeof(thip_chain) / 4); w += kBlock)
      dst[w] = src[w];
  }
  const int D = chain->n_dof, n_links = chain->n_links;
  if (tid < D)
  {
    const double* q = x + (static_cast<long long>(b) * pr.N + pr.first_step + u) * D;
    s_q0[tid] = q[tid];
    s_q1[tid] = q[D + tid];
  }
  if (lds_prims)
    for (int w = tid; w < n_prims * 16; w += kBlock)
      s_prim[w] = gprims[w];
  __syncthreads();
  const thip_chain& ch = s_chain;
  const double* prims = lds_prims ? s_prim : gprims;
  const int fx = pr.seg_fixed ? pr.seg_fixed[u] : 0;
  const bool f0 = (fx & 1) != 0, f1 = (fx & 2) != 0;
  const bool cast = pr.cast != 0;
  const long long row0 = item * R;

  // ---- the states of the segment (lvs_count's arithmetic; the count stays a
  // double until it is known to be within the cap: NaN gives 2, inf exceeds it)
  double jd = 0;
  for (int j = 0; j < D; ++j)
    jd += (s_q1[j] - s_q0[j]) * (s_q1[j] - s_q0[j]);
  jd = sqrt(jd);
  double cnt_d = 2.0;
  if (!pr.one_cast && jd > pr.lvs)
    cnt_d = ceil(jd / pr.lvs) + 1.0;
  if (!(cnt_d <= static_cast<double>(kMaxStates)))
  {
    for (int e = tid; e < R; e += kBlock)
    {
      values[row0 + e] = -pr.buffer;
      coeffs[row0 + e] = 1.0;
      int* kout = keys + (row0 + e) * 4;
      kout[0] = kout[1] = kout[2] = kout[3] = -1;
    }
    for (int e = tid; e < R * 2 * D; e += kBlock)
      jac[row0 * 2 * D + e] = 0.0;
    if (tid == 0)
      counts[item] = -1;
    return;
  }
  const int cnt = static_cast<int>(cnt_d);  // 2 .. kMaxStates
  const int n_sub = cast ? cnt - 1 : cnt;
  const int last = cnt - 1;
  const double dt = 1.0 / double(last);
  const int n_sph = M.n_sph;

  // Stage sub-state i: A / B the LDS buffers of its start / end state.  A cast's
  // end state is the next cast's start state, so only sub-state 0 computes both.
  // Barriers: joint values, then poses, then centres; the first one also ends
  // the previous sub-state's reads.
  int A = 0, B = 0;
  auto stage = [&](int i) {
    A = cast ? (i & 1) : 0;
    B = cast ? ((i + 1) & 1) : 0;
    const bool needA = !cast || i == 0;
    __syncthreads();
    if (tid < D && needA)
      s_qs[A][tid] = linspaced(cnt, s_q0[tid], s_q1[tid], i);
    if (cast && tid >= 64 && tid - 64 < D)
      s_qs[B][tid - 64] = linspaced(cnt, s_q0[tid - 64], s_q1[tid - 64], i + 1);
    __syncthreads();
    if (tid < n_links && needA)
    {
      Pose T;
      chain_fk(ch, s_qs[A], tid, T);
      s_T[A][tid] = T;
    }
    if (cast && tid >= 64 && tid - 64 < n_links)
    {
      Pose T;
      chain_fk(ch, s_qs[B], tid - 64, T);
      s_T[B][tid - 64] = T;
    }
    __syncthreads();
    if (tid < n_sph && needA)
      sphere_world(s_T[A][M.link[tid]], M.center[tid], s_ctr[A][tid]);
    if (cast && tid >= 64 && tid - 64 < n_sph)
      sphere_world(s_T[B][M.link[tid - 64]], M.center[tid - 64], s_ctr[B][tid - 64]);
    __syncthreads();
  };

  // ---- phase 1 and 2: scan the keys, rank the sets
  const double ninf = -INFINITY;
  const int n_scene = n_sph * n_prims;  // <= 32 * 1024
  const int total = n_scene + M.n_self_sph;
  int cur = 0, n_run = 0, count = 0;  // the same in every thread
  for (int c0 = 0; c0 < total; c0 += kBlock)
  {
    const int c = c0 + tid;
    const bool valid = c < total;
    int s = 0, p = 0, sb = -1, la = 0, lb = 0;
    double margin = 0.0;
    unsigned key = 0;
    if (valid)
    {
      if (c < n_scene)
      {
        s = c / n_prims;
        p = c - s * n_prims;
        la = M.link[s];
        margin = pr.pmc ? pr.pmc[2 * (s * pr.pw + p)] : pr.margin;
        key = pack_key(la, p, s, -1);
      }
      else
      {
        const int j = c - n_scene;
        s = M.self_sa[j];
        sb = M.self_sb[j];
        la = M.link[s];
        lb = M.link[sb];
        margin = pr.pmc ? pr.pmc[2 * (s * pr.pw + n_prims + sb)] : pr.margin;
        key = pack_key(la, -1 - lb, s, sb);
      }
    }
    // a zero-coefficient pair reads margin -inf (pair_data.hpp): never kept
    const double reach = margin + pr.buffer;
    const bool act0 = valid && M.active[la] != 0, act1 = valid && sb >= 0 && M.active[lb] != 0;
    double m00 = ninf, m01 = ninf, m10 = ninf, m11 = ninf;  // m<side><end>
    bool any = false;
    for (int i = 0; i < n_sub; ++i)
    {
      stage(i);
      if (!valid)
        continue;
      Contact ct;
      eval_contact(M, cast, i, last, dt, s, p, sb, s_ctr[A], s_ctr[B], prims, reach, ct);
      if (!kept_contact(ct.dist, reach, ct.type, f0, f1))
        continue;
      any = true;
      const double err = margin - ct.dist;
      // GradientResultsSet::add
      if (act0 && ct.type[0] != kCCTime1)
        m00 = fmax(m00, err);
      if (act0 && ct.type[0] != kCCTime0)
        m01 = fmax(m01, err);
      if (act1 && ct.type[1] != kCCTime1)
        m10 = fmax(m10, err);
      if (act1 && ct.type[1] != kCCTime0)
        m11 = fmax(m11, err);
    }
    // getMaxError / getMaxErrorT0 / getMaxErrorT1; -inf: no error at the free end
    const double E = f1 ? fmax(m00, m10) : (f0 ? fmax(m01, m11) : fmax(fmax(m00, m01), fmax(m10, m11)));
    __syncthreads();  // the last sub-state's reads; s_wcnt and the pass arrays of the previous pass
    // the selection step (this compaction, then the ranking below): the same text as csets_kernel's,
    // coll_sets.hip; a change to one is made to both
    const unsigned long long mk = __ballot(any);
    const int lrank = __popcll(mk & ((1ull << lane) - 1ull));
    if (lane == 0)
      s_wcnt[wave] = __popcll(mk);
    __syncthreads();
    int pos = lrank, n_new = 0;
    for (int w = 0; w < kWaves; ++w)
    {
      const int wc = s_wcnt[w];
      pos += (w < wave) ? wc : 0;
      n_new += wc;
    }
    if (any)
    {
      s_perr[pos] = E;
      s_pkey[pos] = key;
      s_pmax[pos][0] = m00;
      s_pmax[pos][1] = m01;
      s_pmax[pos][2] = m10;
      s_pmax[pos][3] = m11;
    }
    __syncthreads();
    count += n_new;
    if (n_new == 0)
      continue;
    const int n_pool = n_run + n_new;
    for (int i = tid; i < n_pool; i += kBlock)
    {
      const bool run = i < n_run;
      const double e = run ? s_rerr[cur][i] : s_perr[i - n_run];
      const unsigned k = run ? s_rkey[cur][i] : s_pkey[i - n_run];
      int rank = 0;
      for (int o = 0; o < n_run; ++o)
        rank += before(s_rerr[cur][o], s_rkey[cur][o], e, k) ? 1 : 0;
      for (int o = 0; o < n_new; ++o)
        rank += before(s_perr[o], s_pkey[o], e, k) ? 1 : 0;
      if (rank < R)
      {
        s_rerr[cur ^ 1][rank] = e;
        s_rkey[cur ^ 1][rank] = k;
        for (int m = 0; m < 4; ++m)
          s_rmax[cur ^ 1][rank][m] = run ? s_rmax[cur][i][m] : s_pmax[i - n_run][m];
      }
    }
    __syncthreads();
    cur ^= 1;
    n_run = min(R, n_pool);
  }

  // ---- phase 3: the selected sets
  const int n_rows = n_run;  // min(R, count)
  if (tid < R)
  {
    const int i = tid;
    int link = -1, other = -1, s = -1, sb = -1;
    double value = -pr.buffer, coeff = 1.0;
    if (i < n_rows)
    {
      unpack_key(s_rkey[cur][i], link, other, s, sb);
      const double E = s_rerr[cur][i];
      if (E != ninf)  // else getValues' branch :125-142 leaves -margin_buffer
        value = E;
      const int col = (sb < 0) ? other : n_prims + sb;
      coeff = pr.pmc ? pr.pmc[2 * (s * pr.pw + col) + 1] : pr.coeff;
    }
    values[row0 + i] = value;
    coeffs[row0 + i] = coeff;
    int* kout = keys + (row0 + i) * 4;
    kout[0] = link;
    kout[1] = other;
    kout[2] = s;
    kout[3] = sb;
  }
  if (tid == 0)
    counts[item] = count;
  if (n_rows == 0)  // no set: zero rows, and no second walk over the sub-states
  {
    for (int e = tid; e < R * 2 * D; e += kBlock)
      jac[row0 * 2 * D + e] = 0.0;
    return;
  }
  for (int e0 = 0; e0 < R * 2 * D; e0 += kBlock)
  {
    const int e = e0 + tid;
    const int i = e / (2 * D), en = (e - i * 2 * D) / D, j = e - (i * 2 + en) * D;
    const bool mine = e < R * 2 * D;
    // a row that stays zero: padding, a fixed end, a set without an error, M <= 0
    bool live = mine && i < n_rows && !(en == 0 ? f0 : f1);
    int la = 0, other = 0, s = 0, sb = -1, lb = 0;
    double margin = 0.0, Mx = 0.0, mx0 = ninf, mx1 = ninf;
    if (live)
    {
      unpack_key(s_rkey[cur][i], la, other, s, sb);
      lb = (sb >= 0) ? M.link[sb] : 0;
      const int col = (sb < 0) ? other : n_prims + sb;
      margin = pr.pmc ? pr.pmc[2 * (s * pr.pw + col)] : pr.margin;
      // getMaxErrorWithBuffer / ...T0 / ...T1: the maximum behind E, plus the buffer
      Mx = s_rerr[cur][i] + pr.buffer;
      mx0 = s_rmax[cur][i][0 + en] + pr.buffer;  // max_error[0].error_with_buffer[en]
      mx1 = s_rmax[cur][i][2 + en] + pr.buffer;
      live = Mx > 0.0 && (mx0 > 0.0 || mx1 > 0.0);
    }
    const double reach = margin + pr.buffer;
    double num = 0.0, den = 0.0;
    int terms = 0;
    for (int k = 0; k < n_sub; ++k)
    {
      stage(k);
      if (!live)
        continue;
      Contact ct;
      eval_contact(M, cast, k, last, dt, s, (sb < 0) ? other : 0, sb, s_ctr[A], s_ctr[B], prims, reach, ct);
      if (!kept_contact(ct.dist, reach, ct.type, f0, f1))
        continue;
      const double ewb = (margin - ct.dist) + pr.buffer;
      const double w = fmax(ewb, 0.0) / Mx;
      for (int sd = 0; sd < ((sb >= 0) ? 2 : 1); ++sd)
      {
        const int link = sd ? lb : la;
        const int type = ct.type[sd];
        if (!M.active[link] || (en == 0 ? type == kCCTime1 : type == kCCTime0) || !((sd ? mx1 : mx0) > 0.0))
          continue;
        // nearest_points_local in the start pose's link frame, back out through R_e
        const Pose& Ta = s_T[A][link];
        const Pose& Te = (en == 0) ? Ta : s_T[B][link];
        const double* pt = ct.pt[sd];
        const double w3[3] = { pt[0] - Ta.t[0], pt[1] - Ta.t[1], pt[2] - Ta.t[2] };
        double pl[3], r[3];
        for (int q = 0; q < 3; ++q)
          pl[q] = Ta.r[0 * 3 + q] * w3[0] + Ta.r[1 * 3 + q] * w3[1] + Ta.r[2 * 3 + q] * w3[2];
        for (int q = 0; q < 3; ++q)
          r[q] = Te.r[q * 3 + 0] * pl[0] + Te.r[q * 3 + 1] * pl[1] + Te.r[q * 3 + 2] * pl[2];
        const double g = side_gradient_at(ch, s_q0, s_q1, type, ct.time[sd], link, r, ct.n, sd ? 1.0 : -1.0, j);
        const double scale = (en == 0) ? 1 - ct.time[sd] : ct.time[sd];
        den += w;
        num += w * (scale * g);
        ++terms;
      }
    }
    if (mine)
    {
      double row = 0.0;
      if (terms > 0 && den != 0.0)
        row = -1.0 * ((1 / den) * num);
      jac[row0 * 2 * D + e] = row;
    }
  }
}
}  // namespace ccs
}  // namespace thip

using namespace thip::ccs;

struct thip_ccsets : thip::sets::Handle
{
  Params pr{};
  int* d_fixed = nullptr;
  std::vector<int> h_counts;
};

static thread_local std::string g_ccsets_create_err;

static int run_on_device(thip_ccsets* c, const double* d_x, double* values, double* jac, double* coeffs, int* counts,
                         int* keys)
{
  auto launch = [&] {
    hipLaunchKernelGGL(ccsets_kernel, dim3(static_cast<unsigned>(c->items)), dim3(kBlock), 0, c->stream, c->d_chain,
                       c->d_model, c->pr, d_x, c->d_scene, c->d_values, c->d_jac, c->d_coeffs, c->d_counts, c->d_keys);
  };
  const int rc = launch_and_fetch(c, "ccsets_kernel", launch, values, jac, coeffs, c->h_counts.data(), keys);
  if (rc != THIP_OK)
    return rc;
  if (counts)
    std::copy(c->h_counts.begin(), c->h_counts.end(), counts);
  for (size_t it = 0; it < c->items; ++it)
    if (c->h_counts[it] < 0)
      return fail(c, "thip_ccsets_run: problem " + std::to_string(it / static_cast<size_t>(c->pr.n_seg)) +
                         " segment " + std::to_string(it % static_cast<size_t>(c->pr.n_seg)) + " needs more than " +
                         std::to_string(THIP_CCSETS_MAX_SUBSTATES) +
                         " sub-states (THIP_CCSETS_MAX_SUBSTATES): its rows are padded");
  return THIP_OK;
}

extern "C" {

void thip_default_ccsets_config(thip_ccsets_config* c)
{
  if (!c)
    return;
  c->margin = 0.0;
  c->coeff = 1.0;
  c->margin_buffer = 0.0;
  c->max_num_cnt = 1;
  c->first_step = 0;
  c->last_step = 1;
  c->evaluator_type = THIP_EVALUATOR_LVS_CONTINUOUS;
  c->longest_valid_segment_length = 0.005;
}

int thip_sizeof_ccsets_config(void) { return static_cast<int>(sizeof(thip_ccsets_config)); }

int thip_ccsets_create(int device, const thip_problem_desc* desc, const thip_ccsets_config* cfg, const int* seg_fixed,
                       int batch, thip_ccsets** out)
{
  if (out)
    *out = nullptr;
  if (!desc || !cfg || !out || batch <= 0)
  {
    g_ccsets_create_err = "thip_ccsets_create: null argument or batch <= 0";
    return THIP_E_INVALID;
  }
  const thip::host::CreateError reject{ g_ccsets_create_err, "thip_ccsets_create: " };
  if (check_descriptor(*desc, *cfg, reject) != THIP_OK)
    return THIP_E_INVALID;
  const int et = cfg->evaluator_type;
  if (et != THIP_EVALUATOR_LVS_DISCRETE && et != THIP_EVALUATOR_CONTINUOUS && et != THIP_EVALUATOR_LVS_CONTINUOUS)
    return reject("evaluator_type " + std::to_string(et) +
                  " (LVS_DISCRETE = 2, CONTINUOUS = 3, LVS_CONTINUOUS = 4 are the continuous sets' evaluators)");
  if (!std::isfinite(cfg->longest_valid_segment_length) || !(cfg->longest_valid_segment_length > 0))
    return reject("longest_valid_segment_length must be finite and > 0");
  // each bound on its own: no sum or difference of caller values before they are known to lie in [0, N)
  const int N = desc->n_steps, first = cfg->first_step, last = cfg->last_step;
  if (first < 0 || first >= N || last < 0 || last >= N)
    return reject("step range [" + std::to_string(first) + ", " + std::to_string(last) + "] outside [0, " +
                  std::to_string(N - 1) + "]");
  if (first >= last)
    return reject("step range [" + std::to_string(first) + ", " + std::to_string(last) +
                  "] holds no segment: first_step < last_step");
  const int n_seg = last - first;
  if (static_cast<long long>(n_seg) * batch > INT_MAX / (THIP_CSETS_MAX_ROWS * 2 * THIP_MAX_DOF))
    return reject("batch * segments exceeds the grid");
  for (int k = 0; seg_fixed && k < n_seg; ++k)
  {
    if (seg_fixed[k] < 0 || seg_fixed[k] > 3)
      return reject("seg_fixed[" + std::to_string(k) + "] = " + std::to_string(seg_fixed[k]) + " outside [0, 3]");
    if (seg_fixed[k] == 3)
      return reject("seg_fixed[" + std::to_string(k) + "]: both ends cannot be fixed!");
  }
  std::vector<int> ssa, ssb;
  std::vector<double> tab;
  if (check_pairs(*desc, cfg->margin, cfg->coeff, reject, ssa, ssb, tab) != THIP_OK)
    return THIP_E_INVALID;

  std::unique_ptr<thip_ccsets, void (*)(thip_ccsets*)> c(new thip_ccsets(), thip_ccsets_destroy);
  c->pr.margin = cfg->margin;
  c->pr.coeff = cfg->coeff;
  c->pr.buffer = cfg->margin_buffer;
  c->pr.lvs = cfg->longest_valid_segment_length;
  c->pr.pw = desc->n_prims + desc->n_spheres;
  c->pr.R = cfg->max_num_cnt;
  c->pr.first_step = first;
  c->pr.n_seg = n_seg;
  c->pr.batch = batch;
  c->pr.N = N;
  c->pr.n_prims = desc->n_prims;
  c->pr.cast = et != THIP_EVALUATOR_LVS_DISCRETE ? 1 : 0;
  c->pr.one_cast = et == THIP_EVALUATOR_CONTINUOUS ? 1 : 0;
  c->h_counts.assign(static_cast<size_t>(batch) * n_seg, 0);
  thip_chain chain;
  std::unique_ptr<Model> md(new Model());
  fill_model(*desc, ssa, ssb, chain, *md);
  std::vector<int> fixed(static_cast<size_t>(n_seg), 0);
  for (int k = 0; seg_fixed && k < n_seg; ++k)
    fixed[k] = seg_fixed[k];

  if (allocate_and_upload(*c, device, batch, *desc, static_cast<size_t>(batch) * n_seg, cfg->max_num_cnt,
                          2 * desc->chain.n_dof, chain, *md, tab, reject) != THIP_OK)
    return THIP_E_HIP;
  hipError_t e;
  if ((e = alloc(*c, c->d_fixed, fixed.size())) != hipSuccess)
    return reject.hip("hipMalloc", e);
  if ((e = hipMemcpy(c->d_fixed, fixed.data(), fixed.size() * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess)
    return reject.hip("hipMemcpy", e);
  c->pr.pmc = c->d_pmc;
  c->pr.seg_fixed = c->d_fixed;
  *out = c.release();
  return THIP_OK;
}

int thip_ccsets_upload(thip_ccsets* cs, const double* scene)
{
  return upload_scene(cs, scene, hipMemcpyHostToDevice, "thip_ccsets_upload");
}

int thip_ccsets_upload_device(thip_ccsets* cs, const double* d_scene)
{
  return upload_scene(cs, d_scene, hipMemcpyDeviceToDevice, "thip_ccsets_upload_device");
}

int thip_ccsets_segments(const thip_ccsets* cs) { return cs ? cs->pr.n_seg : THIP_E_INVALID; }

int thip_ccsets_run(thip_ccsets* cs, const double* x, double* values, double* jac, double* coeffs, int* counts,
                    int* keys)
{
  const double* d_x = nullptr;
  const int rc = stage_x(cs, "thip_ccsets", x, true, d_x);
  return rc != THIP_OK ? rc : run_on_device(cs, d_x, values, jac, coeffs, counts, keys);
}

int thip_ccsets_run_device(thip_ccsets* cs, const double* d_x, double* values, double* jac, double* coeffs,
                           int* counts, int* keys)
{
  const int rc = stage_x(cs, "thip_ccsets", d_x, false, d_x);
  return rc != THIP_OK ? rc : run_on_device(cs, d_x, values, jac, coeffs, counts, keys);
}

double thip_ccsets_last_ms(thip_ccsets* cs) { return cs ? cs->last_ms : -1.0; }

void thip_ccsets_destroy(thip_ccsets* cs)
{
  if (!cs)
    return;
  release(*cs);
  delete cs;
}

const char* thip_ccsets_last_error(thip_ccsets* cs) { return cs ? cs->err.c_str() : g_ccsets_create_err.c_str(); }

}  // extern "C"
