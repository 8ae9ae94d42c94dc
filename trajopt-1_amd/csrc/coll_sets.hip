// Fixed-size discrete collision sets (include/trajopt_hip.h thip_csets_*): the
// rows of trajopt_ifopt's DiscreteCollisionConstraint over a
// SingleTimestepCollisionEvaluator, for every node of every problem of a batch
// in one launch --
//   calcCollisions / calcCollisionsHelper  discrete_collision_evaluators.cpp:89-188
//   getGradient                            trajopt_common/src/collision_utils.cpp:116-190
//   GradientResultsSet::add / getMaxErrorT0  collision_types.cpp:173-247
//   getWeightedAvgGradientT0               weighted_average_methods.cpp:31-68
//   getValues / getJacobian                discrete_collision_constraint.cpp:91-141
// restated on the primitive collision model (collision_device.hpp).
//
//   csets_kernel   one 256-thread workgroup per (problem, node), three phases:
//     1. scan: one chain_fk per link and the world sphere centres to LDS, then
//        the threads stride over the candidates (robot sphere x primitive, then
//        the self sphere pairs) kBlock at a time.  A pass's kept contacts
//        (coefficient not zero, distance <= margin + buffer) are compacted into
//        LDS by a ballot and a prefix over the waves' counts, in candidate
//        order.
//     2. select: the running top R (LDS, double buffered) and the pass's
//        contacts are ranked against each other -- error descending, ties by
//        the packed key (link, other, sphere, other_sphere) ascending: a strict
//        total order, so every rank is unique -- and ranks below R are written
//        to the other buffer at their rank.  No per-thread arrays, any number
//        of passes.
//     3. gradient: only for the min(R, count) selected rows, one thread per
//        (row, dof) over the link poses of phase 1.
// No atomics and no hand-off between workgroups: a problem's rows do not depend
// on its place in the batch, and every run gives the same bits.  fp64.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "coll_sets_common.hpp"
#include "collision_device.hpp"

namespace thip
{
namespace cs
{
using namespace sets;  // coll_sets_common.hpp: Model, the key packing, the row order

struct Params
{
  double margin, coeff, buffer;
  const double* pmc;  // pair_data.hpp table [n_sph][pw][2], or null: margin / coeff for every pair
  int pw;
  int R, first_step, n_nodes, batch, N, n_prims;
};

// d(distance)/d(q_j) of one side of a contact: column j of the link's linear
// jacobian (chain_jacobian's arithmetic over the link poses T) shifted to the
// contact point as the collision rows shift it (term_eval.hip contact_gradient:
// the point goes to the link frame and back), dotted with the normal; sg = -1
// for the first link, +1 for the second link of a self contact.
__device__ double side_gradient(const thip_chain& ch, const Pose* T, int link, const double* pt, const double* normal,
                                double sg, int j)
{
  const Pose& lt = T[link];
  const double w3[3] = { pt[0] - lt.t[0], pt[1] - lt.t[1], pt[2] - lt.t[2] };
  double pl[3], r[3];
  for (int k = 0; k < 3; ++k)
    pl[k] = lt.r[0 * 3 + k] * w3[0] + lt.r[1 * 3 + k] * w3[1] + lt.r[2 * 3 + k] * w3[2];
  for (int i = 0; i < 3; ++i)
    r[i] = lt.r[i * 3 + 0] * pl[0] + lt.r[i * 3 + 1] * pl[1] + lt.r[i * 3 + 2] * pl[2];
  const unsigned path = chain_path(ch, link);
  double g = 0.0;
  for (int k = 1; k <= link; ++k)
  {
    const int type = ch.joint_type[k];
    if (type == THIP_JOINT_FIXED || !((path >> k) & 1u) || ch.joint_dof[k] != j)
      continue;
    const double* ax = ch.joint_axis[k];
    double a[3];
    for (int i = 0; i < 3; ++i)
      a[i] = T[k].r[i * 3 + 0] * ax[0] + T[k].r[i * 3 + 1] * ax[1] + T[k].r[i * 3 + 2] * ax[2];
    double l0 = a[0], l1 = a[1], l2 = a[2];
    if (type != THIP_JOINT_PRISMATIC)
    {
      const double d[3] = { lt.t[0] - T[k].t[0], lt.t[1] - T[k].t[1], lt.t[2] - T[k].t[2] };
      l0 = (a[1] * d[2] - a[2] * d[1]) + (a[1] * r[2] - a[2] * r[1]);
      l1 = (a[2] * d[0] - a[0] * d[2]) + (a[2] * r[0] - a[0] * r[2]);
      l2 = (a[0] * d[1] - a[1] * d[0]) + (a[0] * r[1] - a[1] * r[0]);
    }
    g = sg * (normal[0] * l0 + normal[1] * l1 + normal[2] * l2);
  }
  return g;
}

__global__ __launch_bounds__(kBlock) void csets_kernel(const thip_chain* chain, const Model* model, Params pr,
                                                      const double* x, const double* scene, double* values,
                                                      double* jac, double* coeffs, int* counts, int* keys)
{
  const long long item = blockIdx.x;
  if (item >= static_cast<long long>(pr.n_nodes) * pr.batch)
    return;
  const int b = static_cast<int>(item / pr.n_nodes), u = static_cast<int>(item % pr.n_nodes);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ thip_chain s_chain;
  __shared__ double s_q[THIP_MAX_DOF];
  __shared__ Pose s_T[THIP_MAX_LINKS];
  __shared__ double s_ctr[THIP_MAX_SPHERES][3];
  __shared__ double s_prim[kLdsPrims * 16];
  __shared__ double s_rerr[2][kMaxRows];  // the running top R, double buffered
  __shared__ unsigned s_rkey[2][kMaxRows];
  __shared__ double s_perr[kBlock];  // one pass's kept contacts, candidate order
  __shared__ unsigned s_pkey[kBlock];
  __shared__ int s_wcnt[kWaves];
  __shared__ double s_nrm[kMaxRows][3];  // the selected rows' normal and contact points
  __shared__ double s_pt[kMaxRows][2][3];

  const Model& M = *model;
  const int n_prims = pr.n_prims, R = pr.R;
  // the prologue (chain and scene to LDS): the same text as ccsets_kernel's, coll_sets_cont.hip
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
    s_q[tid] = x[(static_cast<long long>(b) * pr.N + pr.first_step + u) * D + tid];
  if (lds_prims)
    for (int w = tid; w < n_prims * 16; w += kBlock)
      s_prim[w] = gprims[w];
  __syncthreads();
  const thip_chain& ch = s_chain;
  const double* prims = lds_prims ? s_prim : gprims;

  // ---- phase 1: link poses, sphere centres, distance scan
  if (tid < n_links)
  {
    Pose T;
    chain_fk(ch, s_q, tid, T);
    s_T[tid] = T;
  }
  __syncthreads();
  const int n_sph = M.n_sph;
  if (tid < n_sph)
    sphere_world(s_T[M.link[tid]], M.center[tid], s_ctr[tid]);
  __syncthreads();

  const int n_scene = n_sph * n_prims;  // <= 32 * 1024
  const int total = n_scene + M.n_self_sph;
  int cur = 0, n_run = 0, count = 0;  // the same in every thread
  for (int c0 = 0; c0 < total; c0 += kBlock)
  {
    const int c = c0 + tid;
    bool kept = false;
    double err = 0.0;
    unsigned key = 0;
    if (c < total)
    {
      double dist, n[3], margin;
      if (c < n_scene)
      {
        const int s = c / n_prims, p = c - s * n_prims;
        double pt[3];
        sphere_prim_distance(s_ctr[s], M.radius[s], prims + 16 * p, dist, n, pt);
        margin = pr.pmc ? pr.pmc[2 * (s * pr.pw + p)] : pr.margin;
        key = pack_key(M.link[s], p, s, -1);
      }
      else
      {
        const int j = c - n_scene;
        const int s = M.self_sa[j], sb = M.self_sb[j];
        double pa[3], pb[3], ta, tb;
        self_sphere_distance(s_ctr[s], s_ctr[s], M.radius[s], s_ctr[sb], s_ctr[sb], M.radius[sb], false, dist, n, pa,
                             pb, ta, tb);
        margin = pr.pmc ? pr.pmc[2 * (s * pr.pw + n_prims + sb)] : pr.margin;
        key = pack_key(M.link[s], -1 - M.link[sb], s, sb);
      }
      // a zero-coefficient pair reads margin -inf (pair_data.hpp): never kept
      kept = dist <= margin + pr.buffer;
      err = margin - dist;
    }
    // the selection step (this compaction, then the ranking below): the same text as ccsets_kernel's,
    // coll_sets_cont.hip; a change to one is made to both
    const unsigned long long m = __ballot(kept);
    const int lrank = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0)
      s_wcnt[wave] = __popcll(m);
    __syncthreads();
    int pos = lrank, n_new = 0;
    for (int w = 0; w < kWaves; ++w)
    {
      const int wc = s_wcnt[w];
      pos += (w < wave) ? wc : 0;
      n_new += wc;
    }
    if (kept)
    {
      s_perr[pos] = err;
      s_pkey[pos] = key;
    }
    __syncthreads();  // also: s_wcnt is read before the next pass writes it
    count += n_new;
    if (n_new == 0)
      continue;
    // ---- phase 2: rank the running rows and the pass's contacts together
    const int n_pool = n_run + n_new;
    for (int i = tid; i < n_pool; i += kBlock)
    {
      const double e = (i < n_run) ? s_rerr[cur][i] : s_perr[i - n_run];
      const unsigned k = (i < n_run) ? s_rkey[cur][i] : s_pkey[i - n_run];
      int rank = 0;
      for (int o = 0; o < n_run; ++o)
        rank += before(s_rerr[cur][o], s_rkey[cur][o], e, k) ? 1 : 0;
      for (int o = 0; o < n_new; ++o)
        rank += before(s_perr[o], s_pkey[o], e, k) ? 1 : 0;
      if (rank < R)
      {
        s_rerr[cur ^ 1][rank] = e;
        s_rkey[cur ^ 1][rank] = k;
      }
    }
    __syncthreads();
    cur ^= 1;
    n_run = min(R, n_pool);
  }

  // ---- phase 3: the selected rows
  const int n_rows = n_run;  // min(R, count)
  const long long row0 = item * R;
  if (tid < R)
  {
    const int i = tid;
    int link = -1, other = -1, s = -1, sb = -1;
    double value = -pr.buffer, coeff = 1.0;
    if (i < n_rows)
    {
      unpack_key(s_rkey[cur][i], link, other, s, sb);
      value = s_rerr[cur][i];
      const int col = (sb < 0) ? other : n_prims + sb;
      coeff = pr.pmc ? pr.pmc[2 * (s * pr.pw + col) + 1] : pr.coeff;
      double dist, ta, tb;
      if (sb < 0)
      {
        sphere_prim_distance(s_ctr[s], M.radius[s], prims + 16 * other, dist, s_nrm[i], s_pt[i][0]);
        s_pt[i][1][0] = s_pt[i][1][1] = s_pt[i][1][2] = 0.0;
      }
      else
        self_sphere_distance(s_ctr[s], s_ctr[s], M.radius[s], s_ctr[sb], s_ctr[sb], M.radius[sb], false, dist,
                             s_nrm[i], s_pt[i][0], s_pt[i][1], ta, tb);
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
  __syncthreads();
  for (int e = tid; e < R * D; e += kBlock)
  {
    const int i = e / D, j = e - i * D;
    double row = 0.0;
    if (i < n_rows)
    {
      int link, other, s, sb;
      unpack_key(s_rkey[cur][i], link, other, s, sb);
      // a set whose error_with_buffer is not positive has weight zero
      // (weighted_average_methods.cpp:49): a zero gradient
      if (s_rerr[cur][i] + pr.buffer > 0.0)
      {
        double g = 0.0;
        int sides = 0;
        if (M.active[link])
        {
          g += side_gradient(ch, s_T, link, s_pt[i][0], s_nrm[i], -1.0, j);
          ++sides;
        }
        if (sb >= 0 && M.active[M.link[sb]])
        {
          g += side_gradient(ch, s_T, M.link[sb], s_pt[i][1], s_nrm[i], 1.0, j);
          ++sides;
        }
        // getWeightedAvgGradientT0 (weighted_average_methods.cpp:41-68) adds the
        // set's weight to total_weight once per link that has a gradient: a self
        // pair with both links active comes out as (g0 + g1) / 2, not g0 + g1
        if (sides == 2)
          g = 0.5 * g;
        row = 0.0 - g;  // getJacobian: -1 * grad_vec (discrete_collision_constraint.cpp:137)
      }
    }
    jac[row0 * D + e] = row;
  }
}
}  // namespace cs
}  // namespace thip

using namespace thip::cs;

struct thip_csets : thip::sets::Handle
{
  Params pr{};
};

static thread_local std::string g_csets_create_err;

static int run_on_device(thip_csets* c, const double* d_x, double* values, double* jac, double* coeffs, int* counts,
                         int* keys)
{
  auto launch = [&] {
    hipLaunchKernelGGL(csets_kernel, dim3(static_cast<unsigned>(c->items)), dim3(kBlock), 0, c->stream, c->d_chain,
                       c->d_model, c->pr, d_x, c->d_scene, c->d_values, c->d_jac, c->d_coeffs, c->d_counts, c->d_keys);
  };
  return launch_and_fetch(c, "csets_kernel", launch, values, jac, coeffs, counts, keys);
}

extern "C" {

void thip_default_csets_config(thip_csets_config* c)
{
  if (!c)
    return;
  c->margin = 0.0;
  c->coeff = 1.0;
  c->margin_buffer = 0.0;
  c->max_num_cnt = 1;
  c->first_step = 0;
  c->last_step = 0;
}

int thip_sizeof_csets_config(void) { return static_cast<int>(sizeof(thip_csets_config)); }

int thip_csets_create(int device, const thip_problem_desc* desc, const thip_csets_config* cfg, int batch,
                      thip_csets** out)
{
  if (out)
    *out = nullptr;
  if (!desc || !cfg || !out || batch <= 0)
  {
    g_csets_create_err = "thip_csets_create: null argument or batch <= 0";
    return THIP_E_INVALID;
  }
  const thip::host::CreateError reject{ g_csets_create_err, "thip_csets_create: " };
  if (check_descriptor(*desc, *cfg, reject) != THIP_OK)
    return THIP_E_INVALID;
  // each bound on its own: no sum or difference of caller values before they are known to lie in [0, N)
  const int N = desc->n_steps, first = cfg->first_step, last = cfg->last_step;
  if (first < 0 || first >= N || last < 0 || last >= N)
    return reject("step range [" + std::to_string(first) + ", " + std::to_string(last) + "] outside [0, " +
                  std::to_string(N - 1) + "]");
  if (last < first)
    return reject("inverted step range [" + std::to_string(first) + ", " + std::to_string(last) + "]");
  const int n_nodes = last - first + 1;
  if (static_cast<long long>(n_nodes) * batch > INT_MAX / (THIP_CSETS_MAX_ROWS * 4))
    return reject("batch * nodes exceeds the grid");
  std::vector<int> ssa, ssb;
  std::vector<double> tab;
  if (check_pairs(*desc, cfg->margin, cfg->coeff, reject, ssa, ssb, tab) != THIP_OK)
    return THIP_E_INVALID;

  std::unique_ptr<thip_csets, void (*)(thip_csets*)> c(new thip_csets(), thip_csets_destroy);
  c->pr.margin = cfg->margin;
  c->pr.coeff = cfg->coeff;
  c->pr.buffer = cfg->margin_buffer;
  c->pr.pw = desc->n_prims + desc->n_spheres;
  c->pr.R = cfg->max_num_cnt;
  c->pr.first_step = first;
  c->pr.n_nodes = n_nodes;
  c->pr.batch = batch;
  c->pr.N = N;
  c->pr.n_prims = desc->n_prims;
  thip_chain chain;
  std::unique_ptr<Model> md(new Model());
  fill_model(*desc, ssa, ssb, chain, *md);
  if (allocate_and_upload(*c, device, batch, *desc, static_cast<size_t>(batch) * n_nodes, cfg->max_num_cnt,
                          desc->chain.n_dof, chain, *md, tab, reject) != THIP_OK)
    return THIP_E_HIP;
  c->pr.pmc = c->d_pmc;
  *out = c.release();
  return THIP_OK;
}

int thip_csets_upload(thip_csets* cs, const double* scene)
{
  return upload_scene(cs, scene, hipMemcpyHostToDevice, "thip_csets_upload");
}

int thip_csets_upload_device(thip_csets* cs, const double* d_scene)
{
  return upload_scene(cs, d_scene, hipMemcpyDeviceToDevice, "thip_csets_upload_device");
}

int thip_csets_nodes(const thip_csets* cs) { return cs ? cs->pr.n_nodes : THIP_E_INVALID; }

int thip_csets_run(thip_csets* cs, const double* x, double* values, double* jac, double* coeffs, int* counts,
                   int* keys)
{
  const double* d_x = nullptr;
  const int rc = stage_x(cs, "thip_csets", x, true, d_x);
  return rc != THIP_OK ? rc : run_on_device(cs, d_x, values, jac, coeffs, counts, keys);
}

int thip_csets_run_device(thip_csets* cs, const double* d_x, double* values, double* jac, double* coeffs, int* counts,
                          int* keys)
{
  const int rc = stage_x(cs, "thip_csets", d_x, false, d_x);
  return rc != THIP_OK ? rc : run_on_device(cs, d_x, values, jac, coeffs, counts, keys);
}

double thip_csets_last_ms(thip_csets* cs) { return cs ? cs->last_ms : -1.0; }

void thip_csets_destroy(thip_csets* cs)
{
  if (!cs)
    return;
  release(*cs);
  delete cs;
}

const char* thip_csets_last_error(thip_csets* cs) { return cs ? cs->err.c_str() : g_csets_create_err.c_str(); }

}  // extern "C"
