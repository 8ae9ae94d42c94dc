// Batched trajectory collision check (include/trajopt_hip.h thip_check_*):
// tesseract's checkTrajectory as the reference's tests run it after a solve,
// one verdict and one clearance figure per problem, from trajectories on the
// device.
//
//   traj_check_kernel  one 256-thread workgroup per (unit, problem); a unit is a
//                      waypoint (DISCRETE) or a step pair with its LVS sub-states
//                      (collision_terms.cpp:846-852).  Sub-states are taken
//                      kChunk at a time: each (sub-state, sphere-carrying link)
//                      gets ONE chain_fk, the world sphere centres go to LDS
//                      (a cast reads sub-states i and i + 1, so a continuous
//                      chunk holds kChunk + 1 states and chunks overlap by one),
//                      then the threads stride over the chunk's candidates.
//                      Candidates are numbered in coll_eval_kernel's flattened
//                      ContactResultMap order (term_eval.hip); every thread keeps
//                      its smallest distance with that number (the lower number
//                      wins a tie) and a contact count, reduced by shuffles in a
//                      wave and through LDS across waves.  One record per unit.
//   traj_fold_kernel   one wave per problem folds the unit records in unit order.
// No atomics, no hand-off between workgroups: the same bits every run.  fp64;
// the distance functions are collision_device.hpp's, unchanged.  No gradients,
// no contact records, no fixed-step filter, no buffer, no per-pair margins.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "collision_device.hpp"
#include "desc_lowering.hpp"
#include "device_handle.hpp"
#include "kin_device.hpp"

namespace thip
{
namespace chk
{
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = THIP_CHECK_CHUNK;
constexpr int kLdsPrims = THIP_MAX_PRIMS;  // scenes up to this size are staged in LDS
constexpr long long kNoCand = LLONG_MAX;

// the robot spheres grouped by link, ascending (ContactResultMap key order), and
// the self-collision sphere pairs in key order (self_pairs.hpp)
struct Model
{
  int n_sph, n_groups;
  int grp_link[THIP_MAX_SPHERES];
  int grp_s0[THIP_MAX_SPHERES];  // spheres in the groups before this one
  int grp_ns[THIP_MAX_SPHERES];
  int sph_order[THIP_MAX_SPHERES];
  int slot_grp[THIP_MAX_SPHERES];  // group of position k of sph_order
  double center[THIP_MAX_SPHERES][3];
  double radius[THIP_MAX_SPHERES];
  int link[THIP_MAX_SPHERES];
  int n_self_keys, n_self_sph;
  int self_sa[THIP_MAX_SELF_SPHERE_PAIRS];
  int self_sb[THIP_MAX_SELF_SPHERE_PAIRS];
  int self_key[THIP_MAX_SELF_SPHERE_PAIRS];  // key of sphere pair j
  int self_kp[THIP_MAX_SELF_PAIRS + 1];
};

struct Params
{
  int single;      // DISCRETE: one state per unit
  int continuous;  // casts between consecutive sub-states
  double lvs, margin;
  int first_step, n_units, batch, N, n_prims;
};

struct UnitRec
{
  double dist, cc_time;
  long long n_cand;
  int count, link, other, sphere, substate, pad_;
};

__device__ __forceinline__ void sphere_world(const Pose& T, const double* cl, double* c)
{
  for (int r = 0; r < 3; ++r)
    c[r] = T.r[r * 3 + 0] * cl[0] + T.r[r * 3 + 1] * cl[1] + T.r[r * 3 + 2] * cl[2] + T.t[r];
}

__device__ __forceinline__ bool before(double d, long long i, double bd, long long bi)
{
  return d < bd || (d == bd && i < bi);
}

__global__ __launch_bounds__(kBlock) void traj_check_kernel(const thip_chain* chain, const Model* model, Params pr,
                                                           const double* x, const double* scene, UnitRec* recs,
                                                           double* unit_min)
{
  const long long item = blockIdx.x;
  if (item >= static_cast<long long>(pr.n_units) * pr.batch)
    return;
  const int b = static_cast<int>(item / pr.n_units), u = static_cast<int>(item % pr.n_units);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ thip_chain s_chain;
  __shared__ double s_q[2][THIP_MAX_DOF];
  __shared__ double s_ctr[kChunk + 1][THIP_MAX_SPHERES][3];
  __shared__ double s_prim[kLdsPrims * 16];
  __shared__ double s_wd[kWaves];
  __shared__ long long s_wi[kWaves];
  __shared__ int s_wc[kWaves];

  const Model& M = *model;
  const int n_prims = pr.n_prims;
  const double* gprims = scene + static_cast<long long>(b) * (n_prims > 0 ? n_prims : 1) * 16;
  const bool lds_prims = n_prims <= kLdsPrims;
  {
    const int* src = reinterpret_cast<const int*>(chain);
    int* dst = reinterpret_cast<int*>(&s_chain);
    for (int w = tid; w < static_cast<int>(sizeof(thip_chain) / 4); w += kBlock)
      dst[w] = src[w];
  }
  const int D = chain->n_dof;
  const int t0 = pr.first_step + u;
  if (tid < 2 * D)
  {
    const int e = tid / D, j = tid % D;
    const int t = (e == 1 && !pr.single) ? t0 + 1 : t0;
    s_q[e][j] = x[(static_cast<long long>(b) * pr.N + t) * D + j];
  }
  if (lds_prims)
    for (int w = tid; w < n_prims * 16; w += kBlock)
      s_prim[w] = gprims[w];
  __syncthreads();
  const thip_chain& ch = s_chain;
  const double* prims = lds_prims ? s_prim : gprims;
  const double* q0 = s_q[0];
  const double* q1 = s_q[1];

  // sub-states (DiscreteCollisionEvaluator / CastCollisionEvaluator, collision_terms.cpp:846-852)
  const int cnt = pr.single ? 1 : lvs_count(q0, q1, D, pr.lvs);
  const int n_sub = pr.single ? 1 : (pr.continuous ? cnt - 1 : cnt);
  const int last = cnt - 1;
  const double dt = pr.single ? 0.0 : 1.0 / double(last);
  const int n_sph = M.n_sph, n_groups = M.n_groups;
  const long long scene_total = static_cast<long long>(n_sph) * n_prims * n_sub;
  const long long total = scene_total + static_cast<long long>(M.n_self_sph) * n_sub;

  double bd = HUGE_VAL, bcc = 0.0;
  long long bi = kNoCand;
  int blink = -1, bother = -1, bsph = -1, bsub = -1, count = 0;

  for (int i0 = 0; i0 < n_sub; i0 += kChunk)
  {
    const int nc = min(kChunk, n_sub - i0);
    const int nst = pr.continuous ? nc + 1 : nc;
    // one FK per (state of the chunk, sphere-carrying link): world centres to LDS
    for (int it = tid; it < nst * n_groups; it += kBlock)
    {
      const int j = it / n_groups, g = it - j * n_groups;
      double q[THIP_MAX_DOF];
      for (int k = 0; k < D; ++k)
        q[k] = pr.single ? q0[k] : linspaced(cnt, q0[k], q1[k], i0 + j);
      Pose T;
      chain_fk(ch, q, M.grp_link[g], T);
      const int s0 = M.grp_s0[g], ng = M.grp_ns[g];
      for (int e = 0; e < ng; ++e)
      {
        const int s = M.sph_order[s0 + e];
        sphere_world(T, M.center[s], s_ctr[j][s]);
      }
    }
    __syncthreads();
    const int K = n_prims * nc;
    const int n_scene_loc = n_sph * K;
    const int n_loc = n_scene_loc + M.n_self_sph * nc;
    for (int c = tid; c < n_loc; c += kBlock)
    {
      double dist, cc = 0.0, n[3];
      long long gi;
      int il, link, other, s;
      if (c < n_scene_loc)
      {
        // (group, primitive, sub-state, sphere of the group) in map order
        const int g = M.slot_grp[c / K];
        const int s0 = M.grp_s0[g], ng = M.grp_ns[g];
        const int rr = c - s0 * K;
        const int p = rr / (nc * ng), r2 = rr - p * (nc * ng);
        il = r2 / ng;
        const int e = r2 - il * ng;
        s = M.sph_order[s0 + e];
        link = M.grp_link[g];
        other = p;
        gi = static_cast<long long>(s0) * n_prims * n_sub + (static_cast<long long>(p) * n_sub + (i0 + il)) * ng + e;
        const double* prim = prims + 16 * p;
        double pt[3];
        if (pr.continuous)
        {
          double ts = 0;
          swept_sphere_prim_distance(s_ctr[il][s], s_ctr[il + 1][s], M.radius[s], prim, dist, n, pt, ts);
          cc = (double(i0 + il) + ts) * dt;
        }
        else
        {
          sphere_prim_distance(s_ctr[il][s], M.radius[s], prim, dist, n, pt);
          if (!pr.single)
            cc = double(i0 + il) * dt;
        }
      }
      else
      {
        // a self-collision candidate: key (link pair), sub-state, sphere pair of the key
        const int r = c - n_scene_loc;
        const int k = M.self_key[r / nc];
        const int k0 = M.self_kp[k], npk = M.self_kp[k + 1] - k0;
        const int rr = r - k0 * nc;
        il = rr / npk;
        const int e = rr - il * npk, j = k0 + e;
        s = M.self_sa[j];
        const int sb = M.self_sb[j];
        link = M.link[s];
        other = -1 - sb;
        gi = scene_total + static_cast<long long>(k0) * n_sub + static_cast<long long>(i0 + il) * npk + e;
        const int il1 = pr.continuous ? il + 1 : il;
        double pa[3], pb[3], ta, tb;
        self_sphere_distance(s_ctr[il][s], s_ctr[il1][s], M.radius[s], s_ctr[il][sb], s_ctr[il1][sb], M.radius[sb],
                             pr.continuous != 0, dist, n, pa, pb, ta, tb);
        if (pr.continuous)
          cc = (double(i0 + il) + ta) * dt;
        else if (!pr.single)
          cc = double(i0 + il) * dt;
      }
      count += (dist < pr.margin) ? 1 : 0;
      if (before(dist, gi, bd, bi))
      {
        bd = dist;
        bi = gi;
        bcc = cc;
        blink = link;
        bother = other;
        bsph = s;
        bsub = pr.single ? 0 : i0 + il;
      }
    }
    __syncthreads();  // the next chunk overwrites the centres
  }

  // wave64 reduction by shuffles, then across the waves through LDS
  double wd = bd;
  long long wi = bi;
  int wc = count;
  for (int off = 32; off > 0; off >>= 1)
  {
    const double od = __shfl_xor(wd, off);
    const long long oi = __shfl_xor(wi, off);
    wc += __shfl_xor(wc, off);
    if (before(od, oi, wd, wi))
    {
      wd = od;
      wi = oi;
    }
  }
  if (lane == 0)
  {
    s_wd[wave] = wd;
    s_wi[wave] = wi;
    s_wc[wave] = wc;
  }
  __syncthreads();
  wd = s_wd[0];
  wi = s_wi[0];
  wc = s_wc[0];
  for (int w = 1; w < kWaves; ++w)
  {
    if (before(s_wd[w], s_wi[w], wd, wi))
    {
      wd = s_wd[w];
      wi = s_wi[w];
    }
    wc += s_wc[w];
  }
  UnitRec& rec = recs[item];
  if (tid == 0)
  {
    rec.count = wc;
    rec.n_cand = total > 0 ? total : 0;
    rec.pad_ = 0;
    if (unit_min)
      unit_min[item] = wd;
    if (wi == kNoCand)
    {
      rec.dist = HUGE_VAL;
      rec.cc_time = 0.0;
      rec.link = rec.other = rec.sphere = rec.substate = -1;
    }
  }
  // candidate numbers are unique: only the minimum's thread decodes its record
  if (wi != kNoCand && bi == wi)
  {
    rec.dist = bd;
    rec.cc_time = bcc;
    rec.link = blink;
    rec.other = bother;
    rec.sphere = bsph;
    rec.substate = bsub;
  }
}

// one wave per problem: the units in order (the earlier unit wins a tie)
__global__ __launch_bounds__(64) void traj_fold_kernel(const UnitRec* recs, Params pr, thip_check_result* results)
{
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= pr.batch)
    return;
  const UnitRec* r = recs + static_cast<long long>(b) * pr.n_units;
  double bd = HUGE_VAL;
  long long bu = kNoCand, n_cand = 0;
  int count = 0, first = INT_MAX;
  for (int u = lane; u < pr.n_units; u += 64)
  {
    if (r[u].link >= 0 && before(r[u].dist, u, bd, bu))
    {
      bd = r[u].dist;
      bu = u;
    }
    count += r[u].count;
    n_cand += r[u].n_cand;
    if (r[u].count > 0)
      first = min(first, u);
  }
  for (int off = 32; off > 0; off >>= 1)
  {
    const double od = __shfl_xor(bd, off);
    const long long ou = __shfl_xor(bu, off);
    count += __shfl_xor(count, off);
    n_cand += __shfl_xor(n_cand, off);
    first = min(first, __shfl_xor(first, off));
    if (before(od, ou, bd, bu))
    {
      bd = od;
      bu = ou;
    }
  }
  if (lane != 0)
    return;
  thip_check_result& o = results[b];
  o.found = count > 0 ? 1 : 0;
  o.n_contacts = count;
  o.first_unit = first == INT_MAX ? -1 : pr.first_step + first;
  o.n_candidates = n_cand;
  if (bu == kNoCand)
  {
    o.min_distance = HUGE_VAL;
    o.min_t = o.min_link = o.min_other = o.min_sphere = o.min_substate = -1;
    o.min_cc_time = 0.0;
    return;
  }
  const UnitRec& m = r[bu];
  o.min_distance = m.dist;
  o.min_t = pr.first_step + static_cast<int>(bu);
  o.min_link = m.link;
  o.min_other = m.other;
  o.min_sphere = m.sphere;
  o.min_substate = m.substate;
  o.min_cc_time = m.cc_time;
}
}  // namespace chk
}  // namespace thip

using namespace thip::chk;

struct thip_check : thip::host::Handle
{
  Params pr{};
  int D = 0;
  thip_chain* d_chain = nullptr;
  Model* d_model = nullptr;
  double* d_scene = nullptr;
  double* d_x = nullptr;  // staging of host trajectories
  UnitRec* d_recs = nullptr;
  double* d_unit_min = nullptr;
  thip_check_result* d_results = nullptr;
};

static thread_local std::string g_check_create_err;

namespace
{
// thip_check_run (x on the host) and thip_check_run_device
int run(thip_check* c, bool on_host, const double* x, thip_check_result* results, double* unit_min)
{
  if (!c)
    return THIP_E_INVALID;
  const size_t B = static_cast<size_t>(c->batch), nu = static_cast<size_t>(c->pr.n_units);
  const double* d_x = nullptr;
  if (const int rc = stage_x(c, "thip_check", on_host, x, results != nullptr, " / results", c->d_x,
                             B * static_cast<size_t>(c->pr.N) * c->D, d_x);
      rc != THIP_OK)
    return rc;
  auto launch = [&] {
    hipLaunchKernelGGL(traj_check_kernel, dim3(static_cast<unsigned>(B * nu)), dim3(kBlock), 0, c->stream, c->d_chain,
                       c->d_model, c->pr, d_x, c->d_scene, c->d_recs, c->d_unit_min);
    if (const int rc = launched(c, "traj_check_kernel"); rc != THIP_OK)
      return rc;
    hipLaunchKernelGGL(traj_fold_kernel, dim3(c->batch), dim3(64), 0, c->stream, c->d_recs, c->pr, c->d_results);
    return launched(c, "traj_fold_kernel");
  };
  auto fetch = [&] {
    const hipError_t e = to_host(c, results, c->d_results, B * sizeof(thip_check_result));
    return e != hipSuccess ? e : to_host(c, unit_min, c->d_unit_min, B * nu * sizeof(double));
  };
  return timed_run(c, "traj_check_kernel", launch, fetch);
}
}  // namespace

extern "C" {

void thip_default_check_config(thip_check_config* c)
{
  if (!c)
    return;
  c->type = 1;
  c->lvs = HUGE_VAL;
  c->margin = 0.0;
  c->first_step = 0;
  c->last_step = -1;
}

int thip_sizeof_check_config(void) { return static_cast<int>(sizeof(thip_check_config)); }
int thip_sizeof_check_result(void) { return static_cast<int>(sizeof(thip_check_result)); }

int thip_check_create(int device, const thip_problem_desc* desc, const thip_check_config* cfg, int batch,
                      thip_check** out)
{
  if (out)
    *out = nullptr;
  if (!desc || !cfg || !out || batch <= 0)
  {
    g_check_create_err = "thip_check_create: null argument or batch <= 0";
    return THIP_E_INVALID;
  }
  const thip::host::CreateError reject{ g_check_create_err, "thip_check_create: " };
  {
    const std::string why = thip::lowering::abi_mismatch(*desc);
    if (!why.empty())
      return reject(why);
  }
  const thip_chain& ch = desc->chain;
  const int N = desc->n_steps;
  if (const char* why = thip::lowering::chain_range_finding(ch))
    return reject(why);
  if (const char* why = thip::lowering::chain_table_finding(ch))
    return reject(why);
  if (N < 1 || N > THIP_EVAL_MAX_STEPS)
    return reject("n_steps out of range");
  if (desc->n_prims < 0 || desc->n_prims > THIP_EVAL_MAX_PRIMS)
    return reject("n_prims out of range");
  if (desc->n_spheres < 1 || desc->n_spheres > THIP_MAX_SPHERES)
    return reject("n_spheres out of range (a check needs at least one robot sphere)");
  for (int s = 0; s < desc->n_spheres; ++s)
  {
    if (desc->sphere_link[s] < 1 || desc->sphere_link[s] >= ch.n_links)
      return reject("bad sphere link of robot sphere " + std::to_string(s));
    if (!(desc->sphere_radius[s] >= 0))
      return reject("bad sphere radius of robot sphere " + std::to_string(s));
  }
  if (cfg->type < 0 || cfg->type > 2)
    return reject("bad type " + std::to_string(cfg->type) + " (0 LVS_DISCRETE, 1 LVS_CONTINUOUS, 2 DISCRETE)");
  if (cfg->type != 2 && !(cfg->lvs > 0))
    return reject("lvs (longest_valid_segment_length) must be positive for an LVS kind");
  if (!std::isfinite(cfg->margin))
    return reject("margin is not finite");
  const int first = cfg->first_step, last = cfg->last_step < 0 ? N - 1 : cfg->last_step;
  if (first < 0 || first >= N || last >= N || last < first || (cfg->type != 2 && last == first))
    return reject("empty or inverted step range [" + std::to_string(cfg->first_step) + ", " +
                  std::to_string(cfg->last_step) + "]");
  const int n_units = cfg->type == 2 ? last - first + 1 : last - first;
  if (static_cast<long long>(n_units) * batch > INT_MAX)
    return reject("batch * units exceeds the grid");
  std::vector<int> ssa, ssb, skp;
  {
    const std::string why = thip::self_sphere_pairs(*desc, ssa, ssb, skp);
    if (!why.empty())
      return reject(why);
  }

  std::unique_ptr<thip_check, void (*)(thip_check*)> c(new thip_check(), thip_check_destroy);
  c->device = device;
  c->batch = batch;
  c->D = ch.n_dof;
  c->pr.single = cfg->type == 2;
  c->pr.continuous = cfg->type == 1;
  c->pr.lvs = cfg->lvs;
  c->pr.margin = cfg->margin;
  c->pr.first_step = first;
  c->pr.n_units = n_units;
  c->pr.batch = batch;
  c->pr.N = N;
  c->pr.n_prims = desc->n_prims;
  thip_chain chain = ch;
  thip::lowering::fill_serial_parents(chain);
  Model md{};
  {
    const thip_problem_desc& d = *desc;
    thip::lowering::fill_sphere_model(d, ssa, ssb, md);
    std::copy(d.sphere_link, d.sphere_link + d.n_spheres, md.link);
    thip::lowering::store_sphere_groups(thip::lowering::group_spheres_by_link(d), md);
    for (int g = 0; g < md.n_groups; ++g)
      for (int k = md.grp_s0[g]; k < md.grp_s0[g] + md.grp_ns[g]; ++k)
        md.slot_grp[k] = g;
    md.n_self_keys = static_cast<int>(skp.size()) - 1;
    for (size_t k = 0; k < skp.size(); ++k)
      md.self_kp[k] = skp[k];
    for (int k = 0; k < md.n_self_keys; ++k)
      for (int j = skp[static_cast<size_t>(k)]; j < skp[static_cast<size_t>(k) + 1]; ++j)
        md.self_key[j] = k;
  }
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess)
    return reject.hip("hipSetDevice", e);
  const size_t B = static_cast<size_t>(batch), nu = static_cast<size_t>(n_units);
  const size_t np = static_cast<size_t>(std::max(desc->n_prims, 1));
  if ((e = alloc(*c, c->d_chain, 1)) != hipSuccess || (e = alloc(*c, c->d_model, 1)) != hipSuccess ||
      (e = alloc(*c, c->d_scene, B * np * 16)) != hipSuccess ||
      (e = alloc(*c, c->d_x, B * static_cast<size_t>(N) * c->D)) != hipSuccess ||
      (e = alloc(*c, c->d_recs, B * nu)) != hipSuccess || (e = alloc(*c, c->d_unit_min, B * nu)) != hipSuccess ||
      (e = alloc(*c, c->d_results, B)) != hipSuccess)
    return reject.hip("hipMalloc", e);
  if ((e = open_stream(*c)) != hipSuccess)
    return reject.hip("hipStreamCreate", e);
  if ((e = open_events(*c)) != hipSuccess)
    return reject.hip("hipEventCreate", e);
  // results are written field by field: clear once so the padding bytes are the same every run
  if ((e = hipMemcpyAsync(c->d_chain, &chain, sizeof(thip_chain), hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
      (e = hipMemcpyAsync(c->d_model, &md, sizeof(Model), hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
      (e = hipMemsetAsync(c->d_scene, 0, B * np * 16 * sizeof(double), c->stream)) != hipSuccess ||
      (e = hipMemsetAsync(c->d_recs, 0, B * nu * sizeof(UnitRec), c->stream)) != hipSuccess ||
      (e = hipMemsetAsync(c->d_results, 0, B * sizeof(thip_check_result), c->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(c->stream)) != hipSuccess)
    return reject.hip("hipMemcpy", e);
  *out = c.release();
  return THIP_OK;
}

int thip_check_upload(thip_check* chk, const double* scene)
{
  return chk ? upload_scene(chk, chk->d_scene, chk->pr.n_prims, scene, hipMemcpyHostToDevice, "thip_check_upload")
             : THIP_E_INVALID;
}

int thip_check_upload_device(thip_check* chk, const double* d_scene)
{
  return chk ? upload_scene(chk, chk->d_scene, chk->pr.n_prims, d_scene, hipMemcpyDeviceToDevice,
                            "thip_check_upload_device")
             : THIP_E_INVALID;
}

int thip_check_units(const thip_check* chk) { return chk ? chk->pr.n_units : THIP_E_INVALID; }

int thip_check_run(thip_check* chk, const double* x, thip_check_result* results, double* unit_min)
{
  return run(chk, true, x, results, unit_min);
}

int thip_check_run_device(thip_check* chk, const double* d_x, thip_check_result* results, double* unit_min)
{
  return run(chk, false, d_x, results, unit_min);
}

double thip_check_last_ms(thip_check* chk) { return chk ? chk->last_ms : -1.0; }

void thip_check_destroy(thip_check* chk)
{
  if (!chk)
    return;
  release(*chk);
  delete chk;
}

const char* thip_check_last_error(thip_check* chk) { return chk ? chk->err.c_str() : g_check_create_err.c_str(); }

}  // extern "C"
