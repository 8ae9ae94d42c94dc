// What the discrete (coll_sets.hip) and the continuous (coll_sets_cont.hip)
// collision sets share: the robot model, the key packing and the row order, the
// validation of thip_*_create, and the handle's buffers with their allocation
// and fetch; the life cycle itself (stream, events, upload, the start of a run,
// the timed launch, release) is device_handle.hpp's, as for every handle.  Both
// kernels rest on one invariant: unique keys (check_pairs)
// under a strict total order (pack_key, before) and no atomics, so a problem's
// rows do not depend on its place in the batch and every run gives the same
// bits.  The kernels' prologue and selection step (compaction, ranking) stay
// written out in each kernel: as shared inline functions they compiled to
// other code, and ccsets_kernel measured 1.3 % slower.
// Both .hip files are linked into one library: everything here is inline, a
// template or a plain struct.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "desc_lowering.hpp"
#include "device_handle.hpp"
#include "kin_device.hpp"

namespace thip
{
namespace sets
{
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxRows = THIP_CSETS_MAX_ROWS;
constexpr int kLdsPrims = THIP_MAX_PRIMS;  // scenes up to this size are staged in LDS

struct Model
{
  int n_sph, n_self_sph;
  double center[THIP_MAX_SPHERES][3];
  double radius[THIP_MAX_SPHERES];
  int link[THIP_MAX_SPHERES];
  int active[THIP_MAX_LINKS];  // a joint moves the link (getGradient's has_gradient / isActiveLinkId)
  int self_sa[THIP_MAX_SELF_SPHERE_PAIRS];
  int self_sb[THIP_MAX_SELF_SPHERE_PAIRS];
};

// (link, other, sphere, other_sphere) packed so that unsigned order is the
// tuple's ascending order: link < 32, other in [-32, 1024), sphere < 32,
// other_sphere in [-1, 32)
static_assert(THIP_MAX_LINKS <= 32 && THIP_MAX_SPHERES <= 32 && THIP_EVAL_MAX_PRIMS + 32 <= 2048, "key packing");
__device__ __forceinline__ unsigned pack_key(int link, int other, int sphere, int osphere)
{
  return (static_cast<unsigned>(link) << 22) | (static_cast<unsigned>(other + 32) << 11) |
         (static_cast<unsigned>(sphere) << 6) | static_cast<unsigned>(osphere + 1);
}
__device__ __forceinline__ void unpack_key(unsigned k, int& link, int& other, int& sphere, int& osphere)
{
  link = static_cast<int>(k >> 22);
  other = static_cast<int>((k >> 11) & 2047u) - 32;
  sphere = static_cast<int>((k >> 6) & 31u);
  osphere = static_cast<int>(k & 63u) - 1;
}

// row order: error (the continuous sets' E) descending, then the key ascending
__device__ __forceinline__ bool before(double e, unsigned k, double oe, unsigned ok)
{
  return e > oe || (e == oe && k < ok);
}

__device__ __forceinline__ void sphere_world(const Pose& T, const double* cl, double* c)
{
  for (int r = 0; r < 3; ++r)
    c[r] = T.r[r * 3 + 0] * cl[0] + T.r[r * 3 + 1] * cl[1] + T.r[r * 3 + 2] * cl[2] + T.t[r];
}

// ---------------------------------------------------------------- host side
// thip_*_create's checks of the descriptor and of the config fields both kinds
// of set have (Cfg: thip_csets_config or thip_ccsets_config).  THIP_OK, or
// what reject returned for the first finding.
template <class Cfg>
inline int check_descriptor(const thip_problem_desc& desc, const Cfg& cfg, const host::CreateError& reject)
{
  {
    const std::string why = lowering::abi_mismatch(desc);
    if (!why.empty())
      return reject(why);
  }
  const thip_chain& ch = desc.chain;
  if (const char* why = lowering::chain_range_finding(ch))
    return reject(why);
  if (const char* why = lowering::chain_table_finding(ch))
    return reject(why);
  if (desc.n_steps < 1 || desc.n_steps > THIP_EVAL_MAX_STEPS)
    return reject("n_steps out of range");
  if (desc.n_prims < 0 || desc.n_prims > THIP_EVAL_MAX_PRIMS)
    return reject("n_prims out of range");
  if (desc.n_spheres == 0)
    return reject("the descriptor has no robot spheres: collision sets need the robot's sphere model "
                  "(n_spheres / sphere_link / sphere_center / sphere_radius)");
  if (desc.n_spheres < 0 || desc.n_spheres > THIP_MAX_SPHERES)
    return reject("n_spheres out of range");
  for (int s = 0; s < desc.n_spheres; ++s)
  {
    if (desc.sphere_link[s] < 1 || desc.sphere_link[s] >= ch.n_links)
      return reject("bad sphere link of robot sphere " + std::to_string(s));
    if (!(desc.sphere_radius[s] >= 0) || !std::isfinite(desc.sphere_radius[s]))
      return reject("bad sphere radius of robot sphere " + std::to_string(s));
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(desc.sphere_center[s][i]))
        return reject("bad sphere center of robot sphere " + std::to_string(s));
  }
  if (!std::isfinite(cfg.margin))
    return reject("margin is not finite");
  if (!std::isfinite(cfg.coeff))
    return reject("coeff is not finite");
  if (!std::isfinite(cfg.margin_buffer))
    return reject("margin_buffer is not finite");
  if (cfg.max_num_cnt < 1 || cfg.max_num_cnt > THIP_CSETS_MAX_ROWS)
    return reject("max_num_cnt " + std::to_string(cfg.max_num_cnt) + " out of range [1, " +
                  std::to_string(THIP_CSETS_MAX_ROWS) + "]");
  return THIP_OK;
}

// The checks that follow each file's own (step range, grid, ...): term 0's
// pair overrides and the self pairs.  Fills the self sphere pairs (ssa, ssb)
// and tab, term 0's overrides over margin and coeff (pair_data.hpp).
inline int check_pairs(const thip_problem_desc& desc, double margin, double coeff, const host::CreateError& reject,
                       std::vector<int>& ssa, std::vector<int>& ssb, std::vector<double>& tab)
{
  if (desc.n_coll_pairs < 0 || desc.n_coll_pairs > THIP_MAX_COLL_PAIRS)
    return reject("n_coll_pairs out of range");
  for (int k = 0; k < desc.n_coll_pairs; ++k)
  {
    const thip_coll_pair& e = desc.coll_pairs[k];
    if (e.term != 0)
      continue;  // another term's override: not read
    if (e.link < 0 || e.link >= desc.chain.n_links)
      return reject("coll_pairs[" + std::to_string(k) + "].link out of range");
    if (e.other >= 0 ? e.other >= desc.n_prims : (e.other < -desc.chain.n_links))
      return reject("coll_pairs[" + std::to_string(k) + "].other out of range");
    if (!std::isfinite(e.margin) || !std::isfinite(e.coeff))
      return reject("coll_pairs[" + std::to_string(k) + "] margin / coeff must be finite");
  }
  std::vector<int> skp;
  const std::string why = thip::self_sphere_pairs(desc, ssa, ssb, skp);
  if (!why.empty())
    return reject(why);
  // the selection needs unique keys: a link pair listed twice, in either
  // order, would put the same contacts into the pool twice
  for (int k = 1; k < desc.n_self_pairs; ++k)
    for (int o = 0; o < k; ++o)
    {
      const int a = desc.self_pair[k][0], b = desc.self_pair[k][1];
      const int oa = desc.self_pair[o][0], ob = desc.self_pair[o][1];
      if ((a == oa && b == ob) || (a == ob && b == oa))
        return reject("self_pair[" + std::to_string(k) + "] repeats self_pair[" + std::to_string(o) +
                      "]: each link pair may be listed once");
    }
  std::unique_ptr<thip_problem_desc> d2(new thip_problem_desc(desc));
  d2->coll_enabled = 1;
  d2->coll_margin = margin;
  d2->coll_coeff = coeff;
  d2->n_coll_pairs = 0;
  for (int k = 0; k < desc.n_coll_pairs; ++k)
    if (desc.coll_pairs[k].term == 0)
      d2->coll_pairs[d2->n_coll_pairs++] = desc.coll_pairs[k];
  thip::coll_pair_table(*d2, 0, tab);
  return THIP_OK;
}

// The device's chain (a serial chain gets its parent table) and robot model of
// a checked descriptor.
inline void fill_model(const thip_problem_desc& desc, const std::vector<int>& ssa, const std::vector<int>& ssb,
                       thip_chain& chain, Model& md)
{
  chain = desc.chain;
  lowering::fill_serial_parents(chain);
  md = Model();
  lowering::fill_sphere_model(desc, ssa, ssb, md);
  std::copy(desc.sphere_link, desc.sphere_link + desc.n_spheres, md.link);
  for (int k = 1; k < chain.n_links; ++k)
    md.active[k] = (chain.joint_type[k] != THIP_JOINT_FIXED || md.active[chain.parent[k]]) ? 1 : 0;
}

// What struct thip_csets and struct thip_ccsets are made of, over the base every
// handle has (device_handle.hpp).  items: the launch's workgroups (batch x nodes
// or segments), rows: items x max_num_cnt, jac_width: D or 2 D.
struct Handle : host::Handle
{
  int D = 0, N = 0, n_prims = 0;
  size_t items = 0, rows = 0, jac_width = 0;
  thip_chain* d_chain = nullptr;
  Model* d_model = nullptr;
  double* d_pmc = nullptr;
  double* d_scene = nullptr;
  double* d_x = nullptr;  // staging of host trajectories
  double* d_values = nullptr;
  double* d_jac = nullptr;
  double* d_coeffs = nullptr;
  int* d_counts = nullptr;
  int* d_keys = nullptr;
};

// A new handle's sizes, buffers, stream and events; chain, model and pair table
// uploaded, the scene zeroed.  THIP_OK, or what bad.hip worded; the handle is
// released by its owner then.
inline int allocate_and_upload(Handle& h, int device, int batch, const thip_problem_desc& desc, size_t items, int R,
                               size_t jac_width, const thip_chain& chain, const Model& md,
                               const std::vector<double>& tab, const host::CreateError& bad)
{
  h.device = device;
  h.batch = batch;
  h.D = desc.chain.n_dof;
  h.N = desc.n_steps;
  h.n_prims = desc.n_prims;
  h.items = items;
  h.rows = items * static_cast<size_t>(R);
  h.jac_width = jac_width;
  hipError_t e;
  if ((e = hipSetDevice(h.device)) != hipSuccess)
    return bad.hip("hipSetDevice", e);
  const size_t B = static_cast<size_t>(h.batch), np = static_cast<size_t>(std::max(h.n_prims, 1));
  if ((e = host::alloc(h, h.d_chain, 1)) != hipSuccess || (e = host::alloc(h, h.d_model, 1)) != hipSuccess ||
      (e = host::alloc(h, h.d_scene, B * np * 16)) != hipSuccess ||
      (e = host::alloc(h, h.d_x, B * static_cast<size_t>(h.N) * h.D)) != hipSuccess ||
      (e = host::alloc(h, h.d_values, h.rows)) != hipSuccess ||
      (e = host::alloc(h, h.d_jac, h.rows * h.jac_width)) != hipSuccess ||
      (e = host::alloc(h, h.d_coeffs, h.rows)) != hipSuccess || (e = host::alloc(h, h.d_counts, h.items)) != hipSuccess ||
      (e = host::alloc(h, h.d_keys, h.rows * 4)) != hipSuccess ||
      (!tab.empty() && (e = host::alloc(h, h.d_pmc, tab.size())) != hipSuccess))
    return bad.hip("hipMalloc", e);
  if ((e = host::open_stream(h)) != hipSuccess)
    return bad.hip("hipStreamCreate", e);
  if ((e = host::open_events(h)) != hipSuccess)
    return bad.hip("hipEventCreate", e);
  if ((e = hipMemcpyAsync(h.d_chain, &chain, sizeof(thip_chain), hipMemcpyHostToDevice, h.stream)) != hipSuccess ||
      (e = hipMemcpyAsync(h.d_model, &md, sizeof(Model), hipMemcpyHostToDevice, h.stream)) != hipSuccess ||
      (!tab.empty() && (e = hipMemcpyAsync(h.d_pmc, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice,
                                           h.stream)) != hipSuccess) ||
      (e = hipMemsetAsync(h.d_scene, 0, B * np * 16 * sizeof(double), h.stream)) != hipSuccess ||
      (e = hipStreamSynchronize(h.stream)) != hipSuccess)
    return bad.hip("hipMemcpy", e);
  return THIP_OK;
}

// thip_*_upload / thip_*_upload_device (`who`)
inline int upload_scene(Handle* h, const double* scene, hipMemcpyKind kind, const char* who)
{
  return h ? host::upload_scene(h, h->d_scene, h->n_prims, scene, kind, who) : THIP_E_INVALID;
}

// The start of <api>_run and of <api>_run_device; api: "thip_csets" or "thip_ccsets"
inline int stage_x(Handle* h, const char* api, const double* x, bool on_host, const double*& d_x)
{
  if (!h)
    return THIP_E_INVALID;
  return host::stage_x(h, api, on_host, x, true, "", h->d_x,
                       static_cast<size_t>(h->batch) * static_cast<size_t>(h->N) * h->D, d_x);
}

// launch() between the two events, then the results to the host (a null
// destination is skipped), the stream drained and the kernel's time taken.
template <class Launch>
inline int launch_and_fetch(Handle* h, const char* kernel, Launch launch, double* values, double* jac, double* coeffs,
                            int* counts, int* keys)
{
  auto run = [&] {
    launch();
    return host::launched(h, kernel);
  };
  auto fetch = [&] {
    hipError_t e;
    if ((e = host::to_host(h, values, h->d_values, h->rows * sizeof(double))) != hipSuccess ||
        (e = host::to_host(h, jac, h->d_jac, h->rows * h->jac_width * sizeof(double))) != hipSuccess ||
        (e = host::to_host(h, coeffs, h->d_coeffs, h->rows * sizeof(double))) != hipSuccess ||
        (e = host::to_host(h, counts, h->d_counts, h->items * sizeof(int))) != hipSuccess)
      return e;
    return host::to_host(h, keys, h->d_keys, h->rows * 4 * sizeof(int));
  };
  return host::timed_run(h, kernel, run, fetch);
}
}  // namespace sets
}  // namespace thip
