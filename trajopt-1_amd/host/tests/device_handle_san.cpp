// The seven C-ABI handles' life cycle (csrc/device_handle.hpp) under
// AddressSanitizer + UBSan, with the .hip files' host code compiled in:
//   * every <api>_create on the smallest valid problem (a 1-dof prismatic chain,
//     2 links, one sphere, 4 steps; thip_qp_create: a 2 x 2 pattern).  Without a
//     device it returns THIP_E_HIP, leaves *out null and words
//     "<api>_create: hipSetDevice: <the runtime's text>"; LeakSanitizer's clean
//     exit shows the half-built handle was released.  With a device it succeeds
//     and the handle is destroyed.
//   * every entry point of every handle with a null handle: THIP_E_INVALID (-1
//     from thip_eval_cart_vel_pairs and thip_qp_factor_nnz, a negative last_ms, a
//     null thip_device_x), and a destroy that returns.
// Own main; no kernel is launched; built by `make san`.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>

#include "../../../include/trajopt_hip.h"

namespace
{
int g_fail = 0, g_created = 0, g_refused = 0;

#define CHECK(cond, what)                                               \
  do                                                                    \
  {                                                                     \
    if (!(cond))                                                        \
    {                                                                   \
      std::printf("FAIL %s: %s\n", std::string(what).c_str(), #cond);   \
      g_fail++;                                                         \
    }                                                                   \
  } while (0)

std::unique_ptr<thip_problem_desc> smallest_desc()
{
  std::unique_ptr<thip_problem_desc> p(new thip_problem_desc());
  thip_problem_desc& d = *p;
  d.abi_version = THIP_ABI_VERSION;
  d.n_steps = 4;
  d.chain.n_links = 2;
  d.chain.n_dof = 1;
  d.chain.joint_type[1] = THIP_JOINT_PRISMATIC;
  d.chain.joint_dof[1] = 0;
  d.chain.joint_axis[1][0] = 1.0;
  d.chain.joint_origin[1][0] = d.chain.joint_origin[1][5] = d.chain.joint_origin[1][10] = 1.0;
  d.chain.base_pose[0] = d.chain.base_pose[5] = d.chain.base_pose[10] = 1.0;
  d.chain.lower[0] = -1.0;
  d.chain.upper[0] = 1.0;
  d.jv_enabled = 1;
  d.jv_first_step = 0;
  d.jv_last_step = -1;
  d.jv_coeffs[0] = 1.0;
  d.n_spheres = 1;
  d.sphere_link[0] = 1;
  d.sphere_radius[0] = 0.05;
  thip_default_sqp_params(&d.sqp);
  thip_default_osqp_settings(&d.osqp);
  return p;
}

// what *out holds before a create, which must overwrite it
template <class H>
H* stale()
{
  return reinterpret_cast<H*>(static_cast<uintptr_t>(0x10));
}

// what a create must do here: hipSetDevice(0)'s own outcome says which
template <class H>
void expect_create(const char* api, int rc, H* h, const char* (*last_error)(H*), void (*destroy)(H*))
{
  const hipError_t e = hipSetDevice(0);
  if (e == hipSuccess)
  {
    CHECK(rc == THIP_OK && h != nullptr, std::string(api) + "_create with a device: " + last_error(nullptr));
    if (h && h != stale<H>())
      destroy(h);
    g_created++;
    return;
  }
  const std::string want = std::string(api) + "_create: hipSetDevice: " + hipGetErrorString(e);
  const std::string got = last_error(nullptr);
  CHECK(rc == THIP_E_HIP, std::string(api) + "_create rc " + std::to_string(rc) + ": " + got);
  CHECK(h == nullptr, std::string(api) + "_create left *out set");
  CHECK(got == want, std::string(api) + "_create worded '" + got + "', not '" + want + "'");
  if (h && h != stale<H>())
    destroy(h);
  g_refused++;
}

void creates()
{
  const std::unique_ptr<thip_problem_desc> d = smallest_desc();
  {
    thip_ctx* h = stale<thip_ctx>();
    const int rc = thip_create(0, d.get(), 1, &h);
    expect_create("thip", rc, h, thip_last_error, thip_destroy);
  }
  {
    thip_eval* h = stale<thip_eval>();
    const int rc = thip_eval_create(0, d.get(), 1, &h);
    expect_create("thip_eval", rc, h, thip_eval_last_error, thip_eval_destroy);
  }
  {
    thip_terms* h = stale<thip_terms>();
    const int rc = thip_terms_create(0, d.get(), 1, &h);
    expect_create("thip_terms", rc, h, thip_terms_last_error, thip_terms_destroy);
  }
  {
    thip_check_config cfg;
    thip_default_check_config(&cfg);
    thip_check* h = stale<thip_check>();
    const int rc = thip_check_create(0, d.get(), &cfg, 1, &h);
    expect_create("thip_check", rc, h, thip_check_last_error, thip_check_destroy);
  }
  {
    thip_csets_config cfg;
    thip_default_csets_config(&cfg);
    thip_csets* h = stale<thip_csets>();
    const int rc = thip_csets_create(0, d.get(), &cfg, 1, &h);
    expect_create("thip_csets", rc, h, thip_csets_last_error, thip_csets_destroy);
  }
  {
    thip_ccsets_config cfg;
    thip_default_ccsets_config(&cfg);
    thip_ccsets* h = stale<thip_ccsets>();
    const int rc = thip_ccsets_create(0, d.get(), &cfg, nullptr, 1, &h);
    expect_create("thip_ccsets", rc, h, thip_ccsets_last_error, thip_ccsets_destroy);
  }
  {
    // P = diag(1, 1), A = one row (1, 1)
    const int Pp[3] = { 0, 1, 2 }, Pi[2] = { 0, 1 }, Ap[3] = { 0, 1, 2 }, Ai[2] = { 0, 0 };
    thip_qp* h = stale<thip_qp>();
    const int rc = thip_qp_create(0, 2, 1, Pp, Pi, Ap, Ai, 1, &h);
    expect_create("thip_qp", rc, h, thip_qp_last_error, thip_qp_destroy);
  }
}

void null_handles()
{
  double v[16] = {};
  int n[16] = {};
  long long w[64] = {};
  const std::string what = "null handle";
  // thip_ctx
  CHECK(thip_set_stream(nullptr, nullptr) == THIP_E_INVALID, what);
  CHECK(thip_upload(nullptr, v, v, v) == THIP_E_INVALID, what);
  CHECK(thip_upload_joint_targets(nullptr, v) == THIP_E_INVALID, what);
  CHECK(thip_upload_device(nullptr, v, v, v) == THIP_E_INVALID, what);
  CHECK(thip_sqp_run(nullptr) == THIP_E_INVALID, what);
  CHECK(thip_synchronize(nullptr) == THIP_E_INVALID, what);
  CHECK(thip_linearize(nullptr, v, v, v) == THIP_E_INVALID, what);
  CHECK(thip_fwd_kin(nullptr, v, v) == THIP_E_INVALID, what);
  CHECK(thip_download(nullptr, v, nullptr) == THIP_E_INVALID, what);
  CHECK(thip_device_x(nullptr) == nullptr, what);
  CHECK(thip_last_kernel_ms(nullptr) < 0, what);
  CHECK(thip_debug_trace(nullptr, 1) == THIP_E_INVALID, what);
  CHECK(thip_debug_get_trace(nullptr, v, n) == THIP_E_INVALID, what);
  CHECK(thip_collision_rows(nullptr, v, v, 1, n) == THIP_E_INVALID, what);
  CHECK(thip_debug_profile(nullptr, 1) == THIP_E_INVALID, what);
  CHECK(thip_debug_get_profile(nullptr, w) == THIP_E_INVALID, what);
  CHECK(thip_debug_layout(nullptr, w, w, w) == THIP_E_INVALID, what);
  CHECK(thip_debug_workspace(nullptr, v, n) == THIP_E_INVALID, what);
  CHECK(thip_debug_solve_layout(nullptr, n, 1) == THIP_E_INVALID, what);
  thip_destroy(nullptr);
  // thip_eval
  CHECK(thip_eval_upload(nullptr, v, v) == THIP_E_INVALID, what);
  CHECK(thip_eval_cart_pose(nullptr, 0, v, v, v) == THIP_E_INVALID, what);
  CHECK(thip_eval_cart_pose_all(nullptr, v, v, v) == THIP_E_INVALID, what);
  CHECK(thip_eval_cart_vel_pairs(nullptr) == -1, what);
  CHECK(thip_eval_cart_vel_all(nullptr, v, v, v) == THIP_E_INVALID, what);
  CHECK(thip_eval_collision(nullptr, 0, v, v, 1, n) == THIP_E_INVALID, what);
  thip_eval_destroy(nullptr);
  // thip_terms
  CHECK(thip_terms_counts(nullptr, n, n) == THIP_E_INVALID, what);
  CHECK(thip_terms_slots(nullptr, nullptr) == THIP_E_INVALID, what);
  CHECK(thip_terms_upload(nullptr, v, v) == THIP_E_INVALID, what);
  CHECK(thip_terms_upload_device(nullptr, v, v) == THIP_E_INVALID, what);
  CHECK(thip_terms_upload_joint_targets(nullptr, v) == THIP_E_INVALID, what);
  CHECK(thip_terms_upload_joint_targets_device(nullptr, v) == THIP_E_INVALID, what);
  CHECK(thip_terms_run(nullptr, v, v, v) == THIP_E_INVALID, what);
  CHECK(thip_terms_run_device(nullptr, v, v, v) == THIP_E_INVALID, what);
  CHECK(thip_terms_last_ms(nullptr) < 0, what);
  thip_terms_destroy(nullptr);
  // thip_check
  thip_check_result res;
  CHECK(thip_check_upload(nullptr, v) == THIP_E_INVALID, what);
  CHECK(thip_check_upload_device(nullptr, v) == THIP_E_INVALID, what);
  CHECK(thip_check_units(nullptr) == THIP_E_INVALID, what);
  CHECK(thip_check_run(nullptr, v, &res, v) == THIP_E_INVALID, what);
  CHECK(thip_check_run_device(nullptr, v, &res, v) == THIP_E_INVALID, what);
  CHECK(thip_check_last_ms(nullptr) < 0, what);
  thip_check_destroy(nullptr);
  // thip_csets, thip_ccsets
  CHECK(thip_csets_upload(nullptr, v) == THIP_E_INVALID, what);
  CHECK(thip_csets_upload_device(nullptr, v) == THIP_E_INVALID, what);
  CHECK(thip_csets_nodes(nullptr) == THIP_E_INVALID, what);
  CHECK(thip_csets_run(nullptr, v, v, v, v, n, n) == THIP_E_INVALID, what);
  CHECK(thip_csets_run_device(nullptr, v, v, v, v, n, n) == THIP_E_INVALID, what);
  CHECK(thip_csets_last_ms(nullptr) < 0, what);
  thip_csets_destroy(nullptr);
  CHECK(thip_ccsets_upload(nullptr, v) == THIP_E_INVALID, what);
  CHECK(thip_ccsets_upload_device(nullptr, v) == THIP_E_INVALID, what);
  CHECK(thip_ccsets_segments(nullptr) == THIP_E_INVALID, what);
  CHECK(thip_ccsets_run(nullptr, v, v, v, v, n, n) == THIP_E_INVALID, what);
  CHECK(thip_ccsets_run_device(nullptr, v, v, v, v, n, n) == THIP_E_INVALID, what);
  CHECK(thip_ccsets_last_ms(nullptr) < 0, what);
  thip_ccsets_destroy(nullptr);
  // thip_qp
  thip_qp_info info;
  thip_osqp_settings st;
  thip_default_osqp_settings(&st);
  thip_qp* none = nullptr;
  CHECK(thip_qp_solve(nullptr, v, v, v, v, v, &st, nullptr, nullptr, nullptr, v, v, &info) == THIP_E_INVALID, what);
  CHECK(thip_qp_solve_some(nullptr, 1, v, v, v, v, v, &st, nullptr, nullptr, nullptr, nullptr, v, v, &info) ==
            THIP_E_INVALID,
        what);
  CHECK(thip_qp_submit(nullptr, 1, v, v, v, v, v, &st, nullptr, nullptr, nullptr, nullptr) == THIP_E_INVALID, what);
  CHECK(thip_qp_stage(nullptr, 1, v, v, v, v, v, &st, nullptr, nullptr, nullptr, nullptr) == THIP_E_INVALID, what);
  CHECK(thip_qp_launch_staged(&none, 1) == THIP_E_INVALID, what);
  CHECK(thip_qp_collect(nullptr, v, v, &info) == THIP_E_INVALID, what);
  CHECK(thip_qp_factor_nnz(nullptr) == -1, what);
  CHECK(thip_qp_shape(nullptr, w) == THIP_E_INVALID, what);
  CHECK(thip_qp_setup(nullptr, v, v, v, v, v, &st, &info) == THIP_E_INVALID, what);
  CHECK(thip_qp_update_vec(nullptr, v, v, v, &info) == THIP_E_INVALID, what);
  CHECK(thip_qp_update_mat(nullptr, v, v, &info) == THIP_E_INVALID, what);
  CHECK(thip_qp_warm_start(nullptr, v, v) == THIP_E_INVALID, what);
  CHECK(thip_qp_solve_resident(nullptr, v, v, &info) == THIP_E_INVALID, what);
  thip_qp_destroy(nullptr);
}
}  // namespace

int main()
{
  creates();
  null_handles();
  std::printf("device_handle_san: created=%d refused=%d fail=%d\n", g_created, g_refused, g_fail);
  return g_fail ? 1 : 0;
}
