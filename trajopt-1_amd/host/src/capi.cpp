// C entry points of the host front door (include/trajopt_host.h).
#include "trajopt_host.h"

#include <algorithm>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "trajopt_amd/batch_sqp.hpp"
#include "trajopt_amd/term_evaluator.hpp"

namespace
{
thread_local long long g_batch_qp_launches = 0, g_batch_qp_solves = 0;

void setErr(char* err, int err_len, const std::string& msg)
{
  if (!err || err_len <= 0)
    return;
  const std::size_t n = std::min<std::size_t>(msg.size(), static_cast<std::size_t>(err_len - 1));
  std::memcpy(err, msg.data(), n);
  err[n] = '\0';
}

trajopt::TrajOptProb::Ptr construct(const char* json_text, const double* scene, int n_prims)
{
  if (!json_text)
    throw std::runtime_error("null json text");
  if (n_prims < 0 || (n_prims > 0 && !scene))
    throw std::runtime_error("bad scene");
  const Json::Value root = Json::parse(json_text);
  std::string manip;
  if (root.isMember("basic_info") && root["basic_info"].isMember("manip"))
    json_marshal::childFromJson(root["basic_info"], manip, "manip");
  // the built-in environment of the group (the PR2, or spherebot for "manipulator"),
  // then the caller's primitives after the environment's own
  auto env = trajopt::Environment::builtin(manip);
  for (int p = 0; p < n_prims; ++p)
  {
    std::array<double, 16> rec{};
    std::copy(scene + 16 * p, scene + 16 * (p + 1), rec.begin());
    env->addSceneObject("scene_" + std::to_string(p), rec);  // the caller's primitive p
  }
  return trajopt::ConstructProblem(root, env);
}
}  // namespace

extern "C" {

int thost_lower_json(const char* json_text, const double* scene, int n_prims, thip_problem_desc* desc, double* init,
                     double* cart_targets, double* jpos_targets, double* scene_out, char* err, int err_len)
{
  try
  {
    auto prob = construct(json_text, scene, n_prims);
    if (desc)
      *desc = prob->desc();
    if (init)  // the joint columns
    {
      const trajopt::LoweredProblem lp = prob->lowered();
      std::copy(lp.init.begin(), lp.init.end(), init);
    }
    if (cart_targets)
      std::copy(prob->cart_targets.begin(), prob->cart_targets.end(), cart_targets);
    if (jpos_targets)
      std::copy(prob->jpos_targets.begin(), prob->jpos_targets.end(), jpos_targets);
    if (scene_out)
      std::copy(prob->scene.begin(), prob->scene.end(), scene_out);
    setErr(err, err_len, "");
    return 0;
  }
  catch (const std::exception& e)
  {
    setErr(err, err_len, e.what());
    return -1;
  }
}

int thost_check_json_batch(const char* const* json_texts, int batch, const double* scenes, int n_prims,
                           const double* trajectories, const thip_check_config* config, int device,
                           thip_check_result* results, char* err, int err_len)
{
  try
  {
    if (!json_texts || batch <= 0 || !trajectories || !config || !results)
      throw std::runtime_error("thost_check_json_batch: null argument or batch <= 0");
    // the C-ABI config back to the front door's (type: the coll_continuous encoding)
    trajopt::CollisionCheckConfig cc;
    if (config->type < 0 || config->type > 2)
      throw std::runtime_error("thost_check_json_batch: bad type " + std::to_string(config->type));
    cc.type = config->type == 2   ? trajopt::CollisionEvaluatorType::DISCRETE
              : config->type == 0 ? trajopt::CollisionEvaluatorType::LVS_DISCRETE
                                  : trajopt::CollisionEvaluatorType::LVS_CONTINUOUS;
    cc.longest_valid_segment_length = config->lvs;
    cc.contact_margin = config->margin;
    cc.first_step = config->first_step;
    cc.last_step = config->last_step;
    std::vector<trajopt::TrajOptProb::Ptr> probs;
    std::vector<trajopt::TrajArray> trajs;
    const double* x = trajectories;
    for (int b = 0; b < batch; ++b)
    {
      probs.push_back(construct(json_texts[b], scenes ? scenes + static_cast<std::size_t>(b) * n_prims * 16 : nullptr,
                                n_prims));
      const int N = probs.back()->GetNumSteps(), D = probs.back()->GetNumDOF();
      trajopt::TrajArray t(static_cast<std::size_t>(N));
      for (auto& row : t)
      {
        row.assign(x, x + D);
        x += D;
      }
      trajs.push_back(std::move(t));
    }
    const auto rep = trajopt::checkTrajectory(probs, trajs, cc, device);
    for (int b = 0; b < batch; ++b)
    {
      const trajopt::TrajectoryCheckReport& r = rep[static_cast<std::size_t>(b)];
      thip_check_result o;
      std::memset(&o, 0, sizeof(o));
      o.found = r.found ? 1 : 0;
      o.n_contacts = r.n_contacts;
      o.first_unit = r.first_step;
      o.n_candidates = r.n_candidates;
      o.min_distance = r.min_distance;
      o.min_t = r.min_step;
      o.min_link = r.min_link;
      o.min_other = r.min_other;
      o.min_sphere = r.min_sphere;
      o.min_substate = r.min_substate;
      o.min_cc_time = r.min_cc_time;
      results[b] = o;
    }
    setErr(err, err_len, "");
    return 0;
  }
  catch (const std::exception& e)
  {
    setErr(err, err_len, e.what());
    return -1;
  }
}

int thost_eval_json_batch(const char* const* json_texts, int batch, const double* scenes, int n_prims,
                          const double* trajectories, int route, int device, int* n_costs, int* n_cnts,
                          double* cost_vals, double* cnt_viols, char* names, int names_len, int* slot_map, char* err,
                          int err_len)
{
  try
  {
    if (!json_texts || batch <= 0 || route < THOST_EVAL_DEVICE || route > THOST_EVAL_NAMES)
      throw std::runtime_error("thost_eval_json_batch: null argument, batch <= 0 or bad route");
    if (route != THOST_EVAL_NAMES && !trajectories)
      throw std::runtime_error("thost_eval_json_batch: null trajectories");
    std::vector<trajopt::TrajOptProb::Ptr> probs;
    std::vector<trajopt::TrajArray> trajs;
    const double* x = trajectories;
    for (int b = 0; b < batch; ++b)
    {
      probs.push_back(construct(json_texts[b], scenes ? scenes + static_cast<std::size_t>(b) * n_prims * 16 : nullptr,
                                n_prims));
      probs.back()->device = device;
      const int N = probs.back()->GetNumSteps(), D = probs.back()->GetNumDOF();
      trajopt::TrajArray t(static_cast<std::size_t>(N));
      for (auto& row : t)
      {
        if (x)
        {
          row.assign(x, x + D);
          x += D;
        }
      }
      trajs.push_back(std::move(t));
    }
    // the slot map of problem 0 (no device call): counts, names, order
    if (!probs[0]->lowerable())
      throw std::runtime_error("thost_eval_json_batch: the batched kernels do not take this problem (" +
                               trajopt::whyNotLowerable(*probs[0]) +
                               "): evaluate it on the host loop (Cost::value / Constraint::violation)");
    int nc = 0, nv = 0;
    const std::vector<thip_term_slot> table = trajopt::termSlotTable(probs[0]->desc(), nc, nv);
    const trajopt::TermSlotMap map = trajopt::termSlotMap(*probs[0], table, nc, nv);
    if (n_costs)
      *n_costs = nc;
    if (n_cnts)
      *n_cnts = nv;
    if (slot_map)
    {
      std::copy(map.cost_pos.begin(), map.cost_pos.end(), slot_map);
      std::copy(map.cnt_pos.begin(), map.cnt_pos.end(), slot_map + nc);
    }
    if (names)
    {
      std::string all;
      for (const auto& n : map.cost_names)
        all += n + "\n";
      for (const auto& n : map.cnt_names)
        all += n + "\n";
      if (static_cast<int>(all.size()) + 1 > names_len)
        throw std::runtime_error("thost_eval_json_batch: names need " + std::to_string(all.size() + 1) + " bytes");
      std::memcpy(names, all.c_str(), all.size() + 1);
    }
    if (route == THOST_EVAL_NAMES)
    {
      setErr(err, err_len, "");
      return 0;
    }
    if ((nc > 0 && !cost_vals) || (nv > 0 && !cnt_viols))
      throw std::runtime_error("thost_eval_json_batch: null cost_vals / cnt_viols");
    if (route == THOST_EVAL_DEVICE)
    {
      trajopt::TermEvaluator ev(probs, device);
      const auto res = ev.evaluate(trajs);
      for (int b = 0; b < batch; ++b)
      {
        const auto& r = res[static_cast<std::size_t>(b)];
        std::copy(r.cost_vals.begin(), r.cost_vals.end(), cost_vals + static_cast<std::size_t>(b) * nc);
        std::copy(r.cnt_viols.begin(), r.cnt_viols.end(), cnt_viols + static_cast<std::size_t>(b) * nv);
      }
    }
    else
    {
      for (int b = 0; b < batch; ++b)
      {
        auto& p = *probs[static_cast<std::size_t>(b)];
        const trajopt::DblVec xb = trajopt::trajToDblVec(trajs[static_cast<std::size_t>(b)]);
        p.prefetch(xb);
        const auto& costs = p.getCosts();
        const auto cnts = p.getConstraints();
        if (static_cast<int>(costs.size()) != nc || static_cast<int>(cnts.size()) != nv)
          throw std::runtime_error("thost_eval_json_batch: problem " + std::to_string(b) +
                                   " does not share problem 0's terms");
        for (int i = 0; i < nc; ++i)
          cost_vals[static_cast<std::size_t>(b) * nc + i] = costs[static_cast<std::size_t>(i)]->value(xb);
        for (int i = 0; i < nv; ++i)
          cnt_viols[static_cast<std::size_t>(b) * nv + i] = cnts[static_cast<std::size_t>(i)]->violation(xb);
      }
    }
    setErr(err, err_len, "");
    return 0;
  }
  catch (const std::exception& e)
  {
    setErr(err, err_len, e.what());
    return -1;
  }
}

int thost_solve_json(const char* json_text, const double* scene, int n_prims, int device, double* x,
                     thip_result* result, int* native, char* err, int err_len)
{
  try
  {
    if (!x)
      throw std::runtime_error("thost_solve_json: null x");
    auto prob = construct(json_text, scene, n_prims);
    const bool lowered = prob->lowerable();
    trajopt::BasicTrustRegionSQP opt(prob, device);
    opt.initialize(trajopt::trajToDblVec(prob->GetInitTraj()));
    opt.optimize();
    const sco::OptResults& r = opt.results();
    std::copy(r.x.begin(), r.x.end(), x);
    if (result)
    {
      std::memset(result, 0, sizeof(*result));
      result->status = static_cast<int>(r.status);
      result->n_sqp_iters = r.n_sqp_iters;
      result->n_qp_solves = r.n_qp_solves;
      result->n_func_evals = r.n_func_evals;
      result->n_admm_iters = r.n_admm_iters;
      result->total_cost = r.total_cost;
      result->max_cnt_viol = r.max_cnt_viol;
      result->flags = r.flags;
    }
    if (native)
      *native = lowered ? 1 : 0;
    setErr(err, err_len, "");
    return 0;
  }
  catch (const std::exception& e)
  {
    setErr(err, err_len, e.what());
    return -1;
  }
}

void thost_last_batch_qp_stats(long long* launches, long long* qps)
{
  if (launches)
    *launches = g_batch_qp_launches;
  if (qps)
    *qps = g_batch_qp_solves;
}

void thost_set_host_loop_workers(int n) { trajopt::BatchTrustRegionSQP::setDefaultHostLoopWorkers(n); }

int thost_solve_json_batch(const char* const* json_texts, int batch, const double* scenes, int n_prims, int device,
                           double* x, thip_result* results, char* err, int err_len)
{
  return thost_solve_json_batch_multi(json_texts, batch, scenes, n_prims, &device, 1, x, results, err, err_len);
}

namespace
{
void toResult(const sco::OptResults& r, thip_result& o)
{
  std::memset(&o, 0, sizeof(o));
  o.status = static_cast<int>(r.status);
  o.n_sqp_iters = r.n_sqp_iters;
  o.n_qp_solves = r.n_qp_solves;
  o.n_func_evals = r.n_func_evals;
  o.n_admm_iters = r.n_admm_iters;
  o.total_cost = r.total_cost;
  o.max_cnt_viol = r.max_cnt_viol;
  o.flags = r.flags;
}
}  // namespace

int thost_solve_json_batch_terms(const char* const* json_texts, int batch, const double* scenes, int n_prims,
                                 int device, int drop_in, double* x, thip_result* results, int* sizes,
                                 double* cost_vals, int cap_costs, double* cnt_viols, int cap_cnts, char* err,
                                 int err_len)
{
  try
  {
    if (!json_texts || batch <= 0 || !x || !sizes || cap_costs < 0 || cap_cnts < 0 || (cap_costs > 0 && !cost_vals) ||
        (cap_cnts > 0 && !cnt_viols))
      throw std::runtime_error("thost_solve_json_batch_terms: bad arguments");
    std::vector<trajopt::TrajOptProb::Ptr> probs;
    for (int b = 0; b < batch; ++b)
      probs.push_back(construct(json_texts[b], scenes ? scenes + static_cast<std::size_t>(b) * n_prims * 16 : nullptr,
                                n_prims));
    std::vector<sco::OptResults> res;
    if (drop_in)
      for (const auto& p : probs)
      {
        trajopt::BasicTrustRegionSQP opt(p, device);
        opt.initialize(trajopt::trajToDblVec(p->GetInitTraj()));
        opt.optimize();
        res.push_back(opt.results());
      }
    else
      res = trajopt::BatchTrustRegionSQP(probs, device).optimize();
    sizes[0] = static_cast<int>(res[0].cost_vals.size());
    sizes[1] = static_cast<int>(res[0].cnt_viols.size());
    for (std::size_t b = 0; b < res.size(); ++b)
    {
      const auto& r = res[b];
      if (static_cast<int>(r.cost_vals.size()) > cap_costs || static_cast<int>(r.cnt_viols.size()) > cap_cnts)
        throw std::runtime_error("thost_solve_json_batch_terms: problem " + std::to_string(b) + " has " +
                                 std::to_string(r.cost_vals.size()) + " cost values and " +
                                 std::to_string(r.cnt_viols.size()) + " violations");
      std::copy(r.x.begin(), r.x.end(), x + b * r.x.size());
      std::copy(r.cost_vals.begin(), r.cost_vals.end(), cost_vals + b * static_cast<std::size_t>(cap_costs));
      std::copy(r.cnt_viols.begin(), r.cnt_viols.end(), cnt_viols + b * static_cast<std::size_t>(cap_cnts));
      if (results)
        toResult(r, results[b]);
    }
    setErr(err, err_len, "");
    return 0;
  }
  catch (const std::exception& e)
  {
    setErr(err, err_len, e.what());
    return -1;
  }
}

int thost_solve_json_stream(const char* const* json_texts, int n_batches, int batch, const double* scenes, int n_prims,
                            const int* devices, int n_devices, int inflight, double* x, thip_result* results, char* err,
                            int err_len)
{
  try
  {
    if (!json_texts || n_batches <= 0 || batch <= 0 || !x || !devices || n_devices <= 0)
      throw std::runtime_error("thost_solve_json_stream: bad arguments");
    std::vector<std::vector<trajopt::TrajOptProb::Ptr>> batches(static_cast<std::size_t>(n_batches));
    for (int j = 0; j < n_batches; ++j)
      for (int b = 0; b < batch; ++b)
      {
        const std::size_t i = static_cast<std::size_t>(j) * batch + b;
        batches[static_cast<std::size_t>(j)].push_back(
            construct(json_texts[i], scenes ? scenes + i * static_cast<std::size_t>(n_prims) * 16 : nullptr, n_prims));
      }
    const auto res = trajopt::MultiDeviceBatchSQP::optimizeStream(
        batches, std::vector<int>(devices, devices + n_devices), inflight);
    std::size_t i = 0;
    for (const auto& rb : res)
      for (const auto& r : rb)
      {
        std::copy(r.x.begin(), r.x.end(), x + i * r.x.size());
        if (results)
          toResult(r, results[i]);
        ++i;
      }
    setErr(err, err_len, "");
    return 0;
  }
  catch (const std::exception& e)
  {
    setErr(err, err_len, e.what());
    return -1;
  }
}

int thost_solve_json_batch_multi(const char* const* json_texts, int batch, const double* scenes, int n_prims,
                                 const int* devices, int n_devices, double* x, thip_result* results, char* err,
                                 int err_len)
{
  try
  {
    if (!json_texts || batch <= 0 || !x)
      throw std::runtime_error("thost_solve_json_batch: bad arguments");
    if (!devices || n_devices <= 0)
      throw std::runtime_error("thost_solve_json_batch_multi: no devices");
    std::vector<trajopt::TrajOptProb::Ptr> probs;
    for (int b = 0; b < batch; ++b)
      probs.push_back(construct(json_texts[b], scenes ? scenes + static_cast<std::size_t>(b) * n_prims * 16 : nullptr,
                                n_prims));
    trajopt::MultiDeviceBatchSQP opt(probs, std::vector<int>(devices, devices + n_devices));
    const auto res = opt.optimize();
    g_batch_qp_launches = opt.qpLaunches();
    g_batch_qp_solves = opt.qpSolves();
    for (int b = 0; b < batch; ++b)
    {
      const auto& r = res[static_cast<std::size_t>(b)];
      std::copy(r.x.begin(), r.x.end(), x + static_cast<std::size_t>(b) * r.x.size());
      if (results)
      {
        thip_result& o = results[b];
        std::memset(&o, 0, sizeof(o));
        o.status = static_cast<int>(r.status);
        o.n_sqp_iters = r.n_sqp_iters;
        o.n_qp_solves = r.n_qp_solves;
        o.n_func_evals = r.n_func_evals;
        o.n_admm_iters = r.n_admm_iters;
        o.total_cost = r.total_cost;
        o.max_cnt_viol = r.max_cnt_viol;
        o.flags = r.flags;
      }
    }
    setErr(err, err_len, "");
    return 0;
  }
  catch (const std::exception& e)
  {
    setErr(err, err_len, e.what());
    return -1;
  }
}

struct thost_batch
{
  std::unique_ptr<trajopt::BatchTrustRegionSQP> solver;
  bool solved = false;
};

int thost_batch_create(const char* const* json_texts, int batch, const double* scenes, int n_prims, int device,
                       thost_batch** out, char* err, int err_len)
{
  try
  {
    if (!json_texts || batch <= 0 || !out)
      throw std::runtime_error("thost_batch_create: bad arguments");
    std::vector<trajopt::TrajOptProb::Ptr> probs;
    for (int b = 0; b < batch; ++b)
      probs.push_back(construct(json_texts[b], scenes ? scenes + static_cast<std::size_t>(b) * n_prims * 16 : nullptr,
                                n_prims));
    auto h = std::make_unique<thost_batch>();
    h->solver = std::make_unique<trajopt::BatchTrustRegionSQP>(probs, device);
    h->solver->setHostLoopWorkers(batch);  // every problem's loop at once: each QP round is one launch per pattern
    *out = h.release();
    setErr(err, err_len, "");
    return 0;
  }
  catch (const std::exception& e)
  {
    setErr(err, err_len, e.what());
    return -1;
  }
}

int thost_batch_solve(thost_batch* h, double* x, thip_result* results, char* err, int err_len)
{
  try
  {
    if (!h || !x)
      throw std::runtime_error("thost_batch_solve: bad arguments");
    if (h->solved && h->solver->hostLoops())
      throw std::runtime_error("thost_batch_solve: a host-loop batch is solved once (its models keep their warm starts)");
    const auto res = h->solver->optimize();
    h->solved = true;
    for (std::size_t b = 0; b < res.size(); ++b)
    {
      const auto& r = res[b];
      std::copy(r.x.begin(), r.x.end(), x + b * r.x.size());
      if (results)
        toResult(r, results[b]);
    }
    setErr(err, err_len, "");
    return 0;
  }
  catch (const std::exception& e)
  {
    setErr(err, err_len, e.what());
    return -1;
  }
}

int thost_batch_stats(const thost_batch* h, int* host_loops, long long* qp_launches, long long* qps, double* qp_bytes,
                      double* qp_seconds)
{
  if (!h)
    return -1;
  if (host_loops)
    *host_loops = h->solver->hostLoops() ? 1 : 0;
  if (qp_launches)
    *qp_launches = h->solver->qpLaunches();
  if (qps)
    *qps = h->solver->qpSolves();
  if (qp_bytes)
    *qp_bytes = h->solver->qpBytes();
  if (qp_seconds)
    *qp_seconds = h->solver->qpLaunchSeconds();
  return 0;
}

int thost_batch_qp_shape(const thost_batch* h, long long* out)
{
  if (!h || !h->solver || !out)
    return -1;
  out[0] = h->solver->qpAdmmIters();
  std::copy(h->solver->qpMaxShape(), h->solver->qpMaxShape() + 6, out + 1);
  return 0;
}

void thost_batch_destroy(thost_batch* h) { delete h; }
}
