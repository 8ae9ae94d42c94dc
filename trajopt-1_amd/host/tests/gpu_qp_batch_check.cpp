// GpuQPBatch's rendezvous without a device (its own main; built with
// -fsanitize=thread by `make tsan-qpbatch`).  Eight client threads drive a slot
// each through a fake step function injected at construction; they submit
// different numbers of rounds, on two QP patterns, and leave at different times;
// some clear() their slot on the way, so indices of a group are given back and
// taken again.  Every request carries (client, sequence number) in its gradient,
// and the fake step echoes it in x.  Checked:
//   - when a round runs, every client that has not left is waiting in it;
//   - every request is served exactly once, in order, and gets its own answer;
//   - one step per group and round, within the group's capacity;
//   - it terminates (a watchdog ends the program otherwise).
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

#include "trajopt_sqp/gpu_qp_batch.h"

using trajopt_ifopt::Jacobian;
using trajopt_sqp::GpuQPBatch;

namespace
{
constexpr int kClients = 8;
std::atomic<int> g_failures{ 0 };
#define CHECK(c)                                                         \
  do                                                                     \
  {                                                                      \
    if (!(c))                                                            \
    {                                                                    \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      ++g_failures;                                                      \
    }                                                                    \
  } while (0)

// what the fake device knows; its calls come from inside a round (one thread at a time), the clients' flags are atomics
struct Fake
{
  std::atomic<int> running{ kClients };           // clients that have not left
  std::atomic<bool> waiting[kClients];            // client is inside a submit
  std::atomic<int> served[kClients];              // requests of the client answered so far
  std::map<thip_qp*, std::pair<int, int>> shape;  // handle -> (n, capacity)
  long long steps = 0, creates = 0;
  int next_handle = 1;
};

Jacobian diag(long n, double v)
{
  Jacobian J(n, n);
  for (long r = 0; r < n; ++r)
  {
    J.startVec(r);
    J.insertBack(r, r) = v;
  }
  J.finalize();
  return J;
}

Jacobian row(long n)
{
  Jacobian J(1, n);
  J.startVec(0);
  for (long c = 0; c < n; ++c)
    J.insertBack(0, c) = 1.0;
  J.finalize();
  return J;
}

GpuQPBatch::Device fakeDevice(Fake& f)
{
  GpuQPBatch::Device d;
  d.create = [&f](int, int n, int, const int*, const int*, const int*, const int*, int batch, thip_qp** out) {
    thip_qp* h = reinterpret_cast<thip_qp*>(static_cast<std::uintptr_t>(0x1000 * f.next_handle++));
    f.shape[h] = { n, batch };
    ++f.creates;
    *out = h;
    return THIP_OK;
  };
  d.destroy = [&f](thip_qp* h) { f.shape.erase(h); };
  d.last_error = [](thip_qp*) { return std::string("fake"); };
  d.step = [&f](thip_qp* h, const int* ops, const double*, const double* q, const double*, const double*, const double*,
                const thip_osqp_settings*, const double*, const double*, double* x, double*, thip_qp_info* info) {
    ++f.steps;
    CHECK(f.shape.count(h) == 1);
    const int n = f.shape[h].first, B = f.shape[h].second;
    // a round runs only when every client that has not left is waiting in it
    int waiting = 0;
    for (int c = 0; c < kClients; ++c)
      waiting += f.waiting[c].load() ? 1 : 0;
    CHECK(waiting == f.running.load());
    int selected = 0;
    for (int b = 0; b < B; ++b)
    {
      if (!ops[b])
        continue;
      ++selected;
      // every request of the driver sends its gradient: (client, sequence number)
      CHECK((ops[b] & (THIP_QP_OP_SETUP | THIP_QP_OP_VEC_Q)) != 0);
      const int client = static_cast<int>(q[b * n]), seq = static_cast<int>(q[b * n + 1]);
      CHECK(client >= 0 && client < kClients);
      if (client < 0 || client >= kClients)
        continue;
      CHECK(f.waiting[client].load());
      CHECK(f.served[client].load() == seq);  // not served twice, none skipped
      ++f.served[client];
      info[b] = thip_qp_info{};
      info[b].status = 1;
      info[b].iter = 1;
      if (ops[b] & THIP_QP_OP_SOLVE)
        for (int j = 0; j < n; ++j)
          x[b * n + j] = q[b * n + j];
    }
    CHECK(selected >= 1);
    return THIP_OK;
  };
  return d;
}

void client(int c, Fake& f, const std::shared_ptr<GpuQPBatch>& batch)
{
  const long n = (c % 2) ? 3 : 2;  // two patterns: two groups
  const int rounds = 3 + 2 * c;    // everyone leaves at another time
  auto slot = batch->makeSlot();
  auto load = [&](int seq) {
    slot->updateHessianMatrix(diag(n, 1.0 + seq));
    trajopt_ifopt::VectorXd g(static_cast<std::size_t>(n), 0.5);
    g[0] = c;
    g[1] = seq;
    slot->updateGradient(g);
    slot->updateLinearConstraintsMatrix(row(n));
    slot->updateBounds({ -1.0 }, { 1.0 });
  };
  slot->init(n, 1);
  for (int seq = 0; seq < rounds; ++seq)
  {
    if (seq == 2 + c / 2)  // give the workspace back: the next solve sets up again
    {
      slot->clear();
      slot->init(n, 1);
    }
    load(seq);
    f.waiting[c] = true;
    const bool ok = slot->solve();
    f.waiting[c] = false;
    CHECK(ok);
    const trajopt_ifopt::VectorXd x = slot->getSolution();
    CHECK(static_cast<long>(x.size()) == n && static_cast<int>(x[0]) == c && static_cast<int>(x[1]) == seq);
    CHECK(f.served[c].load() == seq + 1);
  }
  CHECK(slot->n_solves == rounds && slot->n_rounds == rounds && slot->n_setups == 2);
  slot.reset();
  --f.running;
  batch->leave();
}
}  // namespace

int main()
{
  Fake f;
  for (int c = 0; c < kClients; ++c)
  {
    f.waiting[c] = false;
    f.served[c] = 0;
  }
  // polls an atomic: this compiler's ThreadSanitizer does not see through condition_variable::wait_for
  std::atomic<bool> finished{ false };
  std::thread watchdog([&] {
    for (int tenths = 0; !finished.load(); ++tenths)
    {
      if (tenths > 1200)
      {
        std::fprintf(stderr, "gpu_qp_batch_check: the batch did not terminate\n");
        std::_Exit(2);
      }
      std::this_thread::sleep_for(std::chrono::milliseconds(100));
    }
  });
  GpuQPBatch::Stats st;
  {
    auto batch = std::make_shared<GpuQPBatch>(0, fakeDevice(f));
    for (int c = 0; c < kClients; ++c)
      batch->enter();
    std::vector<std::thread> threads;
    for (int c = 0; c < kClients; ++c)
      threads.emplace_back(client, c, std::ref(f), batch);
    for (auto& t : threads)
      t.join();
    st = batch->stats();
  }
  finished = true;
  watchdog.join();
  // the longest client has 3 + 2 * 7 = 17 requests and takes part in every round
  CHECK(st.rounds == 3 + 2 * (kClients - 1));
  CHECK(st.step_launches == f.steps && st.step_launches >= st.rounds && st.step_launches <= 2 * st.rounds);
  CHECK(st.groups == f.creates && st.max_group == kClients / 2);
  CHECK(f.shape.empty());  // every handle destroyed
  for (int c = 0; c < kClients; ++c)
    CHECK(f.served[c].load() == 3 + 2 * c);
  if (g_failures.load())
  {
    std::fprintf(stderr, "gpu_qp_batch_check: %d check(s) failed\n", g_failures.load());
    return 1;
  }
  std::printf("gpu_qp_batch_check ok: %lld rounds, %lld steps, %lld groups\n", st.rounds, st.step_launches, st.groups);
  return 0;
}
