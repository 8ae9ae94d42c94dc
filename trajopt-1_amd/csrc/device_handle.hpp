// Host side: the life cycle every opaque handle of the C-ABI shares (thip_ctx,
// thip_qp, thip_eval, thip_terms, thip_check, thip_csets, thip_ccsets).  Each
// handle's struct derives from Handle and states only its own fields; alloc()
// records what it allocates, so release() frees it and no destroy lists its
// buffers again.  Host only: no kernel reads anything declared here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/trajopt_hip.h"

namespace thip
{
namespace host
{
struct Handle
{
  int device = 0, batch = 0;
  hipStream_t stream = nullptr;
  bool owns_stream = false;  // false: the caller's (thip_set_stream), not destroyed here
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the kernels of a run; null where a handle takes no time
  bool uploaded = false;
  double last_ms = -1.0;
  std::string err;
  std::vector<void*> owned;  // device allocations, freed by release()
};

inline int fail(Handle* h, const std::string& m)
{
  h->err = m;
  return THIP_E_INVALID;
}
inline int hipfail(Handle* h, const char* what, hipError_t e)
{
  h->err = std::string(what) + ": " + hipGetErrorString(e);
  return THIP_E_HIP;
}

// <api>_create's failures, worded into the API's thread-local string: prefix is "<api>_create: "
struct CreateError
{
  std::string& text;
  const char* prefix;
  int operator()(const std::string& m) const  // a refusal
  {
    text = prefix + m;
    return THIP_E_INVALID;
  }
  int hip(const std::string& what, hipError_t e) const
  {
    text = prefix + what + ": " + hipGetErrorString(e);
    return THIP_E_HIP;
  }
};

template <class T>
inline hipError_t alloc(Handle& h, T*& p, size_t count)
{
  void* v = nullptr;
  const hipError_t e = hipMalloc(&v, count * sizeof(T));
  if (e == hipSuccess)
    h.owned.push_back(v);
  p = static_cast<T*>(v);
  return e;
}

// frees one buffer ahead of release(); p is null afterwards
template <class T>
inline void drop(Handle& h, T*& p)
{
  const auto it = std::find(h.owned.begin(), h.owned.end(), static_cast<void*>(p));
  if (it != h.owned.end())
  {
    hipFree(*it);
    h.owned.erase(it);
  }
  p = nullptr;
}

// a buffer that grows at run time: the old one freed, the new one recorded in its place
template <class T>
inline hipError_t regrow(Handle& h, T*& p, size_t count)
{
  drop(h, p);
  return alloc(h, p, count);
}

inline hipError_t open_stream(Handle& h)
{
  const hipError_t e = hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking);
  h.owns_stream = e == hipSuccess;
  return e;
}
inline hipError_t open_events(Handle& h)
{
  const hipError_t e = hipEventCreate(&h.ev0);
  return e != hipSuccess ? e : hipEventCreate(&h.ev1);
}

// Drains the stream, frees what alloc() recorded, then the events and the
// stream it owns; the caller deletes the object.  Safe on a half-built handle;
// one that holds nothing (a create refused before its first device call) makes
// no runtime call.
inline void release(Handle& h)
{
  if (!h.stream && !h.ev0 && !h.ev1 && h.owned.empty())
    return;
  hipSetDevice(h.device);
  if (h.stream)
    hipStreamSynchronize(h.stream);
  for (void* p : h.owned)
    hipFree(p);
  h.owned.clear();
  if (h.ev0)
    hipEventDestroy(h.ev0);
  if (h.ev1)
    hipEventDestroy(h.ev1);
  if (h.owns_stream && h.stream)
    hipStreamDestroy(h.stream);
  h.stream = nullptr;
}

// A temporary of one call: freed on every return path.
template <class T>
struct Scoped
{
  T* p = nullptr;
  Scoped() = default;
  Scoped(const Scoped&) = delete;
  Scoped& operator=(const Scoped&) = delete;
  ~Scoped() { hipFree(p); }
  hipError_t alloc(size_t count) { return hipMalloc(&p, count * sizeof(T)); }
  operator T*() const { return p; }
};

// What follows takes a handle the caller has found non-null.

// <api>_upload / <api>_upload_device (`who`) of a handle whose only input is the scene
inline int upload_scene(Handle* h, double* d_scene, int n_prims, const double* scene, hipMemcpyKind kind,
                        const char* who)
{
  if (n_prims > 0 && !scene)
    return fail(h, std::string(who) + ": scene required when n_prims > 0");
  hipError_t e;
  if ((e = hipSetDevice(h->device)) != hipSuccess)
    return hipfail(h, "hipSetDevice", e);
  if (n_prims > 0 &&
      ((e = hipMemcpyAsync(d_scene, scene, static_cast<size_t>(h->batch) * static_cast<size_t>(n_prims) * 16 * sizeof(double),
                           kind, h->stream)) != hipSuccess ||
       (e = hipStreamSynchronize(h->stream)) != hipSuccess))
    return hipfail(h, "hipMemcpy(scene)", e);
  h->uploaded = true;
  return THIP_OK;
}

// The start of <api>_run (x on the host: staged in `staging`, `doubles` long)
// and of <api>_run_device.  rest_ok / rest: the call's other required
// arguments and their names in its "null x ..." message (" / results", or "").
// d_x: where the kernel reads.
inline int stage_x(Handle* h, const char* api, bool on_host, const double* x, bool rest_ok, const char* rest,
                   double* staging, size_t doubles, const double*& d_x)
{
  const std::string who = std::string(api) + (on_host ? "_run" : "_run_device");
  if (!x || !rest_ok)
    return fail(h, who + (on_host ? ": null x" : ": null d_x") + rest);
  if (!h->uploaded)
    return fail(h, who + ": " + api + "_upload first");
  hipError_t e;
  if ((e = hipSetDevice(h->device)) != hipSuccess)
    return hipfail(h, "hipSetDevice", e);
  if (on_host && (e = hipMemcpyAsync(staging, x, doubles * sizeof(double), hipMemcpyHostToDevice, h->stream)) != hipSuccess)
    return hipfail(h, "hipMemcpy(x)", e);
  d_x = on_host ? staging : x;
  return THIP_OK;
}

// after a launch: THIP_OK, or "<kernel> launch: <hip error>"
inline int launched(Handle* h, const char* kernel)
{
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? THIP_OK : hipfail(h, (std::string(kernel) + " launch").c_str(), e);
}

// a result to the host on the handle's stream; a null destination is skipped
inline hipError_t to_host(Handle* h, void* dst, const void* src, size_t bytes)
{
  return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess;
}

// launch() (THIP_OK or its own failure) between the two events, then fetch()
// (the to_host calls), the stream drained and the kernels' time taken.  what:
// the name a failing fetch or drain is reported under.
template <class Launch, class Fetch>
inline int timed_run(Handle* h, const char* what, Launch launch, Fetch fetch)
{
  hipError_t e;
  if ((e = hipEventRecord(h->ev0, h->stream)) != hipSuccess)
    return hipfail(h, "hipEventRecord", e);
  if (const int rc = launch(); rc != THIP_OK)
    return rc;
  if ((e = hipEventRecord(h->ev1, h->stream)) != hipSuccess)
    return hipfail(h, "hipEventRecord", e);
  if ((e = fetch()) != hipSuccess || (e = hipStreamSynchronize(h->stream)) != hipSuccess)
    return hipfail(h, what, e);
  float ms = -1.0f;
  h->last_ms = hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess ? static_cast<double>(ms) : -1.0;
  return THIP_OK;
}
}  // namespace host
}  // namespace thip
