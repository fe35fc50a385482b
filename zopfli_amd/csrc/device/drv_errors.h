// Driver part: the calling thread's error state (g_err, its class, Fail*), HIPCHK, KCHK, DeviceGuard, DEVICE_ENTRY and
// zmx_last_error*.  Needs the kernel headers' types and zmx_knobs.h; KCHK expands where zmx_pool.h and zmx_ctx are known.
#pragma once

namespace {

using zamd::Knobs;   // the ZOPFLI_AMD_* switches of this file (zmx_knobs.h)

thread_local std::string g_err;   // per calling thread (zmx_last_error)
thread_local bool g_last_oom = false;   // the last failure of this thread was an allocation the device could not serve
// What KIND of failure the last one of this thread was (zmx_last_error_class): callers decide by this code, never by the
// message's text (the text holds the failing expression and __FILE__: "PoolAlloc(...)", a build path).
thread_local int g_err_class = ZMX_ERR_NONE;

int Fail(const char* what, hipError_t e, const char* file, int line) {
  char buf[512];
  std::snprintf(buf, sizeof(buf), "%s: %s (%s:%d)", what, hipGetErrorString(e), file, line);
  g_err = buf;
  g_last_oom = e == hipErrorOutOfMemory;
  g_err_class = g_last_oom ? ZMX_ERR_OUT_OF_MEMORY : ZMX_ERR_DEVICE;
  if (g_last_oom) (void)hipGetLastError();
  return -1;
}
// a request the device layer refuses whoever runs it: bad arguments, a size limit, a pool that overflows after its retries
int FailMsg(const std::string& m) {
  g_err = m;
  g_err_class = ZMX_ERR_REFUSED;
  return -1;
}
// the device did something it should not have (a kernel's guard fired, consistency flags): another context may fare better
int FailFault(const std::string& m) {
  g_err = m;
  g_err_class = ZMX_ERR_DEVICE;
  return -1;
}
constexpr int kTooLarge = -2;   // zmx_tables_build*: the batch does not fit the code budget, try fewer blocks
// refused as it is (this batch, anywhere), but the caller may come back with fewer blocks
int FailTooLarge(const std::string& m) {
  FailMsg(m);
  return kTooLarge;
}

#define HIPCHK(expr)                                                  \
  do {                                                                \
    hipError_t e_ = (expr);                                           \
    if (e_ != hipSuccess) return Fail(#expr, e_, __FILE__, __LINE__); \
  } while (0)

// Every zmx_* entry point runs on its context's device and leaves the calling thread's current HIP
// device as it found it.
struct DeviceGuard {
  int old = -1;
  hipError_t err;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&old) != hipSuccess) old = -1;
    err = hipSetDevice(device);
  }
  ~DeviceGuard() { if (old >= 0) (void)hipSetDevice(old); }
};
// The first statement of an entry that can fail: on `device` until it returns, or the failure to get there.  (Those that
// cannot report — zmx_ctx_destroy, zmx_tables_free, zmx_cost_stores_free, zmx_internal_device_free — take the guard alone.)
#define DEVICE_ENTRY(device)     \
  DeviceGuard dev_guard(device); \
  HIPCHK(dev_guard.err)

}  // namespace

// after every kernel launch: the launch error, and in guard mode the red zones
#define KCHK(c, name)                                            \
  do {                                                           \
    HIPCHK(hipGetLastError());                                   \
    if (GuardOn()) { const int rc_ = (c)->pool.GuardVerify((c)->stream, name); if (rc_) return rc_; } \
  } while (0)

extern "C" {
const char* zmx_last_error(void) { return g_err.c_str(); }
int zmx_last_error_class(void) { return g_err_class; }
}  // extern "C"
