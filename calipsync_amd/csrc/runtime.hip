// Process-wide runtime state of the engine library: the option table (environment read once), the
// per-thread "options of the call in progress", the per-(kernel, device) launch attributes, and the handles' shared
// create check and weight ownership (handle.h).
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>

#include "common.h"
#include "handle.h"

namespace {

struct OptField {
  const char* name;   // option name == environment variable without the CASYNC_ prefix, lower case
  int CasyncOptions::*field;
};
const OptField kFields[] = {
    {"lanes", &CasyncOptions::lanes},
    {"trunk_lanes", &CasyncOptions::trunk_lanes},
    {"lane_skew", &CasyncOptions::lane_skew},
    {"overlap", &CasyncOptions::overlap},
    {"gemm_streamk", &CasyncOptions::gemm_streamk},
    {"gemm_glds", &CasyncOptions::gemm_glds},
    {"gemm_cfg", &CasyncOptions::gemm_cfg},
    {"gemm_ring128", &CasyncOptions::gemm_ring128},
    {"gemm_small_m", &CasyncOptions::gemm_small_m},
    {"skip_early", &CasyncOptions::skip_early},
    {"gemm_single64", &CasyncOptions::gemm_single64},
    {"gemm_persist", &CasyncOptions::gemm_persist},
    {"lane_streamk", &CasyncOptions::lane_streamk},
    {"gemm_conc", &CasyncOptions::gemm_conc},
    {"gemm_conc_tiles", &CasyncOptions::gemm_conc_tiles},
    {"fuse_ir", &CasyncOptions::fuse_ir},
    {"fuse_up", &CasyncOptions::fuse_up},
    {"fuse_min_hw", &CasyncOptions::fuse_min_hw},
    {"fuse_q", &CasyncOptions::fuse_q},
    {"ups_commute", &CasyncOptions::ups_commute},
    {"fuse_dw", &CasyncOptions::fuse_dw},
    {"fuse_dw_min", &CasyncOptions::fuse_dw_min},
    {"fuse_dw_min40", &CasyncOptions::fuse_dw_min40},
    {"fuse_dw_deep", &CasyncOptions::fuse_dw_deep},
    {"att_bf16", &CasyncOptions::att_bf16},
    {"ir_dw_mfma", &CasyncOptions::ir_dw_mfma},
    {"bf16_plan", &CasyncOptions::bf16_plan},
    {"inc_mfma", &CasyncOptions::inc_mfma},
    {"ups_commute_bf16", &CasyncOptions::ups_commute_bf16},
    {"fuse_dw_bf16", &CasyncOptions::fuse_dw_bf16},
    {"fuse_dw_bf16_bn", &CasyncOptions::fuse_dw_bf16_bn},
    {"fuse_dw_bf16_min", &CasyncOptions::fuse_dw_bf16_min},
    {"dw_lds", &CasyncOptions::dw_lds},
    {"dw_lds_bytes", &CasyncOptions::dw_lds_bytes},
    {"att_nz", &CasyncOptions::att_nz},
    {"kv_early", &CasyncOptions::kv_early},
    {"conv_skip", &CasyncOptions::conv_skip},
};

thread_local const CasyncOptions* t_current = nullptr;

}  // namespace

CasyncOptions& casync_default_options() {
  static CasyncOptions defaults;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const OptField& f : kFields) {
      char env[64] = "CASYNC_";
      size_t n = strlen(env);
      for (const char* p = f.name; *p && n + 1 < sizeof(env); ++p) env[n++] = (char)(*p >= 'a' && *p <= 'z' ? *p - 32 : *p);
      env[n] = 0;
      const char* v = getenv(env);
      if (v && *v) defaults.*(f.field) = atoi(v);
    }
  });
  return defaults;
}

const CasyncOptions& casync_opts() { return t_current ? *t_current : casync_default_options(); }

int casync_option_ref(CasyncOptions& o, const char* name, int** slot) {
  if (name)
    for (const OptField& f : kFields)
      if (strcmp(f.name, name) == 0) {
        *slot = &(o.*(f.field));
        return CASYNC_OK;
      }
  casync_set_error("unknown option '%s'", name ? name : "(null)");
  return CASYNC_ERR_ARG;
}

CasyncOptScope::CasyncOptScope(const CasyncOptions* o) : prev(t_current) { t_current = o; }
CasyncOptScope::~CasyncOptScope() { t_current = prev; }

int casync_ensure_dyn_lds(unsigned long long* once_mask, const void* fn, int bytes) {
  int dev = 0;
  CASYNC_CHECK_HIP(hipGetDevice(&dev));
  auto* mask = reinterpret_cast<std::atomic<unsigned long long>*>(once_mask);
  const unsigned long long bit = dev >= 0 && dev < 64 ? 1ull << dev : 0;
  if (bit && (mask->load(std::memory_order_acquire) & bit)) return CASYNC_OK;
  CASYNC_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  if (bit) mask->fetch_or(bit, std::memory_order_release);
  return CASYNC_OK;
}

// ---- handle.h --------------------------------------------------------------------------------------------------------
int casync_require_gfx950(const char* what, int device_id) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    casync_set_error("%s: no HIP device visible", what);
    return CASYNC_ERR_NO_DEVICE;
  }
  CASYNC_REQUIRE(device_id >= 0 && device_id < n, "%s: device %d of %d", what, device_id, n);
  hipDeviceProp_t prop;
  CASYNC_CHECK_HIP(hipGetDeviceProperties(&prop, device_id));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    casync_set_error("%s: device %d is %s; this library is built for gfx950 only", what, device_id, prop.gcnArchName);
    return CASYNC_ERR_NO_DEVICE;
  }
  return CASYNC_OK;
}

// bf16 image of the packed buffer, made at weight load (not on the forward path); the packed total is a multiple of 64
static int refresh_w16(PackedWeights& p, int device, int64_t n) {
  DeviceGuard guard(device);
  CASYNC_CHECK_HIP(guard.err);
  if (!p.w16) CASYNC_CHECK_HIP(hipMalloc((void**)&p.w16, n * sizeof(bf16_t)));
  if (int st = launch_f32_to_bf16(p.w, p.w16, (long long)n, 0)) return st;
  CASYNC_CHECK_HIP(hipDeviceSynchronize());
  return CASYNC_OK;
}

int PackedWeights::load_host(const char* what, int device, const float* packed, int64_t n, int64_t total, bool want_bf16) {
  CASYNC_REQUIRE(packed, "%s: null", what);
  CASYNC_REQUIRE(n == total, "%s: %lld floats, layout needs %lld", what, (long long)n, (long long)total);
  {
    DeviceGuard guard(device);
    CASYNC_CHECK_HIP(guard.err);
    if (!owned) CASYNC_CHECK_HIP(hipMalloc((void**)&owned, n * sizeof(float)));
    CASYNC_CHECK_HIP(hipMemcpy(owned, packed, n * sizeof(float), hipMemcpyHostToDevice));
  }
  w = owned;
  return want_bf16 ? refresh_w16(*this, device, n) : CASYNC_OK;
}

int PackedWeights::adopt_device(const char* what, int device, const float* packed_dev, int64_t n, int64_t total, bool want_bf16) {
  CASYNC_REQUIRE(packed_dev, "%s: null", what);
  CASYNC_REQUIRE(n == total, "%s: %lld floats, layout needs %lld", what, (long long)n, (long long)total);
  CASYNC_REQUIRE(((uintptr_t)packed_dev % 256) == 0, "%s: buffer must be 256-B aligned", what);
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, packed_dev) == hipSuccess && attr.type == hipMemoryTypeDevice)
    CASYNC_REQUIRE(attr.device == device, "%s: buffer lives on device %d, the engine on %d", what, attr.device, device);
  else
    (void)hipGetLastError();
  w = packed_dev;
  return want_bf16 ? refresh_w16(*this, device, n) : CASYNC_OK;
}

void PackedWeights::release() {
  if (owned) (void)hipFree(owned);
  if (w16) (void)hipFree(w16);
  w = owned = nullptr;
  w16 = nullptr;
}
