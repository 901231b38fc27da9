// What the four engine handles (engine.hip, hubert.hip, landmark.hip, facedet.hip) have in common: the table of a packed
// buffer, the device guard, the check in front of every create and the ownership of the weights.  Host code only; the
// bodies that are more than a line are in runtime.hip.  A new handle starts from these.
#pragma once

#include <string>
#include <vector>

#include "common.h"

inline int64_t round64(int64_t n) { return (n + 63) / 64 * 64; }   // floats up to a 256-B boundary

// name -> (offset, size) in floats of every tensor of a packed buffer, in the order they were added
struct PackedLayout {
  struct Entry {
    std::string name;
    int64_t off, size;
  };
  std::vector<Entry> e;
  int64_t total = 0;
  int64_t add(const std::string& name, int64_t size) {   // -> its offset; every tensor starts 256-B aligned
    const int64_t at = total;
    e.push_back({name, at, size});
    total += round64(size);
    return at;
  }
  int64_t off(const std::string& name) const {   // -1: no such tensor
    for (const Entry& x : e)
      if (x.name == name) return x.off;
    return -1;
  }
  int count() const { return (int)e.size(); }
  bool has(int i) const { return i >= 0 && i < count(); }
  // what the casync_*_packed_{name,offset,size} accessors return
  const char* name(int i) const { return has(i) ? e[i].name.c_str() : nullptr; }
  int64_t offset(int i) const { return has(i) ? e[i].off : -1; }
  int64_t size(int i) const { return has(i) ? e[i].size : -1; }
};

// hipSetDevice for the life of a scope (the caller's device is restored on exit)
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) err = hipSetDevice(dev);
    else if (err == hipSuccess) prev = -1;   // nothing to restore
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// In front of every create: a device is visible, device_id names one of them and it is a gfx950.  `what` opens the message.
int casync_require_gfx950(const char* what, int device_id);

// The packed weights of one handle on its device.  `what` opens every message; `total` is the handle's layout total.
struct PackedWeights {
  const float* w = nullptr;   // fp32, `owned` or a buffer of the caller's (adopt_device); null until a load
  float* owned = nullptr;     // allocated by the first load_host, kept for the next one
  bf16_t* w16 = nullptr;      // bf16 image of w at the same element offsets, handles that asked for it only
  int load_host(const char* what, int device, const float* packed, int64_t n, int64_t total, bool want_bf16);
  // packed_dev stays the caller's and must outlive the handle's use of it; refused when it lives on another device
  int adopt_device(const char* what, int device, const float* packed_dev, int64_t n, int64_t total, bool want_bf16);
  void release();   // under the destroy path's DeviceGuard
};
