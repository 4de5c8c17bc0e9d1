// Guard mode of DeviceArray (mfgpu_device.h): padded, poisoned and registered allocations, and the mfgpu_debug_guard_*
// entry points that switch the mode and inspect the guards.  Host code only; the fills are hipMemset, the reads hipMemcpy.
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "mfgpu_device.h"

namespace mfgpu {

std::atomic<size_t> g_guard_bytes{0};

namespace {

constexpr size_t kPayloadAlign = 256;  // what a kernel may assume of a bare hipMalloc
constexpr size_t kGuardMax = (size_t)1 << 30;
constexpr int kFill = 0xFF;  // all-ones bytes: a NaN as double and as float
constexpr int kReportMax = 8;  // damaged guards the report describes

struct Entry {
  size_t bytes, guard, front;  // payload, back guard, front padding (the guard rounded up to kPayloadAlign)
  uint64_t ordinal;
};
struct Registry {
  std::mutex m;
  std::map<char *, Entry> live;  // by base pointer
  uint64_t next = 0;
};
// never destroyed: handles that outlive main's statics still unregister
Registry &registry() {
  static Registry *r = new Registry;
  return *r;
}

size_t front_bytes(size_t guard) { return (guard + kPayloadAlign - 1) / kPayloadAlign * kPayloadAlign; }

// the damaged byte of g[0, n) nearest the payload, which lies behind (front guard) or in front of (back guard) g; -1: none
long long nearest_damage(const std::vector<unsigned char> &g, bool front_side) {
  const long long n = (long long)g.size();
  if (front_side) {
    for (long long i = n - 1; i >= 0; --i)
      if (g[i] != kFill) return i;
  } else {
    for (long long i = 0; i < n; ++i)
      if (g[i] != kFill) return i;
  }
  return -1;
}

}  // namespace

int guard_alloc(void **payload, size_t *front, size_t bytes, size_t guard, bool zero, bool poison) {
  const size_t off = front_bytes(guard);
  char *base = nullptr;
  HIP_TRY(hipMalloc((void **)&base, off + bytes + guard));
  hipError_t e;
  if (poison && !zero) {
    e = hipMemset(base, kFill, off + bytes + guard);
  } else {
    e = hipMemset(base, kFill, off);
    if (e == hipSuccess && zero) e = hipMemset(base + off, 0, bytes);
    if (e == hipSuccess) e = hipMemset(base + off + bytes, kFill, guard);
  }
  // (as the zero fill of DeviceArray::alloc: complete before the first kernel on any stream)
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    hipFree(base);
    return hip_check(e, "guard fill");
  }
  Registry &r = registry();
  {
    std::lock_guard<std::mutex> lock(r.m);
    r.live[base] = Entry{bytes, guard, off, r.next++};
  }
  *payload = base + off;
  *front = off;
  return 0;
}

void guard_free(void *payload, size_t front) {
  char *base = static_cast<char *>(payload) - front;
  Registry &r = registry();
  {
    std::lock_guard<std::mutex> lock(r.m);
    r.live.erase(base);
  }
  hipFree(base);
}

namespace {

int guard_check(uint64_t *n_live, uint64_t *n_damaged, char *report, size_t len) {
  if (!n_live || !n_damaged || (len && !report)) return einval("mfgpu_debug_guard_check: NULL result");
  *n_live = *n_damaged = 0;
  if (len) report[0] = 0;
  Registry &r = registry();
  std::lock_guard<std::mutex> lock(r.m);
  if (r.live.empty()) return 0;
  HIP_TRY(hipDeviceSynchronize());
  std::string text;
  std::vector<unsigned char> host;
  for (const auto &kv : r.live) {
    const Entry &en = kv.second;
    ++*n_live;
    for (int side = 0; side < 2; ++side) {  // 0: front, 1: back
      const size_t n = side ? en.guard : en.front;
      host.resize(n);
      HIP_TRY(hipMemcpy(host.data(), kv.first + (side ? en.front + en.bytes : 0), n, hipMemcpyDeviceToHost));
      const long long at = nearest_damage(host, side == 0);
      if (at < 0) continue;
      if (++*n_damaged > (uint64_t)kReportMax) continue;
      char line[160];
      if (side)
        std::snprintf(line, sizeof line, "array #%llu (%zu payload bytes): back guard, offset +%lld: 0x%02x\n",
                      (unsigned long long)en.ordinal, en.bytes, at, (unsigned)host[at]);
      else
        std::snprintf(line, sizeof line, "array #%llu (%zu payload bytes): front guard, offset -%lld: 0x%02x\n",
                      (unsigned long long)en.ordinal, en.bytes, (long long)n - at, (unsigned)host[at]);
      text += line;
    }
  }
  if (len) {
    std::strncpy(report, text.c_str(), len - 1);
    report[len - 1] = 0;
  }
  return 0;
}

}  // namespace
}  // namespace mfgpu

using namespace mfgpu;

extern "C" {

int mfgpu_debug_guard_begin(size_t guard_bytes) {
  if (guard_bytes == 0 || guard_bytes > kGuardMax) return einval("mfgpu_debug_guard_begin: guard_bytes outside [1, 2^30]");
  g_guard_bytes.store(guard_bytes);
  return 0;
}

int mfgpu_debug_guard_end(void) {
  g_guard_bytes.store(0);
  return 0;
}

int mfgpu_debug_guard_layout(size_t bytes, size_t guard_bytes, size_t *total, size_t *payload_offset) {
  if (!total || !payload_offset) return einval("mfgpu_debug_guard_layout: NULL result");
  if (guard_bytes == 0 || guard_bytes > kGuardMax) return einval("mfgpu_debug_guard_layout: guard_bytes outside [1, 2^30]");
  *payload_offset = front_bytes(guard_bytes);
  *total = *payload_offset + bytes + guard_bytes;
  return 0;
}

int mfgpu_debug_guard_check(uint64_t *n_live, uint64_t *n_damaged, char *report, size_t len) {
  return guard_check(n_live, n_damaged, report, len);
}

int mfgpu_debug_guard_selftest(uint64_t *n_damaged, char *report, size_t len, int *poisoned_ok, int *zeroed_ok) {
  if (!poisoned_ok || !zeroed_ok) return einval("mfgpu_debug_guard_selftest: NULL result");
  if (!g_guard_bytes.load()) return einval("mfgpu_debug_guard_selftest: guard mode is off");
  constexpr size_t n = 37;  // 296 bytes: the back guard begins off the 256-byte grid
  DeviceArray<double> poisoned, zeroed;
  int rc;
  if ((rc = poisoned.alloc(n)) || (rc = zeroed.alloc(n, true))) return rc;
  unsigned char host[n * sizeof(double)];
  HIP_TRY(hipMemcpy(host, poisoned.get(), sizeof host, hipMemcpyDeviceToHost));
  *poisoned_ok = 1;
  for (unsigned char b : host) *poisoned_ok &= b == kFill;
  HIP_TRY(hipMemcpy(host, zeroed.get(), sizeof host, hipMemcpyDeviceToHost));
  *zeroed_ok = 1;
  for (unsigned char b : host) *zeroed_ok &= b == 0;
  // two damages, both inside the poisoned array's own allocation (the guards are at least one byte and the front
  // padding at least 256; a short back guard takes fewer bytes)
  const unsigned char planted[8] = {0x5a, 0x5a, 0x5a, 0x5a, 0x5a, 0x5a, 0x5a, 0x5a};
  char *p = reinterpret_cast<char *>(poisoned.get());
  const size_t back = g_guard_bytes.load() < 8 ? g_guard_bytes.load() : 8;
  HIP_TRY(hipMemcpy(p + poisoned.bytes(), planted, back, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(p - 8, planted, 8, hipMemcpyHostToDevice));
  uint64_t n_live = 0;
  return guard_check(&n_live, n_damaged, report, len);
}

}  // extern "C"
