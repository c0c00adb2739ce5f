#include "common.h"

#include <stdlib.h>

#include <functional>
#include <mutex>

namespace nabu {
char *err_buf() {
  static thread_local char buf[512] = {0};
  return buf;
}
int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return e ? atoi(e) : dflt;
}

// one answer per device, remembered by the calling thread (the current device is a per-thread setting)
template <typename Q>
static int per_thread_and_device(int &cached_dev, int &cached, Q query) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (dev != cached_dev) {
    cached = query(dev);
    (void)hipGetLastError();
    cached_dev = dev;
  }
  return cached;
}
int device_cus() {
  static thread_local int cached_dev = -1, cached = 0;
  return per_thread_and_device(cached_dev, cached, [](int dev) {
    int v = 0;
    return hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0 ? v : 0;
  });
}
int device_lds_bytes() {
  static thread_local int cached_dev = -1, cached = 0;
  return per_thread_and_device(cached_dev, cached, [](int dev) {
    int lds = 0;
    for (hipDeviceAttribute_t n : {hipDeviceAttributeMaxSharedMemoryPerBlock, hipDeviceAttributeSharedMemPerBlockOptin,
                                   hipDeviceAttributeMaxSharedMemoryPerMultiprocessor}) {
      int v = 0;
      if (hipDeviceGetAttribute(&v, n, dev) == hipSuccess && v > lds) lds = v;
    }
    return lds;
  });
}

// what is known about a (function, device): open addressing, a handful of probes, entries never leave
namespace {
constexpr size_t LDS_MAX = 160 * 1024;     // what a CU has
constexpr int SLOTS = 1024, PROBES = 8;
struct Grant { const void *fn; int dev; size_t bytes; };
struct Occupancy { const void *fn; int dev, threads, blocks; size_t lds; };
std::mutex g_mutex;
Grant g_grants[SLOTS];
Occupancy g_occupancy[SLOTS];
size_t slot_of(const void *fn, int dev, int probe) {
  return (std::hash<const void *>()(fn) * 31 + (size_t)dev + (size_t)probe) % SLOTS;
}
}  // namespace

int ensure_dynamic_lds(const void *fn, size_t bytes) {
  if (bytes > LDS_MAX) return fail(NABU_EUNSUP, "%zu bytes of LDS per workgroup: a CU has %zu", bytes, LDS_MAX);
  if (bytes > 64 * 1024) {     // (up to there: the runtime's default)
    int dev = 0;
    NABU_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_mutex);
    Grant *g = nullptr;
    for (int i = 0; i < PROBES && !g; ++i) {
      Grant &c = g_grants[slot_of(fn, dev, i)];
      if (!c.fn) c = Grant{fn, dev, 0};
      if (c.fn == fn && c.dev == dev) g = &c;
    }
    if (g && g->bytes >= bytes) return 0;
    NABU_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (g) g->bytes = bytes;
  }
  return 0;
}

int max_blocks_per_cu(const void *fn, int threads, size_t lds, int *blocks) {
  NABU_TRY(ensure_dynamic_lds(fn, lds));
  int dev = 0;
  NABU_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_mutex);
  Occupancy *free_slot = nullptr;
  for (int i = 0; i < PROBES; ++i) {
    Occupancy &c = g_occupancy[slot_of(fn, dev, i)];
    if (c.fn == fn && c.dev == dev && c.threads == threads && c.lds == lds) { *blocks = c.blocks; return 0; }
    if (!c.fn && !free_slot) free_slot = &c;
  }
  NABU_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, fn, threads, lds));
  if (free_slot) *free_slot = Occupancy{fn, dev, threads, *blocks, lds};
  return 0;
}
}  // namespace nabu

extern "C" int nabu_version(void) { return NABU_ABI_VERSION; }
extern "C" const char *nabu_last_error(void) { return nabu::err_buf(); }
