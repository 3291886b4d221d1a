// Device memory of a context: one ledger (DeviceCtx::mem) records every buffer the context keeps, with its size.
// Allocation, growth and release go through the helpers below and nowhere else, so that csp_device_bytes is the ledger's
// total and csp_symbolic_destroy frees whatever the ledger still holds without naming a buffer.
// Direct hipMalloc / hipFree remain only for memory that is NOT a context's:
//   * function-local temporaries freed before the function returns (dpar in tune_placement, capi.hip),
//   * the process-static stamp buffer of SMCP_FLOW_STAMPS (flow_chol, capi.hip): a diagnostic that outlives every context.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/smcp_amd.h"
#include "switches.hpp"

namespace smcp {

struct DevLedger {
  std::unordered_map<const void*, int64_t> held;   // buffer -> bytes
  int64_t total = 0;
};

// hipMalloc of n bytes, recorded the moment it succeeds (the typed helpers below and tune_placement, which must not take
// the SMCP_CONTIG / SMCP_POISON paths of dev_alloc)
inline hipError_t dev_malloc(DevLedger& mem, void** p, size_t n) {
  const hipError_t e = hipMalloc(p, n);
  if (e == hipSuccess) { mem.held[*p] = (int64_t)n; mem.total += (int64_t)n; }
  return e;
}
// the one way to free: hipFree (which waits for the device), forget the entry, clear the pointer
template <class T>
int dev_free(DevLedger& mem, T*& p) {
  if (!p) return 0;
  const hipError_t e = hipFree((void*)p);
  auto it = mem.held.find((const void*)p);
  if (it != mem.held.end()) { mem.total -= it->second; mem.held.erase(it); }
  p = nullptr;
  return e == hipSuccess ? 0 : SMCP_EHIP;
}
template <class... T>
int dev_free(DevLedger& mem, T*&... p) {
  int rc = 0;
  ((rc = dev_free(mem, p) ? SMCP_EHIP : rc), ...);
  return rc;
}
// everything still recorded (csp_symbolic_destroy)
inline void dev_free_all(DevLedger& mem) {
  for (auto& kv : mem.held) (void)hipFree(const_cast<void*>(kv.first));
  mem.held.clear();
  mem.total = 0;
}

template <class T>
int dev_upload(T** dst, const T* src, size_t count, DevLedger& mem) {
  size_t n = std::max<size_t>(count, 1) * sizeof(T);
  if (dev_malloc(mem, (void**)dst, n) != hipSuccess) return SMCP_ENOMEM;
  if (count && hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return SMCP_EHIP;
  return 0;
}
template <class T>
int dev_upload(T** dst, const std::vector<T>& src, DevLedger& mem) {
  return dev_upload(dst, src.data(), src.size(), mem);
}
template <class T>
int dev_alloc(T** dst, int64_t count, DevLedger& mem) {
  size_t n = (size_t)std::max<int64_t>(count, 1) * sizeof(T);
  // SMCP_CONTIG=1 (placement studies): large buffers from physically contiguous memory (hipDeviceMallocContiguous)
  static int contig = -1;
  if (contig < 0) { const char* e = sw_str("SMCP_CONTIG"); contig = (e && e[0] == '1') ? 1 : 0; }
  hipError_t arc = hipErrorUnknown;
  if (contig && n >= ((size_t)1 << 24)) {
    arc = hipExtMallocWithFlags((void**)dst, n, hipDeviceMallocContiguous);
    if (arc == hipSuccess) { mem.held[(const void*)*dst] = (int64_t)n; mem.total += (int64_t)n; }
  }
  if (arc != hipSuccess) { (void)hipGetLastError(); arc = dev_malloc(mem, (void**)dst, n); }
  if (arc != hipSuccess) return SMCP_ENOMEM;
  // SMCP_POISON=1 (hunting reads of never-written workspace): every fp64 buffer starts as 4.5e150 in every entry instead of
  // whatever the previous owner of the memory left there -- which, in a re-run of the same test, is the same data at the same
  // addresses and hides the read.  Index arrays are left alone (a poisoned index would fault, not mis-compute).
  if (std::is_same<T, double>::value) {
    static int poison = -1;
    if (poison < 0) poison = sw_on("SMCP_POISON", 0);
    if (poison && hipMemset((void*)*dst, 0x5F, n) != hipSuccess) return SMCP_EHIP;
  }
  { static int dbg = -1; if (dbg < 0) { const char* e = sw_str("SMCP_DEBUG_ADDR"); dbg = (e && e[0] == '1') ? 1 : 0; }      // placement studies
    if (dbg && n >= ((size_t)1 << 24)) fprintf(stderr, "smcp_amd: alloc %zu MB at %p\n", n >> 20, (void*)*dst); }
  return 0;
}

// The one growth routine: grows a scratch buffer that no call keeps to at least `need` elements; its contents are lost.
// An older buffer is freed only once the stream has drained: launches of earlier calls may still use it.
template <class T>
int dev_grow(T** buf, int64_t* len, int64_t need, DevLedger& mem, hipStream_t st) {
  if (*len >= need) return 0;
  if (*buf) {
    *len = 0;
    if (hipStreamSynchronize(st) != hipSuccess) return SMCP_EHIP;
    if (int rc = dev_free(mem, *buf)) return rc;
  }
  if (int rc = dev_alloc(buf, need, mem)) return rc;
  *len = need;
  return 0;
}

}  // namespace smcp
