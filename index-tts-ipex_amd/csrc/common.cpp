#include "itts_common.h"
#include <mutex>
namespace itts {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
const char* last_error() { return g_err.c_str(); }

int allow_dynamic_lds(DynLdsLatch& latch, const void* kernel, int bytes) {
  int dev = 0;
  ITTS_HIP_CHECK(hipGetDevice(&dev));
  std::atomic<int>& done = latch.done_on[dev & 63];
  if (done.load(std::memory_order_acquire)) return OK;
  ITTS_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  done.store(1, std::memory_order_release);
  return OK;
}
}  // namespace itts
