/*
 * slot_emul_common.h -- what the slot_*_emul.cpp files share: the set_error the library's plan headers report through (one text
 * per thread for all three files, read with slot_emul_last_error), and the few helpers around a launch.
 */
#ifndef SLOT_EMUL_COMMON_H
#define SLOT_EMUL_COMMON_H
#include <hip/hip_runtime.h>
#include <initializer_list>
#include <memory>
#include <string>

inline thread_local std::string slot_emul_error;

namespace {

int set_error(const char *what)
{
  slot_emul_error = what;
  return -1;
}

int launched(hipError_t e) { return e == hipSuccess ? 0 : set_error("the launcher refused its arguments"); }

/* DEVICE mem wants the c16 arrays 4-byte aligned */
bool aligned4(std::initializer_list<const void *> arrays)
{
  for (const void *p : arrays)
    if (reinterpret_cast<uintptr_t>(p) & 3u)
      return false;
  return true;
}
const uint32_t *c16(const int16_t *p) { return reinterpret_cast<const uint32_t *>(p); }
uint32_t *c16(int16_t *p) { return reinterpret_cast<uint32_t *>(p); }

/* a call's tables in an allocation of exactly their size (the library uploads that many bytes) */
template <typename T> std::unique_ptr<uint8_t[]> tables_copy(const T &tab, size_t bytes)
{
  std::unique_ptr<uint8_t[]> p(new uint8_t[bytes]);
  tab.write(p.get());
  return p;
}
template <typename T> std::unique_ptr<uint8_t[]> tables_copy(const T &tab) { return tables_copy(tab, tab.bytes()); }

/* around the launch of a kernel with a barrier, a shuffle or a ballot: real threads (hip_host_run.h) */
struct WithThreads {
  WithThreads() { hip_host::launch_with_threads = true; }
  ~WithThreads() { hip_host::launch_with_threads = false; }
};

} // namespace
#endif
