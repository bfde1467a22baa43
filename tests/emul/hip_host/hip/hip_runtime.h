/*
 * hip/hip_runtime.h -- host meanings for the HIP qualifiers and the few HIP names the slot-level .hip files use, so that a plain
 * host compiler reads those files as they are (test infrastructure: tests/emul/ puts this directory on the include path ahead
 * of the ROCm one; nothing in openairinterface5g_amd/ may include it).  A kernel becomes an ordinary function that reads
 * threadIdx / blockIdx / blockDim / gridDim, which hip_host_run.h sets (thread-local) for every work-item of a grid.
 *
 *   __shared__       one static copy: workgroups run one after the other, and the work-items of a running workgroup share it
 *   __syncthreads()  a barrier of the running workgroup's work-items (real threads, hip_host_run.h: run_grid_threads)
 *   __shfl_xor,      a per-wave exchange array of 64 lanes, a wave barrier between the writes and the reads (two arrays in turn)
 *   __ballot
 *   hipLaunchKernelGGL  runs the grid on the spot, so the .hip files' own launchers (their dispatch) are the ones that run
 *   __hip_atomic_*   the __atomic_* builtins; the scope is dropped (one process is one agent)
 *   extern __shared__  (dynamic LDS) a heap buffer of exactly the launch's lds_bytes, poisoned before every workgroup
 *   readfirstlane    hip_host_wave_first: lane 0's value through the exchange slots
 *   s_sleep, s_setprio, s_getreg, fence, wall_clock64  a yield, nothing, 0, a full fence, a counter that moves with every look
 */
#ifndef HIP_HOST_RUNTIME_H
#define HIP_HOST_RUNTIME_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))
#define __launch_bounds__(...)
#define __shared__ static
#define __constant__

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1 };
typedef struct hip_host_stream *hipStream_t;

struct dim3 {
  uint32_t x, y, z;
  constexpr dim3(uint32_t x_ = 1, uint32_t y_ = 1, uint32_t z_ = 1) : x(x_), y(y_), z(z_) {}
};
/* 16-byte aligned as HIP's: an access through a uint4 pointer is one the kernel claims aligned.  A vector type, not a struct:
 * UBSan checks the alignment of a vector load or store, and lets the copy of an over-aligned struct through a cast pointer pass */
typedef uint32_t uint4 __attribute__((ext_vector_type(4)));
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }

inline thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;

typedef int32_t int4 __attribute__((ext_vector_type(4)));
static inline int4 make_int4(int32_t x, int32_t y, int32_t z, int32_t w) { return int4{x, y, z, w}; }

static inline int __popc(uint32_t x) { return __builtin_popcount(x); }
static inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }

/* ---- what needs the other work-items of the workgroup: the runner has the two waits and the exchange slots ---- */
#include "../hip_host_run.h"

/* a launch runs the grid on the spot (the stream is not looked at); its dynamic LDS is a heap buffer of exactly lds_bytes, which
 * a kernel declares with HIP_HOST_DYNAMIC_LDS (the host meaning of `extern __shared__ type name[]`) */
#define hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, ...) \
  hip_host::launch((grid), (block), (size_t)(lds_bytes), [&] { kernel(__VA_ARGS__); })
#define HIP_HOST_DYNAMIC_LDS(type, name) type *const name = static_cast<type *>(hip_host::dynamic_lds())
static inline hipError_t hipGetLastError() { return hipSuccess; }

static inline void __syncthreads() { hip_host::workgroup_barrier(); }

template <typename T> static inline T __shfl_xor(T v, int lane_mask)
{
  static_assert(sizeof(T) <= 8, "exchange slots are 8 bytes");
  uint64_t *x = hip_host::wave_exchange();
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t bits = 0;
  memcpy(&bits, &v, sizeof v);
  x[lane] = bits;
  hip_host::wave_barrier();
  bits = x[(lane ^ (uint32_t)lane_mask) & 63u];
  memcpy(&v, &bits, sizeof v);
  return v;
}

/* bit l = lane l's predicate; every lane of the wave takes part */
static inline unsigned long long __ballot(int pred)
{
  uint64_t *x = hip_host::wave_exchange();
  x[threadIdx.x & 63u] = pred != 0;
  hip_host::wave_barrier();
  unsigned long long m = 0;
  for (uint32_t l = 0; l < 64u; l++)
    m |= (unsigned long long)x[l] << l;
  return m;
}

/* lane 0's value to every lane of the wave: the host meaning of a value the device takes with readfirstlane (the translation
 * units of the decoder kernels give it to LDPC_UNIFORM: with one thread per lane `(x)` would leave every lane its own).  LANE 0,
 * not the first ACTIVE lane as on the device: a wave whose lane 0 has returned from the kernel while other lanes still ask would
 * read a stale slot.  The files run today leave their kernels wave-uniformly; a file that does not needs the runner to track the
 * lowest live lane. */
template <typename T> static inline T hip_host_wave_first(T v)
{
  static_assert(sizeof(T) <= 8, "exchange slots are 8 bytes");
  uint64_t *x = hip_host::wave_exchange();
  uint64_t bits = 0;
  memcpy(&bits, &v, sizeof v);
  x[threadIdx.x & 63u] = bits;
  hip_host::wave_barrier();
  bits = x[0];
  memcpy(&v, &bits, sizeof v);
  return v;
}
static inline int __any(int pred) { return __ballot(pred) != 0; }

#define __HIP_MEMORY_SCOPE_WORKGROUP 0
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __HIP_MEMORY_SCOPE_SYSTEM 0
#define __hip_atomic_fetch_max(p, v, order, scope) __atomic_fetch_max((p), (v), (order))
#define __hip_atomic_fetch_add(p, v, order, scope) __atomic_fetch_add((p), (v), (order))
#define __hip_atomic_load(p, order, scope) __atomic_load_n((p), (order))
#define __hip_atomic_store(p, v, order, scope) __atomic_store_n((p), (v), (order))
static inline int atomicAdd(int *p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline unsigned atomicAdd(unsigned *p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline int atomicXor(int *p, int v) { return __atomic_fetch_xor(p, v, __ATOMIC_RELAXED); }
static inline unsigned atomicXor(unsigned *p, unsigned v) { return __atomic_fetch_xor(p, v, __ATOMIC_RELAXED); }

/* what only the hardware means: priorities and register reads are nothing, a sleep gives the core away, a fence is a full one,
 * the s_barrier is the workgroup's, and the clocks are a counter that moves with every look (a wait for a later time ends) */
#define __builtin_amdgcn_s_sleep(n) std::this_thread::yield()
#define __builtin_amdgcn_s_setprio(n) ((void)0)
#define __builtin_amdgcn_s_getreg(r) 0u
#define __builtin_amdgcn_fence(...) __atomic_thread_fence(__ATOMIC_SEQ_CST)
#define __builtin_amdgcn_s_barrier() hip_host::workgroup_barrier()
static inline unsigned long long wall_clock64() { return hip_host::ticks.fetch_add(1, std::memory_order_relaxed) + 1; }
static inline long long clock64() { return (long long)wall_clock64(); }

/* kernel attributes: nothing to set (the dynamic LDS of a launch is as large as the launch says) */
enum hipFuncAttribute { hipFuncAttributeMaxDynamicSharedMemorySize = 8 };
static inline hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }
#endif
