/*
 * hip/hip_runtime.h -- host meanings for the HIP qualifiers and the few HIP names the slot-level .hip files use, so that a plain
 * host compiler reads those files as they are (test infrastructure: tests/emul/ puts this directory on the include path ahead
 * of the ROCm one; nothing in openairinterface5g_amd/ may include it).  A kernel becomes an ordinary function that reads
 * threadIdx / blockIdx / blockDim / gridDim, which hip_host_run.h sets (thread-local) for every work-item of a grid.
 *
 *   __shared__       one static copy: workgroups run one after the other, and the work-items of a running workgroup share it
 *   __syncthreads()  a barrier of the running workgroup's work-items (real threads, hip_host_run.h: run_grid_threads)
 *   __shfl_xor,      a per-wave exchange array of 64 lanes between two wave barriers
 *   __ballot
 *   hipLaunchKernelGGL  runs the grid on the spot, so the .hip files' own launchers (their dispatch) are the ones that run
 *   __hip_atomic_*   the __atomic_* builtins; the scope is dropped (one process is one agent)
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

static inline int __popc(uint32_t x) { return __builtin_popcount(x); }

/* ---- what needs the other work-items of the workgroup: the runner has the two waits and the exchange slots ---- */
#include "../hip_host_run.h"

/* a launch runs the grid on the spot (the stream and the dynamic LDS size are not looked at) */
#define hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, ...) hip_host::launch((grid), (block), [&] { kernel(__VA_ARGS__); })
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
  hip_host::wave_barrier();
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
  hip_host::wave_barrier();
  return m;
}

#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_fetch_max(p, v, order, scope) __atomic_fetch_max((p), (v), (order))
#define __hip_atomic_fetch_add(p, v, order, scope) __atomic_fetch_add((p), (v), (order))
#define __hip_atomic_load(p, order, scope) __atomic_load_n((p), (order))
#endif
