/*
 * hip_host_run.h -- the workgroup runner of the host shim (included by the stub hip/hip_runtime.h, behind dim3 and the index
 * variables).  A kernel is a function that reads threadIdx / blockIdx / blockDim / gridDim:
 *
 *   run_grid(grid, n_thr, call)          barrier-free kernels: two nested loops on the calling thread
 *   run_grid_threads(grid, n_thr, call)  kernels with __syncthreads() or __shfl_xor: one workgroup at a time, one real thread
 *                                        per work-item.  A work-item that returns leaves the barriers, as a finished wave does.
 *
 * A launch's dynamic LDS (extern __shared__) is one heap buffer of exactly the launch's lds_bytes, 16-byte aligned, filled with
 * the poison byte 0x5a before every workgroup: a kernel that reads LDS it has not written gets poison, and one that walks past
 * what the launcher asked for is seen by AddressSanitizer in the stand-alone sanitized programs.
 *
 * The runner proves nothing about barrier placement beyond "the result is right when barriers hold", nothing about memory
 * order (every barrier here is a full fence) and nothing about occupancy.
 */
#ifndef HIP_HOST_RUN_H
#define HIP_HOST_RUN_H
#include <cstdio>
#include <cstdlib>
#include <climits>
#include <atomic>
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <thread>
#include <vector>

namespace hip_host {

/* a barrier whose party shrinks when a member leaves.  No mutex: {members, waiting} is one atomic word, and the waiters sleep on
 * the round counter (a futex), so that the up to 1024 threads a release wakes do not queue up for a lock one after the other --
 * that queue was three quarters of the emulation's time */
class Barrier {
  std::atomic<uint64_t> state{0}; /* members << 32 | waiting */
  std::atomic<uint32_t> round{0};
  static_assert(sizeof(std::atomic<uint32_t>) == sizeof(uint32_t), "the futex word");
  void release()
  {
    round.fetch_add(1);
    syscall(SYS_futex, reinterpret_cast<uint32_t *>(&round), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
  }

public:
  void reset(uint32_t n) { state.store((uint64_t)n << 32); }
  void wait()
  {
    const uint32_t r = round.load(); /* (cannot move before this thread has arrived: the release needs it) */
    uint64_t s = state.load();
    for (;;) {
      const uint32_t members = (uint32_t)(s >> 32), waiting = (uint32_t)s + 1;
      const bool last = waiting == members;
      if (state.compare_exchange_weak(s, last ? (uint64_t)members << 32 : ((uint64_t)members << 32) | waiting)) {
        if (last) {
          release();
          return;
        }
        break;
      }
    }
    while (round.load() == r)
      syscall(SYS_futex, reinterpret_cast<uint32_t *>(&round), FUTEX_WAIT_PRIVATE, r, nullptr, nullptr, 0);
  }
  void leave()
  {
    uint64_t s = state.load();
    for (;;) {
      const uint32_t members = (uint32_t)(s >> 32) - 1, waiting = (uint32_t)s;
      const bool last = members && waiting == members;
      if (state.compare_exchange_weak(s, last ? (uint64_t)members << 32 : ((uint64_t)members << 32) | waiting)) {
        if (last)
          release();
        return;
      }
    }
  }
};

#define HIP_HOST_WAVE 64u
#define HIP_HOST_MAX_THREADS 1024u

struct Workgroup {
  Barrier all;
  Barrier wave[HIP_HOST_MAX_THREADS / HIP_HOST_WAVE];
  /* two sets of slots, taken in turn: a lane may write the next exchange's slot while a slower lane still reads this one's, so an
   * exchange needs one wave barrier (between its writes and its reads), not two */
  uint64_t exchange[2][HIP_HOST_MAX_THREADS / HIP_HOST_WAVE][HIP_HOST_WAVE];
};
inline Workgroup *running = nullptr; /* set by run_grid_threads; nullptr under run_grid: a barrier there is a bug of the test */

/* the running launch's dynamic LDS */
#define HIP_HOST_LDS_POISON 0x5a
inline uint8_t *dynamic_lds_buf = nullptr;
inline size_t dynamic_lds_bytes = 0;
inline void *dynamic_lds() { return dynamic_lds_buf; }
inline void poison_lds()
{
  if (dynamic_lds_bytes)
    memset(dynamic_lds_buf, HIP_HOST_LDS_POISON, dynamic_lds_bytes);
}
/* wall_clock64 / clock64: a counter that moves with every look, so that a wait for a later time ends */
inline std::atomic<unsigned long long> ticks{0};

inline void need_threads()
{
  if (!running) {
    fprintf(stderr, "hip_host: a kernel launched with run_grid reached a barrier or a shuffle\n");
    abort();
  }
}
inline void workgroup_barrier()
{
  need_threads();
  running->all.wait();
}
inline void wave_barrier()
{
  need_threads();
  running->wave[threadIdx.x / HIP_HOST_WAVE].wait();
}
/* 0 at a workgroup's start.  The single barrier per exchange rests on every lane of a wave making the SAME number of exchange calls
 * (__shfl_xor, __ballot, __any, hip_host_wave_first) in a workgroup: a divergent one -- some lanes call, others do not -- would pair
 * different sets of slots from then on, silently, without a hang.  The kernels run here make them wave-uniformly, as the device's
 * full-wave forms of these operations require anyway. */
inline thread_local uint32_t exchange_turn = 0;
inline uint64_t *wave_exchange()
{
  need_threads();
  return running->exchange[exchange_turn++ & 1u][threadIdx.x / HIP_HOST_WAVE];
}

/* grid = (x, y) workgroups of n_thr work-items */
template <typename Call> void run_grid(dim3 grid, uint32_t n_thr, Call call)
{
  gridDim = grid;
  blockDim = dim3(n_thr);
  for (uint32_t by = 0; by < grid.y; by++)
    for (uint32_t bx = 0; bx < grid.x; bx++) {
      blockIdx = dim3(bx, by);
      poison_lds();
      for (uint32_t t = 0; t < n_thr; t++) {
        threadIdx = dim3(t);
        call();
      }
    }
}

template <typename Call> void run_grid_threads(dim3 grid, uint32_t n_thr, Call call)
{
  if (n_thr > HIP_HOST_MAX_THREADS || n_thr % HIP_HOST_WAVE) {
    fprintf(stderr, "hip_host: run_grid_threads takes whole waves, %u threads at the most\n", HIP_HOST_MAX_THREADS);
    abort();
  }
  static Workgroup wg;
  /* the work-items' threads live for the whole grid (starting a thread costs more than a barrier, under the sanitizers many times
   * more): between two workgroups they meet, work-item 0 arms the barriers and poisons the LDS, and they meet again */
  static Barrier between;
  const uint32_t n_wg = grid.x * grid.y;
  auto arm = [n_thr] {
    wg.all.reset(n_thr);
    for (uint32_t w = 0; w < n_thr / HIP_HOST_WAVE; w++)
      wg.wave[w].reset(HIP_HOST_WAVE);
    poison_lds();
  };
  arm();
  between.reset(n_thr);
  running = &wg;
  std::vector<std::thread> items;
  items.reserve(n_thr);
  for (uint32_t t = 0; t < n_thr; t++)
    items.emplace_back([=, &call] {
      gridDim = grid;
      blockDim = dim3(n_thr);
      threadIdx = dim3(t);
      for (uint32_t b = 0; b < n_wg; b++) {
        blockIdx = dim3(b % grid.x, b / grid.x);
        exchange_turn = 0;
        call();
        wg.wave[t / HIP_HOST_WAVE].leave();
        wg.all.leave();
        if (b + 1 < n_wg) {
          between.wait(); /* every work-item has left the workgroup's barriers */
          if (t == 0)
            arm();
          between.wait();
        }
      }
    });
  for (std::thread &th : items)
    th.join();
  running = nullptr;
}

/* what the stub's hipLaunchKernelGGL comes to, so that the .hip files' own launchers (their dispatch on n_rx, mode, ...) run as
 * they are.  The caller of a launcher whose kernel has barriers sets launch_with_threads around it. */
inline bool launch_with_threads = false;
template <typename Call> void launch(dim3 grid, dim3 block, size_t lds_bytes, Call call)
{
  if (grid.z != 1 || block.y != 1 || block.z != 1) {
    fprintf(stderr, "hip_host: grids of two dimensions and workgroups of one at the most\n");
    abort();
  }
  void *lds = nullptr;
  if (lds_bytes && posix_memalign(&lds, 16, lds_bytes) != 0) {
    fprintf(stderr, "hip_host: no memory for %zu bytes of LDS\n", lds_bytes);
    abort();
  }
  dynamic_lds_buf = static_cast<uint8_t *>(lds);
  dynamic_lds_bytes = lds_bytes;
  if (launch_with_threads)
    run_grid_threads(grid, block.x, call);
  else
    run_grid(grid, block.x, call);
  dynamic_lds_buf = nullptr;
  dynamic_lds_bytes = 0;
  free(lds);
}

} // namespace hip_host
#endif
