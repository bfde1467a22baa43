/*
 * hip_host_run.h -- the workgroup runner of the host shim (included by the stub hip/hip_runtime.h, behind dim3 and the index
 * variables).  A kernel is a function that reads threadIdx / blockIdx / blockDim / gridDim:
 *
 *   run_grid(grid, n_thr, call)          barrier-free kernels: two nested loops on the calling thread
 *   run_grid_threads(grid, n_thr, call)  kernels with __syncthreads() or __shfl_xor: one workgroup at a time, one real thread
 *                                        per work-item.  A work-item that returns leaves the barriers, as a finished wave does.
 *
 * The runner proves nothing about barrier placement beyond "the result is right when barriers hold", nothing about memory
 * order (every barrier here is a full fence) and nothing about occupancy.
 */
#ifndef HIP_HOST_RUN_H
#define HIP_HOST_RUN_H
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

namespace hip_host {

/* a barrier whose party shrinks when a member leaves */
class Barrier {
  std::mutex mu;
  std::condition_variable cv;
  uint32_t members = 0, waiting = 0;
  uint64_t round = 0;
  void release_locked()
  {
    waiting = 0;
    round++;
    cv.notify_all();
  }

public:
  void reset(uint32_t n)
  {
    members = n;
    waiting = 0;
  }
  void wait()
  {
    std::unique_lock<std::mutex> lk(mu);
    if (++waiting == members) {
      release_locked();
      return;
    }
    const uint64_t r = round;
    cv.wait(lk, [&] { return round != r; });
  }
  void leave()
  {
    std::unique_lock<std::mutex> lk(mu);
    members--;
    if (members && waiting == members)
      release_locked();
  }
};

#define HIP_HOST_WAVE 64u
#define HIP_HOST_MAX_THREADS 1024u

struct Workgroup {
  Barrier all;
  Barrier wave[HIP_HOST_MAX_THREADS / HIP_HOST_WAVE];
  uint64_t exchange[HIP_HOST_MAX_THREADS / HIP_HOST_WAVE][HIP_HOST_WAVE];
};
inline Workgroup *running = nullptr; /* set by run_grid_threads; nullptr under run_grid: a barrier there is a bug of the test */

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
inline uint64_t *wave_exchange()
{
  need_threads();
  return running->exchange[threadIdx.x / HIP_HOST_WAVE];
}

/* grid = (x, y) workgroups of n_thr work-items */
template <typename Call> void run_grid(dim3 grid, uint32_t n_thr, Call call)
{
  gridDim = grid;
  blockDim = dim3(n_thr);
  for (uint32_t by = 0; by < grid.y; by++)
    for (uint32_t bx = 0; bx < grid.x; bx++) {
      blockIdx = dim3(bx, by);
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
  for (uint32_t b = 0; b < grid.x * grid.y; b++) {
    wg.all.reset(n_thr);
    for (uint32_t w = 0; w < n_thr / HIP_HOST_WAVE; w++)
      wg.wave[w].reset(HIP_HOST_WAVE);
    running = &wg;
    std::vector<std::thread> items;
    items.reserve(n_thr);
    for (uint32_t t = 0; t < n_thr; t++)
      items.emplace_back([=, &call] {
        gridDim = grid;
        blockDim = dim3(n_thr);
        blockIdx = dim3(b % grid.x, b / grid.x);
        threadIdx = dim3(t);
        call();
        wg.wave[t / HIP_HOST_WAVE].leave();
        wg.all.leave();
      });
    for (std::thread &th : items)
      th.join();
    running = nullptr;
  }
}

/* what the stub's hipLaunchKernelGGL comes to, so that the .hip files' own launchers (their dispatch on n_rx, mode, ...) run as
 * they are.  The caller of a launcher whose kernel has barriers sets launch_with_threads around it. */
inline bool launch_with_threads = false;
template <typename Call> void launch(dim3 grid, dim3 block, Call call)
{
  if (grid.z != 1 || block.y != 1 || block.z != 1) {
    fprintf(stderr, "hip_host: grids of two dimensions and workgroups of one at the most\n");
    abort();
  }
  if (launch_with_threads)
    run_grid_threads(grid, block.x, call);
  else
    run_grid(grid, block.x, call);
}

} // namespace hip_host
#endif
