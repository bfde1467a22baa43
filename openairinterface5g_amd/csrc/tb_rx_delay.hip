/*
 * tb_rx_delay.hip -- the PUSCH delay search on the GPU (nr_delay.h): one workgroup per (descriptor, antenna) of the interpolating
 * estimators, over a host-built workgroup table with jumped Gold registers, one launch per fft_size so that a launch's LDS is its
 * own transform's.  A workgroup's threads compute the LS values of the symbol's 4-RE groups into LDS as complex fp32 (8 fft_size
 * bytes: 64 KB at 8192), zero the rest, run the in-place stages of nr_delay.h with a barrier behind each -- a stage's butterflies
 * touch disjoint entries, butterfly b goes to thread b mod 1024 -- and reduce |y|^2 to the largest sample and the lowest position
 * that has it: per thread, by shuffles in the wave, across the sixteen waves through the first entries of the same LDS buffer.
 *
 * The running maximum over a descriptor's antennas is not formed here: no workgroup waits for another inside a launch.  Every
 * workgroup stores (peak, position) to the call's results, and a second launch, one thread per descriptor, walks the antennas in
 * order and writes est_delay and peak.  The arithmetic is nr_delay.h's alone; the host check form runs the
 * same functions.
 */
#include "tb_rx_delay.h"
#include "nr_gold.h"

namespace {

#define NR_DLY_WAVES (NR_DLY_THREADS / 64)

__global__ void __launch_bounds__(NR_DLY_THREADS)
nr_rx_delay_search_kernel(const rx_delay_wg *__restrict__ wgs, const rx_delay_job *__restrict__ jobs, const uint32_t *__restrict__ rx, uint64_t rx_ant_stride,
                          rx_delay_res *__restrict__ res)
{
  NR_DLY_DYNAMIC_LDS(nr_dly_c, buf);
  const rx_delay_wg w = wgs[blockIdx.x];
  const rx_delay_job j = jobs[w.job];
  const uint32_t N = j.fft_size, tid = threadIdx.x;
  const nr_dly_c *tw = j.tw;
  const uint32_t *one = reinterpret_cast<const uint32_t *>(tw + N);
  const uint32_t *sym = rx + j.rx_off + (uint64_t)w.ant * rx_ant_stride;

  /* the LS values.  A thread's groups ascend, so its Gold registers only ever step forward from the workgroup's */
  uint32_t x1 = w.x1, x2 = w.x2, word = w.w0;
  for (uint32_t g = tid; g < 3u * j.rb_size; g += NR_DLY_THREADS) {
    const uint32_t first_bit = 2u * (j.dmrs_offset + nr_dly_first_pilot(j.mode, g));
    for (; word < (first_bit >> 5); word++) {
      x1 = nr_gold_step1(x1);
      x2 = nr_gold_step2(x2);
    }
    const uint64_t lo = x1 ^ x2, hi = nr_gold_step1(x1) ^ nr_gold_step2(x2);
    uint32_t o[4];
    nr_dly_ls4(j.mode, sym, N, j.start_re, j.port, j.dmrs_offset, (lo | (hi << 32)) >> (first_bit & 31u), one, g, o);
#pragma unroll
    for (int k = 0; k < 4; k++)
      buf[4u * g + k] = nr_dly_from_c16(o[k]);
  }
  for (uint32_t k = 12u * j.rb_size + tid; k < N; k += NR_DLY_THREADS) {
    nr_dly_c z;
    z.r = 0.0f;
    z.i = 0.0f;
    buf[k] = z;
  }
  __syncthreads();

  const uint32_t M = nr_dly_pow2(N), lm = nr_dly_log2(M);
  if (nr_dly_radix3(N)) {
    for (uint32_t k = tid; k < M; k += NR_DLY_THREADS)
      nr_dly_r3(buf, tw, M, k);
    __syncthreads();
  }
  for (uint32_t ll = lm; ll >= 1u; ll--) {
    for (uint32_t b = tid; b < N / 2u; b += NR_DLY_THREADS)
      nr_dly_r2(buf, tw, N, ll, b);
    __syncthreads();
  }

  float best = 0.0f;
  uint32_t best_n = 0;
  for (uint32_t p = tid; p < N; p += NR_DLY_THREADS) {
    const float v = nr_dly_power(buf[p]);
    const uint32_t n = nr_dly_index(N, lm, p);
    if (nr_dly_better(v, n, best, best_n)) {
      best = v;
      best_n = n;
    }
  }
  for (int off = 32; off; off >>= 1) {
    const float v = __shfl_xor(best, off);
    const uint32_t n = __shfl_xor(best_n, off);
    if (nr_dly_better(v, n, best, best_n)) {
      best = v;
      best_n = n;
    }
  }
  __syncthreads(); /* every thread has read its samples: the buffer's first entries take the waves' results */
  uint32_t *part = reinterpret_cast<uint32_t *>(buf);
  if ((tid & 63u) == 0) {
    memcpy(&part[2u * (tid >> 6)], &best, 4);
    part[2u * (tid >> 6) + 1u] = best_n;
  }
  __syncthreads();
  if (tid != 0)
    return;
  for (uint32_t k = 1; k < NR_DLY_WAVES; k++) {
    float v;
    memcpy(&v, &part[2u * k], 4);
    if (nr_dly_better(v, part[2u * k + 1u], best, best_n)) {
      best = v;
      best_n = part[2u * k + 1u];
    }
  }
  rx_delay_res r;
  r.peak = best;
  r.pos = best_n;
  res[blockIdx.x] = r;
}

/* the launches before it on the stream are complete: plain loads see their results */
__global__ void __launch_bounds__(64)
nr_rx_delay_combine_kernel(const rx_delay_job *__restrict__ jobs, uint32_t n_job, uint32_t n_rx, uint32_t flags, const rx_delay_res *__restrict__ res,
                           int32_t *__restrict__ est_delay, float *__restrict__ peak)
{
  const uint32_t d = blockIdx.x * 64u + threadIdx.x;
  if (d >= n_job)
    return;
  const rx_delay_job j = jobs[d];
  float best = 0.0f;
  uint32_t pos = 0;
  for (uint32_t a = 0; a < n_rx; a++) {
    if (!nr_che_is_avg(j.mode)) {
      const rx_delay_res r = res[j.first_res + a];
      if (flags == NR_DLY_PER_ANTENNA || r.peak > best) {
        best = r.peak;
        pos = r.pos;
      }
    }
    est_delay[j.delay_off + a] = nr_dly_fold(j.fft_size, pos);
    if (peak)
      peak[j.delay_off + a] = best;
  }
}

} // namespace

hipError_t nr_launch_rx_delay_search(uint32_t fft_size, const rx_delay_wg *wgs, uint32_t n_wg, const rx_delay_job *jobs, const uint32_t *rx,
                                     uint64_t rx_ant_stride, rx_delay_res *res, hipStream_t s)
{
  if (n_wg == 0)
    return hipSuccess;
  if (fft_size < 2u * NR_DLY_WAVES || fft_size > 8192u)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(nr_rx_delay_search_kernel, dim3(n_wg), dim3(NR_DLY_THREADS), (size_t)fft_size * sizeof(nr_dly_c), s, wgs, jobs, rx, rx_ant_stride, res);
  return hipGetLastError();
}

hipError_t nr_launch_rx_delay_combine(const rx_delay_job *jobs, uint32_t n_job, uint32_t n_rx, uint32_t flags, const rx_delay_res *res, int32_t *est_delay,
                                      float *peak, hipStream_t s)
{
  if (n_job == 0)
    return hipSuccess;
  hipLaunchKernelGGL(nr_rx_delay_combine_kernel, dim3((n_job + 63u) / 64u), dim3(64), 0, s, jobs, n_job, n_rx, flags, res, est_delay, peak);
  return hipGetLastError();
}
