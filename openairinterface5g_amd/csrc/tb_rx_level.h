/*
 * tb_rx_level.h -- the channel level launches' workgroup body, shared by the single-layer front (tb_rx_front.hip) and the
 * two-layer MMSE receiver (tb_rx_mmse.hip): workgroup (block b, array a) sums the terms of b's measurement symbol on array a
 * (an antenna, or a (layer, antenna) pair); the block's maximum and the count of arrays done are device-scope atomics, and the
 * last array to arrive writes the block's log2_maxh.  The callers differ in the term of one RE and in the final formula.
 */
#ifndef TB_RX_LEVEL_H
#define TB_RX_LEVEL_H
#include <hip/hip_runtime.h>
#include "nr_rx_front.h"
#include "tb_rx_front.h"

/* term(r): RE r's term of the sum of :454 (int32); final(avgs): log2_maxh from the maximum of the arrays' averages.  n_arr arrays
 * per block, blockIdx.x = b n_arr + a (the caller has derived b and a from it the same way) */
template <typename Term, typename Final>
__device__ __forceinline__ void rx_level_sum(uint32_t b, uint32_t n_arr, uint32_t nb_re, uint32_t len, Term term, Final final, int32_t *mx, int32_t *cnt,
                                             int32_t *out)
{
  __shared__ uint32_t part[NR_RXF_THREADS / 64];
  uint32_t sum = 0; /* wrapping int32 */
  for (uint32_t r = threadIdx.x; r < nb_re; r += NR_RXF_THREADS)
    sum += (uint32_t)term(r);
  for (int off = 32; off; off >>= 1)
    sum += __shfl_xor(sum, off);
  if ((threadIdx.x & 63u) == 0)
    part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x != 0)
    return;
  sum = 0;
  for (int k = 0; k < NR_RXF_THREADS / 64; k++)
    sum += part[k];
  /* mx starts at 0: avgs = max(0, ...) (:1634-1637) */
  __hip_atomic_fetch_max(&mx[b], nr_rxf_level_avg((int32_t)sum, len), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  /* release: the maximum above is out before the count; acquire: the last one sees every maximum before it */
  if (__hip_atomic_fetch_add(&cnt[b], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != (int32_t)n_arr - 1)
    return;
  *out = final(__hip_atomic_load(&mx[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
#endif
