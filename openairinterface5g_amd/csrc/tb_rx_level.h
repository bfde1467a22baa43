/*
 * tb_rx_level.h -- the channel level launches' workgroup body, shared by the single-layer front (tb_rx_front.hip) and the
 * two-layer receivers (tb_rx_mmse.hip, tb_rx_ml.hip): workgroup (block b, array a) sums the terms of b's measurement symbol on array a
 * (an antenna, or a (layer, antenna) pair); the block's maximum and the count of arrays done are device-scope atomics, and the
 * last array to arrive writes the block's log2_maxh.  The callers differ in the term of one RE and in the final formula; the two
 * two-layer receivers, which share the term, differ in the formula alone (rx2_level_body).
 */
#ifndef TB_RX_LEVEL_H
#define TB_RX_LEVEL_H
#include <hip/hip_runtime.h>
#include "nr_rx_front.h"
#include "nr_rx_grid.h"
#include "nr_rx_mmse.h"
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

/* the level kernels of the two-layer receivers (tb_rx_mmse.hip, tb_rx_ml.hip): the sum over the n_pair = 2 n_rx (layer, antenna)
 * pairs with the MMSE level's term, scaled by shift_ch_ext of max_ch[tb]; the receivers differ in final(avgs) */
template <typename Final>
__device__ __forceinline__ void rx2_level_body(const rx_front_grid_lvl_job *__restrict__ jobs, const uint32_t *__restrict__ ch, uint32_t n_pair,
                                               uint64_t ant_stride, const int32_t *__restrict__ max_ch, Final final, int32_t *mx, int32_t *cnt,
                                               int32_t *__restrict__ log2_maxh)
{
  const uint32_t b = blockIdx.x / n_pair, a = blockIdx.x % n_pair;
  const rx_front_grid_lvl_job j = jobs[b];
  const uint32_t len = nr_rxf_level_len(j.nb_re), x = (uint32_t)nr_rxf_factor2(len), sce = nr_rxm_shift_ch_ext(max_ch[j.tb]);
  const uint32_t *h = ch + j.ch_off + (size_t)a * ant_stride;
  rx_level_sum(b, n_pair, j.nb_re, len, [&](uint32_t r) { return nr_rxm_level_term(h[nr_rxg_p(j.pattern, r)], x, sce); }, final, mx, cnt,
               &log2_maxh[j.tb]);
}
#endif
