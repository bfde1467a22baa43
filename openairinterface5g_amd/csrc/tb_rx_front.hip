/*
 * tb_rx_front.hip -- the UL receive front for gfx950 (nr_rx_front.h): the reference's nr_ulsch_channel_compensation() for one
 * layer (openair1/PHY/NR_TRANSPORT/nr_ulsch_demodulation.c:468-577) over every OFDM symbol of every transport block of a slot in
 * one launch, writing straight into the planar symbol records nrLDPC_hip_ulsch_decode_symbols reads, and the channel level of the
 * blocks' first symbols with the shift log2_maxh it gives (:434-466, :1612-1647).
 *
 * Compensation is memory bound by construction: 8 n_rx bytes in and 2 Qm bytes out per RE, a handful of integer operations
 * between them.  A thread takes NR_RXF_GROUP consecutive REs; the groups of a segment are laid so that plane 0's stores are 16-byte
 * aligned (the segment's first RE rarely is: nb_re per symbol is 12, 6 or 8 per RB), with a short head and tail stored word by word.
 */
#include <hip/hip_runtime.h>
#include "nr_rx_front.h"
#include "tb_rx_front.h"

typedef uint32_t rxf_u32x4 __attribute__((ext_vector_type(4)));

/* 16 bytes at a 4-byte aligned address (the inputs' offsets and strides are the caller's; planes 1.. sit `plane` words behind
 * plane 0, any remainder mod 4) */
__device__ __forceinline__ void rxf_load4(uint32_t (&w)[NR_RXF_GROUP], const uint32_t *p)
{
  rxf_u32x4 v;
  __builtin_memcpy(&v, p, sizeof v);
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}
__device__ __forceinline__ void rxf_store4(uint32_t *p, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
  const rxf_u32x4 v = {a, b, c, d};
  __builtin_memcpy(p, &v, sizeof v);
}

/* NRX > 0: that many antennas, every load issued before the first use; NRX = 0: n_rx antennas one after another */
template <int NRX>
__global__ void __launch_bounds__(NR_RXF_THREADS)
nr_rx_compensation_kernel(const rx_front_wg *__restrict__ wgs, const rx_front_seg_job *__restrict__ jobs, const uint32_t *__restrict__ rx,
                          const uint32_t *__restrict__ ch, uint32_t n_rx, uint64_t ant_stride, const int32_t *__restrict__ shift,
                          uint32_t *__restrict__ rec)
{
  const rx_front_wg w = wgs[blockIdx.x];
  const rx_front_seg_job j = jobs[w.seg];
  const int32_t nb_re = (int32_t)j.nb_re;
  const int32_t r0 = (int32_t)((w.piece * NR_RXF_THREADS + threadIdx.x) * NR_RXF_GROUP) - (int32_t)j.phase;
  if (r0 >= nb_re)
    return;
  const uint32_t s = nr_rxf_shift(shift[j.tb]), np = j.Qm >> 1;
  const int32_t amp[3] = {nr_rxf_amp(j.Qm, 0), nr_rxf_amp(j.Qm, 1), nr_rxf_amp(j.Qm, 2)};
  const uint32_t *y0 = rx + j.rx_off, *h0 = ch + j.ch_off;
  uint32_t *o = rec + j.out_off;
  const uint32_t nrx = NRX ? (uint32_t)NRX : n_rx;

  if (r0 >= 0 && r0 + NR_RXF_GROUP <= nb_re) {
    nr_rxf_acc_t acc[NR_RXF_GROUP] = {};
    if constexpr (NRX > 0) {
      uint32_t hv[NRX][NR_RXF_GROUP], yv[NRX][NR_RXF_GROUP];
#pragma unroll
      for (int a = 0; a < NRX; a++) {
        rxf_load4(hv[a], h0 + (size_t)a * ant_stride + r0);
        rxf_load4(yv[a], y0 + (size_t)a * ant_stride + r0);
      }
#pragma unroll
      for (int a = 0; a < NRX; a++)
#pragma unroll
        for (int u = 0; u < NR_RXF_GROUP; u++)
          nr_rxf_mac(&acc[u], hv[a][u], yv[a][u], s, amp);
    } else {
      for (uint32_t a = 0; a < nrx; a++) {
        uint32_t hv[NR_RXF_GROUP], yv[NR_RXF_GROUP];
        rxf_load4(hv, h0 + (size_t)a * ant_stride + r0);
        rxf_load4(yv, y0 + (size_t)a * ant_stride + r0);
#pragma unroll
        for (int u = 0; u < NR_RXF_GROUP; u++)
          nr_rxf_mac(&acc[u], hv[u], yv[u], s, amp);
      }
    }
    /* plane 0 at r0 is 16-byte aligned: that is what `phase` was chosen for */
    *reinterpret_cast<rxf_u32x4 *>(o + r0) = (rxf_u32x4){acc[0].w[0], acc[1].w[0], acc[2].w[0], acc[3].w[0]};
#pragma unroll
    for (uint32_t k = 1; k < 4; k++)
      if (k < np)
        rxf_store4(o + (size_t)k * j.plane + r0, acc[0].w[k], acc[1].w[k], acc[2].w[k], acc[3].w[k]);
    return;
  }
  /* head (REs before the first aligned group) and tail */
  const int32_t hi = r0 + NR_RXF_GROUP < nb_re ? r0 + NR_RXF_GROUP : nb_re;
  for (int32_t r = r0 < 0 ? 0 : r0; r < hi; r++) {
    nr_rxf_acc_t acc = {};
    for (uint32_t a = 0; a < nrx; a++)
      nr_rxf_mac(&acc, h0[(size_t)a * ant_stride + r], y0[(size_t)a * ant_stride + r], s, amp);
    o[r] = acc.w[0];
#pragma unroll
    for (uint32_t k = 1; k < 4; k++)
      if (k < np)
        o[(size_t)k * j.plane + r] = acc.w[k];
  }
}

hipError_t nr_launch_rx_compensation(const rx_front_wg *wgs, uint32_t n_wg, const rx_front_seg_job *jobs, const uint32_t *rx, const uint32_t *ch,
                                     uint32_t n_rx, uint64_t ant_stride, const int32_t *shift, uint32_t *rec, hipStream_t s)
{
  if (n_wg == 0)
    return hipSuccess;
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return hipErrorInvalidValue;
#define RXF_LAUNCH(N) hipLaunchKernelGGL(nr_rx_compensation_kernel<N>, dim3(n_wg), dim3(NR_RXF_THREADS), 0, s, wgs, jobs, rx, ch, n_rx, ant_stride, shift, rec)
  switch (n_rx) {
    case 1: RXF_LAUNCH(1); break;
    case 2: RXF_LAUNCH(2); break;
    case 4: RXF_LAUNCH(4); break;
    case 8: RXF_LAUNCH(8); break;
    default: RXF_LAUNCH(0); break;
  }
#undef RXF_LAUNCH
  return hipGetLastError();
}

/* ---- channel level: workgroup (block b, antenna a) sums the terms of b's measurement symbol on antenna a; the block's maximum
 * and the count of antennas done are device-scope atomics, and the last antenna to arrive writes log2_maxh ---- */
__global__ void __launch_bounds__(NR_RXF_THREADS)
nr_rx_level_kernel(const rx_front_lvl_job *__restrict__ jobs, const uint32_t *__restrict__ ch, uint32_t n_rx, uint64_t ant_stride, int32_t *mx,
                   int32_t *cnt, int32_t *__restrict__ log2_maxh)
{
  __shared__ uint32_t part[NR_RXF_THREADS / 64];
  const uint32_t b = blockIdx.x / n_rx, a = blockIdx.x % n_rx;
  const rx_front_lvl_job j = jobs[b];
  const uint32_t len = nr_rxf_level_len(j.nb_re), x = (uint32_t)nr_rxf_factor2(len);
  const uint32_t *h = ch + j.ch_off + (size_t)a * ant_stride;
  uint32_t sum = 0; /* wrapping int32 */
  for (uint32_t r = threadIdx.x; r < j.nb_re; r += NR_RXF_THREADS)
    sum += (uint32_t)nr_rxf_level_term(h[r], x);
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
  if (__hip_atomic_fetch_add(&cnt[b], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != (int32_t)n_rx - 1)
    return;
  log2_maxh[j.tb] = nr_rxf_log2_maxh(__hip_atomic_load(&mx[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), n_rx);
}

hipError_t nr_launch_rx_level(const rx_front_lvl_job *jobs, uint32_t n_tb, const uint32_t *ch, uint32_t n_rx, uint64_t ant_stride, int32_t *state,
                              int32_t *log2_maxh, hipStream_t s)
{
  if (n_tb == 0)
    return hipSuccess;
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(nr_rx_level_kernel, dim3(n_tb * n_rx), dim3(NR_RXF_THREADS), 0, s, jobs, ch, n_rx, ant_stride, state, state + n_tb, log2_maxh);
  return hipGetLastError();
}
