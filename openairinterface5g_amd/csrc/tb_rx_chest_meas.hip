/*
 * tb_rx_chest_meas.hip -- PUSCH DMRS channel estimation that also forms the reference's max_ch and nvar, and the time average of
 * the estimates over an allocation's DMRS symbols.
 *
 * Estimation: the workgroup table, the unit decomposition and the stores are tb_rx_chest.hip's, one launch per estimator mode.
 * A thread computes its unit's estimates and, from the same registers, the unit's share of the measurements (nr_chest.h: its pair's
 * int32 LS maximum and four noise terms; the TYPE2 pair it owns; an interior PRB's maximum).  The shares are reduced in the wave
 * with __shfl_xor and across the workgroup's four waves through LDS; thread 0 then issues one device-scope fetch_max on the block's
 * maximum and, for the interpolating modes, one 64-bit fetch_add on the descriptor's noise_amp2.  Integer maximum and integer sum
 * do not depend on the order.  A one-thread-per-block kernel behind the last launch divides each descriptor's sum by its
 * nest_count, sums the block's quotients as uint32, divides by nvar_div and stores max_ch[tb] and nvar[tb].  The accumulators
 * arrive as zeros with the call's tables, so every call starts from its own.
 *
 * Time average: a thread owns four consecutive c16 of one plane of one descriptor, reads them from each DMRS symbol and writes
 * the first symbol's: 16 bytes at a time where that symbol's address allows, word by word otherwise, each symbol by its own
 * alignment.  The arithmetic is nr_chest.h's alone; the host check forms run the same functions.
 */
#include "tb_rx_chest_meas.h"
#include "nr_chest.h"
#include "nr_gold.h"

namespace {

#define NR_CHE_WAVES (NR_CHE_THREADS / 64)

/* the unit's pilot bits from the workgroup's jumped registers (as tb_rx_chest.hip's chest_bits) */
__device__ __forceinline__ uint64_t chest_meas_bits(const rx_chest_wg &w, uint32_t first_bit)
{
  uint32_t a = w.x1, b = w.x2;
  for (uint32_t n = (first_bit >> 5) - w.w0; n != 0; n--) {
    a = nr_gold_step1(a);
    b = nr_gold_step2(b);
  }
  const uint64_t lo = a ^ b, hi = nr_gold_step1(a) ^ nr_gold_step2(b);
  return (lo | (hi << 32)) >> (first_bit & 31u);
}

template <uint32_t MODE>
__global__ void __launch_bounds__(NR_CHE_THREADS)
nr_rx_chest_meas_kernel(const rx_chest_wg *__restrict__ wgs, const rx_chest_job *__restrict__ jobs, const rx_chest_meas_job *__restrict__ mjobs,
                        const uint32_t *__restrict__ rx, uint64_t rx_ant_stride, uint32_t *__restrict__ ch, uint64_t ch_ant_stride,
                        const int32_t *__restrict__ est_delay, int32_t *mx, uint64_t *noise)
{
  constexpr bool INTERP = MODE == NR_CHE_TYPE1_INTERP || MODE == NR_CHE_TYPE2_INTERP;
  __shared__ int32_t part_max[NR_CHE_WAVES];
  __shared__ uint64_t part_noise[NR_CHE_WAVES];
  const rx_chest_wg w = wgs[blockIdx.x];
  const rx_chest_job j = jobs[w.job];
  const uint32_t u = w.piece * NR_CHE_THREADS + threadIdx.x;
  int32_t m = 0;
  uint64_t ns = 0;
  /* a thread behind the last unit computes nothing and takes part in the reduction with zeros */
  if (u < nr_che_units(MODE, j.rb_size)) {
    const uint32_t N = j.fft_size;
    const uint32_t *sym = rx + j.rx_off + (uint64_t)w.ant * rx_ant_stride;
    uint32_t *dst = ch + j.ch_off + (uint64_t)w.ant * ch_ant_stride + (uint64_t)u * nr_che_unit_res(MODE);
    const uint64_t bits = chest_meas_bits(w, 2u * (j.dmrs_offset + nr_che_unit_first_pilot(MODE, u)));
    const bool aligned = (reinterpret_cast<uintptr_t>(dst) & 15u) == 0;
    if constexpr (INTERP) {
      const int32_t d = est_delay ? est_delay[j.delay_off + w.ant] : 0;
      const uint32_t *inv = j.tab + (uint64_t)nr_che_inv_delay_idx(d) * N;
      uint32_t o[4];
      if constexpr (MODE == NR_CHE_TYPE1_INTERP) {
        nr_che_t1_interp(sym, N, j.start_re, j.rb_size, j.port, j.dmrs_offset, bits, j.tab + (uint64_t)nr_che_delay_idx(d) * N, inv, u, o);
        ns = nr_che_t1_meas(sym, N, j.start_re, j.port, j.dmrs_offset, bits, u, o, &m);
      } else {
        nr_che_t2_interp(sym, N, j.start_re, j.port, j.dmrs_offset, bits, inv, u, o);
        ns = nr_che_t2_meas(sym, N, j.start_re, j.port, j.dmrs_offset, bits, u, &m);
      }
      if (aligned)
        *reinterpret_cast<uint4 *>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
      else {
#pragma unroll
        for (int k = 0; k < 4; k++)
          dst[k] = o[k];
      }
    } else {
      const uint32_t v = nr_che_avg(MODE, sym, N, j.start_re, j.port, j.dmrs_offset, bits, u);
      m = nr_che_avg_meas(j.rb_size, u, v, 0);
      /* 12 equal words: the words up to the first 16-byte boundary, whole 16-byte stores, the rest */
      const uint32_t head = aligned ? 0u : (uint32_t)((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) >> 2);
      uint32_t k = 0;
      for (; k < head; k++)
        dst[k] = v;
      for (; k + 4u <= 12u; k += 4u)
        *reinterpret_cast<uint4 *>(dst + k) = make_uint4(v, v, v, v);
      for (; k < 12u; k++)
        dst[k] = v;
    }
  }
  for (int off = 32; off; off >>= 1) {
    const int32_t o = __shfl_xor(m, off);
    m = o > m ? o : m;
    if constexpr (INTERP)
      ns += __shfl_xor(ns, off);
  }
  if ((threadIdx.x & 63u) == 0) {
    part_max[threadIdx.x >> 6] = m;
    if constexpr (INTERP)
      part_noise[threadIdx.x >> 6] = ns;
  }
  __syncthreads();
  if (threadIdx.x != 0)
    return;
  for (int k = 1; k < NR_CHE_WAVES; k++) {
    m = part_max[k] > m ? part_max[k] : m;
    if constexpr (INTERP)
      ns += part_noise[k];
  }
  /* the accumulators start at 0 and every share is >= 0: a zero share changes nothing */
  if (m != 0)
    __hip_atomic_fetch_max(&mx[mjobs[w.job].tb], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if constexpr (INTERP)
    if (ns != 0)
      __hip_atomic_fetch_add(&noise[w.job], ns, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* the launches before it on the stream are complete: plain loads see their atomics' results */
__global__ void __launch_bounds__(64)
nr_rx_chest_finish_kernel(const rx_chest_meas_tb *__restrict__ tbs, uint32_t n_tb, const uint32_t *__restrict__ list,
                          const rx_chest_meas_job *__restrict__ mjobs, const int32_t *__restrict__ mx, const uint64_t *__restrict__ noise,
                          int32_t *__restrict__ max_ch, uint32_t *__restrict__ nvar)
{
  const uint32_t tb = blockIdx.x * 64u + threadIdx.x;
  if (tb >= n_tb)
    return;
  const rx_chest_meas_tb t = tbs[tb];
  uint32_t sum = 0; /* wraps as the reference's uint32 (nr_ulsch_demodulation.c:1471, :1491) */
  for (uint32_t k = 0; k < t.count; k++) {
    const uint32_t d = list[t.first + k];
    sum += nr_che_nvar_tmp(noise[d], mjobs[d].nest_count);
  }
  max_ch[tb] = mx[tb];
  nvar[tb] = sum / t.div;
}

/* four c16 at p: one 16-byte access where p allows */
__device__ __forceinline__ void avg_load4(const uint32_t *p, uint32_t *v)
{
  if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
    const uint4 q = *reinterpret_cast<const uint4 *>(p);
    v[0] = q.x;
    v[1] = q.y;
    v[2] = q.z;
    v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++)
      v[k] = p[k];
  }
}

__global__ void __launch_bounds__(NR_CHE_THREADS)
nr_rx_chest_time_avg_kernel(const rx_chest_avg_wg *__restrict__ wgs, const rx_chest_avg_job *__restrict__ jobs, uint32_t *ch, uint64_t ch_ant_stride)
{
  const rx_chest_avg_wg w = wgs[blockIdx.x];
  const rx_chest_avg_job *j = jobs + w.job; /* ch_off[s] is read where it lies: no register array indexed by s */
  const uint32_t u = w.piece * NR_CHE_THREADS + threadIdx.x, n_sym = j->n_sym;
  if (u >= 3u * j->rb_size)
    return;
  uint32_t *plane = ch + (uint64_t)w.plane * ch_ant_stride + 4u * (uint64_t)u;
  uint32_t *dst = plane + j->ch_off[0];
  uint32_t acc[4];
  avg_load4(dst, acc);
  for (uint32_t s = 1; s < n_sym; s++) {
    uint32_t x[4];
    avg_load4(plane + j->ch_off[s], x);
#pragma unroll
    for (int k = 0; k < 4; k++)
      acc[k] = nr_che_tavg_add(acc[k], x[k]);
  }
#pragma unroll
  for (int k = 0; k < 4; k++)
    acc[k] = nr_che_tavg_div(acc[k], n_sym);
  if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0)
    *reinterpret_cast<uint4 *>(dst) = make_uint4(acc[0], acc[1], acc[2], acc[3]);
  else {
#pragma unroll
    for (int k = 0; k < 4; k++)
      dst[k] = acc[k];
  }
}

} // namespace

hipError_t nr_launch_rx_chest_meas(uint32_t mode, const rx_chest_wg *wgs, uint32_t n_wg, const rx_chest_job *jobs, const rx_chest_meas_job *mjobs,
                                   const uint32_t *rx, uint64_t rx_ant_stride, uint32_t *ch, uint64_t ch_ant_stride, const int32_t *est_delay, int32_t *mx,
                                   uint64_t *noise, hipStream_t s)
{
  if (n_wg == 0)
    return hipSuccess;
#define CHE_LAUNCH(M) \
  hipLaunchKernelGGL(nr_rx_chest_meas_kernel<M>, dim3(n_wg), dim3(NR_CHE_THREADS), 0, s, wgs, jobs, mjobs, rx, rx_ant_stride, ch, ch_ant_stride, est_delay, \
                     mx, noise)
  switch (mode) {
    case NR_CHE_TYPE1_INTERP: CHE_LAUNCH(NR_CHE_TYPE1_INTERP); break;
    case NR_CHE_TYPE2_INTERP: CHE_LAUNCH(NR_CHE_TYPE2_INTERP); break;
    case NR_CHE_TYPE1_AVG: CHE_LAUNCH(NR_CHE_TYPE1_AVG); break;
    case NR_CHE_TYPE2_AVG: CHE_LAUNCH(NR_CHE_TYPE2_AVG); break;
    default: return hipErrorInvalidValue;
  }
#undef CHE_LAUNCH
  return hipGetLastError();
}

hipError_t nr_launch_rx_chest_finish(const rx_chest_meas_tb *tbs, uint32_t n_tb, const uint32_t *list, const rx_chest_meas_job *mjobs, const int32_t *mx,
                                     const uint64_t *noise, int32_t *max_ch, uint32_t *nvar, hipStream_t s)
{
  if (n_tb == 0)
    return hipSuccess;
  hipLaunchKernelGGL(nr_rx_chest_finish_kernel, dim3((n_tb + 63u) / 64u), dim3(64), 0, s, tbs, n_tb, list, mjobs, mx, noise, max_ch, nvar);
  return hipGetLastError();
}

hipError_t nr_launch_rx_chest_time_avg(const rx_chest_avg_wg *wgs, uint32_t n_wg, const rx_chest_avg_job *jobs, uint32_t *ch, uint64_t ch_ant_stride,
                                       hipStream_t s)
{
  if (n_wg == 0)
    return hipSuccess;
  hipLaunchKernelGGL(nr_rx_chest_time_avg_kernel, dim3(n_wg), dim3(NR_CHE_THREADS), 0, s, wgs, jobs, ch, ch_ant_stride);
  return hipGetLastError();
}
