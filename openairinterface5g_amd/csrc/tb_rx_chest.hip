/*
 * tb_rx_chest.hip -- PUSCH DMRS channel estimation on the GPU: one launch per estimator mode over a host-built workgroup table
 * (descriptor, antenna, piece), nothing searched on the device.  A thread owns one output unit of nr_chest.h -- a 4-RE group of
 * the interpolating estimators, a PRB of the averaging ones -- generates the Gold bits of the pilots the unit reads from the
 * workgroup's jumped registers, reads the pilots' REs from the grid (the wrap at fft_size is in nr_chest.h's index), computes in
 * registers and stores its 4 or 12 c16: 16 bytes at a time where the output address allows, word by word otherwise.  The arithmetic
 * is nr_chest.h's alone; the host check form runs the same functions.
 */
#include "tb_rx_chest.h"
#include "nr_chest.h"
#include "nr_gold.h"

namespace {

/* the unit's pilot bits: sequence bit 2 (dmrs_offset + plo) in bit 0.  The workgroup's registers stand at word w0 <= the
 * unit's word; a unit reads at most 10 pilots = 20 bits, so two words hold them */
__device__ __forceinline__ uint64_t chest_bits(const rx_chest_wg &w, uint32_t first_bit)
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
nr_rx_chest_kernel(const rx_chest_wg *__restrict__ wgs, const rx_chest_job *__restrict__ jobs, const uint32_t *__restrict__ rx, uint64_t rx_ant_stride,
                   uint32_t *__restrict__ ch, uint64_t ch_ant_stride, const int32_t *__restrict__ est_delay)
{
  const rx_chest_wg w = wgs[blockIdx.x];
  const rx_chest_job j = jobs[w.job];
  const uint32_t u = w.piece * NR_CHE_THREADS + threadIdx.x;
  if (u >= nr_che_units(MODE, j.rb_size))
    return;
  const uint32_t N = j.fft_size;
  const uint32_t *sym = rx + j.rx_off + (uint64_t)w.ant * rx_ant_stride;
  uint32_t *dst = ch + j.ch_off + (uint64_t)w.ant * ch_ant_stride + (uint64_t)u * nr_che_unit_res(MODE);
  const uint64_t bits = chest_bits(w, 2u * (j.dmrs_offset + nr_che_unit_first_pilot(MODE, u)));
  const bool aligned = (reinterpret_cast<uintptr_t>(dst) & 15u) == 0;
  if constexpr (MODE == NR_CHE_TYPE1_INTERP || MODE == NR_CHE_TYPE2_INTERP) {
    const int32_t d = est_delay ? est_delay[j.delay_off + w.ant] : 0;
    const uint32_t *inv = j.tab + (uint64_t)nr_che_inv_delay_idx(d) * N;
    uint32_t o[4];
    if constexpr (MODE == NR_CHE_TYPE1_INTERP)
      nr_che_t1_interp(sym, N, j.start_re, j.rb_size, j.port, j.dmrs_offset, bits, j.tab + (uint64_t)nr_che_delay_idx(d) * N, inv, u, o);
    else
      nr_che_t2_interp(sym, N, j.start_re, j.port, j.dmrs_offset, bits, inv, u, o);
    if (aligned)
      *reinterpret_cast<uint4 *>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
    else {
#pragma unroll
      for (int k = 0; k < 4; k++)
        dst[k] = o[k];
    }
  } else {
    const uint32_t v = nr_che_avg(MODE, sym, N, j.start_re, j.port, j.dmrs_offset, bits, u);
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

} // namespace

hipError_t nr_launch_rx_chest(uint32_t mode, const rx_chest_wg *wgs, uint32_t n_wg, const rx_chest_job *jobs, const uint32_t *rx, uint64_t rx_ant_stride,
                              uint32_t *ch, uint64_t ch_ant_stride, const int32_t *est_delay, hipStream_t s)
{
  if (n_wg == 0)
    return hipSuccess;
#define CHE_LAUNCH(M) \
  hipLaunchKernelGGL(nr_rx_chest_kernel<M>, dim3(n_wg), dim3(NR_CHE_THREADS), 0, s, wgs, jobs, rx, rx_ant_stride, ch, ch_ant_stride, est_delay)
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
