/*
 * tb_scrambling.hip -- codeword scrambling / unscrambling with the Gold sequence of 38.211 5.2.1 (nr_gold.h) for gfx950:
 * the reference's nr_codeword_scrambling() and nr_codeword_unscrambling() (openair1/PHY/NR_TRANSPORT/nr_scrambling.c:27-78).
 *
 * A workgroup of 256 threads covers NR_SCR_WG_WORDS sequence words.  Each wave first puts its 256 words into LDS: the wave
 * jumps to its first word with one matrix product per set bit of the word index (lane j forms bit j of the product -- a
 * parity -- and a ballot assembles the new registers: lanes 0-31 x1, lanes 32-63 x2), every lane then moves on to its own
 * run of 4 words with at most six products of its own, and walks the run with the 32-bit recurrence.  After a barrier a
 * thread takes one sequence word at a time: 32 input bytes -> one output word, or 32 LLRs negated in place where the
 * sequence has a one.  The sequence costs at most ~1300 VALU instructions per wave for 8192 bits (counted, not measured).
 */
#include <hip/hip_runtime.h>
#define NR_GOLD_TAB_EXTERN
#include "nr_gold_dev.h"
#include "tb_chain.h"

/* out[w] bit k = (in[32w + k] & 1) ^ c(32w + k) for 32w + k < size, 0 behind size (nr_scrambling.c:27-46) */
__global__ void __launch_bounds__(NR_SCR_THREADS) nr_scramble_bits_kernel(const uint8_t *__restrict__ in, uint32_t size, uint32_t c_init,
                                                                          uint32_t *__restrict__ out)
{
  __shared__ uint32_t gold[NR_SCR_WG_WORDS];
  const uint32_t w0 = blockIdx.x * NR_SCR_WG_WORDS;
  nr_gold_fill_wg(gold, c_init, w0);
  __syncthreads();
  const uint32_t nw = (size + 31u) >> 5;
  for (uint32_t k = threadIdx.x; k < NR_SCR_WG_WORDS && w0 + k < nw; k += NR_SCR_THREADS) {
    const uint32_t w = w0 + k, nb = size - 32u * w;
    const uint8_t *p = in + 32 * (size_t)w;
    uint32_t bits = 0;
    if (nb >= 32u && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
      const uint4 v0 = reinterpret_cast<const uint4 *>(p)[0], v1 = reinterpret_cast<const uint4 *>(p)[1];
      const uint32_t d[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
      for (int q = 0; q < 8; q++) /* bit 0 of the four bytes to bits 28..31 by one multiplication (no two products meet) */
        bits |= (((d[q] & 0x01010101u) * 0x10204080u) >> 28) << (4 * q);
    } else {
      const uint32_t n = nb < 32u ? nb : 32u;
      for (uint32_t i = 0; i < n; i++)
        bits |= (uint32_t)(p[i] & 1u) << i;
    }
    bits ^= gold[k];
    if (nb < 32u)
      bits &= (1u << nb) - 1u;
    out[w] = bits;
  }
}

/* llr[i] = -llr[i] (int16, wrapping: -32768 stays) where c(i) = 1, for i < size (nr_scrambling.c:48-78) */
__device__ __forceinline__ uint32_t nr_scr_neg2(uint32_t v, uint32_t s2)
{
  const uint32_t lo = (s2 & 1u) ? ((0u - v) & 0xffffu) : (v & 0xffffu);
  const uint32_t hi = (s2 & 2u) ? ((0u - (v >> 16)) & 0xffffu) : (v >> 16);
  return lo | (hi << 16);
}
__global__ void __launch_bounds__(NR_SCR_THREADS) nr_unscramble_llr_kernel(int16_t *__restrict__ llr, uint32_t size, uint32_t c_init)
{
  __shared__ uint32_t gold[NR_SCR_WG_WORDS];
  const uint32_t w0 = blockIdx.x * NR_SCR_WG_WORDS;
  nr_gold_fill_wg(gold, c_init, w0);
  __syncthreads();
  const uint32_t nw = (size + 31u) >> 5;
  for (uint32_t k = threadIdx.x; k < NR_SCR_WG_WORDS && w0 + k < nw; k += NR_SCR_THREADS) {
    const uint32_t w = w0 + k, nb = size - 32u * w, s = gold[k];
    int16_t *p = llr + 32 * (size_t)w;
    if (nb >= 32u && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
      uint4 *p16 = reinterpret_cast<uint4 *>(p);
      uint4 v[4];
#pragma unroll
      for (int q = 0; q < 4; q++)
        v[q] = p16[q];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t sq = s >> (8 * q);
        v[q].x = nr_scr_neg2(v[q].x, sq);
        v[q].y = nr_scr_neg2(v[q].y, sq >> 2);
        v[q].z = nr_scr_neg2(v[q].z, sq >> 4);
        v[q].w = nr_scr_neg2(v[q].w, sq >> 6);
      }
      if (s)
#pragma unroll
        for (int q = 0; q < 4; q++)
          p16[q] = v[q];
    } else {
      const uint32_t n = nb < 32u ? nb : 32u;
      for (uint32_t i = 0; i < n; i++)
        if ((s >> i) & 1u)
          p[i] = (int16_t)(uint16_t)(0u - (uint32_t)(uint16_t)p[i]);
    }
  }
}

hipError_t nr_launch_scramble_bits(const uint8_t *in, uint32_t size, uint32_t c_init, uint32_t *out, hipStream_t s)
{
  const uint32_t nw = (size + 31u) >> 5;
  if (nw == 0)
    return hipSuccess;
  hipLaunchKernelGGL(nr_scramble_bits_kernel, dim3((nw + NR_SCR_WG_WORDS - 1) / NR_SCR_WG_WORDS), dim3(NR_SCR_THREADS), 0, s, in, size,
                     c_init, out);
  return hipGetLastError();
}
hipError_t nr_launch_unscramble_llr(int16_t *llr, uint32_t size, uint32_t c_init, hipStream_t s)
{
  const uint32_t nw = (size + 31u) >> 5;
  if (nw == 0)
    return hipSuccess;
  hipLaunchKernelGGL(nr_unscramble_llr_kernel, dim3((nw + NR_SCR_WG_WORDS - 1) / NR_SCR_WG_WORDS), dim3(NR_SCR_THREADS), 0, s, llr, size,
                     c_init);
  return hipGetLastError();
}
