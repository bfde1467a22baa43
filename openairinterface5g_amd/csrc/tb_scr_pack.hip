/*
 * tb_scr_pack.hip -- the packed, scrambled output of nrLDPC_hip_dlsch_encode_scrambled for gfx950: every transport block of
 * the call in one launch, from the chain's bit-per-byte output in scratch to ceil(G/32) words of bits XOR the sequence
 * (38.211 7.3.1.1; nr_scrambling.c:27-46) at the block's place in the caller's array.  The same work as
 * nr_scramble_bits_kernel (tb_scrambling.hip) per block; its own translation unit, so that the standalone kernels keep theirs.
 */
#include <hip/hip_runtime.h>
#include "nr_gold_dev.h"
#include "tb_chain.h"

/* out[w] bit k = (in[32w + k] & 1) ^ c(32w + k) for 32w + k < size, 0 behind size (nr_scrambling.c:27-46): the words
 * w0 .. w0 + NR_SCR_WG_WORDS - 1 */
__device__ __forceinline__ void nr_scramble_bits_wg(const uint8_t *__restrict__ in, uint32_t size, uint32_t c_init, uint32_t *__restrict__ out,
                                                    uint32_t w0, uint32_t *gold)
{
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
/* the same for every transport block of an encode call at once: blockIdx.y = block, blockIdx.x = its piece of words */
__global__ void __launch_bounds__(NR_SCR_THREADS) nr_scramble_bits_tb_kernel(const tb_scr_tb_job *__restrict__ jobs, const uint8_t *__restrict__ in,
                                                                             uint8_t *__restrict__ out)
{
  __shared__ uint32_t gold[NR_SCR_WG_WORDS];
  const tb_scr_tb_job j = jobs[blockIdx.y];
  const uint32_t w0 = blockIdx.x * NR_SCR_WG_WORDS;
  if (w0 >= (j.G + 31u) >> 5)
    return;
  nr_scramble_bits_wg(in + j.in_off, j.G, j.c_init, reinterpret_cast<uint32_t *>(out + j.out_off), w0, gold);
}

hipError_t nr_launch_scramble_bits_tb(const tb_scr_tb_job *jobs, uint32_t n_tb, uint32_t max_g, const uint8_t *in, uint8_t *out, hipStream_t s)
{
  const uint32_t nw = (max_g + 31u) >> 5;
  if (nw == 0 || n_tb == 0)
    return hipSuccess;
  hipLaunchKernelGGL(nr_scramble_bits_tb_kernel, dim3((nw + NR_SCR_WG_WORDS - 1) / NR_SCR_WG_WORDS, n_tb), dim3(NR_SCR_THREADS), 0, s, jobs,
                     in, out);
  return hipGetLastError();
}
