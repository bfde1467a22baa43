/*
 * tb_qam.hip -- modulation mapping and soft demapping for gfx950 (nr_qam.h): the reference's nr_modulation() (openair1/PHY/
 * MODULATION/nr_modulation.c:115-244) and nr_ulsch_compute_llr() for one stream (openair1/PHY/NR_TRANSPORT/
 * nr_ulsch_llr_computation.c:316-363) as standalone passes.  Both are memory bound on their output: a thread takes
 * NR_QAM_GROUP consecutive symbols / REs and writes them with 16-byte stores where the buffer allows it.  Also here:
 * nr_layer_mapping() for one codeword (nr_modulation.c:246-270) as a standalone pass, and the symbol encode's three-kernel
 * path (scrambling + mapping + layer mapping of the chain's bit-per-byte output, every transport block in one launch).
 */
#include <hip/hip_runtime.h>
#include "nr_gold_dev.h"
#include "nr_qam.h"
#include "tb_chain.h"
#include "tb_tx_sym.h"

static __constant__ nr_qam_tables_t nr_qam_tab_dev = nr_qam_make_tables();

#define NR_QAM_THREADS 256
#define NR_QAM_GROUP 4 /* symbols / REs per thread: one 16-byte store of points, Qm/2 16-byte stores of LLRs */

typedef uint32_t qam_u32x4 __attribute__((ext_vector_type(4)));

/* point i (i < n_sym) from bits i Qm .. i Qm + Qm - 1 of the packed words in[] (ceil(n_sym Qm / 32) of them) */
template <int QM> __device__ __forceinline__ uint32_t nr_qam_map_one(const uint32_t *__restrict__ in, uint32_t nw, uint32_t i)
{
  const uint32_t b = i * (uint32_t)QM, k = b >> 5, s = b & 31u;
  uint32_t x = in[k] >> s;
  if (s + QM > 32u && k + 1u < nw) /* the symbol straddles two words (64QAM) */
    x |= in[k + 1u] << (32u - s);
  return nr_qam_tab_dev.pt[nr_qam_table_off(QM) + (x & ((1u << QM) - 1u))];
}

template <int QM>
__global__ void __launch_bounds__(NR_QAM_THREADS) nr_modulation_kernel(const uint32_t *__restrict__ in, uint32_t n_sym, uint32_t *__restrict__ out32,
                                                                       int16_t *__restrict__ out16)
{
  const uint32_t i0 = (blockIdx.x * NR_QAM_THREADS + threadIdx.x) * NR_QAM_GROUP;
  if (i0 >= n_sym)
    return;
  const uint32_t nw = (n_sym * (uint32_t)QM + 31u) >> 5;
  uint32_t p[NR_QAM_GROUP];
#pragma unroll
  for (int u = 0; u < NR_QAM_GROUP; u++)
    p[u] = i0 + u < n_sym ? nr_qam_map_one<QM>(in, nw, i0 + u) : 0u;
  if (out32 && (reinterpret_cast<uintptr_t>(out32) & 15u) == 0 && i0 + NR_QAM_GROUP <= n_sym) {
    *reinterpret_cast<qam_u32x4 *>(out32 + i0) = (qam_u32x4){p[0], p[1], p[2], p[3]};
    return;
  }
#pragma unroll
  for (int u = 0; u < NR_QAM_GROUP; u++)
    if (i0 + u < n_sym) {
      if (out32) {
        out32[i0 + u] = p[u];
      } else { /* an output that is only 2-byte aligned */
        out16[2 * (size_t)(i0 + u)] = (int16_t)(uint16_t)p[u];
        out16[2 * (size_t)(i0 + u) + 1] = (int16_t)(uint16_t)(p[u] >> 16);
      }
    }
}

hipError_t nr_launch_modulation(const uint32_t *in, uint32_t length, uint32_t Qm, int16_t *out, hipStream_t s)
{
  const uint32_t n_sym = length / Qm;
  if (n_sym == 0)
    return hipSuccess;
  const uint32_t per_wg = NR_QAM_THREADS * NR_QAM_GROUP, n_wg = (n_sym + per_wg - 1) / per_wg;
  uint32_t *o32 = (reinterpret_cast<uintptr_t>(out) & 3u) == 0 ? reinterpret_cast<uint32_t *>(out) : nullptr;
  switch (Qm) {
    case 2: hipLaunchKernelGGL(nr_modulation_kernel<2>, dim3(n_wg), dim3(NR_QAM_THREADS), 0, s, in, n_sym, o32, out); break;
    case 4: hipLaunchKernelGGL(nr_modulation_kernel<4>, dim3(n_wg), dim3(NR_QAM_THREADS), 0, s, in, n_sym, o32, out); break;
    case 6: hipLaunchKernelGGL(nr_modulation_kernel<6>, dim3(n_wg), dim3(NR_QAM_THREADS), 0, s, in, n_sym, o32, out); break;
    case 8: hipLaunchKernelGGL(nr_modulation_kernel<8>, dim3(n_wg), dim3(NR_QAM_THREADS), 0, s, in, n_sym, o32, out); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

/* planes[k] = y, mag_a, mag_b, mag_c (k < Qm/2), one c16 word per RE; llr: nb_re Qm int16 */
struct nr_llr_planes {
  const uint32_t *p[4];
};
template <int QM>
__global__ void __launch_bounds__(NR_QAM_THREADS) nr_ulsch_llr_kernel(const nr_llr_planes pl, uint32_t nb_re, int16_t *__restrict__ llr, int vec)
{
  constexpr int NP = QM / 2;
  const uint32_t r0 = (blockIdx.x * NR_QAM_THREADS + threadIdx.x) * NR_QAM_GROUP;
  if (r0 >= nb_re)
    return;
  uint32_t w[NR_QAM_GROUP][4];
  if (vec && r0 + NR_QAM_GROUP <= nb_re) { /* every plane and the output 16-byte aligned: 16-byte loads and stores */
#pragma unroll
    for (int k = 0; k < NP; k++) {
      const qam_u32x4 v = *reinterpret_cast<const qam_u32x4 *>(pl.p[k] + r0);
      w[0][k] = v.x; w[1][k] = v.y; w[2][k] = v.z; w[3][k] = v.w;
    }
#pragma unroll
    for (int u = 0; u < NR_QAM_GROUP; u++)
      nr_qam_demap(QM, w[u]);
    /* RE u's level k is word u NP + k of the group's NR_QAM_GROUP NP output words */
    uint32_t *o = reinterpret_cast<uint32_t *>(llr) + (size_t)r0 * NP;
#pragma unroll
    for (int q = 0; q < NP; q++) {
      uint32_t v[4];
#pragma unroll
      for (int t = 0; t < 4; t++)
        v[t] = w[(4 * q + t) / NP][(4 * q + t) % NP];
      reinterpret_cast<qam_u32x4 *>(o)[q] = (qam_u32x4){v[0], v[1], v[2], v[3]};
    }
    return;
  }
  for (uint32_t u = 0; u < NR_QAM_GROUP && r0 + u < nb_re; u++) {
    uint32_t x[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < NP; k++)
      x[k] = pl.p[k][r0 + u];
    nr_qam_demap(QM, x);
#pragma unroll
    for (int k = 0; k < NP; k++) {
      llr[(size_t)(r0 + u) * QM + 2 * k] = (int16_t)(uint16_t)x[k];
      llr[(size_t)(r0 + u) * QM + 2 * k + 1] = (int16_t)(uint16_t)(x[k] >> 16);
    }
  }
}

hipError_t nr_launch_ulsch_llr(const uint32_t *const planes[4], uint32_t nb_re, uint32_t Qm, int16_t *llr, hipStream_t s)
{
  if (nb_re == 0)
    return hipSuccess;
  nr_llr_planes pl{{planes[0], planes[1], planes[2], planes[3]}};
  int vec = (reinterpret_cast<uintptr_t>(llr) & 15u) == 0;
  for (uint32_t k = 0; k < Qm / 2; k++)
    vec &= (reinterpret_cast<uintptr_t>(planes[k]) & 15u) == 0;
  const uint32_t per_wg = NR_QAM_THREADS * NR_QAM_GROUP, n_wg = (nb_re + per_wg - 1) / per_wg;
  switch (Qm) {
    case 2: hipLaunchKernelGGL(nr_ulsch_llr_kernel<2>, dim3(n_wg), dim3(NR_QAM_THREADS), 0, s, pl, nb_re, llr, vec); break;
    case 4: hipLaunchKernelGGL(nr_ulsch_llr_kernel<4>, dim3(n_wg), dim3(NR_QAM_THREADS), 0, s, pl, nb_re, llr, vec); break;
    case 6: hipLaunchKernelGGL(nr_ulsch_llr_kernel<6>, dim3(n_wg), dim3(NR_QAM_THREADS), 0, s, pl, nb_re, llr, vec); break;
    case 8: hipLaunchKernelGGL(nr_ulsch_llr_kernel<8>, dim3(n_wg), dim3(NR_QAM_THREADS), 0, s, pl, nb_re, llr, vec); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

/* ---- layer mapping (nr_layer_mapping, one codeword): out[l stride + i] = in[Nl i + l] ----------------------------------------
 * A thread takes NR_QAM_GROUP layer groups: NL 16-byte loads of consecutive input, one 16-byte store per plane where `in`, `out`
 * and the stride allow it (mode 2); otherwise c16 words one by one (mode 1: 4-byte aligned, mode 0: two int16 halves). */
template <int NL>
__global__ void __launch_bounds__(NR_QAM_THREADS) nr_layer_mapping_kernel(const int16_t *__restrict__ in, uint32_t n_per_layer, int16_t *__restrict__ out,
                                                                          uint32_t stride, int mode)
{
  const uint32_t i0 = (blockIdx.x * NR_QAM_THREADS + threadIdx.x) * NR_QAM_GROUP;
  if (i0 >= n_per_layer)
    return;
  if (mode == 2 && i0 + NR_QAM_GROUP <= n_per_layer) {
    uint32_t w[NL * NR_QAM_GROUP];
    const qam_u32x4 *src = reinterpret_cast<const qam_u32x4 *>(in) + (size_t)NL * (i0 / 4u);
#pragma unroll
    for (int q = 0; q < NL; q++) {
      const qam_u32x4 v = src[q];
      w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int l = 0; l < NL; l++)
      *reinterpret_cast<qam_u32x4 *>(reinterpret_cast<uint32_t *>(out) + (size_t)l * stride + i0) =
          (qam_u32x4){w[l], w[NL + l], w[2 * NL + l], w[3 * NL + l]};
    return;
  }
  for (uint32_t u = 0; u < NR_QAM_GROUP && i0 + u < n_per_layer; u++) {
#pragma unroll
    for (int l = 0; l < NL; l++) {
      const size_t from = (size_t)NL * (i0 + u) + l, to = (size_t)l * stride + i0 + u;
      if (mode) {
        reinterpret_cast<uint32_t *>(out)[to] = reinterpret_cast<const uint32_t *>(in)[from];
      } else {
        out[2 * to] = in[2 * from];
        out[2 * to + 1] = in[2 * from + 1];
      }
    }
  }
}

hipError_t nr_launch_layer_mapping(const int16_t *in, uint32_t n_symbs, uint32_t Nl, int16_t *out, uint32_t stride, hipStream_t s)
{
  const uint32_t n = Nl ? n_symbs / Nl : 0;
  if (n == 0)
    return hipSuccess;
  const uintptr_t a = reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out);
  const int mode = (a & 15u) == 0 && (stride & 3u) == 0 ? 2 : (a & 3u) == 0 ? 1 : 0;
  const uint32_t per_wg = NR_QAM_THREADS * NR_QAM_GROUP, n_wg = (n + per_wg - 1) / per_wg;
  switch (Nl) {
    case 1: hipLaunchKernelGGL(nr_layer_mapping_kernel<1>, dim3(n_wg), dim3(NR_QAM_THREADS), 0, s, in, n, out, stride, mode); break;
    case 2: hipLaunchKernelGGL(nr_layer_mapping_kernel<2>, dim3(n_wg), dim3(NR_QAM_THREADS), 0, s, in, n, out, stride, mode); break;
    case 3: hipLaunchKernelGGL(nr_layer_mapping_kernel<3>, dim3(n_wg), dim3(NR_QAM_THREADS), 0, s, in, n, out, stride, mode); break;
    case 4: hipLaunchKernelGGL(nr_layer_mapping_kernel<4>, dim3(n_wg), dim3(NR_QAM_THREADS), 0, s, in, n, out, stride, mode); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

/* ---- the symbol encode's three-kernel path: scratch bytes -> scrambled, mapped, layer-mapped points --------------------------
 * blockIdx.y = transport block, blockIdx.x = its piece of NR_SYM_WG_SYMS symbols.  A piece starts on a word of the sequence
 * (NR_SYM_WG_SYMS Qm is a multiple of 32) and needs at most NR_SCR_WG_WORDS of them (Qm = 8): one nr_gold_fill_wg. */
#define NR_SYM_WG_SYMS (4u * NR_SCR_WG_WORDS)
__global__ void __launch_bounds__(NR_SCR_THREADS) nr_scramble_map_tb_kernel(const tb_sym_tb_job *__restrict__ jobs, const uint8_t *__restrict__ in,
                                                                            uint8_t *__restrict__ out)
{
  __shared__ uint32_t gold[NR_SCR_WG_WORDS];
  const tb_sym_tb_job j = jobs[blockIdx.y];
  const uint32_t Qm = j.Qm, S = j.G / Qm, s0 = blockIdx.x * NR_SYM_WG_SYMS;
  if (s0 >= S)
    return;
  nr_gold_fill_wg(gold, j.c_init, (s0 * Qm) >> 5);
  __syncthreads();
  const uint32_t n = S - s0 < NR_SYM_WG_SYMS ? S - s0 : NR_SYM_WG_SYMS, plane = S / j.Nl, toff = nr_qam_table_off(Qm);
  const uint8_t *src = in + j.in_off + (size_t)s0 * Qm;
  uint32_t *dst = reinterpret_cast<uint32_t *>(out + j.out_off);
  for (uint32_t k = threadIdx.x; k < n; k += NR_SCR_THREADS) {
    uint32_t x = 0;
    for (uint32_t b = 0; b < Qm; b++) {
      const uint32_t bit = k * Qm + b;
      x |= ((src[bit] ^ (gold[bit >> 5] >> (bit & 31u))) & 1u) << b;
    }
    dst[tb_tx_sym_dst(s0 + k, j.Nl, plane)] = nr_qam_tab_dev.pt[toff + x];
  }
}

hipError_t nr_launch_scramble_map_tb(const tb_sym_tb_job *jobs, uint32_t n_tb, uint32_t max_s, const uint8_t *in, uint8_t *out, hipStream_t s)
{
  if (max_s == 0 || n_tb == 0)
    return hipSuccess;
  hipLaunchKernelGGL(nr_scramble_map_tb_kernel, dim3((max_s + NR_SYM_WG_SYMS - 1) / NR_SYM_WG_SYMS, n_tb), dim3(NR_SCR_THREADS), 0, s, jobs, in,
                     out);
  return hipGetLastError();
}
