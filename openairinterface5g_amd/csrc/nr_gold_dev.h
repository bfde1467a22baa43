/*
 * nr_gold_dev.h -- device side of the Gold sequence (nr_gold.h): the jump tables in constant memory and the wave-wide jump
 * to any word.  Shared by the standalone (un)scrambling kernels (tb_scrambling.hip) and the transport-block chain kernels
 * that scramble on the way (tb_chain.hip, tb_rx_fused.hip through tb_rx_core.h).  HIP only.
 */
#ifndef NR_GOLD_DEV_H
#define NR_GOLD_DEV_H
#include <hip/hip_runtime.h>
#include "nr_gold.h"

/* T^(2^i) of both registers, computed by the compiler (nr_gold_make_tables is constexpr in C++).  One copy per translation
 * unit: internal linkage, except where the includer defines NR_GOLD_TAB_EXTERN first (tb_scrambling.hip, whose standalone
 * kernels were tuned with an external table: the compiler allocates their registers differently for a static one) */
#ifdef NR_GOLD_TAB_EXTERN
__constant__ nr_gold_tables_t nr_gold_tab_dev = nr_gold_make_tables();
#else
static __constant__ nr_gold_tables_t nr_gold_tab_dev = nr_gold_make_tables();
#endif

/* registers of sequence word w (uniform) in every lane of the wave; all 64 lanes active */
__device__ __forceinline__ void nr_gold_jump_wave(uint32_t c_init, uint32_t w, uint32_t lane, uint32_t &x1, uint32_t &x2)
{
  uint32_t a = nr_gold_x1_init(), b = nr_gold_x2_init(c_init);
  const uint32_t n = w + NR_GOLD_NC_WORDS;
  for (int i = 0; i < NR_GOLD_JUMPS; i++) {
    if ((n >> i) & 1u) {
      const uint32_t row = nr_gold_tab_dev.row[i][lane];
      const unsigned long long m = __ballot(__popc(row & (lane < 32u ? a : b)) & 1);
      a = (uint32_t)m;
      b = (uint32_t)(m >> 32);
    }
  }
  x1 = a;
  x2 = b;
}

/* the standalone kernels' workgroup (tb_scrambling.hip) and the transport-block packer (tb_scr_pack.hip) */
#define NR_SCR_THREADS 256
#define NR_SCR_RUN_LOG2 2                                    /* words per lane: 4 */
#define NR_SCR_WAVE_WORDS (64u << NR_SCR_RUN_LOG2)           /* 256 */
#define NR_SCR_WG_WORDS ((NR_SCR_THREADS / 64) * NR_SCR_WAVE_WORDS) /* 1024 */

/* words w0 .. w0 + NR_SCR_WG_WORDS - 1 of the sequence into gold[]; the caller synchronises */
__device__ __forceinline__ void nr_gold_fill_wg(uint32_t *gold, uint32_t c_init, uint32_t w0)
{
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t a, b;
  nr_gold_jump_wave(c_init, w0 + wave * NR_SCR_WAVE_WORDS, lane, a, b);
#pragma unroll
  for (int k = 0; k < 6; k++) /* + lane << NR_SCR_RUN_LOG2 words */
    if ((lane >> k) & 1u) {
      a = nr_gold_apply_cols(&nr_gold_tab_dev.col[NR_SCR_RUN_LOG2 + k][0], a);
      b = nr_gold_apply_cols(&nr_gold_tab_dev.col[NR_SCR_RUN_LOG2 + k][32], b);
    }
  uint32_t *dst = gold + wave * NR_SCR_WAVE_WORDS + (lane << NR_SCR_RUN_LOG2);
#pragma unroll
  for (int k = 0; k < (1 << NR_SCR_RUN_LOG2); k++) {
    dst[k] = a ^ b;
    a = nr_gold_step1(a);
    b = nr_gold_step2(b);
  }
}

#endif
