/*
 * nr_delay.h -- the PUSCH delay search of one DMRS symbol: what nr_est_delay (common/utils/nr/nr_common.c:968-990) looks for in
 * the LS estimates of nr_pusch_channel_estimation (openair1/PHY/NR_ESTIMATION/nr_ul_channel_estimation.c:176-192, :264-272), the
 * position of the largest sample of their IDFT.  Plain C (no HIP headers): the host check form (rx_delay_api.inc.cpp), the kernel
 * (tb_rx_delay.hip) and the kernel run on the CPU compute with the same definitions, one IEEE operation after the other in the
 * same order, so delays and peaks are bit-equal among the three.  The reference's transform is a fixed-point SIMD IDFT
 * (oai_dfts.c) that is not rebuilt; this one runs in fp32.
 *
 * Input, one descriptor (nrLDPC_hip_chest_seg_t) and antenna a, N = fft_size: x[k], 0 <= k < N, indexed from the allocation's
 * first RE as the reference's ul_ls_est is (not by grid position), zero for k >= 12 rb_size.
 *   TYPE1_INTERP  x[4n + j], j = 0..3 = the int16-cast LS value of pilot pair n (:176-192): nr_che_t1_ls32 of nr_chest.h, cast.
 *   TYPE2_INTERP  REs 0..3 of 6-RE block m hold ch & ~3 per component, REs 4, 5 hold ch (:264-272): what nr_che_t2_interp forms
 *     before its rotation, taken from that function with the rotation (256, 0), which (x 256) >> 8 undoes exactly.
 * Every antenna starts from zeros: the reference clears ul_ls_est once before its antenna loop (:150-151) and its type-2 line
 * :270 adds into the array, so there REs 0..3 hold a sum over antennas from antenna 1 on.  That is not reproduced.
 *
 * Transform: y[n] = sum_k x[k] exp(+2 pi i k n / N), unnormalised, P[n] = re^2 + im^2.  In place, decimation in frequency: for
 * N = 3 M one radix-3 stage (nr_dly_r3, butterflies k < M) leaves three blocks of M, block r holding the input of the outputs
 * n = 3q + r; then radix-2 stages (nr_dly_r2) with block lengths L = M, M/2 .. 2 (M = N for a power of two), N/2 butterflies
 * each.  The butterflies of a stage touch disjoint entries, so a stage may run in any order and on any number of threads; between
 * two stages everything of the first must be complete.  Location p then holds y[nr_dly_index(N, p)] (bit reversal inside a
 * block).  Twiddles come from one table of the fft_size, tw[t] = exp(2 pi i t / N) computed in double and rounded once
 * (nr_dly_fill_twiddles of rx_delay_plan.h); no fast intrinsic anywhere.  Contraction into fused multiply-adds is off.
 *
 * Search (nr_common.c:968-990): the scan n = 0 .. N - 1 with P > best from best = 0, position 0 is the maximum with ties to the
 * lowest n (nr_dly_better); position > N / 2 has N subtracted (nr_dly_fold: N / 2 itself stays positive).  The reference clears
 * best and its position per call and carries them from antenna to antenna (its delay_t is cleared at :152-153): antenna a gets
 * the position of the largest sample over antennas 0 .. a, a later antenna's sample winning only when it is larger
 * (NR_DLY_RUNNING_MAX); NR_DLY_PER_ANTENNA clears them per antenna.  No clamping here: nr_che_delay_idx clamps where the
 * estimator reads the value.
 */
#ifndef NR_DELAY_H
#define NR_DELAY_H
#include <stdint.h>
#include "nr_chest.h"

#define NR_DLY_RUNNING_MAX 0u
#define NR_DLY_PER_ANTENNA 1u
#define NR_DLY_ONE_WORDS 8u /* the words behind the twiddles: six rotations (256, 0) and padding */

typedef struct __attribute__((aligned(8))) nr_dly_c {
  float r, i;
} nr_dly_c;

/* the first pilot whose bits group g (x[4g .. 4g + 3]) needs: pair g's, or those of the 6-RE block RE 4g lies in */
NR_CHE_HD uint32_t nr_dly_first_pilot(uint32_t mode, uint32_t g) { return mode == NR_CHE_TYPE1_INTERP ? 2u * g : 2u * ((4u * g) / 6u); }

/* x[4g .. 4g + 3] as c16; bits from pilot nr_dly_first_pilot(mode, g) on; one = six words (256, 0) */
NR_CHE_HD void nr_dly_ls4(uint32_t mode, const uint32_t *rx, uint32_t N, uint32_t k0, uint32_t port, uint32_t dmrs_offset, uint64_t bits,
                          const uint32_t *one, uint32_t g, uint32_t *out)
{
  if (mode == NR_CHE_TYPE1_INTERP) {
    nr_che_c ls = nr_che_t1_ls32(rx, N, k0, port, dmrs_offset, bits, 2u * g, g);
    ls.r = nr_che_cast16(ls.r);
    ls.i = nr_che_cast16(ls.i);
    out[0] = out[1] = out[2] = out[3] = nr_che_pack(ls);
  } else
    nr_che_t2_interp(rx, N, k0, port, dmrs_offset, bits, one, g, out);
}

NR_CHE_HD uint32_t nr_dly_radix3(uint32_t N) { return N % 3u == 0u; }
/* M: the length of the radix-2 part */
NR_CHE_HD uint32_t nr_dly_pow2(uint32_t N) { return nr_dly_radix3(N) ? N / 3u : N; }
NR_CHE_HD uint32_t nr_dly_log2(uint32_t m)
{
  uint32_t l = 0;
  while ((1u << l) < m)
    l++;
  return l;
}
NR_CHE_HD uint32_t nr_dly_brev(uint32_t x, uint32_t bits)
{
  x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
  x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
  x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
  x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
  x = (x >> 16) | (x << 16);
  return bits ? x >> (32u - bits) : 0u;
}
/* the n of the y[n] that location p holds behind the last stage; lm = nr_dly_log2(nr_dly_pow2(N)) */
NR_CHE_HD uint32_t nr_dly_index(uint32_t N, uint32_t lm, uint32_t p)
{
  const uint32_t q = nr_dly_brev(p & ((1u << lm) - 1u), lm);
  return nr_dly_radix3(N) ? 3u * q + (p >> lm) : q;
}
NR_CHE_HD int32_t nr_dly_fold(uint32_t N, uint32_t pos) { return pos > N / 2u ? (int32_t)pos - (int32_t)N : (int32_t)pos; }
/* the scan's order on (P, n): larger, or as large at a lower position */
NR_CHE_HD uint32_t nr_dly_better(float p, uint32_t n, float best, uint32_t best_n) { return p > best || (p == best && n < best_n); }

/* at the head of every function with a float operation: no fused multiply-add is formed from its operations, on the host or on
 * the device, whatever the translation unit's setting is */
#if defined(__clang__)
#define NR_DLY_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define NR_DLY_NO_CONTRACT _Pragma("STDC FP_CONTRACT OFF")
#endif
NR_CHE_HD nr_dly_c nr_dly_from_c16(uint32_t w)
{
  const nr_che_c c = nr_che_unpack(w);
  nr_dly_c v;
  v.r = (float)c.r;
  v.i = (float)c.i;
  return v;
}
NR_CHE_HD nr_dly_c nr_dly_add(nr_dly_c a, nr_dly_c b)
{
  NR_DLY_NO_CONTRACT
  nr_dly_c c;
  c.r = a.r + b.r;
  c.i = a.i + b.i;
  return c;
}
NR_CHE_HD nr_dly_c nr_dly_sub(nr_dly_c a, nr_dly_c b)
{
  NR_DLY_NO_CONTRACT
  nr_dly_c c;
  c.r = a.r - b.r;
  c.i = a.i - b.i;
  return c;
}
NR_CHE_HD nr_dly_c nr_dly_mul(nr_dly_c a, nr_dly_c w)
{
  NR_DLY_NO_CONTRACT
  nr_dly_c c;
  const float rr = a.r * w.r, ii = a.i * w.i, ri = a.r * w.i, ir = a.i * w.r;
  c.r = rr - ii;
  c.i = ri + ir;
  return c;
}
NR_CHE_HD float nr_dly_power(nr_dly_c y)
{
  NR_DLY_NO_CONTRACT
  const float rr = y.r * y.r, ii = y.i * y.i;
  return rr + ii;
}
/* radix-3 butterfly k < M = N / 3 on buf[k], buf[k + M], buf[k + 2M]; tw[M], tw[2M] are the cube roots of one */
NR_CHE_HD void nr_dly_r3(nr_dly_c *buf, const nr_dly_c *tw, uint32_t M, uint32_t k)
{
  const nr_dly_c a = buf[k], b = buf[k + M], c = buf[k + 2u * M], w1 = tw[M], w2 = tw[2u * M];
  buf[k] = nr_dly_add(nr_dly_add(a, b), c);
  buf[k + M] = nr_dly_mul(nr_dly_add(nr_dly_add(a, nr_dly_mul(b, w1)), nr_dly_mul(c, w2)), tw[k]);
  buf[k + 2u * M] = nr_dly_mul(nr_dly_add(nr_dly_add(a, nr_dly_mul(b, w2)), nr_dly_mul(c, w1)), tw[2u * k]);
}
/* radix-2 butterfly b < N / 2 of the stage with block length L = 1 << ll: entries i, i + L/2 of block b / (L/2); the second
 * takes the twiddle exp(2 pi i j / L) = tw[j N / L], which is one in the last stage */
NR_CHE_HD void nr_dly_r2(nr_dly_c *buf, const nr_dly_c *tw, uint32_t N, uint32_t ll, uint32_t b)
{
  const uint32_t h = 1u << (ll - 1u), j = b & (h - 1u), i = ((b >> (ll - 1u)) << ll) + j;
  const nr_dly_c x = buf[i], y = buf[i + h];
  buf[i] = nr_dly_add(x, y);
  const nr_dly_c d = nr_dly_sub(x, y);
  buf[i + h] = ll > 1u ? nr_dly_mul(d, tw[j * (N >> ll)]) : d;
}
#endif
