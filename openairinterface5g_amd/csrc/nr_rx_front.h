/*
 * nr_rx_front.h -- the per-RE arithmetic of the single-layer PUSCH receive front: the matched filter with maximum ratio
 * combining over the receive antennas, nr_ulsch_channel_compensation() (openair1/PHY/NR_TRANSPORT/nr_ulsch_demodulation.c:
 * 468-577, the loop body :505-548) restated one RE at a time, and the channel level / log2_maxh of nr_rx_pusch_tp() (:382-415
 * nr_ulsch_scale_channel, :434-466 nr_ulsch_channel_level, :1612-1647; openair1/PHY/TOOLS/log2_approx.c).  nrOfLayers == 1,
 * rho == NULL.  Plain C (no HIP headers), constexpr in C++: the host checks (rx_front_api.inc.cpp) and the kernels
 * (tb_rx_front.hip) use the same definitions.
 *
 * A c16 value is held as a 32-bit word, re in the low half (nr_qam.h).  int32 sums wrap (they are formed in uint32), int16 sums
 * wrap where the reference uses add_epi16 and saturate where it uses packs_epi32; `>>` on a negative value is arithmetic.
 */
#ifndef NR_RX_FRONT_H
#define NR_RX_FRONT_H
#include <stdint.h>

#if defined(__HIPCC__)
#define NR_RXF_HD __host__ __device__ static inline constexpr
#elif defined(__cplusplus)
#define NR_RXF_HD static inline constexpr
#else
#define NR_RXF_HD static inline
#endif

#define NR_RXF_MAX_RX 8 /* receive antennas */

NR_RXF_HD int32_t nr_rxf_re(uint32_t w) { return (int16_t)(uint16_t)w; }
NR_RXF_HD int32_t nr_rxf_im(uint32_t w) { return (int16_t)(uint16_t)(w >> 16); }
NR_RXF_HD uint32_t nr_rxf_c16(int32_t re, int32_t im) { return (uint32_t)(uint16_t)re | ((uint32_t)(uint16_t)im << 16); }
/* sign_epi16(x, -1) (:507, :523): int16 negation, -32768 stays -32768 */
NR_RXF_HD int32_t nr_rxf_neg16(int32_t x) { return (int16_t)(uint16_t)(0u - (uint32_t)x); }
/* madd_epi16 of one pair (:520, :524, :532): a b + c d in int32; wraps to INT32_MIN when all four are -32768 */
NR_RXF_HD int32_t nr_rxf_madd(int32_t a, int32_t b, int32_t c, int32_t d) { return (int32_t)((uint32_t)(a * b) + (uint32_t)(c * d)); }
/* packs_epi32 (:530, :534) */
NR_RXF_HD int32_t nr_rxf_sat16(int32_t x) { return x > 32767 ? 32767 : (x < -32768 ? -32768 : x); }
/* mulhrs_epi16 (:537-539): (m k + 0x4000) >> 15, the low 16 bits */
NR_RXF_HD int32_t nr_rxf_mulhrs(int32_t m, int32_t k) { return (int16_t)(uint16_t)(uint32_t)((m * k + 0x4000) >> 15); }
/* add_epi16 on both halves of a word (:542-548): wrapping */
NR_RXF_HD uint32_t nr_rxf_add16x2(uint32_t a, uint32_t b) { return ((a + b) & 0xffffu) | ((a & 0xffff0000u) + (b & 0xffff0000u)); }
/* output_shift as srai_epi32 takes it; the kernels read it from device memory, so it is clamped, not refused */
NR_RXF_HD uint32_t nr_rxf_shift(int32_t s) { return s < 0 ? 0u : (s > 31 ? 31u : (uint32_t)s); }

/* QAM_ampa / b / c of :485-503 (impl_defs_top.h:205-222: QAM16_n1; QAM64_n1, _n2; QAM256_n1, _n2, _n3); k = 0, 1, 2 */
NR_RXF_HD int32_t nr_rxf_amp(uint32_t Qm, uint32_t k)
{
  return Qm == 4 ? (k == 0 ? 20724 : 0)
       : Qm == 6 ? (k == 0 ? 20225 : (k == 1 ? 10112 : 0))
       : Qm == 8 ? (k == 0 ? 20106 : (k == 1 ? 10053 : 5026))
                 : 0;
}

/* one RE's rxdataF_comp and ul_ch_mag / b / c while the antennas are added up; starts at zero (:1307-1311) */
typedef struct nr_rxf_acc {
  uint32_t w[4]; /* comp, mag_a, mag_b, mag_c as c16 words (a magnitude has the same value in both halves) */
} nr_rxf_acc_t;

/* one antenna's share of one RE: h = chFext, y = rxFext, s = nr_rxf_shift(output_shift), amp[k] = nr_rxf_amp(Qm, k) */
NR_RXF_HD void nr_rxf_mac(nr_rxf_acc_t *acc, uint32_t h, uint32_t y, uint32_t s, const int32_t *amp)
{
  const int32_t hr = nr_rxf_re(h), hi = nr_rxf_im(h), yr = nr_rxf_re(y), yi = nr_rxf_im(y);
  const int32_t pr = nr_rxf_madd(hr, yr, hi, yi);               /* :520 */
  const int32_t pi = nr_rxf_madd(nr_rxf_neg16(hi), yr, hr, yi); /* :522-524: the shuffle swaps (r, i), conj256 negates element 0 */
  const uint32_t c = nr_rxf_c16(nr_rxf_sat16(pr >> s), nr_rxf_sat16(pi >> s)); /* :526-530 */
  acc->w[0] = nr_rxf_add16x2(acc->w[0], c);                     /* :542 */
  const int32_t m = nr_rxf_sat16(nr_rxf_madd(hr, hr, hi, hi) >> s); /* :532-535 */
  for (int k = 0; k < 3; k++) {                                 /* :537-548 */
    const int32_t v = nr_rxf_mulhrs(m, amp[k]);
    acc->w[1 + k] = nr_rxf_add16x2(acc->w[1 + k], nr_rxf_c16(v, v));
  }
}

/* ---- channel level ---- */
/* log2_approx.c:22-38 / :40-56 */
NR_RXF_HD int32_t nr_rxf_log2_approx(uint32_t x)
{
  int32_t l2 = 0;
  for (int i = 0; i < 31; i++)
    if (x & (1u << i))
      l2 = i + 1;
  return l2;
}
NR_RXF_HD int32_t nr_rxf_factor2(uint32_t x)
{
  int i = 0;
  for (; i < 31; i++)
    if (x & (1u << i))
      break;
  return i;
}
/* the measurement symbol's length as nr_rx_pusch_tp rounds it (:1597); the padding holds zeros */
NR_RXF_HD uint32_t nr_rxf_level_len(uint32_t nb_re) { return (nb_re + 15u) & ~15u; }
/* nr_ulsch_scale_channel with shift_ch_ext = 0 (:392-411): mulhi_epi16(h, 8192) << 3 per component = h with its low 3 bits cleared */
NR_RXF_HD int32_t nr_rxf_scale(int32_t h) { return (int16_t)(uint16_t)((uint32_t)((h * 8192) >> 16) << 3); }
/* one RE's term of the sum of :454: madd(h', h') >> x, x = factor2(len) */
NR_RXF_HD int32_t nr_rxf_level_term(uint32_t h, uint32_t x)
{
  const int32_t r = nr_rxf_scale(nr_rxf_re(h)), i = nr_rxf_scale(nr_rxf_im(h));
  return nr_rxf_madd(r, r, i, i) >> x;
}
/* :457-460: sum = the wrapped int32 sum of the terms of one antenna.  (The reference keeps len >> x in an int16, :444; a
 * carrier has at most 3276 REs per symbol, and the divisor is not cut to 16 bits here.) */
NR_RXF_HD int32_t nr_rxf_level_avg(int32_t sum, uint32_t len) { return sum / (int32_t)(len >> nr_rxf_factor2(len)); }
/* :1636-1647, one layer: avgs = max(0, the antennas' averages) */
NR_RXF_HD int32_t nr_rxf_log2_maxh(int32_t avgs, uint32_t n_rx)
{
  const int32_t v = (nr_rxf_log2_approx((uint32_t)(avgs < 0 ? 0 : avgs)) >> 1) + 1 + nr_rxf_log2_approx(n_rx >> 2);
  return v < 0 ? 0 : v;
}
#endif
