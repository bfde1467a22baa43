/*
 * nr_rx_mmse.h -- the arithmetic of the two-layer PUSCH MMSE receiver for 64QAM and 256QAM, one RE and one quad of four REs at
 * a time: nr_ulsch_mmse_2layers() (openair1/PHY/NR_TRANSPORT/nr_ulsch_demodulation.c:869-1260) with the functions it calls
 * (:580-640 nr_ulsch_det_HhH, :646-687 nr_ulsch_conjch0_mult_ch1, :689-750 nr_ulsch_comp_muli_sum, :756-867
 * nr_ulsch_construct_HhH_elements), the per-layer matched filter in front of it (:505-548, the aatx loop), and the channel level
 * of a two-layer block (:382-415 nr_ulsch_scale_channel in its general branch, :1612-1647).  Plain C (no HIP headers), constexpr in
 * C++: the host form (rx_mmse_api.inc.cpp) and the kernels (tb_rx_mmse.hip) use the same definitions.
 *
 * Layer l, antenna a is estimate array ("pair") l n_rx + a (:917-935, :1290).  The reference names a pair chAL: antenna A, layer L.
 * Every wrap and saturation sits where the reference's instruction has it: adds_epi16 saturates, add_epi16 / add_epi32 / sub_epi32
 * wrap, packs_epi32 saturates, mulhi_epi16 then slli_epi16 cut to 16 bits.  Where the reference aborts (AssertFatal :1181, a
 * determinant lane <= 0) the arithmetic below goes on with what the instructions give.
 */
#ifndef NR_RX_MMSE_H
#define NR_RX_MMSE_H
#include "nr_rx_front.h"

#define NR_RXM_QUAD 4u /* REs per 128-bit vector: the unit that shares the shift b (:726-732, :1179-1185) */

/* adds_epi16 on both halves of a word (:814-828): saturating */
NR_RXF_HD uint32_t nr_rxm_adds16x2(uint32_t a, uint32_t b)
{
  return nr_rxf_c16(nr_rxf_sat16(nr_rxf_re(a) + nr_rxf_re(b)), nr_rxf_sat16(nr_rxf_im(a) + nr_rxf_im(b)));
}
/* nr_ulsch_conjch0_mult_ch1 of one RE (:664-674), which is also the matched filter's term (:520-530): pack(conj(h0) h1 >> s) */
NR_RXF_HD uint32_t nr_rxm_conj_mult(uint32_t h0, uint32_t h1, uint32_t s)
{
  const int32_t ar = nr_rxf_re(h0), ai = nr_rxf_im(h0), br = nr_rxf_re(h1), bi = nr_rxf_im(h1);
  const int32_t pr = nr_rxf_madd(ar, br, ai, bi);               /* :664 */
  const int32_t pi = nr_rxf_madd(nr_rxf_neg16(ai), br, ar, bi); /* :665-668: the shuffles swap (r, i), the sign negates element 0 */
  return nr_rxf_c16(nr_rxf_sat16(pr >> s), nr_rxf_sat16(pi >> s)); /* :669-674 */
}
/* abs_epi32 (:623): INT32_MIN stays */
NR_RXF_HD int32_t nr_rxm_abs32(int32_t x) { return x < 0 ? (int32_t)(0u - (uint32_t)x) : x; }
/* Re(x y) as sign_epi16(x, (1, -1)) and madd_epi16 form it (:605-606, :613-614, :702-703, :712-713) */
NR_RXF_HD int32_t nr_rxm_mul_re(uint32_t x, uint32_t y)
{
  return nr_rxf_madd(nr_rxf_re(x), nr_rxf_re(y), nr_rxf_neg16(nr_rxf_im(x)), nr_rxf_im(y));
}
/* Im(x y): the shuffles swap x to (i, r), then madd_epi16 (:706-708, :716-718) */
NR_RXF_HD int32_t nr_rxm_mul_im(uint32_t x, uint32_t y) { return nr_rxf_madd(nr_rxf_im(x), nr_rxf_re(y), nr_rxf_re(x), nr_rxf_im(y)); }

/* one RE while the antennas are added up; starts at zero (:1284-1285 the padding, :1311 rxdataF_comp) */
typedef struct nr_rxm_re {
  uint32_t y[2];       /* the layers' matched filter outputs */
  uint32_t a, b, c, d; /* H^H H: 00, 01, 10, 11 */
} nr_rxm_re_t;

/* one antenna's share: h0 / h1 = layer 0's / layer 1's estimate on that antenna, y = the antenna's RE, s = nr_rxf_shift(shift).
 * The antennas must come in order: adds_epi16 is not associative.  The first adds into zero, which changes nothing. */
NR_RXF_HD void nr_rxm_mac(nr_rxm_re_t *R, uint32_t h0, uint32_t h1, uint32_t y, uint32_t s)
{
  R->y[0] = nr_rxf_add16x2(R->y[0], nr_rxm_conj_mult(h0, y, s)); /* :520-530, :542 with layer 0's estimates */
  R->y[1] = nr_rxf_add16x2(R->y[1], nr_rxm_conj_mult(h1, y, s)); /* the same, layer 1 */
  R->a = nr_rxm_adds16x2(R->a, nr_rxm_conj_mult(h0, h0, s));     /* :953, :959, :1003, :1010 -> :814-816 */
  R->d = nr_rxm_adds16x2(R->d, nr_rxm_conj_mult(h1, h1, s));     /* :977, :983, :1029, :1035 -> :818-820 */
  R->b = nr_rxm_adds16x2(R->b, nr_rxm_conj_mult(h0, h1, s));     /* :965, :971, :1017, :1023 -> :822-824 */
  R->c = nr_rxm_adds16x2(R->c, nr_rxm_conj_mult(h1, h0, s));     /* :989, :995, :1042, :1048 -> :826-828 */
}
/* the noise variance on the diagonal (:1103-1113: a 32-bit add on the packed c16 word, as written) and the determinant (:605-623).
 * An RE of the zero padding (R all zero) goes through this too: its a and d become nvar. */
NR_RXF_HD int32_t nr_rxm_det(nr_rxm_re_t *R, uint32_t nvar)
{
  if (nvar != 0) {
    R->a += nvar; /* :1108 */
    R->d += nvar; /* :1109 */
  }
  return nr_rxm_abs32((int32_t)((uint32_t)nr_rxm_mul_re(R->a, R->d) - (uint32_t)nr_rxm_mul_re(R->b, R->c))); /* :605-623 */
}

/* ---- per quad ---- */
/* the shift of the magnitudes (:1179-1185): the lanes as uint32 >> 2 */
NR_RXF_HD int32_t nr_rxm_b_mag(const int32_t *det)
{
  uint32_t sum = 0;
  for (int k = 0; k < 4; k++)
    sum += (uint32_t)det[k] >> 2;
  return nr_rxf_log2_approx(sum) - 8;
}
/* the shift of the symbols (:726-732): the lanes as int >> 2.  The two differ only for a lane of INT32_MIN. */
NR_RXF_HD int32_t nr_rxm_b_sym(const int32_t *det)
{
  uint32_t sum = 0;
  for (int k = 0; k < 4; k++)
    sum += (uint32_t)(det[k] >> 2);
  return nr_rxf_log2_approx(sum) - 8;
}
/* srai_epi32 by b, or slli_epi32 by -b (:733-739, :1186-1190); -8 <= b <= 23 */
NR_RXF_HD int32_t nr_rxm_sh(int32_t x, int32_t b) { return b > 0 ? x >> b : (int32_t)((uint32_t)x << (uint32_t)(-b)); }
/* one RE's ul_ch_mag / b / c, the same for both layers (:1191-1215): pack(det shifted), mulhi_epi16 by the amplitude, slli_epi16 1 */
NR_RXF_HD uint32_t nr_rxm_mag(int32_t det, int32_t b, int32_t amp)
{
  const int32_t m = nr_rxf_sat16(nr_rxm_sh(det, b));                              /* :1187-1193 */
  const int32_t v = (int16_t)(uint16_t)((uint32_t)((m * amp) >> 16) << 1);        /* :1199-1204 */
  return nr_rxf_c16(v, v);
}
/* nr_ulsch_comp_muli_sum of one RE: pack((x y - w z) shifted by b) (:702-745) */
NR_RXF_HD uint32_t nr_rxm_muli_sum(uint32_t x, uint32_t y, uint32_t w, uint32_t z, int32_t b)
{
  const int32_t re = (int32_t)((uint32_t)nr_rxm_mul_re(x, y) - (uint32_t)nr_rxm_mul_re(w, z)); /* :721 */
  const int32_t im = (int32_t)((uint32_t)nr_rxm_mul_im(x, y) - (uint32_t)nr_rxm_mul_im(w, z)); /* :722 */
  return nr_rxf_c16(nr_rxf_sat16(nr_rxm_sh(re, b)), nr_rxf_sat16(nr_rxm_sh(im, b)));           /* :733-745 */
}
/* the two layers' symbols of one RE after nr_rxm_det (:1222-1236): y0 d - y1 b and y1 a - y0 c */
NR_RXF_HD uint32_t nr_rxm_sym0(const nr_rxm_re_t *R, int32_t b) { return nr_rxm_muli_sum(R->y[0], R->d, R->y[1], R->b, b); }
NR_RXF_HD uint32_t nr_rxm_sym1(const nr_rxm_re_t *R, int32_t b) { return nr_rxm_muli_sum(R->y[1], R->a, R->y[0], R->c, b); }

/* ---- channel level of a two-layer block ---- */
/* :1614; the reference keeps it in a uint8 */
NR_RXF_HD uint32_t nr_rxm_shift_ch_ext(int32_t max_ch) { return (uint32_t)nr_rxf_log2_approx((uint32_t)(max_ch >> 11)); }
/* nr_ulsch_scale_channel (:392-411), one component: mulhi_epi16(h, ch_amp) then slli_epi16 b */
NR_RXF_HD int32_t nr_rxm_scale(int32_t h, uint32_t shift_ch_ext)
{
  int32_t b = 3, ch_amp = 1024 * 8; /* :392-393 */
  if (shift_ch_ext > 3) {           /* :394-399 */
    b = 0;
    ch_amp >>= (shift_ch_ext - 3u);
    if (ch_amp == 0)
      ch_amp = 1;
  } else {
    b -= (int32_t)shift_ch_ext;     /* :401 */
  }
  return (int16_t)(uint16_t)((uint32_t)((h * ch_amp) >> 16) << b); /* :410-411 */
}
/* one RE's term of the sum of :454 on the scaled estimate, x = factor2(len) */
NR_RXF_HD int32_t nr_rxm_level_term(uint32_t h, uint32_t x, uint32_t shift_ch_ext)
{
  const int32_t r = nr_rxm_scale(nr_rxf_re(h), shift_ch_ext), i = nr_rxm_scale(nr_rxf_im(h), shift_ch_ext);
  return nr_rxf_madd(r, r, i, i) >> x;
}
/* :1639-1647 for two layers and Qm >= 6: avgs = max(0, the 2 n_rx pairs' averages (nr_rxf_level_avg)) */
NR_RXF_HD int32_t nr_rxm_log2_maxh(int32_t avgs)
{
  const int32_t v = (nr_rxf_log2_approx((uint32_t)(avgs < 0 ? 0 : avgs)) >> 1) - 3;
  return v < 0 ? 0 : v;
}
#endif
