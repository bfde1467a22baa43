/*
 * nr_rx_ml.h -- the arithmetic of the two-layer PUSCH max-log ML receiver for QPSK and 16QAM, one RE at a time:
 * nr_ulsch_compute_ML_llr() (openair1/PHY/NR_TRANSPORT/nr_ulsch_llr_computation.c:2100-2129) with nr_ulsch_qpsk_qpsk (:528-682),
 * nr_ulsch_shift_llr (:2076-2098), nr_ulsch_qam16_qam16 (:1124-1350) and its helpers (:820-884), in the 256-bit variants an x86
 * build takes; in front of it nr_ulsch_channel_compensation with rho (nr_ulsch_demodulation.c:505-571), and the channel level of
 * a two-layer block below 64QAM (:1612-1647).  Plain C (no HIP headers), constexpr in C++: the host form (rx_ml_api.inc.cpp) and
 * the kernels (tb_rx_ml.hip) use the same definitions.
 *
 * Every SIMD lane of those functions is one RE and no lane reads another (simde_mm256_separate_real_imag_parts puts RE 16 (i/2)
 * + k into lane k, the stores put it back), so the per-RE form is exact.  adds_epi16 / subs_epi16 saturate, mulhi_epi16 is the
 * exact high half, slli_epi16 cuts to 16 bits, abs_epi16(-32768) stays -32768.  The matched filter and mag_a of a layer are
 * nr_rxf_mac (nr_rx_front.h); rho is formed with nr_rxm_conj_mult / nr_rxm_adds16x2 (nr_rx_mmse.h).
 *
 * Three deliberate deviations, all in which REs are computed, none in an RE's value:
 *   1. the reference's loops run `for (i = 0; i < length >> 3; i += 2)` over 16 REs each.  When nb_re >> 3 is even and nb_re % 8
 *      != 0 (18, 20, 36 REs; a 3- or 11-PRB allocation) the last nb_re % 8 REs are never computed: their LLRs are whatever the
 *      buffer held.  Here all nb_re REs are computed.
 *   2. when nb_re >> 3 is odd the loop computes and stores up to 8 REs behind nb_re.  Here nothing behind nb_re is written.
 *   3. nr_ulsch_shift_llr shifts 4 (nb_re >> 2) REs from an address-dependent start: some QPSK REs are shifted never or twice.
 *      Here every QPSK LLR is shifted exactly once.
 */
#ifndef NR_RX_ML_H
#define NR_RX_ML_H
#include "nr_rx_mmse.h"

#if defined(__clang__)
#define NR_RXL_UNROLL _Pragma("unroll")
#else
#define NR_RXL_UNROLL
#endif

/* ---- the int16 instructions, one lane ---- */
NR_RXF_HD int32_t nr_rxl_adds(int32_t a, int32_t b) { return nr_rxf_sat16(a + b); }
NR_RXF_HD int32_t nr_rxl_subs(int32_t a, int32_t b) { return nr_rxf_sat16(a - b); }
NR_RXF_HD int32_t nr_rxl_abs(int32_t x) { return x < 0 ? nr_rxf_neg16(x) : x; } /* -32768 stays */
NR_RXF_HD int32_t nr_rxl_mulhi(int32_t a, int32_t b) { return (a * b) >> 16; }
NR_RXF_HD int32_t nr_rxl_slli(int32_t x, uint32_t n) { return (int16_t)(uint16_t)((uint32_t)x << n); }
NR_RXF_HD int32_t nr_rxl_max(int32_t a, int32_t b) { return a > b ? a : b; }
/* mulhi_epi16 then slli_epi16 1 */
NR_RXF_HD int32_t nr_rxl_mulhi2(int32_t a, int32_t b) { return nr_rxl_slli(nr_rxl_mulhi(a, b), 1); }

/* ---- compensation with rho (nr_ulsch_demodulation.c:505-571) ---- */
/* one RE while the antennas are added up; starts at zero (:1306-1311) */
typedef struct nr_rxl_re {
  nr_rxf_acc_t l[2];    /* per layer: w[0] = rxdataF_comp, w[1] = ul_ch_maga (:520-548) */
  uint32_t rho01, rho10; /* rho[0][1], rho[1][0] (:550-570) */
} nr_rxl_re_t;

/* one antenna's share: h0 / h1 = layer 0's / layer 1's estimate on that antenna, y = the antenna's RE, s = nr_rxf_shift(shift),
 * amp = {nr_rxf_amp(Qm, 0), 0, 0}.  The antennas must come in order: adds_epi16 is not associative.  rho[0][1] and rho[1][0] are
 * both formed as written: the arithmetic shift makes them differ from each other's conjugate by rounding. */
NR_RXF_HD void nr_rxl_mac(nr_rxl_re_t *R, uint32_t h0, uint32_t h1, uint32_t y, uint32_t s, const int32_t *amp)
{
  nr_rxf_mac(&R->l[0], h0, y, s, amp);                                    /* :520-548, aatx = 0 */
  nr_rxf_mac(&R->l[1], h1, y, s, amp);                                    /* aatx = 1 */
  R->rho01 = nr_rxm_adds16x2(R->rho01, nr_rxm_conj_mult(h0, h1, s));      /* :552-568, aatx = 0, atx = 1 */
  R->rho10 = nr_rxm_adds16x2(R->rho10, nr_rxm_conj_mult(h1, h0, s));      /* aatx = 1, atx = 0 */
}

/* ---- QPSK (nr_ulsch_qpsk_qpsk, nr_ulsch_llr_computation.c:528-682) and nr_ulsch_shift_llr's >> 4 (:2095, called at :2117) ----
 * y0 = the desired stream's matched filter output, y1 = the interfering one's, rho = rho[desired][interfering]; llr[2] */
NR_RXF_HD void nr_rxl_qpsk(uint32_t y0, uint32_t y1, uint32_t rho, int32_t *llr)
{
  const int32_t K = 23170; /* ONE_OVER_2_SQRT_2 (:532) */
  const int32_t y0r = nr_rxl_mulhi2(nr_rxf_re(y0), K), y0i = nr_rxl_mulhi2(nr_rxf_im(y0), K);    /* :540-543 */
  const int32_t y1r = nr_rxf_re(y1) >> 1, y1i = nr_rxf_im(y1) >> 1;                              /* :548-549 */
  const int32_t rho_p = nr_rxl_mulhi(nr_rxl_adds(nr_rxf_re(rho), nr_rxf_im(rho)), K);            /* :563-564 */
  const int32_t rho_m = nr_rxl_mulhi(nr_rxl_subs(nr_rxf_re(rho), nr_rxf_im(rho)), K);            /* :569-570 */
  const int32_t rpm = nr_rxl_abs(nr_rxl_subs(rho_p, y1r)), imm = nr_rxl_abs(nr_rxl_subs(rho_m, y1i)); /* :573-578 */
  const int32_t rmm = nr_rxl_abs(nr_rxl_subs(rho_m, y1r)), ipm = nr_rxl_abs(nr_rxl_subs(rho_p, y1i)); /* :581-586 */
  const int32_t rpp = nr_rxl_abs(nr_rxl_adds(rho_p, y1r)), imp = nr_rxl_abs(nr_rxl_adds(rho_m, y1i)); /* :589-594 */
  const int32_t rmp = nr_rxl_abs(nr_rxl_adds(rho_m, y1r)), ipp = nr_rxl_abs(nr_rxl_adds(rho_p, y1i)); /* :597-602 */
  const int32_t num_re_p = nr_rxl_adds(nr_rxl_adds(nr_rxl_adds(rpm, imm), y0r), y0i);            /* :610-612 */
  const int32_t num_re_m = nr_rxl_subs(nr_rxl_adds(nr_rxl_adds(rmm, ipp), y0r), y0i);            /* :616-618 */
  const int32_t den_re_p = nr_rxl_adds(nr_rxl_subs(nr_rxl_adds(rmp, ipm), y0r), y0i);            /* :622-624 */
  const int32_t den_re_m = nr_rxl_subs(nr_rxl_subs(nr_rxl_adds(rpp, imp), y0r), y0i);            /* :628-630 */
  /* :634-654: num_im_p = num_re_p, num_im_m = den_re_p, den_im_p = num_re_m, den_im_m = den_re_m, the same sums again */
  const int32_t l0 = nr_rxl_subs(nr_rxl_max(num_re_p, num_re_m), nr_rxl_max(den_re_p, den_re_m)); /* :660-665: num - den */
  const int32_t l1 = nr_rxl_subs(nr_rxl_max(num_re_p, den_re_p), nr_rxl_max(num_re_m, den_re_m)); /* :662-666 */
  llr[0] = l0 >> 4; /* :2095 */
  llr[1] = l1 >> 4;
}

/* ---- 16QAM (nr_ulsch_qam16_qam16, :1124-1350) ---- */
/* interference_abs_epi16_256 (:830-837): cmpgt(int_ch_mag, psi) selects c1, else c2 */
NR_RXF_HD int32_t nr_rxl_interference_abs(int32_t psi, int32_t int_ch_mag, int32_t c1, int32_t c2) { return int_ch_mag > psi ? c1 : c2; }
/* prodsum_psi_a_epi16_256 (:820-827) */
NR_RXF_HD int32_t nr_rxl_prodsum_psi_a(int32_t psi_r, int32_t a_r, int32_t psi_i, int32_t a_i)
{
  return nr_rxl_adds(nr_rxl_mulhi2(psi_r, a_r), nr_rxl_mulhi2(psi_i, a_i));
}
/* one half of square_a_epi16_256 (:842-847 = :848-853); the function is the adds_epi16 of its two halves (:854) */
NR_RXF_HD int32_t nr_rxl_square_half(int32_t a, int32_t int_ch_mag, int32_t scale_factor)
{
  return nr_rxl_mulhi2(nr_rxl_mulhi2(nr_rxl_mulhi2(a, a), scale_factor), int_ch_mag);
}
/* max_epi16_256 (:875-884) */
NR_RXF_HD int32_t nr_rxl_max8(int32_t m0, int32_t m1, int32_t m2, int32_t m3, int32_t m4, int32_t m5, int32_t m6, int32_t m7)
{
  return nr_rxl_max(nr_rxl_max(nr_rxl_max(m0, m1), nr_rxl_max(m2, m3)), nr_rxl_max(nr_rxl_max(m4, m5), nr_rxl_max(m6, m7)));
}

/* y0 / mag0 = the desired stream's matched filter output and ul_ch_maga (its real half), y1 / mag1 = the interfering one's,
 * rho = rho[desired][interfering]; llr[4].  The candidate loop below is the reference's loops over j fused: bit metric j needs
 * psi_rs[j], psi_is[j] and what follows from them alone. */
NR_RXF_HD void nr_rxl_qam16(uint32_t y0, uint32_t y1, int32_t mag0, int32_t mag1, uint32_t rho, int32_t *llr)
{
  const int32_t ONE_OVER_SQRT_10 = 20724, ONE_OVER_SQRT_10_Q15 = 10362, THREE_OVER_SQRT_10 = 31086, SQRT_10_OVER_FOUR = 25905,
                ONE_OVER_TWO_SQRT_10 = 10362, NINE_OVER_TWO_SQRT_10 = 23315; /* :1132-1137 */
  const int32_t rr = nr_rxf_re(rho), ri = nr_rxf_im(rho);                       /* :1174 */
  const int32_t rho_rpi = nr_rxl_adds(rr, ri), rho_rmi = nr_rxl_subs(rr, ri);    /* :1175-1176 */
  int32_t rho_rs[8] = {0}, y0_s[8] = {0}, bit_mets[16] = {0};
  rho_rs[0] = nr_rxl_mulhi(rho_rpi, ONE_OVER_SQRT_10);                          /* :1179 */
  rho_rs[4] = nr_rxl_mulhi(rho_rmi, ONE_OVER_SQRT_10);                          /* :1180 */
  rho_rs[3] = nr_rxl_mulhi2(rho_rpi, THREE_OVER_SQRT_10);                       /* :1181 */
  rho_rs[7] = nr_rxl_mulhi2(rho_rmi, THREE_OVER_SQRT_10);                       /* :1182 */
  const int32_t x4 = nr_rxl_mulhi(rr, ONE_OVER_SQRT_10), x5 = nr_rxl_mulhi2(ri, THREE_OVER_SQRT_10); /* :1184-1186 */
  rho_rs[1] = nr_rxl_adds(x4, x5);                                              /* :1188 */
  rho_rs[5] = nr_rxl_subs(x4, x5);                                              /* :1189 */
  const int32_t x6 = nr_rxl_mulhi2(rr, THREE_OVER_SQRT_10), x7 = nr_rxl_mulhi(ri, ONE_OVER_SQRT_10); /* :1191-1193 */
  rho_rs[2] = nr_rxl_adds(x6, x7);                                              /* :1195 */
  rho_rs[6] = nr_rxl_subs(x6, x7);                                              /* :1196 */
  const int32_t y1r = nr_rxf_re(y1), y1i = nr_rxf_im(y1), y0r = nr_rxf_re(y0), y0i = nr_rxf_im(y0); /* :1199, :1217 */
  const int32_t r1 = nr_rxl_mulhi(y0r, ONE_OVER_SQRT_10), i1 = nr_rxl_mulhi(y0i, ONE_OVER_SQRT_10);       /* :1227-1228 */
  const int32_t r3 = nr_rxl_mulhi2(y0r, THREE_OVER_SQRT_10), i3 = nr_rxl_mulhi2(y0i, THREE_OVER_SQRT_10); /* :1229-1230 */
  y0_s[0] = nr_rxl_adds(r1, i1); /* :1233-1243 */
  y0_s[4] = nr_rxl_subs(r1, i1);
  y0_s[1] = nr_rxl_adds(r1, i3);
  y0_s[5] = nr_rxl_subs(r1, i3);
  y0_s[2] = nr_rxl_adds(r3, i1);
  y0_s[6] = nr_rxl_subs(r3, i1);
  y0_s[3] = nr_rxl_adds(r3, i3);
  y0_s[7] = nr_rxl_subs(r3, i3);
  const int32_t ch_mag_over_10 = nr_rxl_mulhi(mag0, ONE_OVER_TWO_SQRT_10);                   /* :1258 */
  const int32_t ch_mag_over_2 = nr_rxl_mulhi2(mag0, SQRT_10_OVER_FOUR);                      /* :1259-1260 */
  const int32_t ch_mag_9_over_10 = nr_rxl_slli(nr_rxl_mulhi(mag0, NINE_OVER_TWO_SQRT_10), 2); /* :1261-1262 */
  const uint8_t rho_rs_indexes[16] = {4, 6, 5, 7, 0, 2, 1, 3, 0, 2, 1, 3, 4, 6, 5, 7};       /* :1208 */
  /* a_r and a_i take two values, so square_a_epi16_256's halves (:842-853) take two: formed once per RE, selected per metric */
  const int32_t sq_1 = nr_rxl_square_half(ONE_OVER_SQRT_10_Q15, mag1, SQRT_10_OVER_FOUR);
  const int32_t sq_3 = nr_rxl_square_half(THREE_OVER_SQRT_10, mag1, SQRT_10_OVER_FOUR);
  NR_RXL_UNROLL
  for (int j = 0; j < 16; j++) {
    /* :1202-1207 */
    const int32_t psi_r = j < 8 ? nr_rxl_abs(nr_rxl_subs(rho_rs[j & 7], y1r)) : nr_rxl_abs(nr_rxl_adds(rho_rs[(j - 4) & 7], y1r));
    /* :1209-1214: subs for j % 8 < 4, adds for the rest */
    const int32_t rq = rho_rs[rho_rs_indexes[j]];
    const int32_t psi_i = (j & 4) ? nr_rxl_abs(nr_rxl_adds(rq, y1i)) : nr_rxl_abs(nr_rxl_subs(rq, y1i));
    const int32_t a_r = nr_rxl_interference_abs(psi_r, mag1, ONE_OVER_SQRT_10_Q15, THREE_OVER_SQRT_10); /* :1247 */
    const int32_t a_i = nr_rxl_interference_abs(psi_i, mag1, ONE_OVER_SQRT_10_Q15, THREE_OVER_SQRT_10); /* :1248 */
    const int32_t psi_a = nr_rxl_prodsum_psi_a(psi_r, a_r, psi_i, a_i);                                 /* :1251 */
    const int32_t a_sq = nr_rxl_adds(mag1 > psi_r ? sq_1 : sq_3, mag1 > psi_i ? sq_1 : sq_3);           /* :1254 -> :854 */
    const int32_t chm = (j & 3) == 0 ? ch_mag_over_10 : ((j & 3) == 3 ? ch_mag_9_over_10 : ch_mag_over_2);
    int32_t b = nr_rxl_subs(psi_a, a_sq);                                                               /* :1268-1297 */
    b = j < 8 ? nr_rxl_adds(b, y0_s[j & 7]) : nr_rxl_subs(b, y0_s[(j - 4) & 7]);
    bit_mets[j] = nr_rxl_subs(b, chm);
  }
  const int32_t *m = bit_mets;
  const int32_t num_re0 = nr_rxl_max8(m[8], m[9], m[10], m[11], m[12], m[13], m[14], m[15]); /* :1305 */
  const int32_t den_re0 = nr_rxl_max8(m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7]);       /* :1307 */
  const int32_t num_re1 = nr_rxl_max8(m[4], m[5], m[6], m[7], m[12], m[13], m[14], m[15]);   /* :1309 */
  const int32_t den_re1 = nr_rxl_max8(m[0], m[1], m[3], m[2], m[8], m[9], m[10], m[11]);     /* :1311 */
  const int32_t num_im0 = nr_rxl_max8(m[2], m[3], m[6], m[7], m[10], m[11], m[14], m[15]);   /* :1313 */
  const int32_t den_im0 = nr_rxl_max8(m[0], m[1], m[4], m[5], m[8], m[9], m[12], m[13]);     /* :1315 */
  const int32_t num_im1 = nr_rxl_max8(m[1], m[3], m[5], m[7], m[9], m[11], m[13], m[15]);    /* :1317 */
  const int32_t den_im1 = nr_rxl_max8(m[0], m[2], m[4], m[6], m[8], m[10], m[12], m[14]);    /* :1319 */
  llr[0] = nr_rxl_subs(den_re0, num_re0); /* :1321-1324: den - num, where QPSK forms num - den; the packing :1332-1349 puts an */
  llr[1] = nr_rxl_subs(den_re1, num_re1); /* RE's four side by side in this order */
  llr[2] = nr_rxl_subs(den_im0, num_im0);
  llr[3] = nr_rxl_subs(den_im1, num_im1);
}

/* the Qm LLRs of layer l of one RE after the antennas are in (:2115-2121: layer 1 is the same function with the streams, the
 * magnitudes and rho swapped) */
NR_RXF_HD void nr_rxl_llr(const nr_rxl_re_t *R, uint32_t Qm, uint32_t l, int32_t *llr)
{
  const uint32_t y0 = R->l[l].w[0], y1 = R->l[l ^ 1u].w[0], rho = l == 0 ? R->rho01 : R->rho10;
  if (Qm == 2)
    nr_rxl_qpsk(y0, y1, rho, llr);
  else
    nr_rxl_qam16(y0, y1, nr_rxf_re(R->l[l].w[1]), nr_rxf_re(R->l[l ^ 1u].w[1]), rho, llr);
}

/* ---- channel level of a two-layer block below 64QAM (:1639-1647): neither the MMSE's - 3 nor the single layer's term ---- */
NR_RXF_HD int32_t nr_rxl_log2_maxh(int32_t avgs)
{
  const int32_t v = nr_rxf_log2_approx((uint32_t)(avgs < 0 ? 0 : avgs)) >> 1;
  return v < 0 ? 0 : v;
}
#endif
