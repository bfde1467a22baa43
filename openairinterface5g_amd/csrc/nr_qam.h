/*
 * nr_qam.h -- the constellations of 38.211 section 5.1 as the reference tabulates them (openair1/PHY/NR_REFSIG/
 * nr_gen_mod_table.c nr_generate_modulation_table), and the per-RE soft demapper of the UL-SCH receiver (openair1/PHY/
 * NR_TRANSPORT/nr_ulsch_llr_computation.c nr_ulsch_compute_llr).  Plain C (no HIP headers), constexpr in C++: the host code
 * (nr_coding_host.c) and the HIP kernels (tb_qam.hip, tb_rx_core.h) use the same definitions.
 *
 * Point of index x (bit b of x = codeword bit iQm + b of symbol i): re from the even bits, im from the odd bits,
 *   level = (1 - 2 x0) (2^(Qm/2 - 1) - (1 - 2 x2) (2^(Qm/2 - 2) - (1 - 2 x4) (... )))   (x1, x3, ... for im)
 *   value = (short)((float)level * 32768.f * s * 0.70711f), s = 0.70711 / 0.31623 / 0.15430 / 0.076696 for Qm = 2/4/6/8
 * -- float32 products evaluated left to right and truncated toward zero, as the reference computes them.
 *
 * Demapper, per RE: A = y (QPSK: A >> 3, arithmetic), B = subs(mag_a, |A|), C = subs(mag_b, |B|), D = subs(mag_c, |C|);
 * the RE's LLRs are A.r A.i B.r B.i C.r C.i D.r D.i cut to Qm values.  |x| is _mm_abs_epi16 (|-32768| = -32768), subs the
 * saturating int16 subtraction.  A c16 value is held as a 32-bit word, re in the low half: LLR word k of an RE is level k.
 */
#ifndef NR_QAM_H
#define NR_QAM_H
#include <stdint.h>

#if defined(__HIPCC__)
#define NR_QAM_HD __host__ __device__ static inline constexpr
#elif defined(__cplusplus)
#define NR_QAM_HD static inline constexpr
#else
#define NR_QAM_HD static inline
#endif

/* the four tables one after another: 4 + 16 + 64 + 256 points, each (re, im) as a word, re in the low half */
#define NR_QAM_POINTS 340
NR_QAM_HD uint32_t nr_qam_table_off(uint32_t Qm) { return Qm == 2 ? 0u : Qm == 4 ? 4u : Qm == 6 ? 20u : 84u; }

/* one axis: bits (x >> first) & 1, (x >> first + 2) & 1, ... of an index, Qm / 2 of them */
NR_QAM_HD int16_t nr_qam_axis(uint32_t Qm, uint32_t x, uint32_t first)
{
  const float val = 32768.0f, sqrt2 = 0.70711f;
  const float s = Qm == 2 ? 0.70711f : Qm == 4 ? 0.31623f : Qm == 6 ? 0.15430f : 0.076696f;
  const int n = (int)Qm / 2;
  int level = 1; /* innermost term first: 2 - (1 - 2 x_last), then 4 - (1 - 2 x_last-1) (that), ...; QPSK: 1 */
  for (int k = 1; k < n; k++)
    level = (1 << k) - (1 - 2 * (int)((x >> (first + 2u * (uint32_t)(n - k))) & 1u)) * level;
  level *= 1 - 2 * (int)((x >> first) & 1u);
  return (int16_t)((float)(short)level * val * s * sqrt2);
}
NR_QAM_HD uint32_t nr_qam_point(uint32_t Qm, uint32_t x)
{
  return (uint32_t)(uint16_t)nr_qam_axis(Qm, x, 0u) | ((uint32_t)(uint16_t)nr_qam_axis(Qm, x, 1u) << 16);
}

typedef struct nr_qam_tables {
  uint32_t pt[NR_QAM_POINTS];
} nr_qam_tables_t;
NR_QAM_HD nr_qam_tables_t nr_qam_make_tables(void)
{
  nr_qam_tables_t t = {{0}};
  for (uint32_t Qm = 2; Qm <= 8; Qm += 2)
    for (uint32_t x = 0; x < (1u << Qm); x++)
      t.pt[nr_qam_table_off(Qm) + x] = nr_qam_point(Qm, x);
  return t;
}

/* ---- demapper, two int16 lanes per word ---- */
NR_QAM_HD uint32_t nr_qam_lanes(int32_t lo, int32_t hi) { return (uint32_t)(uint16_t)lo | ((uint32_t)(uint16_t)hi << 16); }
/* QPSK: (y.r >> 3, y.i >> 3) */
NR_QAM_HD uint32_t nr_qam_shr3(uint32_t y) { return nr_qam_lanes((int16_t)(uint16_t)y >> 3, (int16_t)(uint16_t)(y >> 16) >> 3); }
/* subs(m, abs(x)) per lane */
NR_QAM_HD int32_t nr_qam_subs_abs1(int32_t m, int32_t x)
{
  const int32_t a = x == -32768 ? -32768 : (x < 0 ? -x : x);
  const int32_t d = m - a;
  return d > 32767 ? 32767 : (d < -32768 ? -32768 : d);
}
NR_QAM_HD uint32_t nr_qam_subs_abs(uint32_t m, uint32_t x)
{
  return nr_qam_lanes(nr_qam_subs_abs1((int16_t)(uint16_t)m, (int16_t)(uint16_t)x),
                      nr_qam_subs_abs1((int16_t)(uint16_t)(m >> 16), (int16_t)(uint16_t)(x >> 16)));
}
/* w[0] = y, w[1 .. Qm/2) = mag_a, mag_b, mag_c on entry; the RE's Qm LLRs (level k in w[k]) on exit */
NR_QAM_HD void nr_qam_demap(uint32_t Qm, uint32_t *w)
{
  if (Qm == 2) {
    w[0] = nr_qam_shr3(w[0]);
    return;
  }
  for (uint32_t k = 1; k < Qm / 2; k++)
    w[k] = nr_qam_subs_abs(w[k], w[k - 1]);
}
#endif
