/*
 * nr_pdsch_map.h -- PDSCH resource mapping of one OFDM symbol of one allocation, one layer, one RE at a time: the resource
 * mapping loop of nr_generate_pdsch() (openair1/PHY/NR_TRANSPORT/nr_dlsch.c:205-474) with the DMRS tables of nr_sch_dmrs.c:37-87
 * and the helper semantics of openair1/PHY/TOOLS/tools_defs.h:214-217.  Plain C (no HIP headers): the host check form
 * (tx_map_api.inc.cpp) and the kernel (tb_tx_map.hip) compute with the same definitions.
 *
 * A c16 is one 32-bit word, r in the low half.  i = 0 .. 12 rb_size - 1 is the subcarrier relative to the allocation; it is
 * written at grid subcarrier (start_re + i) mod fft_size.  What an RE is depends on r = i % 12 alone, so a symbol of a layer
 * has two 12-bit masks (nr_pdm_masks): pmask, the pilots of the layer's port, and dmask, the data REs; an RE in neither is 0.
 *   FULL   every RE is data: mulhrs(amp, x) per component, ((x amp >> 14) + 1) >> 1 cast to int16 (:405-412).
 *   DMRS1  pilots at r % 2 == delta (i = 4n + 2k' + delta), data at r % 2 >= ncdm.
 *   DMRS2  pilots at r % 6 in {delta, delta + 1} (i = 6n + k' + delta), data at r % 6 >= 2 ncdm.
 * The pilot test comes first (:316-318), so a port whose CDM group the caller counts among those with data still gets its pilots.
 * Pilot j of the allocation (ascending with i, k' = j & 1) is sequence symbol dmrs_offset + j of the Gold sequence of c_init
 * (nr_gold.c:87-88): the QPSK point (nr_qam.h, Qm = 2) of index bit 0 = sequence bit 2 (dmrs_offset + j), bit 1 = the next,
 * times Wt[l'] Wf[k'] amp at shift 15, an arithmetic shift that floors (c16mulRealShift, :318).  A data RE of a DMRS symbol is
 * x amp >> 15, truncating and not mulhrs (:359).  x is the next unread entry of the layer plane: data RE i reads entry
 * nr_pdm_count(dmask, i) of the symbol's stretch.
 *
 * Two defects of the reference are not reproduced: the scalar tail of the FULL loop that omits the final
 * shift (:428-435, :460-467), and allowed_xlsch_re_in_dmrs_symbol's diff = fft_size at the allocation's first subcarrier
 * (dmrs_nr.c:45-48).  Here the pattern is decided by i, never by the grid subcarrier.
 *
 * Precoding (nr_dlsch.c:486-589): antenna a of an RE whose PRG has pmi = 0 takes layer a's value, or 0 behind the layers, as a
 * copy; with pmi != 0 it is the sum over the layers l = 0 .. Nl - 1 of m_l w[l][a] as nr_layer_precoder_simd computes it
 * (nr_modulation.c:785-811): per term the two madd_epi16 sums as wrapping int32, >> 15, the low 16 bits; w.i negated as an int16
 * (-(-32768) stays -32768); the terms accumulated from 0 with adds_epi16, which saturates (nr_pdm_prec_term, nr_pdm_adds16,
 * nr_pdm_antenna).  The reference's nr_layer_precoder_cm for the RB step at the end of the symbol is not reproduced (DESIGN
 * section 5).  The pilots of all layers come out of one run of Gold bits: it starts at the pilot number that the port with the
 * latest pilots (nr_pdm_last_pmask) has reached, which is at most 2 below every other port's.
 */
#ifndef NR_PDSCH_MAP_H
#define NR_PDSCH_MAP_H
#include <stdint.h>
#include "nr_qam.h"

#if defined(__HIPCC__)
#define NR_PDM_HD __host__ __device__ static inline
#else
#define NR_PDM_HD static inline
#endif

#define NR_PDM_FULL 0u
#define NR_PDM_DMRS1 1u
#define NR_PDM_DMRS2 2u
#define NR_PDM_PATTERNS 3u
#define NR_PDM_MAX_LAYERS 4u
#define NR_PDM_MAX_TX 8u

/* columns delta, Wf(1), Wt(1) of the tables of nr_sch_dmrs.c:37-57 (Wf(0) = Wt(0) = 1): Wf(1) = -1 for odd ports; Wt(1) = -1 for
 * ports 4..7 (type 1) / 6..11 (type 2); delta = the CDM group (type 1) or twice it (type 2) */
NR_PDM_HD uint32_t nr_pdm_ports(uint32_t pattern) { return pattern == NR_PDM_DMRS2 ? 12u : 8u; }
NR_PDM_HD uint32_t nr_pdm_delta(uint32_t pattern, uint32_t port) { return pattern == NR_PDM_DMRS2 ? 2u * ((port % 6u) >> 1) : (port >> 1) & 1u; }
NR_PDM_HD int32_t nr_pdm_wf1(uint32_t port) { return (port & 1u) ? -1 : 1; }
NR_PDM_HD int32_t nr_pdm_wt1(uint32_t pattern, uint32_t port) { return port >= (pattern == NR_PDM_DMRS2 ? 6u : 4u) ? -1 : 1; }
NR_PDM_HD uint32_t nr_pdm_max_ncdm(uint32_t pattern) { return pattern == NR_PDM_DMRS2 ? 3u : 2u; }

NR_PDM_HD uint32_t nr_pdm_popc(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(x);
#else
  return (uint32_t)__builtin_popcount(x);
#endif
}

/* the pilot and data REs of one PRB, bit r = subcarrier r */
NR_PDM_HD void nr_pdm_masks(uint32_t pattern, uint32_t ncdm, uint32_t delta, uint32_t *pmask, uint32_t *dmask)
{
  uint32_t p = 0, d = 0;
  for (uint32_t r = 0; r < 12u; r++) {
    uint32_t pil, dat;
    if (pattern == NR_PDM_FULL) {
      pil = 0;
      dat = 1;
    } else if (pattern == NR_PDM_DMRS1) {
      pil = r % 2u == delta;
      dat = r % 2u >= ncdm;
    } else {
      pil = r % 6u == delta || r % 6u == delta + 1u;
      dat = r % 6u >= 2u * ncdm;
    }
    p |= pil << r;
    d |= (dat && !pil) << r;
  }
  *pmask = p;
  *dmask = d;
}
/* REs of `mask` below allocation subcarrier i: the pilot number of a pilot RE, the layer plane entry of a data RE */
NR_PDM_HD uint32_t nr_pdm_count(uint32_t mask, uint32_t i)
{
  const uint32_t b = i / 12u, r = i - 12u * b;
  return b * nr_pdm_popc(mask) + nr_pdm_popc(mask & ((1u << r) - 1u));
}

NR_PDM_HD uint32_t nr_pdm_pack(int32_t r, int32_t i) { return ((uint32_t)r & 0xffffu) | ((uint32_t)i << 16); }
/* simde_mm_mulhrs_epi16 per component */
NR_PDM_HD uint32_t nr_pdm_mulhrs(uint32_t x, int32_t amp)
{
  const int32_t r = (int16_t)(x & 0xffffu), i = (int16_t)(x >> 16);
  return nr_pdm_pack((((r * amp) >> 14) + 1) >> 1, (((i * amp) >> 14) + 1) >> 1);
}
/* c16mulRealShift(x, w, 15): the int32 product shifted arithmetically, w may be negative */
NR_PDM_HD uint32_t nr_pdm_mul_real15(uint32_t x, int32_t w)
{
  const int32_t r = (int16_t)(x & 0xffffu), i = (int16_t)(x >> 16);
  return nr_pdm_pack((r * w) >> 15, (i * w) >> 15);
}
/* the pilot of sequence symbol s = dmrs_offset + j: its two bits in the low bits of b; w = Wt[l'] amp, wf1 = Wf(1) */
NR_PDM_HD uint32_t nr_pdm_pilot(uint32_t b, uint32_t j, int32_t w, int32_t wf1)
{
  const int32_t a = (int16_t)(nr_qam_point(2u, 0u) & 0xffffu); /* the QPSK table is (+-a, +-a), minus where the bit is set */
  return nr_pdm_mul_real15(nr_pdm_pack((b & 1u) ? -a : a, (b & 2u) ? -a : a), (j & 1u) ? w * wf1 : w);
}

/* what the mapping of one layer's symbol needs, derived once per (segment, layer) */
typedef struct nr_pdm_sym {
  uint32_t pattern, pmask, dmask;
  int32_t amp, w, wf1; /* w = Wt[l'] amp */
} nr_pdm_sym;
NR_PDM_HD nr_pdm_sym nr_pdm_sym_make(uint32_t pattern, uint32_t ncdm, uint32_t l_prime, uint32_t port, int32_t amp)
{
  nr_pdm_sym s;
  s.pattern = pattern;
  nr_pdm_masks(pattern, ncdm, nr_pdm_delta(pattern, port), &s.pmask, &s.dmask);
  s.amp = amp;
  s.w = l_prime ? nr_pdm_wt1(pattern, port) * amp : amp;
  s.wf1 = nr_pdm_wf1(port);
  return s;
}
/* the value of allocation subcarrier i.  lay = the symbol's stretch of the layer plane (entry 0 = sym_off); bits = the Gold
 * bits from sequence symbol dmrs_offset + jlo on, jlo <= the pilot number of i, at most 31 pilots ahead */
NR_PDM_HD uint32_t nr_pdm_re(const nr_pdm_sym *s, const uint32_t *lay, uint32_t i, uint64_t bits, uint32_t jlo)
{
  const uint32_t r = i % 12u;
  if ((s->pmask >> r) & 1u) {
    const uint32_t j = nr_pdm_count(s->pmask, i);
    return nr_pdm_pilot((uint32_t)(bits >> (2u * (j - jlo))), j, s->w, s->wf1);
  }
  if ((s->dmask >> r) & 1u) {
    const uint32_t x = lay[nr_pdm_count(s->dmask, i)];
    return s->pattern == NR_PDM_FULL ? nr_pdm_mulhrs(x, s->amp) : nr_pdm_mul_real15(x, s->amp);
  }
  return 0u;
}
/* the pilot mask of the ports with the largest delta: nr_pdm_count of it is the smallest among all ports at every i */
NR_PDM_HD uint32_t nr_pdm_last_pmask(uint32_t pattern)
{
  uint32_t pm = 0, dm = 0;
  if (pattern != NR_PDM_FULL)
    nr_pdm_masks(pattern, 1u, pattern == NR_PDM_DMRS2 ? 4u : 1u, &pm, &dm);
  return pm;
}

/* ---- precoding: layers to one antenna ---- */
/* one term of nr_layer_precoder_simd: x w >> 15, the sums wrapping in 32 bits, the shifted value cut to 16 bits */
NR_PDM_HD uint32_t nr_pdm_prec_term(uint32_t x, uint32_t w)
{
  const int32_t xr = (int16_t)(x & 0xffffu), xi = (int16_t)(x >> 16), wr = (int16_t)(w & 0xffffu), wi = (int16_t)(w >> 16);
  const int32_t nwi = (int16_t)(-wi); /* c16conj: the negation is cast back to int16 */
  const uint32_t re = (uint32_t)(xr * wr) + (uint32_t)(xi * nwi), im = (uint32_t)(xr * wi) + (uint32_t)(xi * wr);
  return nr_pdm_pack((int32_t)re >> 15, (int32_t)im >> 15);
}
NR_PDM_HD int32_t nr_pdm_sat16(int32_t v) { return v > 32767 ? 32767 : (v < -32768 ? -32768 : v); }
/* simde_mm_adds_epi16 per component */
NR_PDM_HD uint32_t nr_pdm_adds16(uint32_t y, uint32_t t)
{
  return nr_pdm_pack(nr_pdm_sat16((int16_t)(y & 0xffffu) + (int16_t)(t & 0xffffu)), nr_pdm_sat16((int16_t)(y >> 16) + (int16_t)(t >> 16)));
}
/* antenna ant's value of one RE from the mapped values m[l] of its layers l < Nl (the others are not read).  pmi == 0: the copy of
 * layer ant, 0 behind the layers; otherwise w[l] = weights[l][ant] of the PRG's matrix */
NR_PDM_HD uint32_t nr_pdm_antenna(const uint32_t *m, const uint32_t *w, uint32_t Nl, uint32_t ant, uint32_t pmi)
{
  uint32_t y = 0u;
  for (uint32_t l = 0; l < NR_PDM_MAX_LAYERS; l++)
    if (l < Nl) {
      if (pmi)
        y = nr_pdm_adds16(y, nr_pdm_prec_term(m[l], w[l]));
      else if (l == ant)
        y = m[l];
    }
  return y;
}

/* (k0 + off) % N for k0 < N, off < N */
NR_PDM_HD uint32_t nr_pdm_wrap(uint32_t k0, uint32_t off, uint32_t N) { return k0 + off >= N ? k0 + off - N : k0 + off; }
#endif
