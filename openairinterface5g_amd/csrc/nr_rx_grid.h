/*
 * nr_rx_grid.h -- where the data REs of one PUSCH OFDM symbol lie in the FFT output grid and in the full-width channel
 * estimates: nr_ulsch_extract_rbs() (openair1/PHY/NR_TRANSPORT/nr_ulsch_demodulation.c:279-380) in closed form, and the
 * per-allocation arithmetic of nr_rx_pusch_tp() around it (:292 start_re, :417-431 get_nb_re_pusch, :1584-1589 the measurement
 * symbol, :1660-1663 llr_offset).  Plain C (no HIP headers), constexpr in C++: the host checks and extraction
 * (rx_grid_api.inc.cpp) and the kernels (tb_rx_front.hip) index with the same definitions.  delta = 0 as in the reference.
 *
 * A symbol has a pattern; data RE j of the symbol is PUSCH subcarrier p(j) of the allocation:
 *   FULL  (no DMRS in the symbol, :301-312)       all 12 subcarriers of an RB    p(j) = j
 *   DMRS1 (type 1, :313-342)                      the odd ones, 6 per RB         p(j) = 2j + 1
 *   DMRS2 (type 2, :343-379)                      those with p % 6 >= 2, 8       p(j) = 6 (j / 4) + 2 + j % 4
 * It is read from the grid at subcarrier (start_re + p(j)) mod N -- the grid wraps at the OFDM symbol size N -- and its channel
 * estimate at ch[p(j)]: the estimates are indexed linearly from choffset and do not wrap.  The first nb_re data REs of the
 * pattern's sequence are taken; that is get_nb_re_pusch whatever num_dmrs_cdm_grps_no_data is.
 *
 * Why this equals the reference's two-piece loops: start_re = (first_carrier_offset + 12 rb) % N with first_carrier_offset =
 * N - 6 N_RB makes N - start_re a multiple of 6, so the second piece restarts on the same residue mod 2 and mod 6 and idx2
 * carries the channel index on.  An allocation that ends exactly at N takes the two-piece branch on DMRS symbols (`<` at :317
 * and :346, `<=` at :302) with pos_length = 0: the same result.  The one-piece type-2 branch reads rxF[idx] (:352) where every
 * other branch reads rxF[start_re + idx]; that is a defect of the reference and is not reproduced.
 */
#ifndef NR_RX_GRID_H
#define NR_RX_GRID_H
#include "nr_rx_front.h"

#define NR_RXG_FULL 0u
#define NR_RXG_DMRS1 1u
#define NR_RXG_DMRS2 2u
#define NR_RXG_PATTERNS 3u
#define NR_RXG_SYMBOLS 14u /* symbols_per_slot, normal cyclic prefix */

/* PUSCH subcarrier of data RE j */
NR_RXF_HD uint32_t nr_rxg_p(uint32_t pattern, uint32_t j)
{
  return pattern == NR_RXG_DMRS1 ? 2u * j + 1u : (pattern == NR_RXG_DMRS2 ? 6u * (j >> 2) + 2u + (j & 3u) : j);
}
/* data REs of the pattern among PUSCH subcarriers 0 .. n_sc - 1 */
NR_RXF_HD uint32_t nr_rxg_count(uint32_t pattern, uint32_t n_sc)
{
  return pattern == NR_RXG_DMRS1 ? n_sc / 2u : (pattern == NR_RXG_DMRS2 ? 4u * (n_sc / 6u) + (n_sc % 6u > 2u ? n_sc % 6u - 2u : 0u) : n_sc);
}
/* grid subcarrier of PUSCH subcarrier p: start_re < N and p < N, one wrap at the most */
NR_RXF_HD uint32_t nr_rxg_grid_sc(uint32_t start_re, uint32_t p, uint32_t N) { return start_re + p >= N ? start_re + p - N : start_re + p; }

/* ---- per allocation ---- */
/* :292 */
NR_RXF_HD uint32_t nr_rxg_start_re(uint32_t first_carrier_offset, uint32_t bwp_start, uint32_t rb_start, uint32_t N)
{
  return (uint32_t)(((uint64_t)first_carrier_offset + ((uint64_t)rb_start + bwp_start) * 12u) % N);
}
NR_RXF_HD uint32_t nr_rxg_is_dmrs(uint32_t ul_dmrs_symb_pos, uint32_t symbol) { return (ul_dmrs_symb_pos >> symbol) & 1u; }
/* :421: a DMRS symbol whose successor (mod the slot) is one too is not supported by the reference */
NR_RXF_HD uint32_t nr_rxg_double_dmrs(uint32_t ul_dmrs_symb_pos, uint32_t symbol)
{
  return nr_rxg_is_dmrs(ul_dmrs_symb_pos, symbol) & nr_rxg_is_dmrs(ul_dmrs_symb_pos, (symbol + 1u) % NR_RXG_SYMBOLS);
}
/* get_nb_re_pusch (:417-431); dmrs_config_type 0 = type 1, 1 = type 2 as in the PUSCH PDU */
NR_RXF_HD uint32_t nr_rxg_nb_re(uint32_t ul_dmrs_symb_pos, uint32_t symbol, uint32_t dmrs_config_type, uint32_t cdm_grps_no_data, uint32_t rb_size)
{
  return !nr_rxg_is_dmrs(ul_dmrs_symb_pos, symbol) ? rb_size * 12u
         : (dmrs_config_type == 0 ? rb_size * (12u - cdm_grps_no_data * 6u) : rb_size * (12u - cdm_grps_no_data * 4u));
}
NR_RXF_HD uint32_t nr_rxg_symbol_pattern(uint32_t ul_dmrs_symb_pos, uint32_t symbol, uint32_t dmrs_config_type)
{
  return !nr_rxg_is_dmrs(ul_dmrs_symb_pos, symbol) ? NR_RXG_FULL : (dmrs_config_type == 0 ? NR_RXG_DMRS1 : NR_RXG_DMRS2);
}
/* llr_offset[symbol] / Qm (:1661-1663): the data REs of the allocation's symbols before `symbol` */
NR_RXF_HD uint32_t nr_rxg_sym_off(uint32_t ul_dmrs_symb_pos, uint32_t start_symbol, uint32_t symbol, uint32_t dmrs_config_type,
                                  uint32_t cdm_grps_no_data, uint32_t rb_size)
{
  uint32_t off = 0;
  for (uint32_t s = start_symbol; s < symbol; s++)
    off += nr_rxg_nb_re(ul_dmrs_symb_pos, s, dmrs_config_type, cdm_grps_no_data, rb_size);
  return off;
}
/* the measurement symbol (:1584-1589): the first symbol of the allocation with data REs; start_symbol + nr_of_symbols if none */
NR_RXF_HD uint32_t nr_rxg_meas_symbol(uint32_t ul_dmrs_symb_pos, uint32_t start_symbol, uint32_t nr_of_symbols, uint32_t dmrs_config_type,
                                      uint32_t cdm_grps_no_data, uint32_t rb_size)
{
  uint32_t s = start_symbol;
  for (; s < start_symbol + nr_of_symbols; s++)
    if (nr_rxg_nb_re(ul_dmrs_symb_pos, s, dmrs_config_type, cdm_grps_no_data, rb_size) > 0)
      break;
  return s;
}
#endif
