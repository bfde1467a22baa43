/*
 * tb_tx_sym.h -- symbol formation of the fused TX symbol store (tb_chain.hip tb_tx_fused_sym_kernel, nrLDPC_hip_dlsch_encode_symbols):
 * the reference's nr_dlsch_coding output scrambled (nr_scrambling.c:27-46), mapped (nr_modulation, nr_modulation.c:115-244) and
 * layer mapped for one codeword (nr_layer_mapping, nr_modulation.c:246-270) by one thread per modulation symbol, straight from
 * the Qm interleaver sub-streams a selection chunk holds in LDS.
 *
 * Symbol jj of a chunk: its bit i (index bit i of the constellation) is bit jj of sub-stream i -- f[jj Qm + i] of the segment
 * (nr_rate_matching.c:262-268) -- XOR codeword bit (b_lo + jj Qm + i) of the sequence; its point goes to layer plane s mod Nl,
 * entry s div Nl of the TB's record, s = the symbol's place in the codeword.  Every segment's E is a multiple of Qm Nl
 * (nr_hip_get_E), so a segment owns whole symbols: each point is written by exactly one thread, and nothing is read back.
 * Compiles as HIP device code and as plain host C++ (tests/emul/tb_tx_sym_emul.cpp runs the same code on the CPU).
 */
#ifndef TB_TX_SYM_H
#define TB_TX_SYM_H
#include <stdint.h>

#if defined(__HIPCC__)
#define TB_TX_HD __device__ __forceinline__
#else
#define TB_TX_HD static inline
#endif

/* one selection chunk of one segment */
struct tb_tx_sym_chunk {
  const uint32_t *sel;  /* sub-stream i, symbol jj: bit jj & 31 of sel[i * sel_stride + jj / 32] */
  uint32_t sel_stride;
  const uint32_t *seq;  /* the chunk's sequence words: seq[0] = word b_lo / 32 of the TB's sequence */
  uint32_t q0;          /* b_lo % 32: bit of seq[0] that goes with the chunk's first bit */
  uint32_t s0;          /* codeword symbol of the chunk's first symbol (bit_off / Qm + jj0) */
  uint32_t Nl, plane;   /* layers (1..4), words from one layer plane to the next */
};

/* constellation index of symbol jj of the chunk: its Qm interleaved bits XOR its Qm sequence bits (for Qm = 6 they can
 * straddle two sequence words; the second is read only then, and it lies inside the chunk's words) */
template <int QM> TB_TX_HD uint32_t tb_tx_sym_index(const tb_tx_sym_chunk &c, uint32_t jj)
{
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < QM; i++)
    x |= ((c.sel[(uint32_t)i * c.sel_stride + (jj >> 5)] >> (jj & 31u)) & 1u) << i;
  const uint32_t b = c.q0 + jj * (uint32_t)QM, k = b >> 5, sh = b & 31u;
  uint32_t q = c.seq[k] >> sh;
  if (sh + (uint32_t)QM > 32u)
    q |= c.seq[k + 1u] << (32u - sh);
  return (x ^ q) & ((1u << QM) - 1u);
}

/* word of the TB's record that codeword symbol s goes to: plane s mod Nl, entry s div Nl (no division: Nl is 1..4) */
TB_TX_HD uint32_t tb_tx_sym_dst(uint32_t s, uint32_t Nl, uint32_t plane)
{
  const uint32_t k = Nl == 3u ? (uint32_t)(((uint64_t)s * 0xAAAAAAABull) >> 33) : s >> (Nl >> 1);
  return (s - k * Nl) * plane + k;
}

/* the chunk's nsym points: thread tid of nt stores symbols tid, tid + nt, ...; tab = the 2^QM points of nr_qam.h (nr_qam_point) */
template <int QM>
TB_TX_HD void tb_tx_sym_store(const tb_tx_sym_chunk &c, const uint32_t *tab, uint32_t nsym, uint32_t *out32, uint32_t tid, uint32_t nt)
{
  for (uint32_t jj = tid; jj < nsym; jj += nt)
    out32[tb_tx_sym_dst(c.s0 + jj, c.Nl, c.plane)] = tab[tb_tx_sym_index<QM>(c, jj)];
}
#endif
