/*
 * tb_tx_core.h -- per-thread bodies of the fused DL segment kernel's own phases (tb_chain.hip tb_tx_fused_body: one workgroup
 * takes a code block from the transport block's bytes to its rate-matched, interleaved output), the mirror of tb_rx_core.h:
 *   the segment word     dword w of c_r = b[r*(K'-L) ..] || CRC24B || fillers in LDS (nr_segmentation.c:147-175), from the
 *                        byte-aligned source, with the TB CRC bytes patched in (the block's last segment);
 *   the CB CRC piece     a thread's share of the CRC24B over that image, moved to the end of the string;
 *   the information-column word of the encoder's general path (Zc % 32 != 0; ldpc_enc_packed_core.h phase 0);
 *   the selection item   32 bits of an interleaver sub-stream, gathered from the packed code word
 *                        (nr_rate_matching.c:424-501, :240-303: f[i + jj*Qm] = e[i*E/Qm + jj], e[k] = d[position of rank
 *                        (rank0 + k) mod V], d[p] = code word bit p + 2Z);
 *   tb_tx_store_syms     the bit-per-byte store of a selection chunk (the packed and the symbol store: tb_tx_scr.h, tb_tx_sym.h).
 * The encoder's phases between them are ldpc_enc_packed_core.h / ldpc_enc_packed32.h.  Compiles as HIP device code and as
 * plain host C++ (tests/emul walks a workgroup's threads through the selection and the store against the oracle); no phase has
 * a dependency between threads except through the caller's barriers.
 */
#ifndef TB_TX_CORE_H
#define TB_TX_CORE_H
#include <stdint.h>
#include <type_traits>
#include "ldpc_enc_packed_core.h"

#ifndef TB_TX_HD
#if defined(__HIPCC__)
#define TB_TX_HD __device__ __forceinline__
#else
#define TB_TX_HD static inline
#endif
#endif

#if defined(__HIP_DEVICE_COMPILE__)
TB_TX_HD uint32_t tb_tx_umulhi(uint32_t a, uint32_t b) { return __umulhi(a, b); }
TB_TX_HD uint32_t tb_tx_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbyte(hi, lo, sh); }
#else
TB_TX_HD uint32_t tb_tx_umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
TB_TX_HD uint32_t tb_tx_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (sh & 3))); }
#endif

/* ---- the segment word ---------------------------------------------------------------------------------------------------
 * dword w of the segment's LDS image: bytes 4w .. 4w+3 of the source, which starts a0 bytes into the aligned dword lo (hi =
 * the dword behind it: the order of v_alignbyte_b32); the TB CRC bytes at crc_pos .. crc_pos + crc_len (last segment only; tb_crc left aligned); nothing
 * behind the segment's last byte. */
TB_TX_HD uint32_t tb_tx_seg_word(uint32_t hi, uint32_t lo, uint32_t a0, uint32_t w, uint32_t segbytes, uint32_t crc_pos, uint32_t crc_len,
                                 uint32_t tb_crc)
{
  uint32_t v = tb_tx_alignbyte(hi, lo, a0);
#pragma unroll
  for (int b = 0; b < 4; b++) {
    const uint32_t q = 4u * w + (uint32_t)b, kk = q - crc_pos;
    if (kk < crc_len)
      v = (v & ~(0xffu << (8 * b))) | (((tb_crc >> (24 - 8 * kk)) & 0xffu) << (8 * b));
    if (q >= segbytes)
      v &= ~(0xffu << (8 * b));
  }
  return v;
}

/* ---- the CB CRC piece ---------------------------------------------------------------------------------------------------
 * R(x) * Q(x) mod g for left-aligned registers of a degree-DEG generator (poly = x^DEG mod g, left aligned): one Horner
 * step per coefficient of R -- the power Q = x^n mod g is ONE table look-up, where summing pow[] over the set bits of R
 * was a dozen dependent global loads per thread (the TB CRC kernels spent most of their 13-17 us there). */
template <int DEG> TB_TX_HD uint32_t tb_crc_mulmod(uint32_t R, uint32_t Q, uint32_t poly)
{
  uint32_t x = 0;
#pragma unroll
  for (int k = 31; k >= 32 - DEG; k--) {
    x = (x << 1) ^ ((uint32_t)((int32_t)x >> 31) & poly);
    x ^= (0u - ((R >> k) & 1u)) & Q;
  }
  return x;
}
/* CRC piece of a thread: bytes [q0, q0 + qn) of the segment, P = the fewest bytes per thread that fit the pieces into ONE wave
 * (the recurrence over a piece is a chain of dependent table look-ups, but moving a piece's register to the end of the string
 * costs ~200 VALU instructions per wave that has a piece: the kernel is issue bound when a slot's segments fill the GPU);
 * n_after = bits behind the piece */
struct tb_tx_crc_piece {
  uint32_t q0, qn, n_after;
};
TB_TX_HD tb_tx_crc_piece tb_tx_crc_piece_of(uint32_t segbytes, uint32_t tid)
{
  const uint32_t P = (segbytes + 63u) / 64u < 4u ? 4u : (segbytes + 63u) / 64u;
  tb_tx_crc_piece p;
  p.q0 = P * tid;
  p.qn = p.q0 < segbytes ? (segbytes - p.q0 < P ? segbytes - p.q0 : P) : 0u;
  p.n_after = 8u * (segbytes - p.q0 - p.qn);
  return p;
}
/* the power table's entry the piece needs (pow[j] = x^(j + 24) mod g, left aligned), or none: requested with the stage's loads */
TB_TX_HD bool tb_tx_crc_piece_needs_pow(tb_tx_crc_piece p) { return p.qn && p.n_after >= 24u; }
/* CRC24B over the segment's bytes c in LDS: the thread runs the byte-table recurrence of crc_byte.c:184-218 over its
 * piece, then moves its 24-bit register R to the end of the string: R(x) * x^n_after mod g, one Horner step per
 * coefficient of R with xq = x^n_after mod g from the power table (one load per thread).  The first version looked up one
 * power per set BIT in global memory, one dependent load after the other: 40 % of the kernel.  The XOR of the threads'
 * results is the segment's register. */
TB_TX_HD uint32_t tb_tx_crc_piece_reg(tb_tx_crc_piece p, const uint8_t *c, const uint32_t *tab, uint32_t xq)
{
  const uint32_t q0 = p.q0, qn = p.qn, n_after = p.n_after;
  uint32_t reg = 0;
  for (uint32_t i = 0; i < qn; i++)
    reg = (reg << 8) ^ tab[(reg >> 24) ^ c[q0 + i]];
  uint32_t x = reg;
  if (qn && n_after) {
    if (n_after >= 24u) {
      x = tb_crc_mulmod<24>(reg, xq, 0x80006300u); /* (crc_byte.c:50: poly24b) */
    } else { /* 8 or 16 bits behind the piece: as many zero bytes through the table */
      for (uint32_t b = 0; b < n_after; b += 8)
        x = (x << 8) ^ tab[x >> 24];
    }
  }
  return x;
}

/* ---- the information-column word (Zc % 32 != 0) ---------------------------------------------------------------------------
 * word w of information column col from the MSB-first bytes c of the segment (nin of them hold information bits): the rest
 * of the encoder's phase 0 */
TB_TX_HD uint32_t tb_tx_info_word(const uint8_t *c, int nin, int Z, int col, int w)
{
  const uint32_t b0 = (uint32_t)(col * Z + 32 * w), j0 = b0 >> 3;
  uint64_t v = 0;
  for (int q = 0; q < 5; q++)
    v = (v << 8) | ((int)j0 + q < nin ? c[j0 + q] : 0u);
  const uint32_t m = (uint32_t)(v >> (8 - (b0 & 7u)));
  return __builtin_bitreverse32(m) & ldpc_encp_mask(Z, w);
}

/* ---- the selection item -------------------------------------------------------------------------------------------------
 * what the gather needs of a segment's job (wave-uniform) */
struct tb_tx_sel_geom {
  uint32_t Qm, EQ, V, rank0, Foffset, Fin, Z;
  uint32_t z_magic, v_magic; /* reciprocals of Z and V */
  uint32_t bs;               /* words from one packed column of the code word to the next */
  uint32_t twoZ;
};
template <class JobPtr> TB_TX_HD tb_tx_sel_geom tb_tx_sel_geometry(JobPtr j, int Z)
{
  const uint32_t E = j->E, Qm = j->Qm, EQ = E / Qm, V = j->V, rank0 = j->rank0, Foffset = j->Foffset, Fin = j->Fin;
  const uint32_t z_magic = 0xffffffffu / (uint32_t)Z + 1u, bs = (uint32_t)ldpc_encp_W(Z) + 1u, twoZ = 2u * (uint32_t)Z;
  const uint32_t v_magic = V > 1u ? 0xffffffffu / V + 1u : 0u; /* (V = 1: every rank is 0) */
  return tb_tx_sel_geom{Qm, EQ, V, rank0, Foffset, Fin, (uint32_t)Z, z_magic, v_magic, bs, twoZ};
}
/* word w of sub-stream i of the chunk of nsym modulation symbols from symbol jj0 on: bits e[i*E/Qm + jj0 + 32w ..], bits behind
 * nsym zero; B = the code word's packed columns (ldpc_encp_lds::B).  Gathered in runs: a run ends at the circular buffer's
 * wrap, at the filler gap, at the end of a lifted column. */
TB_TX_HD uint32_t tb_tx_sel_word(const tb_tx_sel_geom &g, const uint32_t *B, uint32_t jj0, uint32_t nsym, uint32_t i, uint32_t w)
{
  const uint32_t V = g.V, Foffset = g.Foffset, Z = g.Z;
  const uint32_t k = i * g.EQ + jj0 + 32u * w;
  uint32_t nbits = nsym - 32u * w;
  nbits = nbits > 32u ? 32u : nbits;
  /* (rank0 + k) mod V without a division: quotient from the reciprocal, off by one at most either way */
  const uint32_t x = g.rank0 + k, q = tb_tx_umulhi(x, g.v_magic);
  uint32_t r = x - q * V, v = 0, filled = 0;
  r += (int32_t)r < 0 ? V : 0u;
  r -= r >= V ? V : 0u;
  r = V == 1u ? 0u : r;
  while (filled < nbits) {
    const uint32_t p = (r < Foffset ? r : r + g.Fin) + g.twoZ;
    const uint32_t col = tb_tx_umulhi(p, g.z_magic), t = p - col * Z;
    uint32_t n = nbits - filled;
    n = n < V - r ? n : V - r;
    if (r < Foffset)
      n = n < Foffset - r ? n : Foffset - r;
    n = n < Z - t ? n : Z - t;
    uint32_t chunk = ldpc_bits_at(B + col * g.bs, t);
    if (n < 32u)
      chunk &= (1u << n) - 1u;
    v |= chunk << filled;
    filled += n;
    r += n;
    r = r >= V ? r - V : r;
  }
  return v;
}
/* the chunk's Qm sub-streams into sel[Qm][sel_stride], 32 bits per item, by thread tid of nt */
TB_TX_HD void tb_tx_sel_chunk(const tb_tx_sel_geom &g, const uint32_t *B, uint32_t jj0, uint32_t nsym, uint32_t *sel, uint32_t sel_stride,
                              int tid, int nt)
{
  const uint32_t nw = (nsym + 31) >> 5;
  for (uint32_t it = tid; it < g.Qm * nw; it += nt) {
    const uint32_t i = it / nw, w = it - i * nw;
    sel[i * sel_stride + w] = tb_tx_sel_word(g, B, jj0, nsym, i, w);
  }
}

/* ---- the stores ---------------------------------------------------------------------------------------------------------
 * The store form's instantiation for the run-time Qm: f(tb_tx_qm<QM>) for the one of QMS that Qm equals; false when it is none
 * of them (the caller's fallback). */
template <int QM> using tb_tx_qm = std::integral_constant<int, QM>;
template <int... QMS, class F> TB_TX_HD bool tb_tx_for_qm(uint32_t Qm, F &&f)
{
  return ((Qm == (uint32_t)QMS && (f(tb_tx_qm<QMS>{}), true)) || ...);
}

/* Interleaver output of one chunk of modulation symbols from its QM packed sub-streams (tb_tx_fused_kernel):
 * f[sy * QM + i] = bit sy of sub-stream i.  A thread takes 8 symbols: one byte of every sub-stream in, 8 QM bytes out, every
 * shift a compile-time constant (2 VALU per output byte; the first version did a division and a look-up per byte).
 * `dst` = where the chunk's first symbol goes; its alignment decides the store width. */
template <int QM>
TB_TX_HD void tb_tx_store_syms(const uint32_t *sel, uint32_t sel_stride, uint32_t nsym, uint8_t *__restrict__ dst, int tid, int nt)
{
  const uint32_t ngrp = nsym >> 3, al = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u);
  for (uint32_t g = tid; g < ngrp; g += nt) {
    uint32_t win[QM];
#pragma unroll
    for (int i = 0; i < QM; i++)
      win[i] = sel[i * sel_stride + (g >> 2)] >> (8u * (g & 3u));
    /* output dword w of the group (compile-time shifts); formed right where it is stored, so that at most one is live
     * (all 2 QM of them next to the eight windows pushed the kernel to 99 VGPRs = four waves per SIMD, and a 1664-segment
     * slot then runs in two rounds of workgroups) */
    /* QM = 6, 8: the 8 QM output bits of the group as two bit strings first -- symbols 0..3 and 4..7; bit sy of a sub-stream goes
     * to position sy QM by ONE multiplication (x * (1 + 2^(QM-1) + 2^(2QM-2) + 2^(3QM-3)) puts bit k of a nibble at k + (QM-1) j
     * for j = 0..3, of which j = k is the wanted QM k; no two of the sixteen positions coincide when QM - 1 >= 4, so nothing
     * carries) -- then every nibble of a string becomes a dword of bytes by another one.  84 instead of ~150 VALU per group. */
    uint32_t f_lo = 0, f_hi = 0;
    if constexpr (QM == 6 || QM == 8) {
      constexpr uint32_t M = 1u | (1u << (QM - 1)) | (1u << (2 * QM - 2)) | (1u << (3 * QM - 3));
      constexpr uint32_t K = 1u | (1u << QM) | (1u << (2 * QM)) | (1u << (3 * QM));
#pragma unroll
      for (int i = 0; i < QM; i++) {
        f_lo |= (((win[i] & 0xfu) * M) & K) << i;
        f_hi |= ((((win[i] >> 4) & 0xfu) * M) & K) << i;
      }
    }
    auto word = [&](int w) -> uint32_t {
      if constexpr (QM == 6 || QM == 8) {
        const uint32_t nib = ((w < QM ? f_lo : f_hi) >> (4 * (w < QM ? w : w - QM))) & 0xfu;
        return (nib * 0x00204081u) & 0x01010101u;
      }
      uint32_t v = 0;
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int m = 4 * w + b, sy = m / QM, i = m - sy * QM;
        v |= ((win[i] >> sy) & 1u) << (8 * b);
      }
      return v;
    };
    uint8_t *o = dst + (size_t)g * (8 * QM);
    if (al == 0) {
#pragma unroll
      for (int w = 0; w < 2 * QM; w++)
        reinterpret_cast<uint32_t *>(o)[w] = word(w);
    } else if (al == 2) {
#pragma unroll
      for (int w = 0; w < 2 * QM; w++) {
        const uint32_t v = word(w);
        reinterpret_cast<uint16_t *>(o)[2 * w] = (uint16_t)v;
        reinterpret_cast<uint16_t *>(o)[2 * w + 1] = (uint16_t)(v >> 16);
      }
    } else {
#pragma unroll
      for (int w = 0; w < 2 * QM; w++) {
        const uint32_t v = word(w);
#pragma unroll
        for (int b = 0; b < 4; b++)
          o[4 * w + b] = (uint8_t)(v >> (8 * b));
      }
    }
  }
  for (uint32_t m = ngrp * 8u * QM + tid; m < nsym * QM; m += nt) { /* the last, partial group */
    const uint32_t sy = m / QM, i = m - sy * QM;
    dst[m] = (uint8_t)((sel[i * sel_stride + (sy >> 5)] >> (sy & 31u)) & 1u);
  }
}
/* the same for a Qm that is no modulation of NR (kept correct): a division and a look-up per byte */
TB_TX_HD void tb_tx_store_syms_any(uint32_t Qm, const uint32_t *sel, uint32_t sel_stride, uint32_t nsym, uint8_t *__restrict__ dst, int tid,
                                   int nt)
{
  for (uint32_t m = tid; m < nsym * Qm; m += nt) {
    const uint32_t sy = m / Qm, i = m - sy * Qm;
    dst[m] = (uint8_t)((sel[i * sel_stride + (sy >> 5)] >> (sy & 31u)) & 1u);
  }
}
#endif
