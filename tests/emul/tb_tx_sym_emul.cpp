/*
 * tb_tx_sym_emul.cpp -- CPU emulation of the fused TX kernel's symbol store (tb_tx_sym.h, tb_tx_fused_sym_kernel): one segment's
 * selection chunks in turn, each with its Qm sub-streams packed as the kernel packs them into LDS, its sequence words (the host
 * jump-ahead of nr_gold.h) and the constellation of nr_qam.h, the workgroup's threads walked one after another.  Built by
 * tests/test_tb_tx_sym_emul.py with the host compiler.
 */
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../openairinterface5g_amd/csrc/tb_tx_sym.h"
#include "../../openairinterface5g_amd/csrc/nr_gold.h"
#include "../../openairinterface5g_amd/csrc/nr_qam.h"

static void fill_seq(uint32_t *seq, uint32_t c_init, uint32_t w0, uint32_t nw)
{
  static const nr_gold_tables_t T = nr_gold_make_tables();
  uint32_t a, b;
  nr_gold_jump(&T, c_init, w0, &a, &b);
  for (uint32_t i = 0; i < nw; i++) {
    seq[i] = a ^ b;
    a = nr_gold_step1(a);
    b = nr_gold_step2(b);
  }
}

template <int QM>
static void emul_store(const uint8_t *f, uint32_t E, uint32_t Nl, uint32_t plane, uint32_t c_init, uint32_t bit_off, uint32_t chunk, int nt,
                       uint32_t *rec)
{
  static const nr_qam_tables_t Q = nr_qam_make_tables();
  const uint32_t EQ = E / QM, sel_stride = chunk / 32 + 1;
  std::vector<uint32_t> sel(QM * sel_stride), seq(chunk * QM / 32 + 2);
  for (uint32_t jj0 = 0; jj0 < EQ; jj0 += chunk) {
    const uint32_t nsym = EQ - jj0 < chunk ? EQ - jj0 : chunk;
    /* the gather: bit jj of sub-stream i = f[(jj0 + jj) Qm + i] (f[jj Qm + i] = e[i E/Qm + jj], the interleaver) */
    std::fill(sel.begin(), sel.end(), 0x5a5a5a5au); /* poison: every bit the store reads is written here */
    for (uint32_t i = 0; i < (uint32_t)QM; i++)
      for (uint32_t w = 0; w < (nsym + 31) / 32; w++) {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 32 && 32 * w + k < nsym; k++)
          v |= (uint32_t)(f[(size_t)(jj0 + 32 * w + k) * QM + i] & 1u) << k;
        sel[i * sel_stride + w] = v;
      }
    const uint32_t b_lo = bit_off + jj0 * QM, b_hi = b_lo + nsym * QM, w0 = b_lo >> 5, nw = ((b_hi + 31u) >> 5) - w0;
    std::fill(seq.begin(), seq.end(), 0xa5a5a5a5u);
    fill_seq(seq.data(), c_init, w0, nw);
    const tb_tx_sym_chunk ch{sel.data(), sel_stride, seq.data(), b_lo & 31u, bit_off / QM + jj0, Nl, plane};
    for (int tid = 0; tid < nt; tid++)
      tb_tx_sym_store<QM>(ch, Q.pt + nr_qam_table_off(QM), nsym, rec, (uint32_t)tid, (uint32_t)nt);
  }
}

/* one segment: f = its E interleaved bits (one per byte), codeword bits bit_off .. bit_off + E - 1 of the sequence of c_init;
 * rec = the TB's record (Nl planes `plane` words apart).  chunk = symbols per selection chunk (the kernel: TB_TX_SEL_SYMS,
 * a multiple of 32).  0, or -1 for arguments the kernel never sees */
extern "C" int tb_emul_tx_sym(const uint8_t *f, uint32_t E, uint32_t Qm, uint32_t Nl, uint32_t plane, uint32_t c_init, uint32_t bit_off,
                              uint32_t chunk, int nt, uint32_t *rec)
{
  if (Nl < 1 || Nl > 4 || E % (Qm * Nl) || bit_off % (Qm * Nl) || chunk == 0 || chunk % 32)
    return -1;
  switch (Qm) {
    case 2: emul_store<2>(f, E, Nl, plane, c_init, bit_off, chunk, nt, rec); break;
    case 4: emul_store<4>(f, E, Nl, plane, c_init, bit_off, chunk, nt, rec); break;
    case 6: emul_store<6>(f, E, Nl, plane, c_init, bit_off, chunk, nt, rec); break;
    case 8: emul_store<8>(f, E, Nl, plane, c_init, bit_off, chunk, nt, rec); break;
    default: return -1;
  }
  return 0;
}
