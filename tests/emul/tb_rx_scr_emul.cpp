/*
 * tb_rx_scr_emul.cpp -- CPU emulation of the scrambled de-matching phases (tb_rx_core.h with the unscrambling flag): the
 * workgroup's threads walked phase by phase, as tb_rx_scr_phases_za() orders them -- one chunk of symbols with the symbols
 * loaded ahead, or several chunks with the sequence staged for each in turn.  The staged sequence words come from the host
 * jump-ahead of nr_gold.h (the kernels' wave-wide jump needs a GPU: the -m gpu tests cover it).  Built by
 * tests/test_tb_scrambled_emul.py with the host compiler.
 */
#include <string.h>
#include <vector>
#include "../../openairinterface5g_amd/csrc/tb_rx_core.h"
#include "../../openairinterface5g_amd/csrc/nr_gold.h"
#include "../../openairinterface5g_amd/csrc/nr_coding_host.h"

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
static void emul_za(const tb_rx_geom &g, const int16_t *f, int16_t *e_lds, int8_t *l, int nt, uint32_t c_init, uint32_t bit_off)
{
  const uint32_t EQ = g.E / QM, CH = tb_rx_scr_chunk(QM), nlaps = tb_rx_laps(g);
  uint32_t *seq = reinterpret_cast<uint32_t *>(e_lds + g.span);
  std::vector<tb_rx_ahead> first(nt);
  for (int tid = 0; tid < nt; tid++) {
    tb_rx_phase_load_first<QM>(g, f, (uint32_t)tid, (uint32_t)nt, first[tid]);
    tb_rx_phase_zero(g, e_lds, l, (uint32_t)tid, (uint32_t)nt);
  }
  if (EQ <= CH) {
    const uint32_t w0 = bit_off >> 5, nw = ((bit_off + EQ * QM + 31u) >> 5) - w0 + 1u;
    if (nw > TB_RX_SCR_WORDS)
      return;
    fill_seq(seq, c_init, w0, nw);
    const tb_rx_scr sc{seq, bit_off - 32u * w0};
    if (nlaps == 1) {
      for (int tid = 0; tid < nt; tid++)
        tb_rx_phase_scatter_lap<QM, true, true>(g, f, e_lds, 0, 1, (uint32_t)tid, (uint32_t)nt, first[tid], &sc);
    } else {
      for (uint32_t lap = 0; lap < nlaps; lap++)
        for (int tid = 0; tid < nt; tid++)
          tb_rx_phase_scatter_lap<QM, false, true>(g, f, e_lds, lap, nlaps, (uint32_t)tid, (uint32_t)nt, first[tid], &sc);
    }
    return;
  }
  for (uint32_t c0 = 0; c0 < EQ; c0 += CH) {
    const uint32_t c1 = EQ - c0 < CH ? EQ : c0 + CH;
    const uint32_t w0 = (bit_off + c0 * QM) >> 5, nw = ((bit_off + c1 * QM + 31u) >> 5) - w0 + 1u;
    if (nw > TB_RX_SCR_WORDS)
      return;
    fill_seq(seq, c_init, w0, nw);
    const tb_rx_scr sc{seq, bit_off - 32u * w0};
    for (uint32_t lap = 0; lap < nlaps; lap++)
      for (int tid = 0; tid < nt; tid++) {
        if (nlaps == 1)
          tb_rx_phase_scatter_chunk<QM, true>(g, f, e_lds, 0, 1, (uint32_t)tid, (uint32_t)nt, sc, c0, c1);
        else
          tb_rx_phase_scatter_chunk<QM, false>(g, f, e_lds, lap, nlaps, (uint32_t)tid, (uint32_t)nt, sc, c0, c1);
      }
  }
}

/* as tests/emul/ldpc_emul.cpp tb_emul_rx_dematch, for LLRs that are codeword bits bit_off .. bit_off + E - 1 of the sequence
 * of c_init; returns the LDS image's int16 slots, or -1 */
extern "C" int tb_emul_rx_dematch_scr(uint32_t Tbslbrm, int BG, uint32_t Zc, uint32_t C, uint32_t F, uint32_t K, int rv, uint32_t E,
                                      uint32_t Qm, uint32_t num_llr, int clear, int nt, uint32_t c_init, uint32_t bit_off,
                                      const int16_t *f, int16_t *w, int8_t *l)
{
  nr_hip_rm_t rm;
  if (nr_hip_rate_match_geometry(Tbslbrm, BG, Zc, C, F, K, rv, E, &rm) != 0)
    return -1;
  tb_rx_seg_job j;
  memset(&j, 0, sizeof(j));
  j.E = E; j.Qm = Qm; j.Ncb = rm.Ncb; j.Foffset = rm.Foffset; j.Fin = rm.Fin; j.V = rm.V; j.rank0 = rm.rank0;
  j.clear = clear ? 1u : 0u;
  j.K = K; j.F = F; j.Z = Zc; j.num_llr = num_llr;
  j.c_init = c_init; j.bit_off = bit_off;
  const tb_rx_geom g = tb_rx_geometry(&j);
  /* the image and the sequence words behind it, as the kernels' launches size them */
  std::vector<tb_u32x4> lds((g.span * 2 + TB_RX_SCR_LDS) / 16); /* the image (span a multiple of 8) and the sequence words behind it, no more */
  memset(lds.data(), 0x5a, lds.size() * sizeof(tb_u32x4)); /* poison: phase Z and the staging must initialise what is read */
  int16_t *e_lds = reinterpret_cast<int16_t *>(lds.data());
  switch (Qm) {
    case 2: emul_za<2>(g, f, e_lds, l, nt, c_init, bit_off); break;
    case 4: emul_za<4>(g, f, e_lds, l, nt, c_init, bit_off); break;
    case 6: emul_za<6>(g, f, e_lds, l, nt, c_init, bit_off); break;
    default: emul_za<8>(g, f, e_lds, l, nt, c_init, bit_off); break;
  }
  for (int tid = 0; tid < nt; tid++)
    tb_rx_phase_stream(g, e_lds, w, l, (uint32_t)tid, (uint32_t)nt);
  return (int)g.span;
}
