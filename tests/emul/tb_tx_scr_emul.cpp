/*
 * tb_tx_scr_emul.cpp -- CPU emulation of the fused TX kernel's packed, scrambled store (tb_tx_scr.h, tb_tx_fused_scr_kernel):
 * one transport block's segments, planned by the library's own tb_tx_scr_plan, each selection chunk with its Qm sub-streams
 * packed as the kernel packs them into LDS and its sequence words (the host jump-ahead of nr_gold.h), the workgroup's
 * threads walked one after another.  The segments' chunks run in an order the caller gives (segments in any order, chunks
 * of different segments interleaved), as the GPU's workgroups may.  Built by tests/test_tb_tx_scr_emul.py with the host
 * compiler.
 */
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../openairinterface5g_amd/csrc/tb_tx_scr.h"
#include "../../openairinterface5g_amd/csrc/nr_gold.h"

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

struct seg_state {
  uint32_t next;     /* next selection chunk of the segment */
  uint32_t carry[2]; /* the workgroup's LDS carry words (poisoned: the first chunk never reads them) */
};

/* chunk k of segment q: f = the TB's G interleaved bits (one per byte, segments back to back) */
template <int QM>
static void emul_chunk(const tb_tx_seg_job &j, seg_state &st, const uint8_t *f, uint32_t chunk, int nt, uint32_t *out32,
                       uint32_t *tickets, uint32_t *parts)
{
  const uint32_t EQ = j.E / QM, sel_stride = chunk / 32 + 1, k = st.next++, jj0 = k * chunk;
  const uint32_t nsym = EQ - jj0 < chunk ? EQ - jj0 : chunk, nw = (nsym + 31) / 32;
  std::vector<uint32_t> sel(QM * sel_stride, 0x5a5a5a5au), seq(chunk * QM / 32 + 2, 0xa5a5a5a5u); /* poison */
  /* the gather: bit jj of sub-stream i = f[(jj0 + jj) Qm + i] of the segment (f[jj Qm + i] = e[i E/Qm + jj]); bits behind
   * nsym in a sub-stream's last word are 0, as the kernel's gather leaves them */
  const uint8_t *fs = f + j.bit_off;
  for (uint32_t i = 0; i < (uint32_t)QM; i++)
    for (uint32_t w = 0; w < nw; w++) {
      uint32_t v = 0;
      for (uint32_t b = 0; b < 32 && 32 * w + b < nsym; b++)
        v |= (uint32_t)(fs[(size_t)(jj0 + 32 * w + b) * QM + i] & 1u) << b;
      sel[i * sel_stride + w] = v;
    }
  const uint32_t b_lo = j.bit_off + jj0 * QM, b_hi = b_lo + nsym * QM;
  fill_seq(seq.data(), j.c_init, b_lo >> 5, ((b_hi + 31u) >> 5) - (b_lo >> 5));
  const bool last_chunk = jj0 + nsym == EQ;
  for (int tid = 0; tid < nt; tid++)
    tb_tx_store_scr<QM>(&j, sel.data(), sel_stride, seq.data(), st.carry, k, b_lo, b_hi, last_chunk, out32, tickets, parts, tid, nt);
}

/* One transport block of C segments (lengths E[0..C-1], multiples of Qm; codeword bits from 0), sequence of c_init.
 * steps[0 .. n_steps-1]: segment indices -- each runs that segment's next selection chunk of `chunk` symbols (the kernel:
 * TB_TX_SEL_SYMS; a multiple of 32); every segment must be run to its end.  out32: the block's (G + 31) / 32 words;
 * tickets / parts: the call's ticket and part arrays (tickets zero on entry, zero again on exit), room for tk_cap / pt_cap;
 * plan[0], plan[1] = tickets and parts the plan used.  0, -1 for arguments the kernel never sees, -2 for a bad step list */
extern "C" int tb_emul_tx_scr(uint32_t C, const uint32_t *E, uint32_t Qm, uint32_t c_init, const uint8_t *f, uint32_t chunk, int nt,
                              const uint32_t *steps, uint32_t n_steps, uint32_t *out32, uint32_t *tickets, uint32_t tk_cap, uint32_t *parts,
                              uint32_t pt_cap, uint32_t *plan)
{
  if (C == 0 || chunk == 0 || chunk % 32 || nt < 1 || (Qm != 2 && Qm != 4 && Qm != 6 && Qm != 8))
    return -1;
  std::vector<tb_tx_seg_job> jobs(C);
  uint32_t bit_off = 0;
  for (uint32_t r = 0; r < C; r++) {
    if (E[r] == 0 || E[r] % Qm)
      return -1;
    tb_tx_seg_job &j = jobs[r];
    memset(&j, 0, sizeof(j));
    j.r = r; j.C = C; j.E = E[r]; j.Qm = Qm; j.c_init = c_init; j.bit_off = bit_off;
    bit_off += E[r];
  }
  uint32_t n_tickets = 0;
  size_t n_parts = 0;
  tb_tx_scr_plan(jobs.data(), C, &n_tickets, &n_parts);
  plan[0] = n_tickets;
  plan[1] = (uint32_t)n_parts;
  if (n_tickets > tk_cap || n_parts > pt_cap)
    return -1;
  std::vector<seg_state> st(C);
  for (auto &s : st)
    s = seg_state{0, {0xdeadbeefu, 0xdeadbeefu}};
  for (uint32_t s = 0; s < n_steps; s++) {
    const uint32_t q = steps[s];
    if (q >= C || st[q].next * chunk >= E[q] / Qm)
      return -2;
    switch (Qm) {
      case 2: emul_chunk<2>(jobs[q], st[q], f, chunk, nt, out32, tickets, parts); break;
      case 4: emul_chunk<4>(jobs[q], st[q], f, chunk, nt, out32, tickets, parts); break;
      case 6: emul_chunk<6>(jobs[q], st[q], f, chunk, nt, out32, tickets, parts); break;
      default: emul_chunk<8>(jobs[q], st[q], f, chunk, nt, out32, tickets, parts); break;
    }
  }
  for (uint32_t q = 0; q < C; q++)
    if (st[q].next * chunk < E[q] / Qm)
      return -2;
  return 0;
}
