/*
 * tb_tx_scr.h -- the packed, scrambled store of the fused TX kernel (tb_chain.hip tb_tx_fused_scr_kernel,
 * nrLDPC_hip_dlsch_encode_scrambled): a selection chunk's interleaved bits XOR the codeword's sequence, 32 to a word, with
 * the words that two chunks or two segments share put together from their parts; and the host plan of the shared words.
 * Compiles as HIP device code and as plain host C++ (tests/emul/tb_tx_scr_emul.cpp runs the same code on the CPU, the
 * workgroups and their threads one after another).
 */
#ifndef TB_TX_SCR_H
#define TB_TX_SCR_H
#include <stdint.h>
#include <map>
#include <utility>
#include <vector>
#include "tb_jobs.h"

#ifndef TB_TX_HD
#if defined(__HIPCC__)
#define TB_TX_HD __device__ __forceinline__
#else
#define TB_TX_HD static inline
#endif
#endif

/* A packed word that several segments' bits share (segment boundaries are not word boundaries): each segment leaves its part
 * in its slot and takes a ticket; the last to arrive ORs the parts, stores the word and resets the ticket.  No workgroup
 * waits for another, and nobody read-modify-writes the caller's array.  No fences, as in the fused RX kernel
 * (tb_rx_fused.hip): the part is a device-scope atomic store that has completed (vmcnt) before the ticket is taken, and the
 * last arrival reads the parts with device-scope atomic loads -- an agent-scope release would write back the XCD's whole L2
 * for every boundary word (the first version did: 81 us for the slot's 1664 segments against 20 unscrambled).  On the host
 * (the emulation) the segments run one after another, so the n-th arrival is the last one and plain loads and stores do. */
TB_TX_HD void tb_tx_settle_word(uint32_t *dst, uint32_t bits, uint32_t ticket, uint32_t part, uint32_t part0, uint32_t n,
                                uint32_t *tickets, uint32_t *parts)
{
#if defined(__HIPCC__)
  __hip_atomic_store(&parts[part], bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const uint32_t before = __hip_atomic_fetch_add(&tickets[ticket], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  parts[part] = bits;
  const uint32_t before = tickets[ticket]++;
#endif
  if (before + 1u != n)
    return;
  uint32_t v = 0;
  for (uint32_t k = 0; k < n; k++)
#if defined(__HIPCC__)
    v |= __hip_atomic_load(&parts[part0 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    v |= parts[part0 + k];
#endif
  *dst = v;
#if defined(__HIPCC__)
  __hip_atomic_store(&tickets[ticket], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); /* zero again for the next call */
#else
  tickets[ticket] = 0u;
#endif
}
/* Packed, scrambled output of one selection chunk (the scrambled instantiation of tb_tx_fused_kernel, beside
 * tb_tx_store_syms): codeword bits [b_lo, b_hi) of the TB = f[jj0 Qm ..] of the segment.  A thread forms whole 32-bit words
 * of interleaved bits from the Qm sub-streams in LDS, XORs the sequence words (seq[0] = word b_lo / 32) over the bits this
 * chunk holds, and stores a dword.  A word the chunk shares with the previous chunk takes that chunk's part from carry[];
 * one it shares with the next chunk leaves its part there; one it shares with another segment goes through a ticket.  The
 * bits behind G in the TB's last word are 0. */
template <int QM, typename J>
TB_TX_HD void tb_tx_store_scr(J j, const uint32_t *sel, uint32_t sel_stride, const uint32_t *seq, uint32_t *carry, uint32_t k,
                              uint32_t b_lo, uint32_t b_hi, bool last_chunk, uint32_t *out32, uint32_t *tickets,
                              uint32_t *parts, int tid, int nt)
{
  const bool first_chunk = k == 0, last_seg = j->r + 1u == j->C;
  const uint32_t w_lo = b_lo >> 5, w_hi = (b_hi + 31u) >> 5, lo = j->bit_off;
  for (uint32_t w = w_lo + (uint32_t)tid; w < w_hi; w += (uint32_t)nt) {
    const uint32_t n0 = 32u * w > b_lo ? 32u * w : b_lo, n1 = 32u * w + 32u < b_hi ? 32u * w + 32u : b_hi;
    uint32_t bits = 0;
    for (uint32_t n = n0; n < n1; n++) {
      const uint32_t mc = n - b_lo, sy = mc / (uint32_t)QM, i = mc - sy * (uint32_t)QM;
      bits |= ((sel[i * sel_stride + (sy >> 5)] >> (sy & 31u)) & 1u) << (n & 31u);
    }
    const uint32_t nb = n1 - n0, present = nb == 32u ? ~0u : ((1u << nb) - 1u) << (n0 & 31u);
    bits ^= seq[w - w_lo] & present;
    const bool before = 32u * w < b_lo, after = 32u * w + 32u > b_hi && !(last_chunk && last_seg);
    if (before && !first_chunk)
      bits |= carry[(k - 1u) & 1u];
    if (after && !last_chunk) {
      carry[k & 1u] = bits;
    } else if ((before && first_chunk) || after) {
      if (w == (lo >> 5) && (lo & 31u))
        tb_tx_settle_word(out32 + w, bits, j->h_ticket, j->h_part, j->h_part0, j->h_n, tickets, parts);
      else
        tb_tx_settle_word(out32 + w, bits, j->t_ticket, j->t_part, j->t_part0, j->t_n, tickets, parts);
    } else {
      out32[w] = bits;
    }
  }
}

/* The host plan of one transport block's shared words (tb_api.inc.cpp; jobs = its C segments, r = 0 .. C-1, bit_off and E
 * set): a segment's first word when it starts inside a word, its last word when it ends inside one and is not the block's
 * last segment (behind G the last word is 0: complete) -- once per segment and word; each word gets a ticket and one part
 * slot per segment that touches it.  Tickets and parts are numbered on from *n_tickets / *n_parts, which advance. */
static inline void tb_tx_scr_plan(tb_tx_seg_job *jobs, size_t n_seg, uint32_t *n_tickets, size_t *n_parts)
{
  std::map<uint32_t, std::vector<std::pair<size_t, int>>> shared;
  for (size_t q = 0; q < n_seg; q++) {
    const uint32_t lo = jobs[q].bit_off, hi = lo + jobs[q].E;
    const bool head = (lo & 31u) != 0, last = jobs[q].r + 1 == jobs[q].C;
    if (head)
      shared[lo >> 5].push_back({q, 0});
    if (!last && (hi & 31u) && !(head && ((hi - 1) >> 5) == (lo >> 5)))
      shared[(hi - 1) >> 5].push_back({q, 1});
  }
  for (const auto &kv : shared) {
    const uint32_t tk = (*n_tickets)++, p0 = (uint32_t)*n_parts, n = (uint32_t)kv.second.size();
    for (uint32_t k = 0; k < n; k++) {
      tb_tx_seg_job &q = jobs[kv.second[k].first];
      if (kv.second[k].second == 0) {
        q.h_ticket = tk; q.h_part = p0 + k; q.h_part0 = p0; q.h_n = n;
      } else {
        q.t_ticket = tk; q.t_part = p0 + k; q.t_part0 = p0; q.t_n = n;
      }
    }
    *n_parts += n;
  }
}
#endif
