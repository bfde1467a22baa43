/*
 * slot_plan.h -- the part of the slot-level entry points that is plain arithmetic on descriptors: the layout of a call's
 * descriptor tables, the write-set overlap check, the DMRS sequence helpers and the small checks more than one call needs.  No
 * HIP calls, no DeviceCall, no staging: ldpc_api.cpp includes it ahead of slot_call.inc.cpp, and the CPU emulation of the kernels
 * (tests/emul/) includes the same file, so the plans the emulated kernels run on are the library's own.
 *
 * The including file provides, in its anonymous namespace and ahead of this header,
 *     int set_error(const char *what);     -- records the refusal's text and returns -1
 * Everything here lands in the includer's anonymous namespace.
 */
#ifndef SLOT_PLAN_H
#define SLOT_PLAN_H
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/nrLDPC_hip.h"
#include "nr_coding_host.h"
#include "nr_rx_grid.h"

#define NR_SCR_MAX_BITS (1u << 21) /* one codeword: G <= 1.5 Mbit (the sequence's jump tables reach 2^17 - 50 words) */

namespace {

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

int check_mem(const char *who, int32_t mem)
{
  if (mem != NRLDPC_HIP_MEM_HOST && mem != NRLDPC_HIP_MEM_DEVICE)
    return set_error((std::string(who) + ": mem must be NRLDPC_HIP_MEM_HOST or NRLDPC_HIP_MEM_DEVICE").c_str());
  return 0;
}

int qam_check_qm(uint32_t Qm)
{
  if (Qm != 2 && Qm != 4 && Qm != 6 && Qm != 8)
    return set_error("modulation: Qm must be 2, 4, 6 or 8");
  return 0;
}

/* ---- two arrays back to back, each padded to 16 bytes: a call's descriptor tables (the workgroup table, then the job table) or
 * its jobs and their state (b == nullptr: nb zeroed elements) ---- */
template <typename A, typename B> struct Table2 {
  const A *a;
  size_t na;
  const B *b;
  size_t nb;
  static size_t bytes(size_t na, size_t nb) { return align_up(na * sizeof(A), 16) + align_up(nb * sizeof(B), 16); }
  size_t bytes() const { return bytes(na, nb); }
  void write(uint8_t *dst) const
  {
    memcpy(dst, a, na * sizeof(A));
    if (b)
      memcpy(dst + align_up(na * sizeof(A), 16), b, nb * sizeof(B));
    else
      memset(dst + align_up(na * sizeof(A), 16), 0, align_up(nb * sizeof(B), 16));
  }
  /* the two parts of a copy at base */
  const A *first(const uint8_t *base) const { return reinterpret_cast<const A *>(base); }
  B *second(uint8_t *base) const { return reinterpret_cast<B *>(base + align_up(na * sizeof(A), 16)); }
};
template <typename A, typename B> Table2<A, const B> table2(const std::vector<A> &a, const std::vector<B> &b)
{
  return Table2<A, const B>{a.data(), a.size(), b.data(), b.size()};
}

/* ---- the write set of a call: [lo, hi) ranges that must not overlap ---- */
struct Range64 {
  uint64_t lo, hi;
};
/* true when two of the ranges overlap (r comes back sorted); lo, hi: the span of all of them, UINT64_MAX and 0 when there are none */
bool ranges_overlap(std::vector<Range64> &r, uint64_t &lo, uint64_t &hi)
{
  lo = UINT64_MAX;
  hi = 0;
  for (const Range64 &x : r) {
    lo = std::min(lo, x.lo);
    hi = std::max(hi, x.hi);
  }
  std::sort(r.begin(), r.end(), [](const Range64 &a, const Range64 &b) { return a.lo < b.lo; });
  for (size_t i = 1; i < r.size(); i++)
    if (r[i].lo < r[i - 1].hi)
      return true;
  return false;
}

/* ---- DMRS sequences ---- */
/* c_init of the DMRS of one OFDM symbol, PUSCH and PDSCH alike (nr_gold.c:87-88, 107-108) */
uint32_t dmrs_c_init(uint32_t slot, uint32_t symbol, uint32_t scrambling_id, uint32_t scid)
{
  return (uint32_t)(((1ull << 17) * (NR_RXG_SYMBOLS * slot + symbol + 1u) * (2ull * scrambling_id + 1u) + 2ull * scrambling_id + scid) & 0x7fffffffull);
}
/* the sequence from symbol k on, two bits a symbol (the low two: the DMRS value of k itself), out of Gold words w0, w0 + 1, ...;
 * gold holds one word beyond the one k's bits lie in */
uint64_t dmrs_bits(const std::vector<uint32_t> &gold, uint32_t w0, uint32_t k)
{
  const uint32_t w = (k >> 4) - w0;
  return ((uint64_t)gold[w] | ((uint64_t)gold[w + 1] << 32)) >> ((2u * k) & 31u);
}
/* the words that hold symbols k0 .. k0 + n - 1 (n >= 1) and one more, for dmrs_bits; false when they cannot be generated */
bool dmrs_gold_words(uint32_t c_init, uint32_t k0, uint32_t n, std::vector<uint32_t> &gold, uint32_t &w0)
{
  w0 = k0 >> 4;
  gold.resize(((k0 + n - 1u) >> 4) - w0 + 2u);
  return nr_hip_gold_words(c_init, w0, (uint32_t)gold.size(), gold.data()) == 0;
}

} // namespace
#endif
