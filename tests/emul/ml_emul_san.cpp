/*
 * ml_emul_san.cpp -- the two-layer ML receiver's kernels (tb_rx_ml.hip, #included as it is and read against the host shim
 * hip_host/) on arrays that are exactly as long as include/nrLDPC_hip.h says a DEVICE mem caller's must be.  A stand-alone
 * program, built with -fsanitize=address,undefined by tests/test_ml_kernels_emul.py: every array is a heap allocation of its
 * own, so a read or a write in front of the first element a call may touch or behind the last one is a report, and so is a
 * misaligned vector access or an arithmetic overflow.  An entry point is the DEVICE mem branch of the library call: checks, plan
 * (rx_plan.h, the library's own), place at bias 0, tables, launch, in place on the caller's arrays.
 *
 * Shapes: fft_size 128 with 1, 2 and 3 PRBs of every pattern (6- and 18-RE segments: partial groups), the grid's wrap between two
 * groups, inside one and absent, one 1080-RE segment (two workgroups, the wrap in the second); n_rx 1..4 (2 and 4: the unrolled
 * kernels; 1 and 3: the loop); Qm 2 and 4, and calls of two segments that mix them; the LLR array's first written word 0..3
 * words behind a 16-byte boundary.  Results are compared here with the element-by-element loop over nr_rx_ml.h, and every
 * case's extracted inputs and LLRs go to the file named by argv[1], where the test compares them with ml_2layers_host.
 * Exit status 0 and nothing on stderr: clean.
 */
#include "slot_emul_common.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rx_plan.h"
#include "tb_rx_ml.hip"

namespace {

const uint32_t CANARY = 0x5a5a5a5au;
long n_calls = 0, n_bad = 0;
FILE *dump = nullptr;

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd()
{
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}
/* a c16 of moderate size now and then, full scale otherwise */
uint32_t rnd_c16() { return (rnd() & 3u) ? rnd() : nr_rxf_c16((int32_t)(rnd() % 2001u) - 1000, (int32_t)(rnd() % 2001u) - 1000); }

/* elements lo .. hi - 1 of an array: a heap allocation of exactly hi - lo elements; base() is where element 0 would be */
template <typename T> struct Exact {
  uint64_t lo, hi;
  std::unique_ptr<T[]> mem;
  Exact(uint64_t lo_, uint64_t hi_) : lo(lo_), hi(hi_), mem(new T[hi_ - lo_]) {}
  T *base() const { return reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(mem.get()) - lo * sizeof(T)); }
  T &operator[](uint64_t i) const
  {
    if (i < lo || i >= hi) {
      fprintf(stderr, "the test itself indexes outside an array\n");
      abort();
    }
    return mem[i - lo];
  }
  template <typename F> void fill(F f)
  {
    for (uint64_t i = lo; i < hi; i++)
      mem[i - lo] = f();
  }
};
typedef Exact<uint32_t> Words;
const int16_t *i16(const Words &w) { return reinterpret_cast<const int16_t *>(w.base()); }
int16_t *i16w(Words &w) { return reinterpret_cast<int16_t *>(w.base()); }

/* ---- the DEVICE mem branches of the two calls ---- */
int32_t emul_ml_2layers_grid(const int16_t *rxdataF, const int16_t *ul_ch, uint32_t n_rx, uint64_t rx_ant_stride, uint64_t ch_ant_stride,
                             const nrLDPC_hip_rx_grid_seg_t *seg, uint32_t n_seg, const int32_t *shift, int16_t *llr)
{
  if (rxf_check_common("ml_2layers_grid", n_rx, NRLDPC_HIP_MEM_DEVICE) != 0)
    return -1;
  if (!aligned4({rxdataF, ul_ch, shift, llr}))
    return set_error("ml_2layers_grid: every array 4-byte aligned");
  RxFrontPlan p;
  std::vector<rx_front_grid_job> gj;
  if (rxl_plan(seg, n_seg, n_rx, rx_ant_stride, ch_ant_stride, p, gj) != 0)
    return -1;
  if (gj.empty())
    return 0;
  rxl_place(p, gj, 0, 0, 0);
  const auto tab = table2(p.wgs, gj);
  const auto base = tables_copy(tab);
  return launched(nr_launch_rx_ml_grid(tab.first(base.get()), (uint32_t)p.wgs.size(), tab.second(base.get()), c16(rxdataF), c16(ul_ch), n_rx,
                                       rx_ant_stride, ch_ant_stride, shift, c16(llr), nullptr));
}

int32_t emul_channel_level_grid_ml(const int16_t *ul_ch, uint32_t n_rx, uint64_t ch_ant_stride, const nrLDPC_hip_rx_grid_seg_t *first_sym, uint32_t n_tb,
                                   const int32_t *max_ch, int32_t *log2_maxh)
{
  if (rxf_check_common("channel_level_grid_ml", n_rx, NRLDPC_HIP_MEM_DEVICE) != 0)
    return -1;
  if (n_tb == 0)
    return 0;
  std::vector<rx_front_grid_lvl_job> lvl;
  uint64_t ch_lo, ch_hi;
  if (rxg_plan_level(first_sym, n_tb, 2u * n_rx, ch_ant_stride, lvl, ch_lo, ch_hi) != 0)
    return -1;
  const auto tab = rxf_level_tables(lvl);
  const auto base = tables_copy(tab);
  WithThreads t;
  return launched(nr_launch_rx_level_grid_ml(tab.first(base.get()), n_tb, c16(ul_ch), n_rx, ch_ant_stride, max_ch, tab.second(base.get()), log2_maxh,
                                             nullptr));
}

void called(int32_t rc, const char *what)
{
  n_calls++;
  if (rc != 0) {
    fprintf(stderr, "%s: refused: %s\n", what, slot_emul_error.c_str());
    n_bad++;
  }
}

/* ---- the grid segments: pattern, PRBs, where the wrap falls (the cases of slot_emul_san.cpp) ---- */
struct GridCase {
  uint32_t pattern, nb_re, fft_size, start_re;
};
std::vector<GridCase> grid_cases()
{
  static const uint32_t per_rb[3] = {12, 6, 8};
  std::vector<GridCase> v;
  for (uint32_t rb : {1u, 2u, 3u})
    for (uint32_t pattern = 0; pattern < 3; pattern++) {
      const uint32_t nb = per_rb[pattern] * rb, w = 4u * std::max(1u, nb / 8u); /* the first RE behind the wrap */
      v.push_back({pattern, nb, 128, 128 - nr_rxg_p(pattern, w)});      /* between two groups */
      v.push_back({pattern, nb, 128, 128 - nr_rxg_p(pattern, w + 1u)}); /* inside a group */
      v.push_back({pattern, nb, 128, 7});                               /* absent */
      v.push_back({pattern, nb, 128, 0});
    }
  v.push_back({NR_RXG_FULL, 1080, 2048, 2048 - 4u * 257u}); /* 90 PRBs: a second workgroup, the wrap in it */
  v.push_back({NR_RXG_FULL, 1080, 2048, 2048 - (4u * 257u + 1u)});
  v.push_back({NR_RXG_FULL, 1080, 2048, 3});
  return v;
}
nrLDPC_hip_rx_grid_seg_t grid_seg(const GridCase &c, uint32_t Qm)
{
  nrLDPC_hip_rx_grid_seg_t g;
  memset(&g, 0, sizeof g);
  g.Qm = (uint8_t)Qm;
  g.pattern = (uint8_t)c.pattern;
  g.nb_re = c.nb_re;
  g.fft_size = c.fft_size;
  g.start_re = c.start_re;
  return g;
}

/* the element-by-element form of one segment into want[first ..], and the case's record for the test */
void expect(const nrLDPC_hip_rx_grid_seg_t &g, uint32_t n_rx, const Words &rx, uint64_t rx_stride, const Words &ch, uint64_t ch_stride, int32_t shift,
            Words &want, uint64_t first)
{
  const uint32_t Qm = g.Qm, s = nr_rxf_shift(shift);
  const int32_t amp[3] = {nr_rxf_amp(Qm, 0), 0, 0};
  std::vector<uint32_t> ext_rx((size_t)n_rx * g.nb_re), ext_ch((size_t)2u * n_rx * g.nb_re);
  for (uint32_t r = 0; r < g.nb_re; r++) {
    const uint32_t p = nr_rxg_p(g.pattern, r), sc = nr_rxg_grid_sc(g.start_re, p, g.fft_size);
    nr_rxl_re_t R = {};
    for (uint32_t a = 0; a < n_rx; a++) {
      const uint32_t y = rx[g.rx_off + a * rx_stride + sc], h0 = ch[g.ch_off + a * ch_stride + p], h1 = ch[g.ch_off + (n_rx + a) * ch_stride + p];
      nr_rxl_mac(&R, h0, h1, y, s, amp);
      ext_rx[(size_t)a * g.nb_re + r] = y;
      ext_ch[(size_t)a * g.nb_re + r] = h0;
      ext_ch[(size_t)(n_rx + a) * g.nb_re + r] = h1;
    }
    for (uint32_t l = 0; l < 2; l++) {
      int32_t L[4] = {0, 0, 0, 0};
      nr_rxl_llr(&R, Qm, l, L);
      for (uint32_t k = 0; k < Qm / 2u; k++)
        want[first + (uint64_t)Qm * r + (Qm / 2u) * l + k] = nr_rxf_c16(L[2 * k], L[2 * k + 1]);
    }
  }
  if (dump) {
    const uint32_t head[4] = {n_rx, Qm, g.nb_re, (uint32_t)shift};
    fwrite(head, 4, 4, dump);
    fwrite(ext_rx.data(), 4, ext_rx.size(), dump);
    fwrite(ext_ch.data(), 4, ext_ch.size(), dump);
    fwrite(&want[first], 4, (size_t)Qm * g.nb_re, dump);
  }
}

void same(const Words &got, const Words &want, uint32_t a, uint32_t b, uint32_t c)
{
  for (uint64_t i = got.lo; i < got.hi; i++)
    if (got[i] != want[i]) {
      fprintf(stderr, "ml_2layers_grid (%u, %u, %u): word %llu is %08x, the element-wise form has %08x\n", a, b, c, (unsigned long long)i, got[i], want[i]);
      n_bad++;
      return;
    }
}

void run_ml()
{
  uint32_t turn = 0;
  for (uint32_t n_rx = 1; n_rx <= 4; n_rx++)
    for (uint32_t Qm : {2u, 4u}) {
      Exact<int32_t> shift(0, 1);
      shift[0] = (int32_t)((n_rx + Qm) % 10u);
      for (const GridCase &c : grid_cases()) {
        /* `lead` canary words in front of the first LLR: its 16-byte phase.  The inputs stay exact. */
        std::vector<uint32_t> leads = {0u, 1u, 2u, 3u};
        if (c.nb_re > 64u)
          leads = {turn++ % 4u};
        for (uint32_t lead : leads) {
          nrLDPC_hip_rx_grid_seg_t g = grid_seg(c, Qm);
          g.plane = 2u * c.nb_re;
          g.rec_off = 2u * lead;
          uint64_t lo, hi;
          rxg_rx_range(g, lo, hi);
          const uint32_t p0 = nr_rxg_p(g.pattern, 0), p1 = nr_rxg_p(g.pattern, g.nb_re - 1u) + 1u;
          const uint64_t rx_stride = g.fft_size + 3u, ch_stride = p1 + 2u;
          Words rx(lo, hi + (n_rx - 1u) * rx_stride), ch(p0, p1 + (2u * n_rx - 1u) * ch_stride);
          rx.fill(rnd_c16);
          ch.fill(rnd_c16);
          Words llr(0, lead + (uint64_t)Qm * c.nb_re), want(llr.lo, llr.hi);
          llr.fill([] { return CANARY; });
          want.fill([] { return CANARY; });
          expect(g, n_rx, rx, rx_stride, ch, ch_stride, shift[0], want, lead);
          called(emul_ml_2layers_grid(i16(rx), i16(ch), n_rx, rx_stride, ch_stride, &g, 1, shift.base(), i16w(llr)), "ml_2layers_grid");
          same(llr, want, n_rx, Qm, c.nb_re * 10000u + c.start_re);
        }
      }
    }
}

/* one call, two blocks, QPSK and 16QAM: two OFDM symbols of one grid, each block's segment with an odd sym_off */
void run_mixed()
{
  for (uint32_t n_rx : {2u, 3u}) {
    const uint32_t N = 128, nb = 18;
    nrLDPC_hip_rx_grid_seg_t g[2];
    Exact<int32_t> shift(0, 2);
    shift[0] = 3;
    shift[1] = 7;
    const uint64_t rx_stride = 2u * N, ch_stride = 40;
    /* symbol 0: FULL from subcarrier 100 (18 REs, no wrap); symbol 1: DMRS1 from 120 (wraps) */
    g[0] = grid_seg({NR_RXG_FULL, nb, N, 100}, 2);
    g[1] = grid_seg({NR_RXG_DMRS1, nb, N, 120}, 4);
    g[0].tb = 0;
    g[1].tb = 1;
    g[0].plane = g[1].plane = 2u * (nb + 5u);
    g[0].sym_off = 5;
    g[1].sym_off = 3;
    g[1].rx_off = N;
    /* block 0's LLRs: words 2 * 5 .. 2 * 23 - 1; block 1 behind them at int16 rec_off = 2 * 46 + 2: words 47 + 4 * 3 .. 47 + 4 * 21 - 1 */
    g[0].rec_off = 0;
    g[1].rec_off = 2u * 47u;
    const uint64_t f0 = 2u * 5u, f1 = 47u + 4u * 3u;
    Words rx(0, (n_rx - 1u) * rx_stride + 2u * N), ch(0, (2u * n_rx - 1u) * ch_stride + 36u), llr(f0, f1 + 4u * nb), want(llr.lo, llr.hi);
    rx.fill(rnd_c16);
    ch.fill(rnd_c16);
    llr.fill([] { return CANARY; });
    want.fill([] { return CANARY; });
    expect(g[0], n_rx, rx, rx_stride, ch, ch_stride, shift[0], want, f0);
    expect(g[1], n_rx, rx, rx_stride, ch, ch_stride, shift[1], want, f1);
    called(emul_ml_2layers_grid(i16(rx), i16(ch), n_rx, rx_stride, ch_stride, g, 2, shift.base(), i16w(llr)), "ml_2layers_grid, mixed");
    same(llr, want, n_rx, 24, 0);
  }
}

/* the level kernel (a barrier, a shuffle, atomics: 256 real threads a workgroup) */
void run_level()
{
  for (uint32_t pattern = 0; pattern < 3; pattern++)
    for (uint32_t n_rx : {2u, 3u}) {
      const uint32_t n_ch = 2u * n_rx, nb = (pattern == 0 ? 12u : pattern == 1 ? 6u : 8u) * 3u;
      nrLDPC_hip_rx_grid_seg_t g = grid_seg({pattern, nb, 128, 100}, 2);
      g.plane = 4u * nb;
      const uint32_t p0 = nr_rxg_p(pattern, 0), p1 = nr_rxg_p(pattern, nb - 1u) + 1u;
      const uint64_t stride = p1 + 1u;
      Words ch(p0, p1 + (n_ch - 1u) * stride);
      ch.fill(rnd_c16);
      Exact<int32_t> out(0, 1), max_ch(0, 1);
      out[0] = -7;
      max_ch[0] = pattern == 1 ? 9000 : 1500;
      const uint32_t len = nr_rxf_level_len(nb), x = (uint32_t)nr_rxf_factor2(len), sce = nr_rxm_shift_ch_ext(max_ch[0]);
      int32_t avgs = 0;
      for (uint32_t a = 0; a < n_ch; a++) {
        uint32_t sum = 0;
        for (uint32_t r = 0; r < nb; r++)
          sum += (uint32_t)nr_rxm_level_term(ch[a * stride + nr_rxg_p(pattern, r)], x, sce);
        avgs = std::max(avgs, nr_rxf_level_avg((int32_t)sum, len));
      }
      called(emul_channel_level_grid_ml(i16(ch), n_rx, stride, &g, 1, max_ch.base(), out.base()), "channel_level_grid_ml");
      if (out[0] != nr_rxl_log2_maxh(avgs)) {
        fprintf(stderr, "channel_level_grid_ml (pattern %u): %d, the element-wise form has %d\n", pattern, out[0], nr_rxl_log2_maxh(avgs));
        n_bad++;
      }
    }
}

} // namespace

int main(int argc, char **argv)
{
  if (argc > 1 && !(dump = fopen(argv[1], "wb"))) {
    fprintf(stderr, "cannot write %s\n", argv[1]);
    return 2;
  }
  run_ml();
  run_mixed();
  run_level();
  if (dump)
    fclose(dump);
  printf("%ld calls, %ld mismatches or refusals\n", n_calls, n_bad);
  return n_bad == 0 && n_calls > 0 ? 0 : 1;
}
