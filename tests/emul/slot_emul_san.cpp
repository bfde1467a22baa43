/*
 * slot_emul_san.cpp -- the slot-level kernels (slot_rx_emul.cpp, slot_tx_emul.cpp, slot_scr_emul.cpp: the .hip files on the CPU)
 * on arrays that are exactly as long as include/nrLDPC_hip.h says a DEVICE mem caller's must be.  A stand-alone program, built
 * with -fsanitize=address,undefined by tests/test_slot_kernels_san.py: every array is a heap allocation of its own, so a read or
 * a write in front of the first element a call may touch or behind the last one is a report, and so is a misaligned vector
 * access or an arithmetic overflow.  A call has one descriptor, which is then the first and the last: its ranges begin at the
 * allocation's first element and end at its last, the last antenna's or layer's plane at the stated stride included.  Results
 * are compared with the element-by-element forms (the loops of the *_host calls over the same arithmetic headers).
 *
 * Shapes: the smallest that reach every branch -- fft_size 128, 1, 2 and 3 PRBs of every pattern (nb_re % 4 != 0 and == 0), the
 * grid's wrap between two quads, inside one and absent, one 1080-RE segment (more than a workgroup's piece), the four estimator
 * modes with rb_size 1, 2, 3, 5 at every residue of ch_off mod 4, n_rx 1..4, every Qm, the mapping's (n_tx, Nl) pairs, scrambling
 * sizes 1, 31, 32, 33 and around a workgroup's 1024 words.  The allocations begin 16-byte aligned (the allocator's choice); where a
 * kernel lays its groups by the output address, the output array has 0..3 canary elements in front (leads()) and the inputs
 * stay exact.
 * Exit status 0 and nothing on stderr: clean.
 */
#include <hip/hip_runtime.h> /* the host shim: the plan headers below name hipError_t and hipStream_t */
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

namespace {
int set_error(const char *what)
{
  fprintf(stderr, "refused: %s\n", what);
  return -1;
}
} // namespace
#include "rx_plan.h"
#include "rx_chest_plan.h"
#include "tx_map_plan.h"
#include "nr_qam.h"
#include "tb_jobs.h"

extern "C" {
const char *slot_emul_last_error();
int32_t slot_emul_channel_compensation(const int16_t *, const int16_t *, uint32_t, uint64_t, const nrLDPC_hip_rx_seg_t *, uint32_t, const int32_t *, int16_t *);
int32_t slot_emul_channel_level(const int16_t *, uint32_t, uint64_t, const nrLDPC_hip_rx_seg_t *, uint32_t, int32_t *);
int32_t slot_emul_channel_compensation_grid(const int16_t *, const int16_t *, uint32_t, uint64_t, uint64_t, const nrLDPC_hip_rx_grid_seg_t *, uint32_t,
                                            const int32_t *, int16_t *);
int32_t slot_emul_channel_level_grid(const int16_t *, uint32_t, uint64_t, const nrLDPC_hip_rx_grid_seg_t *, uint32_t, int32_t *);
int32_t slot_emul_mmse_2layers_grid(const int16_t *, const int16_t *, uint32_t, uint64_t, uint64_t, const nrLDPC_hip_rx_grid_seg_t *, uint32_t, const int32_t *,
                                    const uint32_t *, int16_t *);
int32_t slot_emul_channel_level_grid_mmse(const int16_t *, uint32_t, uint64_t, const nrLDPC_hip_rx_grid_seg_t *, uint32_t, const int32_t *, int32_t *);
int32_t slot_emul_pusch_channel_estimation(const int16_t *, uint64_t, int16_t *, uint64_t, uint32_t, const nrLDPC_hip_chest_seg_t *, uint32_t, const int32_t *);
int32_t slot_emul_pdsch_resource_mapping(const int16_t *, int16_t *, uint64_t, uint32_t, const nrLDPC_hip_pdsch_map_seg_t *, uint32_t);
int32_t slot_emul_pdsch_resource_mapping_precoded(const int16_t *, int16_t *, uint64_t, uint32_t, const nrLDPC_hip_pdsch_map_seg_t *,
                                                  const nrLDPC_hip_pdsch_prg_t *, uint32_t, const uint16_t *, uint32_t, const nrLDPC_hip_pm_pdu_t *, uint32_t);
int32_t slot_emul_modulation(const uint32_t *, uint32_t, uint32_t, int16_t *);
int32_t slot_emul_ulsch_llr(const int32_t *, const int32_t *, const int32_t *, const int32_t *, uint32_t, uint32_t, int16_t *);
int32_t slot_emul_layer_mapping(const int16_t *, uint32_t, uint32_t, int16_t *, uint32_t);
int32_t slot_emul_scramble_map_tb(const tb_sym_tb_job *, uint32_t, uint32_t, const uint8_t *, uint8_t *);
int32_t slot_emul_scramble_bits(const uint8_t *, uint32_t, uint32_t, uint32_t *);
int32_t slot_emul_unscramble_llr(int16_t *, uint32_t, uint32_t);
int32_t slot_emul_scramble_bits_tb(const tb_scr_tb_job *, uint32_t, uint32_t, const uint8_t *, uint8_t *);
}

namespace {

const uint32_t CANARY = 0x5a5a5a5au;
long n_calls = 0, n_bad = 0;

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

/* elements lo .. hi - 1 of an array: a heap allocation of exactly hi - lo elements.  base() is where element 0 would be: the
 * calls index from there, and nothing below lo or from hi on belongs to the allocation */
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

void called(int32_t rc, const char *what)
{
  n_calls++;
  if (rc != 0) {
    fprintf(stderr, "%s: refused: %s\n", what, slot_emul_last_error());
    n_bad++;
  }
}
void same(const Words &got, const Words &want, const char *what, uint32_t a, uint32_t b, uint32_t c)
{
  for (uint64_t i = got.lo; i < got.hi; i++)
    if (got[i] != want[i]) {
      fprintf(stderr, "%s (%u, %u, %u): entry %llu is %08x, the element-wise form has %08x\n", what, a, b, c, (unsigned long long)i, got[i], want[i]);
      n_bad++;
      return;
    }
}

/* ---- the grid segments: pattern, PRBs, where the wrap falls ---- */
struct GridCase {
  uint32_t pattern, nb_re, fft_size, start_re;
};
std::vector<GridCase> grid_cases()
{
  static const uint32_t per_rb[3] = {12, 6, 8};
  std::vector<GridCase> v;
  /* 2 PRBs: nb_re % 4 == 0 for every pattern, so the last quad is a whole one and its vector loads end with the arrays (with 1
   * and 3 PRBs of DMRS1 a partial quad follows, and a load that reaches one c16 too far stays inside) */
  for (uint32_t rb : {1u, 2u, 3u})
    for (uint32_t pattern = 0; pattern < 3; pattern++) {
      const uint32_t nb = per_rb[pattern] * rb, w = 4u * std::max(1u, nb / 8u); /* the first RE behind the wrap */
      v.push_back({pattern, nb, 128, 128 - nr_rxg_p(pattern, w)});      /* between two quads */
      v.push_back({pattern, nb, 128, 128 - nr_rxg_p(pattern, w + 1u)}); /* inside a quad */
      v.push_back({pattern, nb, 128, 7});                               /* absent */
      v.push_back({pattern, nb, 128, 0});
    }
  /* 90 PRBs: a second workgroup, the wrap in it */
  v.push_back({NR_RXG_FULL, 1080, 2048, 2048 - 4u * 257u});
  v.push_back({NR_RXG_FULL, 1080, 2048, 2048 - (4u * 257u + 1u)});
  v.push_back({NR_RXG_FULL, 1080, 2048, 3});
  return v;
}
nrLDPC_hip_rx_grid_seg_t grid_seg(const GridCase &c, uint32_t Qm, uint32_t plane)
{
  nrLDPC_hip_rx_grid_seg_t g;
  memset(&g, 0, sizeof g);
  g.Qm = (uint8_t)Qm;
  g.pattern = (uint8_t)c.pattern;
  g.nb_re = c.nb_re;
  g.plane = plane;
  g.fft_size = c.fft_size;
  g.start_re = c.start_re;
  return g;
}
/* the grid and the estimates of one segment for n_rx antennas and n_ch estimate arrays, each exactly as far as the segment reaches */
struct GridArrays {
  uint64_t rx_stride, ch_stride;
  Words rx, ch;
  GridArrays(const nrLDPC_hip_rx_grid_seg_t &g, uint32_t n_rx, uint32_t n_ch, uint64_t lo, uint64_t hi, uint32_t p0, uint32_t p1)
      : rx_stride(g.fft_size + 3u), ch_stride(p1 + 2u), rx(lo, hi + (n_rx - 1u) * rx_stride), ch(p0, p1 + (n_ch - 1u) * ch_stride)
  {
    rx.fill(rnd_c16);
    ch.fill(rnd_c16);
  }
};
GridArrays grid_arrays(const nrLDPC_hip_rx_grid_seg_t &g, uint32_t n_rx, uint32_t n_ch)
{
  uint64_t lo, hi;
  rxg_rx_range(g, lo, hi);
  return GridArrays(g, n_rx, n_ch, lo, hi, nr_rxg_p(g.pattern, 0), nr_rxg_p(g.pattern, g.nb_re - 1u) + 1u);
}

/* The first output element's alignment phase.  An allocation begins 16-byte aligned, so an output array that begins with its
 * first written element has phase 0 alone.  `lead` canary elements in front of it give the phases 1..3 -- the kernels lay their
 * 16-byte stores by the output address, so a first group that begins in front of the segment and a last one that ends behind
 * it (tb_rx_front.hip: r0 < 0; tb_tx_map.hip: i0 < 0; the head of tb_rx_chest.hip) -- while the input arrays stay exact, so
 * that a read such a group makes in front of or behind the segment's inputs is a report.  The long segments take one phase each
 * in turn. */
std::vector<uint32_t> leads(uint32_t n)
{
  static uint32_t turn = 0;
  if (n > 64u)
    return {turn++ % 4u};
  return {0u, 1u, 2u, 3u};
}

/* ---- single layer: compensation on extracted arrays and from the grid, against the loop of compensate_host ---- */
void run_compensation()
{
  for (uint32_t n_rx = 1; n_rx <= 4; n_rx++)
    for (uint32_t Qm = 2; Qm <= 8; Qm += 2) {
      const uint32_t np = Qm / 2u;
      const int32_t amp[3] = {nr_rxf_amp(Qm, 0), nr_rxf_amp(Qm, 1), nr_rxf_amp(Qm, 2)};
      Exact<int32_t> shift(0, 1);
      shift[0] = (int32_t)((n_rx + Qm) % 13u);
      const uint32_t s = nr_rxf_shift(shift[0]);
      /* extracted */
      for (uint32_t nb : {1u, 3u, 4u, 6u, 18u, 1080u})
       for (uint32_t lead : leads(nb)) {
        const uint64_t stride = nb + 1u;
        const uint32_t plane = nb + 2u;
        Words rx(0, (n_rx - 1u) * stride + nb), ch(0, (n_rx - 1u) * stride + nb), rec(0, lead + (uint64_t)(np - 1u) * plane + nb), want(rec.lo, rec.hi);
        rx.fill(rnd_c16);
        ch.fill(rnd_c16);
        rec.fill([] { return CANARY; });
        want.fill([] { return CANARY; });
        for (uint32_t r = 0; r < nb; r++) {
          nr_rxf_acc_t acc = {{0, 0, 0, 0}};
          for (uint32_t a = 0; a < n_rx; a++)
            nr_rxf_mac(&acc, ch[a * stride + r], rx[a * stride + r], s, amp);
          for (uint32_t k = 0; k < np; k++)
            want[lead + (uint64_t)k * plane + r] = acc.w[k];
        }
        nrLDPC_hip_rx_seg_t g;
        memset(&g, 0, sizeof g);
        g.Qm = (uint8_t)Qm;
        g.nb_re = nb;
        g.plane = plane;
        g.rec_off = 2u * lead;
        called(slot_emul_channel_compensation(i16(rx), i16(ch), n_rx, stride, &g, 1, shift.base(), i16w(rec)), "channel_compensation");
        same(rec, want, "channel_compensation", n_rx, Qm, nb * 10u + lead);
      }
      /* from the grid */
      for (const GridCase &c : grid_cases())
       for (uint32_t lead : leads(c.nb_re)) {
        const uint32_t plane = c.nb_re + 1u;
        nrLDPC_hip_rx_grid_seg_t g = grid_seg(c, Qm, plane);
        g.rec_off = 2u * lead;
        GridArrays A = grid_arrays(g, n_rx, n_rx);
        Words rec(0, lead + (uint64_t)(np - 1u) * plane + c.nb_re), want(rec.lo, rec.hi);
        rec.fill([] { return CANARY; });
        want.fill([] { return CANARY; });
        for (uint32_t r = 0; r < c.nb_re; r++) {
          const uint32_t p = nr_rxg_p(c.pattern, r), sc = nr_rxg_grid_sc(c.start_re, p, c.fft_size);
          nr_rxf_acc_t acc = {{0, 0, 0, 0}};
          for (uint32_t a = 0; a < n_rx; a++)
            nr_rxf_mac(&acc, A.ch[a * A.ch_stride + p], A.rx[a * A.rx_stride + sc], s, amp);
          for (uint32_t k = 0; k < np; k++)
            want[lead + (uint64_t)k * plane + r] = acc.w[k];
        }
        called(slot_emul_channel_compensation_grid(i16(A.rx), i16(A.ch), n_rx, A.rx_stride, A.ch_stride, &g, 1, shift.base(), i16w(rec)),
               "channel_compensation_grid");
        same(rec, want, "channel_compensation_grid", n_rx, Qm, c.nb_re * 10000u + c.start_re);
      }
    }
}

/* ---- two layers: the MMSE receiver from the grid, against the loop of mmse_2layers_host ---- */
void run_mmse()
{
  for (uint32_t n_rx : {2u, 4u})
    for (uint32_t Qm : {6u, 8u}) {
      const uint32_t np = Qm / 2u;
      Exact<int32_t> shift(0, 1);
      Exact<uint32_t> nvar(0, 1);
      shift[0] = (int32_t)(n_rx + Qm) % 10;
      nvar[0] = n_rx == 2 ? 70000u : 37u;
      const uint32_t s = nr_rxf_shift(shift[0]);
      for (const GridCase &c : grid_cases()) {
        const uint32_t plane = 2u * c.nb_re + 3u;
        const nrLDPC_hip_rx_grid_seg_t g = grid_seg(c, Qm, plane);
        GridArrays A = grid_arrays(g, n_rx, 2u * n_rx);
        Words rec(0, (uint64_t)(np - 1u) * plane + 2u * c.nb_re), want(rec.lo, rec.hi);
        rec.fill([] { return CANARY; });
        want.fill([] { return CANARY; });
        for (uint32_t r0 = 0; r0 < c.nb_re; r0 += NR_RXM_QUAD) {
          nr_rxm_re_t R[NR_RXM_QUAD] = {};
          int32_t det[NR_RXM_QUAD];
          for (uint32_t u = 0; u < NR_RXM_QUAD; u++) {
            if (r0 + u < c.nb_re) {
              const uint32_t p = nr_rxg_p(c.pattern, r0 + u), sc = nr_rxg_grid_sc(c.start_re, p, c.fft_size);
              for (uint32_t a = 0; a < n_rx; a++)
                nr_rxm_mac(&R[u], A.ch[a * A.ch_stride + p], A.ch[(n_rx + a) * A.ch_stride + p], A.rx[a * A.rx_stride + sc], s);
            }
            det[u] = nr_rxm_det(&R[u], nvar[0]);
          }
          const int32_t bm = nr_rxm_b_mag(det), bs = nr_rxm_b_sym(det);
          for (uint32_t u = 0; u < NR_RXM_QUAD && r0 + u < c.nb_re; u++)
            for (uint32_t l = 0; l < 2; l++)
              for (uint32_t k = 0; k < np; k++)
                want[(uint64_t)k * plane + 2u * (r0 + u) + l] =
                    k == 0 ? (l == 0 ? nr_rxm_sym0(&R[u], bs) : nr_rxm_sym1(&R[u], bs)) : nr_rxm_mag(det[u], bm, nr_rxf_amp(Qm, k - 1u));
        }
        called(slot_emul_mmse_2layers_grid(i16(A.rx), i16(A.ch), n_rx, A.rx_stride, A.ch_stride, &g, 1, shift.base(), nvar.base(), i16w(rec)),
               "mmse_2layers_grid");
        same(rec, want, "mmse_2layers_grid", n_rx, Qm, c.nb_re * 10000u + c.start_re);
      }
    }
}

/* ---- the level kernels (a barrier, a shuffle, atomics: 256 real threads a workgroup, so a handful of them) ---- */
void run_levels()
{
  /* extracted, n_rx 3: 17 REs and 300 */
  for (uint32_t nb : {17u, 300u}) {
    const uint32_t n_rx = 3;
    const uint64_t stride = nb + 5u;
    Words ch(0, (n_rx - 1u) * stride + nb);
    ch.fill(rnd_c16);
    const uint32_t len = nr_rxf_level_len(nb), x = (uint32_t)nr_rxf_factor2(len);
    int32_t avgs = 0;
    for (uint32_t a = 0; a < n_rx; a++) {
      uint32_t sum = 0;
      for (uint32_t r = 0; r < nb; r++)
        sum += (uint32_t)nr_rxf_level_term(ch[a * stride + r], x);
      avgs = std::max(avgs, nr_rxf_level_avg((int32_t)sum, len));
    }
    nrLDPC_hip_rx_seg_t g;
    memset(&g, 0, sizeof g);
    g.Qm = 2;
    g.nb_re = nb;
    g.plane = nb;
    Exact<int32_t> out(0, 1);
    out[0] = -7;
    called(slot_emul_channel_level(i16(ch), n_rx, stride, &g, 1, out.base()), "channel_level");
    if (out[0] != nr_rxf_log2_maxh(avgs, n_rx)) {
      fprintf(stderr, "channel_level (%u REs): %d, the element-wise form has %d\n", nb, out[0], nr_rxf_log2_maxh(avgs, n_rx));
      n_bad++;
    }
  }
  /* from the grid: every pattern, 3 PRBs; single layer with n_rx 2, two layers with n_rx 2 (4 pairs) */
  for (uint32_t pattern = 0; pattern < 3; pattern++)
    for (uint32_t mmse = 0; mmse < 2; mmse++) {
      const uint32_t n_rx = 2, n_ch = mmse ? 4u : 2u, nb = (pattern == 0 ? 12u : pattern == 1 ? 6u : 8u) * 3u;
      const nrLDPC_hip_rx_grid_seg_t g = grid_seg({pattern, nb, 128, 100}, 6, 4u * nb);
      const uint32_t p0 = nr_rxg_p(pattern, 0), p1 = nr_rxg_p(pattern, nb - 1u) + 1u;
      const uint64_t stride = p1 + 1u;
      Words ch(p0, p1 + (n_ch - 1u) * stride);
      ch.fill(rnd_c16);
      Exact<int32_t> out(0, 1), max_ch(0, 1);
      out[0] = -7;
      max_ch[0] = 9000;
      const uint32_t len = nr_rxf_level_len(nb), x = (uint32_t)nr_rxf_factor2(len), sce = nr_rxm_shift_ch_ext(max_ch[0]);
      int32_t avgs = 0;
      for (uint32_t a = 0; a < n_ch; a++) {
        uint32_t sum = 0;
        for (uint32_t r = 0; r < nb; r++) {
          const uint32_t h = ch[a * stride + nr_rxg_p(pattern, r)];
          sum += (uint32_t)(mmse ? nr_rxm_level_term(h, x, sce) : nr_rxf_level_term(h, x));
        }
        avgs = std::max(avgs, nr_rxf_level_avg((int32_t)sum, len));
      }
      const int32_t want = mmse ? nr_rxm_log2_maxh(avgs) : nr_rxf_log2_maxh(avgs, n_rx);
      if (mmse)
        called(slot_emul_channel_level_grid_mmse(i16(ch), n_rx, stride, &g, 1, max_ch.base(), out.base()), "channel_level_grid_mmse");
      else
        called(slot_emul_channel_level_grid(i16(ch), n_rx, stride, &g, 1, out.base()), "channel_level_grid");
      if (out[0] != want) {
        fprintf(stderr, "channel_level_grid%s (pattern %u): %d, the element-wise form has %d\n", mmse ? "_mmse" : "", pattern, out[0], want);
        n_bad++;
      }
    }
}

/* ---- PUSCH DMRS channel estimation, against the loop of pusch_chest_host ---- */
void run_chest()
{
  const uint32_t N = 128;
  std::vector<uint32_t> table;
  che_fill_table(N, table);
  uint32_t idx = 0;
  for (uint32_t mode = 0; mode < NR_CHE_MODES; mode++)
    for (uint32_t rb : {1u, 2u, 3u, 5u})
      for (uint32_t res = 0; res < 4; res++, idx++) {
        const uint32_t n_rx = 1u + idx % 4u;
        nrLDPC_hip_chest_seg_t g;
        memset(&g, 0, sizeof g);
        g.mode = (uint8_t)mode;
        g.port = (uint8_t)((idx * 5u) % nr_che_ports(mode));
        g.fft_size = N;
        static const uint32_t starts[4] = {0u, N - 7u, N - 12u, 9u}; /* no wrap, inside a PRB, between two PRBs, none */
        g.start_re = starts[idx % 4u];
        g.rb_size = rb;
        g.dmrs_offset = idx * 37u;
        g.c_init = rnd() & 0x7fffffffu;
        g.ch_off = res; /* the estimates begin res c16 behind the allocation's 16-byte aligned start, canaries in front of them */
        if (che_check_seg("san", g) != 0) { /* a pilot at subcarrier N - 1 with nushift 1: take the other side of the wrap */
          g.start_re = 3;
          if (che_check_seg("san", g) != 0) {
            n_bad++;
            continue;
          }
        }
        uint32_t lo, hi;
        che_rx_range(g, lo, hi);
        const uint64_t rs = N + 1u, cs = 12u * rb + 1u;
        Words rx(lo, hi + (n_rx - 1u) * rs), ch(0, res + 12u * rb + (n_rx - 1u) * cs), want(ch.lo, ch.hi);
        rx.fill(rnd_c16);
        ch.fill([] { return CANARY; });
        want.fill([] { return CANARY; });
        Exact<int32_t> delay(0, n_rx);
        for (uint32_t a = 0; a < n_rx; a++)
          delay[a] = (int32_t)(rnd() % 41u) - 20;
        std::vector<uint32_t> gold;
        uint32_t w0;
        if (!dmrs_gold_words(g.c_init, g.dmrs_offset, nr_che_pilots_per_rb(mode) * rb, gold, w0)) {
          n_bad++;
          continue;
        }
        for (uint32_t a = 0; a < n_rx; a++) {
          const uint32_t *sym = rx.base() + a * rs, *fwd = table.data() + (size_t)nr_che_delay_idx(delay[a]) * N,
                         *inv = table.data() + (size_t)nr_che_inv_delay_idx(delay[a]) * N;
          uint32_t *out = &want[res + a * cs];
          for (uint32_t u = 0; u < nr_che_units(mode, rb); u++) {
            const uint64_t bits = dmrs_bits(gold, w0, g.dmrs_offset + nr_che_unit_first_pilot(mode, u));
            if (mode == NR_CHE_TYPE1_INTERP)
              nr_che_t1_interp(sym, N, g.start_re, rb, g.port, g.dmrs_offset, bits, fwd, inv, u, out + 4u * u);
            else if (mode == NR_CHE_TYPE2_INTERP)
              nr_che_t2_interp(sym, N, g.start_re, g.port, g.dmrs_offset, bits, inv, u, out + 4u * u);
            else
              for (uint32_t k = 0; k < 12u; k++)
                out[12u * u + k] = nr_che_avg(mode, sym, N, g.start_re, g.port, g.dmrs_offset, bits, u);
          }
        }
        called(slot_emul_pusch_channel_estimation(i16(rx), rs, i16w(ch), cs, n_rx, &g, 1, delay.base()), "channel_estimation");
        same(ch, want, "channel_estimation", mode, rb, res);
      }
}

/* ---- PDSCH resource mapping, unit and precoded, against the loops of pdsch_map_host and pdsch_precode_host ---- */
void run_mapping()
{
  const uint32_t N = 128;
  static const uint32_t pairs[][2] = {{1, 1}, {2, 2}, {4, 4}, {3, 2}, {2, 1}, {4, 2}, {8, 3}};
  static const uint8_t ports[3][4] = {{0, 0, 0, 0}, {0, 1, 4, 5}, {1, 0, 6, 7}};
  static const uint32_t per_rb[3] = {12, 6, 8}; /* ncdm = 1 */
  uint32_t idx = 0;
  for (const auto &pr : pairs)
    for (uint32_t pattern = 0; pattern < NR_PDM_PATTERNS; pattern++)
      for (uint32_t rb : {1u, 3u})
        for (uint32_t k0 : {0u, N - 7u, N - 12u, 5u})
          for (uint32_t precoded = 0; precoded < 2; precoded++, idx++) {
            const uint32_t n_tx = pr[0], Nl = pr[1];
            if (precoded && n_tx < 2)
              continue;
            nrLDPC_hip_pdsch_map_seg_t g;
            memset(&g, 0, sizeof g);
            g.pattern = (uint8_t)pattern;
            g.Nl = (uint8_t)Nl;
            g.ncdm = pattern ? 1 : 0;
            g.l_prime = pattern ? (uint8_t)(idx & 1u) : 0;
            memcpy(g.port, ports[pattern], 4);
            static const int16_t amps[4] = {1, 512, 32767, 9000};
            g.amp = amps[idx % 4u];
            g.fft_size = N;
            g.start_re = k0;
            g.rb_size = rb;
            g.nb_re = per_rb[pattern] * rb;
            g.plane = g.nb_re + 1u;
            g.dmrs_offset = pattern ? idx * 11u : 0;
            g.c_init = pattern ? rnd() & 0x7fffffffu : 0;
            if (txm_check_seg("san", g) != 0) {
              n_bad++;
              continue;
            }
            const uint32_t n_re = 12u * rb;
            const bool wraps = k0 + n_re > N;
            const uint64_t stride = N + 1u, lo = wraps ? 0 : k0, hi = wraps ? N : k0 + n_re;
            const uint32_t lead = (idx / 2u) % 4u; /* canaries in front of antenna 0's symbol: see leads() */
            g.tx_off = lead;
            Words lay(0, (uint64_t)(Nl - 1u) * g.plane + g.nb_re), tx(lo, lead + hi + (n_tx - 1u) * stride), want(tx.lo, tx.hi);
            lay.fill(rnd_c16);
            tx.fill([] { return CANARY; });
            want.fill([] { return CANARY; });
            /* one PRG a PRB: matrices 2, 0 (unit), 1 in turn */
            nrLDPC_hip_pdsch_prg_t prg = {1, 0, rb};
            const uint16_t pmis[5] = {7, 0, 3, 3, 7};
            nrLDPC_hip_pm_pdu_t pm[2];
            memset(pm, 0, sizeof pm);
            for (uint32_t t = 0; t < 2; t++) {
              pm[t].pm_idx = t ? 7 : 3;
              pm[t].numLayers = (uint16_t)Nl;
              pm[t].num_ant_ports = 8;
              for (uint32_t l = 0; l < Nl; l++)
                for (uint32_t a = 0; a < 8; a++) {
                  pm[t].weights[l][a][0] = (int16_t)rnd();
                  pm[t].weights[l][a][1] = (int16_t)rnd();
                }
            }
            TxPrecodePlan pp;
            if (precoded && txp_plan("san", &g, &prg, 1, n_tx, pmis, 5, pm, 2, pp) != 0) {
              n_bad++;
              continue;
            }
            const uint32_t last = nr_pdm_last_pmask(pattern);
            nr_pdm_sym s[NR_PDM_MAX_LAYERS];
            for (uint32_t l = 0; l < Nl; l++)
              s[l] = nr_pdm_sym_make(pattern, g.ncdm, g.l_prime, g.port[l], g.amp);
            std::vector<uint32_t> gold;
            uint32_t w0 = 0;
            if (pattern != NR_PDM_FULL && !dmrs_gold_words(g.c_init, g.dmrs_offset, nr_pdm_count(last, n_re) + 1u, gold, w0)) {
              n_bad++;
              continue;
            }
            for (uint32_t a = 0; a < n_tx; a++)
              for (uint32_t i = 0; i < n_re; i++) {
                uint32_t &dst = want[lead + a * stride + nr_pdm_wrap(k0, i, N)];
                if (!precoded) {
                  if (a >= Nl) {
                    dst = 0;
                    continue;
                  }
                  const uint32_t jlo = nr_pdm_count(s[a].pmask, i);
                  dst = nr_pdm_re(&s[a], lay.base() + (uint64_t)a * g.plane, i, pattern ? dmrs_bits(gold, w0, g.dmrs_offset + jlo) : 0, jlo);
                  continue;
                }
                const uint32_t jlo = nr_pdm_count(last, i), pmx = pp.pmx[pp.prgs[0].pmx_off + (i / 12u) / pp.prgs[0].prg_size];
                const uint64_t bits = pattern ? dmrs_bits(gold, w0, g.dmrs_offset + jlo) : 0;
                uint32_t m[NR_PDM_MAX_LAYERS] = {0, 0, 0, 0}, wt[NR_PDM_MAX_LAYERS] = {0, 0, 0, 0};
                for (uint32_t l = 0; l < Nl; l++) {
                  m[l] = nr_pdm_re(&s[l], lay.base() + (uint64_t)l * g.plane, i, bits, jlo);
                  if (pmx)
                    wt[l] = pp.mats[pmx - 1u].w[l][a];
                }
                dst = nr_pdm_antenna(m, wt, Nl, a, pmx);
              }
            if (precoded)
              called(slot_emul_pdsch_resource_mapping_precoded(i16(lay), i16w(tx), stride, n_tx, &g, &prg, 1, pmis, 5, pm, 2),
                     "pdsch_resource_mapping_precoded");
            else
              called(slot_emul_pdsch_resource_mapping(i16(lay), i16w(tx), stride, n_tx, &g, 1), "pdsch_resource_mapping");
            same(tx, want, precoded ? "pdsch_resource_mapping_precoded" : "pdsch_resource_mapping", n_tx * 10u + Nl, pattern * 10u + rb, k0);
          }
}

/* ---- the standalone QAM passes ---- */
void run_qam()
{
  static const nr_qam_tables_t tab = nr_qam_make_tables();
  for (uint32_t Qm = 2; Qm <= 8; Qm += 2) {
    const uint32_t np = Qm / 2u;
    for (uint32_t n_sym : {1u, 3u, 4u, 5u, 11u, 16u, 1025u}) {
      /* modulation: ceil(length / 32) words in, n_sym points out */
      const uint32_t length = n_sym * Qm, nw = (length + 31u) / 32u;
      Words in(0, nw), out(0, n_sym);
      in.fill(rnd);
      out.fill([] { return CANARY; });
      called(slot_emul_modulation(in.base(), length, Qm, i16w(out)), "modulation");
      for (uint32_t i = 0; i < n_sym; i++) {
        uint32_t x = 0;
        for (uint32_t b = 0; b < Qm; b++)
          x |= ((in[(i * Qm + b) >> 5] >> ((i * Qm + b) & 31u)) & 1u) << b;
        if (out[i] != tab.pt[nr_qam_table_off(Qm) + x]) {
          fprintf(stderr, "modulation (Qm %u, %u symbols): point %u differs\n", Qm, n_sym, i);
          n_bad++;
          break;
        }
      }
      /* soft demapping: Qm / 2 planes of n_sym c16 in, n_sym Qm int16 out */
      std::vector<std::unique_ptr<Words>> pl;
      const int32_t *p[4] = {nullptr, nullptr, nullptr, nullptr};
      for (uint32_t k = 0; k < np; k++) {
        pl.emplace_back(new Words(0, n_sym));
        pl.back()->fill(rnd_c16);
        p[k] = reinterpret_cast<const int32_t *>(pl.back()->base());
      }
      Words llr(0, (uint64_t)n_sym * np), want(0, (uint64_t)n_sym * np);
      llr.fill([] { return CANARY; });
      for (uint32_t r = 0; r < n_sym; r++) {
        uint32_t x[4] = {0, 0, 0, 0};
        for (uint32_t k = 0; k < np; k++)
          x[k] = (*pl[k])[r];
        nr_qam_demap(Qm, x);
        for (uint32_t k = 0; k < np; k++)
          want[(uint64_t)r * np + k] = x[k];
      }
      called(slot_emul_ulsch_llr(p[0], p[1], p[2], p[3], n_sym, Qm, i16w(llr)), "ulsch_llr");
      same(llr, want, "ulsch_llr", Qm, n_sym, 0);
    }
  }
  /* layer mapping: n points in, Nl planes at a stride out, the last plane ends with the array */
  for (uint32_t Nl = 1; Nl <= 4; Nl++)
    for (uint32_t per : {1u, 3u, 4u, 5u, 8u, 1025u})
      for (uint32_t stride : {per, per + 3u, per + 4u}) {
        Words in(0, (uint64_t)per * Nl), out(0, (uint64_t)(Nl - 1u) * stride + per), want(out.lo, out.hi);
        in.fill(rnd);
        out.fill([] { return CANARY; });
        want.fill([] { return CANARY; });
        for (uint32_t l = 0; l < Nl; l++)
          for (uint32_t i = 0; i < per; i++)
            want[(uint64_t)l * stride + i] = in[(uint64_t)Nl * i + l];
        called(slot_emul_layer_mapping(i16(in), per * Nl, Nl, i16w(out), stride), "layer_mapping");
        same(out, want, "layer_mapping", Nl, per, stride);
      }
}

/* ---- scrambling: 256 real threads a workgroup ---- */
void run_scrambling()
{
  uint32_t idx = 0;
  for (uint32_t size : {1u, 31u, 32u, 33u, 32u * 1023u, 32u * 1024u - 5u, 32u * 1024u + 1u, 32u * 1025u}) {
    const uint32_t c_init = (rnd() & 0x7fffffffu) | 1u, nw = (size + 31u) / 32u;
    std::vector<uint32_t> gold(nw);
    if (nr_hip_gold_words(c_init, 0, nw, gold.data()) != 0) {
      n_bad++;
      continue;
    }
    const auto c_bit = [&](uint32_t i) { return (gold[i >> 5] >> (i & 31u)) & 1u; };
    Exact<uint8_t> in(0, size);
    in.fill([] { return (uint8_t)rnd(); });
    /* scrambling: size bytes in, ceil(size / 32) words out */
    Words out(0, nw);
    out.fill([] { return CANARY; });
    called(slot_emul_scramble_bits(in.base(), size, c_init, out.base()), "codeword_scrambling");
    bool ok = true;
    for (uint32_t i = 0; i < 32u * nw && ok; i++)
      ok = ((out[i >> 5] >> (i & 31u)) & 1u) == (i < size ? (in[i] & 1u) ^ c_bit(i) : 0u);
    /* the packer of the encode call: one job */
    Words packed(0, nw);
    packed.fill([] { return CANARY; });
    Exact<tb_scr_tb_job> job(0, 1);
    job[0] = tb_scr_tb_job{0, 0, size, c_init};
    called(slot_emul_scramble_bits_tb(job.base(), 1, size, in.base(), reinterpret_cast<uint8_t *>(packed.base())), "scramble_bits_tb");
    for (uint32_t w = 0; w < nw && ok; w++)
      ok = packed[w] == out[w];
    /* unscrambling: size int16 in place */
    Exact<int16_t> llr(0, size), before(0, size);
    llr.fill([] { return (int16_t)rnd(); });
    llr[0] = -32768;
    for (uint32_t i = 0; i < size; i++)
      before[i] = llr[i];
    called(slot_emul_unscramble_llr(llr.base(), size, c_init), "codeword_unscrambling");
    for (uint32_t i = 0; i < size && ok; i++)
      ok = llr[i] == (c_bit(i) ? (int16_t)(uint16_t)(0u - (uint32_t)(uint16_t)before[i]) : before[i]);
    /* scrambling + mapping + layer mapping of the symbol encode: the sizes that are whole symbols */
    const uint32_t Qm = 2u + 2u * (idx % 4u), Nl = 1u + idx % 4u;
    idx++;
    if (ok && size % (Qm * Nl) == 0) {
      static const nr_qam_tables_t tab = nr_qam_make_tables();
      const uint32_t S = size / Qm, plane = S / Nl;
      Words pts(0, S);
      pts.fill([] { return CANARY; });
      Exact<tb_sym_tb_job> sj(0, 1);
      sj[0] = tb_sym_tb_job{0, 0, size, c_init, Qm, Nl};
      called(slot_emul_scramble_map_tb(sj.base(), 1, S, in.base(), reinterpret_cast<uint8_t *>(pts.base())), "scramble_map_tb");
      for (uint32_t k = 0; k < S && ok; k++) {
        uint32_t x = 0;
        for (uint32_t b = 0; b < Qm; b++)
          x |= ((in[k * Qm + b] & 1u) ^ c_bit(k * Qm + b)) << b;
        ok = pts[(uint64_t)(k % Nl) * plane + k / Nl] == tab.pt[nr_qam_table_off(Qm) + x];
      }
    }
    if (!ok) {
      fprintf(stderr, "scrambling (%u bits): differs from the bit-by-bit form\n", size);
      n_bad++;
    }
  }
}

} // namespace

int main(int argc, char **argv)
{
  const std::string only = argc > 1 ? argv[1] : "";
  const struct {
    const char *name;
    void (*run)();
  } families[] = {{"compensation", run_compensation}, {"mmse", run_mmse}, {"levels", run_levels}, {"chest", run_chest},
                  {"mapping", run_mapping},           {"qam", run_qam},   {"scrambling", run_scrambling}};
  for (const auto &f : families)
    if (only.empty() || only == f.name)
      f.run();
  printf("%ld calls, %ld mismatches or refusals\n", n_calls, n_bad);
  return n_bad == 0 && n_calls > 0 ? 0 : 1;
}
