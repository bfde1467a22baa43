/*
 * rx_chest_plan.h -- what the PUSCH channel estimation call derives from its descriptors before anything is enqueued: the
 * descriptor check, the delay table of an fft_size, the job list, the grid range the pilots lie in and the workgroup table of
 * tb_rx_chest.hip with its jumped Gold registers.  Plain arithmetic (slot_plan.h): rx_chest_api.inc.cpp runs it in front of its
 * DEVICE and HOST scopes, and the CPU emulation of the kernel (tests/emul/) runs the same code.
 */
#ifndef RX_CHEST_PLAN_H
#define RX_CHEST_PLAN_H
#include <cmath>
#include "slot_plan.h"
#include "nr_chest.h"
#include "nr_gold.h"
#include "tb_rx_chest.h"

namespace {

bool che_fft_ok(uint32_t N)
{
  /* freq2time (common/utils/nr/nr_common.c:934-961) */
  static const uint32_t sizes[] = {128, 256, 512, 1024, 1536, 2048, 4096, 6144, 8192};
  for (uint32_t s : sizes)
    if (s == N)
      return true;
  return false;
}

/* init_delay_table (nr_common.c:916-928), one row */
void che_delay_row(uint32_t N, int32_t d, uint32_t *out)
{
  for (uint32_t k = 0; k < N; k++) {
    const double a = 2.0 * M_PI * (double)k * (double)d / (double)N;
    nr_che_c c;
    c.r = (int16_t)round(256.0 * cos(a));
    c.i = (int16_t)round(256.0 * sin(a));
    out[k] = nr_che_pack(c);
  }
}

/* the table of an fft_size: NR_CHE_DELAY_ROWS rows of N c16 */
void che_fill_table(uint32_t N, std::vector<uint32_t> &t)
{
  t.resize((size_t)NR_CHE_DELAY_ROWS * N);
  for (int32_t d = -NR_CHE_MAX_DELAY; d <= NR_CHE_MAX_DELAY; d++)
    che_delay_row(N, d, t.data() + (size_t)nr_che_delay_idx(d) * N);
}

int che_check_seg(const char *who, const nrLDPC_hip_chest_seg_t &g)
{
  const std::string w(who);
  if (g.mode >= NR_CHE_MODES)
    return set_error((w + ": mode must be TYPE1_INTERP, TYPE2_INTERP, TYPE1_AVG or TYPE2_AVG").c_str());
  if (g.port >= nr_che_ports(g.mode))
    return set_error((w + ": port must be 0..7 for type 1 and 0..11 for type 2").c_str());
  if (!che_fft_ok(g.fft_size))
    return set_error((w + ": fft_size must be 128, 256, 512, 1024, 1536, 2048, 4096, 6144 or 8192").c_str());
  if (g.rb_size == 0)
    return set_error((w + ": rb_size is 0").c_str());
  if ((uint64_t)g.rb_size * 12u > g.fft_size)
    return set_error((w + ": the allocation is wider than fft_size").c_str());
  if (g.start_re >= g.fft_size)
    return set_error((w + ": start_re must be below fft_size").c_str());
  if (g.c_init >> 31)
    return set_error((w + ": c_init must be below 2^31").c_str());
  if (g.dmrs_offset > (1u << 20))
    return set_error((w + ": dmrs_offset above 2^20").c_str());
  if (nr_che_reaches_n(g.mode, g.port, g.fft_size, g.start_re, g.rb_size))
    return set_error((w + ": a pilot RE at subcarrier fft_size - 1 with nushift 1 would be read at index fft_size").c_str());
  return 0;
}

/* the c16 range [lo, hi) of the symbol that a descriptor's pilots lie in */
void che_rx_range(const nrLDPC_hip_chest_seg_t &g, uint32_t &lo, uint32_t &hi)
{
  lo = UINT32_MAX;
  hi = 0;
  const uint32_t nu = g.mode == NR_CHE_TYPE1_INTERP ? 0u : nr_che_nushift(g.port), delta = g.mode == NR_CHE_TYPE1_INTERP ? nr_che_delta1(g.port) : 0u;
  for (uint32_t t = 0; t < 12u * g.rb_size; t++) {
    const bool used = nr_che_is_type2(g.mode) ? t % 6u < 2u : !(t & 1u);
    if (!used)
      continue;
    const uint32_t at = nr_che_wrap(g.start_re, t + delta, g.fft_size) + nu;
    lo = std::min(lo, at);
    hi = std::max(hi, at + 1u);
  }
}

const nr_gold_tables_t &che_gold_tables()
{
  static const nr_gold_tables_t t = nr_gold_make_tables();
  return t;
}

struct ChestPlan {
  std::vector<rx_chest_job> jobs;
  std::vector<rx_chest_wg> wgs; /* sorted by mode */
  uint32_t n_wg[NR_CHE_MODES] = {0, 0, 0, 0};
  uint64_t rx_lo = UINT64_MAX, rx_hi = 0, out_lo = UINT64_MAX, out_hi = 0;
};

int che_plan(const nrLDPC_hip_chest_seg_t *seg, uint32_t n_seg, uint32_t n_rx, uint64_t rx_stride, uint64_t ch_stride, ChestPlan &p)
{
  std::vector<Range64> out;
  p.jobs.resize(n_seg);
  for (uint32_t i = 0; i < n_seg; i++) {
    const nrLDPC_hip_chest_seg_t &g = seg[i];
    if (che_check_seg("channel_estimation", g) != 0)
      return -1;
    uint32_t lo, hi;
    che_rx_range(g, lo, hi);
    p.rx_lo = std::min(p.rx_lo, g.rx_off + lo);
    p.rx_hi = std::max(p.rx_hi, g.rx_off + hi + (uint64_t)(n_rx - 1) * rx_stride);
    for (uint32_t a = 0; a < n_rx; a++)
      out.push_back(Range64{g.ch_off + (uint64_t)a * ch_stride, g.ch_off + (uint64_t)a * ch_stride + 12u * g.rb_size});
    rx_chest_job &j = p.jobs[i];
    memset(&j, 0, sizeof j);
    j.rx_off = g.rx_off;
    j.ch_off = g.ch_off;
    j.fft_size = g.fft_size;
    j.start_re = g.start_re;
    j.rb_size = g.rb_size;
    j.dmrs_offset = g.dmrs_offset;
    j.port = g.port;
    j.delay_off = g.delay_off;
  }
  if (ranges_overlap(out, p.out_lo, p.out_hi))
    return set_error("channel_estimation: the output ranges of two (descriptor, antenna) pairs overlap");
  /* the workgroup table, mode by mode; the Gold registers of a piece are the same for every antenna */
  for (uint32_t mode = 0; mode < NR_CHE_MODES; mode++)
    for (uint32_t i = 0; i < n_seg; i++) {
      if (seg[i].mode != mode)
        continue;
      const uint32_t units = nr_che_units(mode, seg[i].rb_size);
      for (uint32_t q = 0; q * NR_CHE_THREADS < units; q++) {
        rx_chest_wg w{};
        w.job = i;
        w.piece = q;
        w.w0 = (2u * (seg[i].dmrs_offset + nr_che_unit_first_pilot(mode, q * NR_CHE_THREADS))) >> 5;
        nr_gold_jump(&che_gold_tables(), seg[i].c_init, w.w0, &w.x1, &w.x2);
        for (uint32_t a = 0; a < n_rx; a++) {
          w.ant = a;
          p.wgs.push_back(w);
          p.n_wg[mode]++;
        }
      }
    }
  return 0;
}

} // namespace
#endif
