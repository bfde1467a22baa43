/*
 * rx_plan.h -- what the UL receive front's calls derive from their descriptors before anything is enqueued: the descriptor
 * checks, the job lists, the c16 ranges of the caller's arrays they reach, and the workgroup tables of tb_rx_front.hip,
 * tb_rx_mmse.hip and tb_rx_ml.hip.  Plain arithmetic (slot_plan.h): rx_front_api.inc.cpp, rx_grid_api.inc.cpp, rx_mmse_api.inc.cpp
 * and rx_ml_api.inc.cpp run it in front of their DEVICE and HOST scopes, and the CPU emulation of the kernels (tests/emul/) runs the same code.
 * There is one grid plan: rxg_job turns a grid segment into its job and input reach for the single-layer and the two-layer
 * receivers alike, and the two two-layer receivers share one plan (rx2_plan) that takes what differs between them as data.
 */
#ifndef RX_PLAN_H
#define RX_PLAN_H
#include "slot_plan.h"
#include "nr_rx_front.h"
#include "nr_rx_grid.h"
#include "nr_rx_mmse.h"
#include "tb_rx_front.h"

namespace {

/* ---- the extracted form (rx_front_api.inc.cpp) ---- */
/* what a call's descriptors come to: the job lists and the c16 ranges of the caller's arrays they reach */
struct RxFrontPlan {
  std::vector<rx_front_seg_job> jobs;
  std::vector<rx_front_wg> wgs;
  std::vector<rx_front_lvl_job> lvl;
  uint64_t rx_lo = UINT64_MAX, rx_hi = 0, ch_lo = UINT64_MAX, ch_hi = 0, out_lo = UINT64_MAX, out_hi = 0;
  uint32_t n_shift = 0; /* 1 + the largest tb */
};

int rxf_check_common(const char *who, uint32_t n_rx, int32_t mem)
{
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return set_error((std::string(who) + ": n_rx must be 1..8").c_str());
  return check_mem(who, mem);
}

/* the segments of a compensation call, without the workgroup table (that needs the address the records are written at) */
int rxf_plan_compensation(const nrLDPC_hip_rx_seg_t *seg, uint32_t n_seg, uint32_t n_rx, uint64_t ant_stride, RxFrontPlan &p)
{
  std::vector<Range64> out;
  p.jobs.reserve(n_seg);
  for (uint32_t i = 0; i < n_seg; i++) {
    const nrLDPC_hip_rx_seg_t &g = seg[i];
    if (qam_check_qm(g.Qm) != 0)
      return set_error("channel_compensation: Qm must be 2, 4, 6 or 8");
    if (g.rec_off & 1u)
      return set_error("channel_compensation: rec_off must be even");
    if ((uint64_t)g.sym_off + g.nb_re > g.plane)
      return set_error("channel_compensation: sym_off + nb_re above plane");
    if ((uint64_t)g.nb_re * g.Qm > NR_SCR_MAX_BITS)
      return set_error("channel_compensation: nb_re * Qm above 2^21");
    p.n_shift = std::max(p.n_shift, g.tb + 1u);
    if (g.nb_re == 0)
      continue;
    const uint64_t first = g.rec_off / 2u + g.sym_off, reach = (uint64_t)(n_rx - 1) * ant_stride + g.nb_re;
    for (uint32_t k = 0; k < g.Qm / 2u; k++)
      out.push_back(Range64{first + (uint64_t)k * g.plane, first + (uint64_t)k * g.plane + g.nb_re});
    p.rx_lo = std::min(p.rx_lo, g.rx_off);
    p.rx_hi = std::max(p.rx_hi, g.rx_off + reach);
    p.ch_lo = std::min(p.ch_lo, g.ch_off);
    p.ch_hi = std::max(p.ch_hi, g.ch_off + reach);
    rx_front_seg_job j{};
    j.rx_off = g.rx_off;
    j.ch_off = g.ch_off;
    j.out_off = first;
    j.plane = g.plane;
    j.nb_re = g.nb_re;
    j.tb = g.tb;
    j.Qm = g.Qm;
    p.jobs.push_back(j);
  }
  if (ranges_overlap(out, p.out_lo, p.out_hi))
    return set_error("channel_compensation: the output ranges of two segments overlap");
  return 0;
}

/* offsets relative to the copies' starts (staged) and the workgroup table for records written at word address rec_word */
void rxf_place(RxFrontPlan &p, uint64_t rx_bias, uint64_t ch_bias, uint64_t out_bias, uint64_t rec_word)
{
  for (size_t i = 0; i < p.jobs.size(); i++) {
    rx_front_seg_job &j = p.jobs[i];
    j.rx_off -= rx_bias;
    j.ch_off -= ch_bias;
    j.out_off -= out_bias;
    j.phase = (uint32_t)((rec_word + j.out_off) & 3u);
    const uint32_t groups = (j.nb_re + j.phase + NR_RXF_GROUP - 1u) / NR_RXF_GROUP;
    for (uint32_t q = 0; q * NR_RXF_THREADS < groups; q++)
      p.wgs.push_back(rx_front_wg{(uint32_t)i, q});
  }
}

int rxf_plan_level(const nrLDPC_hip_rx_seg_t *fs, uint32_t n_tb, uint32_t n_rx, uint64_t ant_stride, RxFrontPlan &p)
{
  std::vector<uint8_t> seen(n_tb, 0);
  p.lvl.resize(n_tb);
  for (uint32_t i = 0; i < n_tb; i++) {
    if (fs[i].tb >= n_tb || seen[fs[i].tb])
      return set_error("channel_level: every tb below n_tb must be named once");
    seen[fs[i].tb] = 1;
    if (fs[i].nb_re == 0)
      return set_error("channel_level: the measurement symbol has no REs");
    if ((uint64_t)fs[i].nb_re * 2u > NR_SCR_MAX_BITS)
      return set_error("channel_level: nb_re above 2^20");
    p.lvl[i] = rx_front_lvl_job{fs[i].ch_off, fs[i].nb_re, fs[i].tb};
    p.ch_lo = std::min(p.ch_lo, fs[i].ch_off);
    p.ch_hi = std::max(p.ch_hi, fs[i].ch_off + (uint64_t)(n_rx - 1) * ant_stride + fs[i].nb_re);
  }
  return 0;
}

/* a level call's blocks, then their zeroed state (maxima, counters: two words a block) */
template <typename Job> Table2<Job, int32_t> rxf_level_tables(const std::vector<Job> &lvl)
{
  return Table2<Job, int32_t>{lvl.data(), lvl.size(), nullptr, 2u * lvl.size()};
}

/* ---- the grid source (rx_grid_api.inc.cpp) ---- */
int rxg_check_seg(const char *who, uint32_t pattern, uint32_t fft_size, uint32_t start_re, uint32_t nb_re)
{
  if (pattern >= NR_RXG_PATTERNS)
    return set_error((std::string(who) + ": pattern must be FULL, DMRS1 or DMRS2").c_str());
  if (fft_size > NR_SCR_MAX_BITS)
    return set_error((std::string(who) + ": fft_size above 2^21").c_str());
  if (fft_size == 0 || start_re >= fft_size)
    return set_error((std::string(who) + ": start_re must be below fft_size").c_str());
  /* the same as p(nb_re - 1) >= fft_size */
  if (nb_re > nr_rxg_count(pattern, fft_size))
    return set_error((std::string(who) + ": nb_re above the pattern's count within fft_size subcarriers (p(nb_re - 1) >= fft_size)").c_str());
  return 0;
}

/* the c16 range [lo, hi) of one antenna's grid that a segment reaches: one piece, or the whole OFDM symbol when it wraps */
void rxg_rx_range(const nrLDPC_hip_rx_grid_seg_t &g, uint64_t &lo, uint64_t &hi)
{
  const uint32_t first = g.start_re + nr_rxg_p(g.pattern, 0), last = g.start_re + nr_rxg_p(g.pattern, g.nb_re - 1u);
  if (last < g.fft_size) {
    lo = g.rx_off + first;
    hi = g.rx_off + last + 1u;
  } else if (first >= g.fft_size) {
    lo = g.rx_off + first - g.fft_size;
    hi = g.rx_off + last - g.fft_size + 1u;
  } else {
    lo = g.rx_off;
    hi = g.rx_off + g.fft_size;
  }
}

/* a grid segment with REs: its job (the grid fields; the segment's own part `s` is the caller's) and, into p, the c16 ranges of the
 * caller's arrays it reaches -- n_rx antennas of the grid, n_ch arrays of the estimates (the antennas', or the 2 n_rx (layer,
 * antenna) pairs') from the estimate of its first PUSCH subcarrier to that of its last */
rx_front_grid_job rxg_job(const nrLDPC_hip_rx_grid_seg_t &g, uint32_t n_rx, uint32_t n_ch, uint64_t rx_stride, uint64_t ch_stride, RxFrontPlan &p)
{
  uint64_t lo, hi;
  rxg_rx_range(g, lo, hi);
  p.rx_lo = std::min(p.rx_lo, lo);
  p.rx_hi = std::max(p.rx_hi, hi + (uint64_t)(n_rx - 1) * rx_stride);
  p.ch_lo = std::min(p.ch_lo, g.ch_off + nr_rxg_p(g.pattern, 0));
  p.ch_hi = std::max(p.ch_hi, g.ch_off + nr_rxg_p(g.pattern, g.nb_re - 1u) + 1u + (uint64_t)(n_ch - 1) * ch_stride);
  rx_front_grid_job j{};
  j.pattern = g.pattern;
  j.fft_size = g.fft_size;
  j.start_re = g.start_re;
  return j;
}

/* the grid checks, then the plan of the extracted form (its checks, output ranges and jobs) with the input ranges of the grid */
int rxg_plan_compensation(const nrLDPC_hip_rx_grid_seg_t *seg, uint32_t n_seg, uint32_t n_rx, uint64_t rx_stride, uint64_t ch_stride, RxFrontPlan &p,
                          std::vector<rx_front_grid_job> &gj)
{
  std::vector<nrLDPC_hip_rx_seg_t> plain(n_seg);
  for (uint32_t i = 0; i < n_seg; i++) {
    const nrLDPC_hip_rx_grid_seg_t &g = seg[i];
    if (rxg_check_seg("channel_compensation_grid", g.pattern, g.fft_size, g.start_re, g.nb_re) != 0)
      return -1;
    nrLDPC_hip_rx_seg_t &q = plain[i];
    memset(&q, 0, sizeof q);
    q.tb = g.tb;
    q.Qm = g.Qm;
    q.nb_re = g.nb_re;
    q.plane = g.plane;
    q.sym_off = g.sym_off;
    q.rx_off = g.rx_off;
    q.ch_off = g.ch_off;
    q.rec_off = g.rec_off;
  }
  if (rxf_plan_compensation(plain.data(), n_seg, 1, 0, p) != 0)
    return -1;
  p.rx_lo = p.ch_lo = UINT64_MAX;
  p.rx_hi = p.ch_hi = 0;
  gj.reserve(p.jobs.size());
  for (uint32_t i = 0; i < n_seg; i++)
    if (seg[i].nb_re != 0)
      gj.push_back(rxg_job(seg[i], n_rx, n_rx, rx_stride, ch_stride, p));
  return 0;
}

/* rxf_place, then the placed segments into the grid jobs (p.jobs and gj run in step: the segments with REs).  A staged copy
 * starts at the first c16 that is reached, which lies behind subcarrier 0: rx_off / ch_off minus the bias may wrap below zero,
 * and the kernels' 64-bit address sums bring it back. */
void rxg_place(RxFrontPlan &p, std::vector<rx_front_grid_job> &gj, uint64_t rx_bias, uint64_t ch_bias, uint64_t out_bias, uint64_t rec_word)
{
  rxf_place(p, rx_bias, ch_bias, out_bias, rec_word);
  for (size_t i = 0; i < gj.size(); i++)
    gj[i].s = p.jobs[i];
}

int rxg_plan_level(const nrLDPC_hip_rx_grid_seg_t *fs, uint32_t n_tb, uint32_t n_rx, uint64_t ch_stride, std::vector<rx_front_grid_lvl_job> &lvl,
                   uint64_t &ch_lo, uint64_t &ch_hi)
{
  std::vector<uint8_t> seen(n_tb, 0);
  lvl.resize(n_tb);
  ch_lo = UINT64_MAX;
  ch_hi = 0;
  for (uint32_t i = 0; i < n_tb; i++) {
    if (fs[i].tb >= n_tb || seen[fs[i].tb])
      return set_error("channel_level_grid: every tb below n_tb must be named once");
    seen[fs[i].tb] = 1;
    if (fs[i].nb_re == 0)
      return set_error("channel_level_grid: the measurement symbol has no REs");
    if ((uint64_t)fs[i].nb_re * 2u > NR_SCR_MAX_BITS)
      return set_error("channel_level_grid: nb_re above 2^20");
    /* the level reads the estimates alone, but the descriptor is the segment's: its grid fields are held to the same rules */
    if (rxg_check_seg("channel_level_grid", fs[i].pattern, fs[i].fft_size, fs[i].start_re, fs[i].nb_re) != 0)
      return -1;
    lvl[i] = rx_front_grid_lvl_job{fs[i].ch_off, fs[i].nb_re, fs[i].tb, fs[i].pattern, 0};
    ch_lo = std::min(ch_lo, fs[i].ch_off + nr_rxg_p(fs[i].pattern, 0));
    ch_hi = std::max(ch_hi, fs[i].ch_off + nr_rxg_p(fs[i].pattern, fs[i].nb_re - 1u) + 1u + (uint64_t)(n_rx - 1) * ch_stride);
  }
  return 0;
}

/* ---- the two-layer receivers (rx_mmse_api.inc.cpp, rx_ml_api.inc.cpp) ---- */
int rxm_check_common(const char *who, uint32_t n_rx, int32_t mem)
{
  if (n_rx != 2 && n_rx != 4)
    return set_error((std::string(who) + ": n_rx must be 2 or 4").c_str());
  return check_mem(who, mem);
}

/* what the plans of the two receivers differ in.  An RE's two layers come to Qm 32-bit words of output; run(Qm) of them lie side
 * by side, and the Qm / run(Qm) runs of an RE are `plane` words apart:
 *   MMSE  run = 2: the layers' entries of one plane; a segment fills codeword symbols 2 sym_off .. 2 (sym_off + nb_re) - 1 of each of
 *         the Qm / 2 planes of the symbol record;
 *   ML    run = Qm: Qm / 2 words of LLRs per layer, the two layers of an RE side by side; a segment fills words rec_off / 2 +
 *         Qm sym_off .. + Qm nb_re - 1 of the LLR array */
struct Rx2Layers {
  const char *who;
  uint8_t qm[2];         /* the modulation orders the receiver takes */
  const char *qm_needed; /* the refusal of any other, with the receiver that takes it */
  uint32_t (*run)(uint32_t Qm);
};
const Rx2Layers RX2_MMSE = {"mmse_2layers_grid", {6, 8}, "mmse_2layers_grid: Qm must be 6 or 8 (two layers of QPSK / 16QAM take the ML receiver, ml_2layers_grid)",
                            [](uint32_t) { return 2u; }};
const Rx2Layers RX2_ML = {"ml_2layers_grid", {2, 4}, "ml_2layers_grid: Qm must be 2 or 4 (two layers of 64QAM / 256QAM take the MMSE receiver, mmse_2layers_grid)",
                          [](uint32_t Qm) { return Qm; }};

/* the checks, the jobs (s.out_off = the word index of the segment's first output word), the output ranges and the input ranges:
 * n_rx antennas of the grid, 2 n_rx pairs of the estimates */
int rx2_plan(const Rx2Layers &rx, const nrLDPC_hip_rx_grid_seg_t *seg, uint32_t n_seg, uint32_t n_rx, uint64_t rx_stride, uint64_t ch_stride, RxFrontPlan &p,
             std::vector<rx_front_grid_job> &gj)
{
  const std::string who = std::string(rx.who) + ": ";
  std::vector<Range64> out;
  gj.reserve(n_seg);
  for (uint32_t i = 0; i < n_seg; i++) {
    const nrLDPC_hip_rx_grid_seg_t &g = seg[i];
    if (rxg_check_seg(rx.who, g.pattern, g.fft_size, g.start_re, g.nb_re) != 0)
      return -1;
    if (g.Qm != rx.qm[0] && g.Qm != rx.qm[1])
      return set_error(rx.qm_needed);
    if (g.rec_off & 1u)
      return set_error((who + "rec_off must be even").c_str());
    if (2u * ((uint64_t)g.sym_off + g.nb_re) > g.plane)
      return set_error((who + "2 (sym_off + nb_re) above plane").c_str());
    if (2u * (uint64_t)g.nb_re * g.Qm > NR_SCR_MAX_BITS)
      return set_error((who + "2 nb_re * Qm above 2^21").c_str());
    p.n_shift = std::max(p.n_shift, g.tb + 1u);
    if (g.nb_re == 0)
      continue;
    const uint64_t run = rx.run(g.Qm), first = g.rec_off / 2u + run * g.sym_off;
    for (uint32_t k = 0; k < g.Qm / run; k++)
      out.push_back(Range64{first + (uint64_t)k * g.plane, first + (uint64_t)k * g.plane + run * g.nb_re});
    rx_front_grid_job j = rxg_job(g, n_rx, 2u * n_rx, rx_stride, ch_stride, p);
    j.s.rx_off = g.rx_off;
    j.s.ch_off = g.ch_off;
    j.s.out_off = first;
    j.s.plane = g.plane;
    j.s.nb_re = g.nb_re;
    j.s.tb = g.tb;
    j.s.Qm = g.Qm;
    gj.push_back(j);
  }
  if (ranges_overlap(out, p.out_lo, p.out_hi))
    return set_error((who + "the output ranges of two segments overlap").c_str());
  return 0;
}

/* offsets relative to the copies' starts (staged; see rxg_place for the wrap below zero) and the workgroup table: a workgroup
 * takes NR_RXF_THREADS groups of NR_RXF_GROUP REs of a segment, counted from its RE 0 (no `phase`: the MMSE quad shares its shift, so the
 * groups cannot be moved against the segment) */
void rx2_place(RxFrontPlan &p, std::vector<rx_front_grid_job> &gj, uint64_t rx_bias, uint64_t ch_bias, uint64_t out_bias)
{
  for (size_t i = 0; i < gj.size(); i++) {
    rx_front_seg_job &j = gj[i].s;
    j.rx_off -= rx_bias;
    j.ch_off -= ch_bias;
    j.out_off -= out_bias;
    const uint32_t groups = (j.nb_re + NR_RXF_GROUP - 1u) / NR_RXF_GROUP;
    for (uint32_t q = 0; q * NR_RXF_THREADS < groups; q++)
      p.wgs.push_back(rx_front_wg{(uint32_t)i, q});
  }
}

/* what a receiver's entry point and the CPU emulation of its kernel call: the one plan with the receiver's constants, the one place */
int rxm_plan(const nrLDPC_hip_rx_grid_seg_t *seg, uint32_t n_seg, uint32_t n_rx, uint64_t rx_stride, uint64_t ch_stride, RxFrontPlan &p,
             std::vector<rx_front_grid_job> &gj)
{
  return rx2_plan(RX2_MMSE, seg, n_seg, n_rx, rx_stride, ch_stride, p, gj);
}
int rxl_plan(const nrLDPC_hip_rx_grid_seg_t *seg, uint32_t n_seg, uint32_t n_rx, uint64_t rx_stride, uint64_t ch_stride, RxFrontPlan &p,
             std::vector<rx_front_grid_job> &gj)
{
  return rx2_plan(RX2_ML, seg, n_seg, n_rx, rx_stride, ch_stride, p, gj);
}
void rxm_place(RxFrontPlan &p, std::vector<rx_front_grid_job> &gj, uint64_t rx_bias, uint64_t ch_bias, uint64_t out_bias) { rx2_place(p, gj, rx_bias, ch_bias, out_bias); }
void rxl_place(RxFrontPlan &p, std::vector<rx_front_grid_job> &gj, uint64_t rx_bias, uint64_t ch_bias, uint64_t out_bias) { rx2_place(p, gj, rx_bias, ch_bias, out_bias); }

} // namespace
#endif
