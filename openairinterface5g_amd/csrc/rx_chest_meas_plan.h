/*
 * rx_chest_meas_plan.h -- what the measuring channel estimation call and the time average call derive from their arguments before
 * anything is enqueued, next to rx_chest_plan.h's plan of the estimation itself: the blocks' descriptor lists with the host-known
 * nest_count, and the time average's checks, job list and workgroup table.  Plain arithmetic (slot_plan.h): rx_chest_api.inc.cpp
 * runs it in front of its DEVICE and HOST scopes, and the CPU emulation of the kernels (tests/emul/) runs the same code.
 */
#ifndef RX_CHEST_MEAS_PLAN_H
#define RX_CHEST_MEAS_PLAN_H
#include "rx_chest_plan.h"
#include "nr_rx_front.h"
#include "tb_rx_chest_meas.h"
#include "job_layout.h"

namespace {

struct ChestMeasPlan {
  std::vector<rx_chest_meas_job> mjobs; /* parallel to ChestPlan::jobs */
  std::vector<rx_chest_meas_tb> tbs;    /* one a block */
  std::vector<uint32_t> list;           /* the descriptors, block after block */
};

/* behind che_plan: seg_tb[i] < n_tb, nvar_div[tb] > 0 */
int che_meas_plan(const nrLDPC_hip_chest_seg_t *seg, uint32_t n_seg, uint32_t n_rx, const uint32_t *seg_tb, const uint32_t *nvar_div, uint32_t n_tb,
                  ChestMeasPlan &m)
{
  m.mjobs.resize(n_seg);
  m.tbs.assign(n_tb, rx_chest_meas_tb{0, 0, 0, 0});
  for (uint32_t t = 0; t < n_tb; t++)
    if ((m.tbs[t].div = nvar_div[t]) == 0)
      return set_error("channel_estimation_meas: nvar_div is 0 for a block");
  for (uint32_t i = 0; i < n_seg; i++) {
    if (seg_tb[i] >= n_tb)
      return set_error("channel_estimation_meas: seg_tb names a block >= n_tb");
    m.mjobs[i].tb = seg_tb[i];
    m.mjobs[i].nest_count = nr_che_nest_per_antenna(seg[i].mode, seg[i].rb_size) * n_rx; /* <= 12 * 682 * 8 */
    m.tbs[seg_tb[i]].count++;
  }
  for (uint32_t t = 1; t < n_tb; t++)
    m.tbs[t].first = m.tbs[t - 1].first + m.tbs[t - 1].count;
  m.list.resize(n_seg);
  std::vector<uint32_t> at(n_tb);
  for (uint32_t i = 0; i < n_seg; i++)
    m.list[m.tbs[seg_tb[i]].first + at[seg_tb[i]]++] = i;
  return 0;
}

/* where the device has the measuring call's tables, its accumulators and its two result arrays */
struct CheMeasDev {
  const rx_chest_meas_job *mjobs;
  const rx_chest_meas_tb *tbs;
  const uint32_t *list;
  int32_t *mx;
  uint64_t *noise;
  int32_t *max_ch;
  uint32_t *nvar;
};

/* the call's tables in one upload: the workgroup table, the jobs and, for the measuring call, its tables and the accumulators,
 * which travel as zeros */
struct CheLayout {
  JobLayout lay;
  size_t wg = 0, job = 0, mjob = 0, tb = 0, list = 0, mx = 0, noise = 0;
  CheLayout(const ChestPlan &p, const ChestMeasPlan *m)
  {
    wg = lay.add(p.wgs);
    job = lay.add(p.jobs);
    if (m) {
      mjob = lay.add(m->mjobs);
      tb = lay.add(m->tbs);
      list = lay.add(m->list);
      mx = lay.zeros(m->tbs.size() * sizeof(int32_t));
      noise = lay.zeros(m->mjobs.size() * sizeof(uint64_t));
    }
  }
  template <typename T> T *at(uint8_t *base, size_t off) const { return reinterpret_cast<T *>(base + off); }
  CheMeasDev meas(uint8_t *base, int32_t *max_ch, uint32_t *nvar) const
  {
    return CheMeasDev{at<rx_chest_meas_job>(base, mjob), at<rx_chest_meas_tb>(base, tb), at<uint32_t>(base, list), at<int32_t>(base, mx),
                      at<uint64_t>(base, noise), max_ch, nvar};
  }
};

struct ChestAvgPlan {
  std::vector<rx_chest_avg_job> jobs;
  std::vector<rx_chest_avg_wg> wgs;
  uint64_t lo = UINT64_MAX, hi = 0; /* the c16 span of everything read or written */
};

int che_avg_plan(const nrLDPC_hip_chest_avg_seg_t *seg, uint32_t n_seg, uint32_t n_plane, uint64_t ch_stride, ChestAvgPlan &p)
{
  if (n_plane < 1 || n_plane > 2u * NR_RXF_MAX_RX)
    return set_error("chest_time_avg: n_plane must be 1..16");
  std::vector<Range64> wr, rd;
  p.jobs.resize(n_seg);
  for (uint32_t i = 0; i < n_seg; i++) {
    const nrLDPC_hip_chest_avg_seg_t &g = seg[i];
    if (g.n_sym < 1 || g.n_sym > NR_CHE_AVG_MAX_SYM)
      return set_error("chest_time_avg: n_sym must be 1..4 (the reference asserts beyond four DMRS symbols)");
    if (g.rb_size == 0 || g.rb_size > (1u << 16))
      return set_error("chest_time_avg: rb_size must be 1..65536");
    rx_chest_avg_job &j = p.jobs[i];
    memset(&j, 0, sizeof j);
    j.n_sym = g.n_sym;
    j.rb_size = g.rb_size;
    for (uint32_t s = 0; s < g.n_sym; s++) {
      j.ch_off[s] = g.ch_off[s];
      if (g.n_sym == 1)
        break; /* nothing is read or written */
      for (uint32_t q = 0; q < n_plane; q++) {
        const uint64_t at = g.ch_off[s] + (uint64_t)q * ch_stride;
        (s == 0 ? wr : rd).push_back(Range64{at, at + 12u * g.rb_size});
        p.lo = std::min(p.lo, at);
        p.hi = std::max(p.hi, at + 12u * g.rb_size);
      }
    }
    if (g.n_sym == 1)
      continue;
    for (uint32_t q = 0; q < n_plane; q++)
      for (uint32_t piece = 0; piece * NR_CHE_THREADS < 3u * g.rb_size; piece++)
        p.wgs.push_back(rx_chest_avg_wg{i, q, piece, 0});
  }
  uint64_t lo, hi;
  if (ranges_overlap(wr, lo, hi))
    return set_error("chest_time_avg: the write ranges of two (descriptor, plane) pairs overlap");
  /* a later symbol's entries that another pair overwrites would be read before or after that, as the launch falls */
  for (const Range64 &r : rd) {
    auto it = std::upper_bound(wr.begin(), wr.end(), r.lo, [](uint64_t v, const Range64 &x) { return v < x.hi; });
    if (it != wr.end() && it->lo < r.hi)
      return set_error("chest_time_avg: a later DMRS symbol's range overlaps a range that is written");
  }
  return 0;
}

} // namespace
#endif
