/*
 * rx_delay_plan.h -- what the PUSCH delay search call derives from its descriptors before anything is enqueued: the checks, the
 * twiddle table of an fft_size, the job list, the workgroup table of tb_rx_delay.hip sorted by fft_size with its jumped Gold
 * registers, and the serial form of the search on the CPU.  Plain arithmetic (slot_plan.h): rx_delay_api.inc.cpp runs it in front
 * of its DEVICE and HOST scopes, and the CPU emulation of the kernel (tests/emul/) runs the same code.
 */
#ifndef RX_DELAY_PLAN_H
#define RX_DELAY_PLAN_H
#include <utility>
#include "rx_chest_plan.h"
#include "tb_rx_delay.h"
#include "job_layout.h"

namespace {

/* tw[t] = exp(2 pi i t / N), t < N, in double and rounded once; then NR_DLY_ONE_WORDS c16 of which six are (256, 0).  As words */
void dly_fill_twiddles(uint32_t N, std::vector<uint32_t> &t)
{
  t.assign(2u * (size_t)N + NR_DLY_ONE_WORDS, 0u);
  for (uint32_t k = 0; k < N; k++) {
    const double a = 2.0 * M_PI * (double)k / (double)N;
    const float c = (float)cos(a), s = (float)sin(a);
    memcpy(&t[2u * (size_t)k], &c, 4);
    memcpy(&t[2u * (size_t)k + 1u], &s, 4);
  }
  nr_che_c one;
  one.r = 256;
  one.i = 0;
  for (uint32_t k = 0; k < 6u; k++)
    t[2u * (size_t)N + k] = nr_che_pack(one);
}

int dly_check_flags(uint32_t flags)
{
  if (flags != NR_DLY_RUNNING_MAX && flags != NR_DLY_PER_ANTENNA)
    return set_error("est_delay: flags must be NRLDPC_HIP_DELAY_RUNNING_MAX or NRLDPC_HIP_DELAY_PER_ANTENNA");
  return 0;
}

struct DelayPlan {
  std::vector<rx_delay_job> jobs;
  std::vector<rx_delay_wg> wgs;                      /* sorted by fft_size */
  std::vector<std::pair<uint32_t, uint32_t>> launch; /* (fft_size, workgroups) in the table's order */
  uint64_t rx_lo = UINT64_MAX, rx_hi = 0;
};

int dly_plan(const nrLDPC_hip_chest_seg_t *seg, uint32_t n_seg, uint32_t n_rx, uint64_t rx_stride, DelayPlan &p)
{
  static const uint32_t sizes[] = {128, 256, 512, 1024, 1536, 2048, 4096, 6144, 8192};
  std::vector<Range64> out;
  p.jobs.resize(n_seg);
  for (uint32_t i = 0; i < n_seg; i++) {
    const nrLDPC_hip_chest_seg_t &g = seg[i];
    if (che_check_seg("est_delay", g) != 0)
      return -1;
    out.push_back(Range64{g.delay_off, (uint64_t)g.delay_off + n_rx});
    rx_delay_job &j = p.jobs[i];
    memset(&j, 0, sizeof j);
    j.rx_off = g.rx_off;
    j.fft_size = g.fft_size;
    j.start_re = g.start_re;
    j.rb_size = g.rb_size;
    j.dmrs_offset = g.dmrs_offset;
    j.port = g.port;
    j.mode = g.mode;
    j.delay_off = g.delay_off;
    if (nr_che_is_avg(g.mode))
      continue; /* takes no delay: nothing is read */
    uint32_t lo, hi;
    che_rx_range(g, lo, hi);
    p.rx_lo = std::min(p.rx_lo, g.rx_off + lo);
    p.rx_hi = std::max(p.rx_hi, g.rx_off + hi + (uint64_t)(n_rx - 1) * rx_stride);
  }
  uint64_t lo, hi;
  if (ranges_overlap(out, lo, hi))
    return set_error("est_delay: the delay ranges of two descriptors overlap");
  for (uint32_t N : sizes) {
    uint32_t n_wg = 0;
    for (uint32_t i = 0; i < n_seg; i++) {
      if (seg[i].fft_size != N || nr_che_is_avg(seg[i].mode))
        continue;
      rx_delay_wg w{};
      w.job = i;
      w.w0 = (2u * seg[i].dmrs_offset) >> 5;
      nr_gold_jump(&che_gold_tables(), seg[i].c_init, w.w0, &w.x1, &w.x2);
      p.jobs[i].first_res = (uint32_t)p.wgs.size();
      for (uint32_t a = 0; a < n_rx; a++) {
        w.ant = a;
        p.wgs.push_back(w);
        n_wg++;
      }
    }
    if (n_wg)
      p.launch.push_back(std::make_pair(N, n_wg));
  }
  return 0;
}

/* the call's tables in one upload, and behind them the search results (library-owned, they travel as zeros with the tables as
 * the measuring estimation's accumulators do) */
struct DelayLayout {
  JobLayout lay;
  size_t wg = 0, job = 0, res = 0;
  explicit DelayLayout(const DelayPlan &p)
  {
    wg = lay.add(p.wgs);
    job = lay.add(p.jobs);
    res = lay.zeros(p.wgs.size() * sizeof(rx_delay_res));
  }
  template <typename T> T *at(uint8_t *base, size_t off) const { return reinterpret_cast<T *>(base + off); }
};

/* the launches over the tables' device copy: one search per fft_size, then the combination */
int dly_launch(const DelayPlan &p, const DelayLayout &l, uint8_t *base, const uint32_t *rx, uint64_t rx_stride, uint32_t n_rx, uint32_t flags,
               int32_t *est_delay, float *peak, hipStream_t s)
{
  const rx_delay_wg *wgs = l.at<rx_delay_wg>(base, l.wg);
  const rx_delay_job *jobs = l.at<rx_delay_job>(base, l.job);
  rx_delay_res *res = l.at<rx_delay_res>(base, l.res);
  uint32_t first = 0;
  for (const std::pair<uint32_t, uint32_t> &q : p.launch) {
    if (nr_launch_rx_delay_search(q.first, wgs + first, q.second, jobs, rx, rx_stride, res + first, s) != hipSuccess)
      return set_error("est_delay: the search launch failed");
    first += q.second;
  }
  if (nr_launch_rx_delay_combine(jobs, (uint32_t)p.jobs.size(), n_rx, flags, res, est_delay, peak, s) != hipSuccess)
    return set_error("est_delay: the combining launch failed");
  return 0;
}

/* one descriptor's antenna on the CPU, serially: rx = the symbol's subcarrier 0; tw = dly_fill_twiddles(fft_size) */
void dly_host_one(const nrLDPC_hip_chest_seg_t &g, const uint32_t *rx, const std::vector<uint32_t> &gold, uint32_t w0, const uint32_t *tw_words,
                  std::vector<nr_dly_c> &buf, float &best, uint32_t &best_n)
{
  const uint32_t N = g.fft_size, M = nr_dly_pow2(N), lm = nr_dly_log2(M);
  const nr_dly_c *tw = reinterpret_cast<const nr_dly_c *>(tw_words);
  const uint32_t *one = tw_words + 2u * (size_t)N;
  nr_dly_c z;
  z.r = z.i = 0.0f;
  buf.assign(N, z);
  for (uint32_t u = 0; u < 3u * g.rb_size; u++) {
    uint32_t o[4];
    nr_dly_ls4(g.mode, rx, N, g.start_re, g.port, g.dmrs_offset, dmrs_bits(gold, w0, g.dmrs_offset + nr_dly_first_pilot(g.mode, u)), one, u, o);
    for (uint32_t k = 0; k < 4u; k++)
      buf[4u * u + k] = nr_dly_from_c16(o[k]);
  }
  if (nr_dly_radix3(N))
    for (uint32_t k = 0; k < M; k++)
      nr_dly_r3(buf.data(), tw, M, k);
  for (uint32_t ll = lm; ll >= 1u; ll--)
    for (uint32_t b = 0; b < N / 2u; b++)
      nr_dly_r2(buf.data(), tw, N, ll, b);
  best = 0.0f;
  best_n = 0;
  for (uint32_t p = 0; p < N; p++) {
    const float v = nr_dly_power(buf[p]);
    const uint32_t n = nr_dly_index(N, lm, p);
    if (nr_dly_better(v, n, best, best_n)) {
      best = v;
      best_n = n;
    }
  }
}

/* one descriptor over its antennas on the CPU: est_delay / peak at delay_off + a */
int dly_host_seg(const nrLDPC_hip_chest_seg_t &g, const uint32_t *rx, uint64_t rx_stride, uint32_t n_rx, uint32_t flags, const uint32_t *tw_words,
                 int32_t *est_delay, float *peak)
{
  std::vector<uint32_t> gold;
  std::vector<nr_dly_c> buf;
  uint32_t w0 = 0;
  if (!nr_che_is_avg(g.mode) && !dmrs_gold_words(g.c_init, g.dmrs_offset, nr_che_pilots_per_rb(g.mode) * g.rb_size, gold, w0))
    return set_error("est_delay_host: the Gold sequence could not be generated");
  float best = 0.0f;
  uint32_t pos = 0;
  for (uint32_t a = 0; a < n_rx; a++) {
    if (!nr_che_is_avg(g.mode)) {
      float v;
      uint32_t n;
      dly_host_one(g, rx + g.rx_off + (uint64_t)a * rx_stride, gold, w0, tw_words, buf, v, n);
      if (flags == NR_DLY_PER_ANTENNA || v > best) {
        best = v;
        pos = n;
      }
    }
    est_delay[(size_t)g.delay_off + a] = nr_dly_fold(g.fft_size, pos);
    if (peak)
      peak[(size_t)g.delay_off + a] = best;
  }
  return 0;
}

} // namespace
#endif
