/*
 * rx_front_api.inc.cpp -- the UL receive front's entry points: channel level and channel compensation of the single-layer PUSCH
 * receiver (included into ldpc_api.cpp; uses the call scopes of slot_call.inc.cpp).  The arithmetic: nr_rx_front.h; the kernels:
 * tb_rx_front.hip.  Everything the kernels index with is checked before anything is enqueued: the checks, the plan and the
 * workgroup table are rx_plan.h's, which the CPU emulation of the kernels shares.
 *
 * This file also holds what the receive front's eight calls share behind their checks and plans (rx_grid_api.inc.cpp,
 * rx_mmse_api.inc.cpp and rx_ml_api.inc.cpp follow it): rx_level_call and rx_receiver_call, the DEVICE and the HOST branch of a
 * level call and of a receiver call.  They need RxFrontPlan, which is why they are here and not in slot_call.inc.cpp.
 */
#include "rx_plan.h"

namespace {

/* only the segments' entries of the bounce that begins at c16 `bias` of the record array go to the caller's array */
void rxf_scatter(const RxFrontPlan &p, const uint8_t *bounce, uint64_t bias, int16_t *records)
{
  for (const rx_front_seg_job &j : p.jobs)
    for (uint32_t k = 0; k < j.Qm / 2u; k++) {
      const uint64_t at = j.out_off + (uint64_t)k * j.plane;
      memcpy(records + 2 * (at + bias), bounce + 4u * at, (size_t)j.nb_re * 4u);
    }
}

/* the single-layer kernels lay a segment's groups for 16-byte aligned stores (`phase`, tb_rx_front.hip): a staged output copy
 * begins at the 16-byte boundary at or below the first c16 that is written, so that it keeps the caller's alignment phase */
uint64_t rxf_aligned_bias(uint64_t out_lo) { return out_lo - (out_lo & 3u); }

/* ---- the two branches of a level call, behind its checks and its plan.  lvl: one job a block, ch_off still the
 * caller's; [ch_lo, ch_hi): the c16 range of the estimates they reach; per_tb: the int32-per-block arrays the kernel reads besides
 * (max_ch, or none).  launch(jobs, ch, per_tb, state, log2_maxh, stream) gets every array where the device reads it. ---- */
template <typename Job, typename Launch>
int rx_level_call(const char *who, std::vector<Job> &lvl, uint64_t ch_lo, uint64_t ch_hi, const int16_t *ch, const std::vector<const void *> &per_tb,
                  int32_t *log2_maxh, int32_t mem, void *stream, Launch launch)
{
  const size_t n_tb = lvl.size();
  const auto tab = rxf_level_tables(lvl);
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    std::vector<DevArray> arrays{{log2_maxh, 4}, {ch, 4}};
    for (const void *a : per_tb)
      arrays.push_back(DevArray{a, 4});
    DeviceCall dc;
    if (dc.open(who, arrays.data(), arrays.size(), DEV_NEEDS_ALIGNED, stream) != 0 || dc.refuse_capture(who) != 0)
      return -1;
    uint8_t *base = dc.upload(tab);
    if (!base)
      return -1;
    HIP_TRY(launch(tab.first(base), reinterpret_cast<const uint32_t *>(ch), per_tb.data(), tab.second(base), log2_maxh, dc.s));
    return 0;
  }
  StagedCall st;
  if (st.open() != 0)
    return -1;
  for (Job &j : lvl)
    j.ch_off -= ch_lo;
  const size_t ch_n = (size_t)(ch_hi - ch_lo) * 4u, out_b = n_tb * 4u;
  const size_t tab_o = st.take(tab.bytes());
  std::vector<size_t> per_tb_o;
  for (size_t i = 0; i < per_tb.size(); i++)
    per_tb_o.push_back(st.take(n_tb * 4u));
  const size_t ch_o = st.take(ch_n);
  if (st.ensure(out_b) != 0)
    return -1;
  tab.write(st.h(tab_o));
  std::vector<const void *> per_tb_d;
  for (size_t i = 0; i < per_tb.size(); i++) {
    memcpy(st.h(per_tb_o[i]), per_tb[i], n_tb * 4u);
    per_tb_d.push_back(st.d(per_tb_o[i]));
  }
  memcpy(st.h(ch_o), ch + 2 * ch_lo, ch_n);
  const auto staged = [&] {
    HIP_TRY(launch(tab.first(st.d(tab_o)), reinterpret_cast<const uint32_t *>(st.d(ch_o)), per_tb_d.data(), tab.second(st.d(tab_o)),
                   reinterpret_cast<int32_t *>(st.d_out()), st.stream()));
    return 0;
  };
  if (st.run(ch_o + ch_n, staged, out_b) != 0)
    return -1;
  memcpy(log2_maxh, st.h_out(), out_b);
  return 0;
}

/* ---- the two branches of a receiver call, behind its checks and its plan.  jobs: the job table, one entry per segment with REs
 * (p.jobs, or the grid jobs that run in step with it); per_tb: the int32-per-block arrays (shift, nvar), p.n_shift entries each.
 *   place(rx_bias, ch_bias, out_lo, rec_word)  makes the jobs' offsets relative to those biases, fills p.wgs, and returns the output
 *                                              bias it chose for a write set that begins at out_lo (rec_word: the word address of
 *                                              the output array, for the receiver whose layout depends on it);
 *   launch(wgs, n_wg, jobs, rx, ch, per_tb, out, stream)  gets every array where the device reads or writes it;
 *   scatter(bounce, bias)                      copies the segments' entries of a staged output that begins at `bias` to the caller.
 * DEVICE mem checks the arrays even when every segment is empty. ---- */
template <typename Job, typename Place, typename Launch, typename Scatter>
int rx_receiver_call(const char *who, RxFrontPlan &p, std::vector<Job> &jobs, uint32_t n_seg, const int16_t *rx, const int16_t *ch,
                     const std::vector<const void *> &per_tb, int16_t *out, int32_t mem, void *stream, Place place, Launch launch, Scatter scatter)
{
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    if (n_seg == 0)
      return 0;
    std::vector<DevArray> arrays{{out, 4}, {rx, 4}, {ch, 4}};
    for (const void *a : per_tb)
      arrays.push_back(DevArray{a, 4});
    DeviceCall dc;
    if (dc.open(who, arrays.data(), arrays.size(), DEV_NEEDS_ALIGNED, stream) != 0 || dc.refuse_capture(who) != 0)
      return -1;
    if (jobs.empty())
      return 0;
    place(0, 0, 0, reinterpret_cast<uintptr_t>(out) >> 2);
    const auto tab = table2(p.wgs, jobs);
    uint8_t *base = dc.upload(tab);
    if (!base)
      return -1;
    HIP_TRY(launch(tab.first(base), (uint32_t)p.wgs.size(), tab.second(base), reinterpret_cast<const uint32_t *>(rx), reinterpret_cast<const uint32_t *>(ch),
                   per_tb.data(), reinterpret_cast<uint32_t *>(out), dc.s));
    return 0;
  }
  if (jobs.empty())
    return 0;
  StagedCall st;
  if (st.open() != 0)
    return -1;
  /* the device works on copies of the ranges the segments reach */
  const uint64_t out_bias = place(p.rx_lo, p.ch_lo, p.out_lo, 0);
  const auto tab = table2(p.wgs, jobs);
  const size_t rx_n = (size_t)(p.rx_hi - p.rx_lo) * 4u, ch_n = (size_t)(p.ch_hi - p.ch_lo) * 4u, out_b = (size_t)(p.out_hi - out_bias) * 4u;
  const size_t tab_o = st.take(tab.bytes());
  std::vector<size_t> per_tb_o;
  for (size_t i = 0; i < per_tb.size(); i++)
    per_tb_o.push_back(st.take((size_t)p.n_shift * 4u));
  const size_t rx_o = st.take(rx_n), ch_o = st.take(ch_n);
  if (st.ensure(out_b) != 0)
    return -1;
  tab.write(st.h(tab_o));
  std::vector<const void *> per_tb_d;
  for (size_t i = 0; i < per_tb.size(); i++) {
    memcpy(st.h(per_tb_o[i]), per_tb[i], (size_t)p.n_shift * 4u);
    per_tb_d.push_back(st.d(per_tb_o[i]));
  }
  memcpy(st.h(rx_o), rx + 2 * p.rx_lo, rx_n);
  memcpy(st.h(ch_o), ch + 2 * p.ch_lo, ch_n);
  const auto staged = [&] {
    HIP_TRY(launch(tab.first(st.d(tab_o)), (uint32_t)p.wgs.size(), tab.second(st.d(tab_o)), reinterpret_cast<const uint32_t *>(st.d(rx_o)),
                   reinterpret_cast<const uint32_t *>(st.d(ch_o)), per_tb_d.data(), reinterpret_cast<uint32_t *>(st.d_out()), st.stream()));
    return 0;
  };
  if (st.run(st.top, staged, out_b) != 0)
    return -1;
  scatter(st.h_out(), out_bias);
  return 0;
}

} // namespace

extern "C" {

int32_t nrLDPC_hip_ulsch_compensate_host(const int16_t *rxFext, const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, uint32_t nb_re,
                                         uint8_t Qm, int32_t shift, int16_t *out)
{
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return set_error("compensate_host: n_rx must be 1..8");
  if (qam_check_qm(Qm) != 0)
    return -1;
  if (nb_re && (!rxFext || !chFext || !out))
    return set_error("null argument");
  const uint32_t s = nr_rxf_shift(shift), np = Qm / 2u;
  const int32_t amp[3] = {nr_rxf_amp(Qm, 0), nr_rxf_amp(Qm, 1), nr_rxf_amp(Qm, 2)};
  for (uint32_t r = 0; r < nb_re; r++) {
    nr_rxf_acc_t acc = {{0, 0, 0, 0}};
    for (uint32_t a = 0; a < n_rx; a++) {
      const int16_t *h = chFext + 2 * ((size_t)a * ant_stride + r), *y = rxFext + 2 * ((size_t)a * ant_stride + r);
      nr_rxf_mac(&acc, nr_rxf_c16(h[0], h[1]), nr_rxf_c16(y[0], y[1]), s, amp);
    }
    for (uint32_t k = 0; k < np; k++) {
      out[2 * ((size_t)k * nb_re + r)] = (int16_t)nr_rxf_re(acc.w[k]);
      out[2 * ((size_t)k * nb_re + r) + 1] = (int16_t)nr_rxf_im(acc.w[k]);
    }
  }
  return 0;
}

int32_t nrLDPC_hip_ulsch_level_host(const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, uint32_t nb_re, int32_t *avg, int32_t *log2_maxh)
{
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return set_error("level_host: n_rx must be 1..8");
  if (nb_re == 0 || (uint64_t)nb_re * 2u > NR_SCR_MAX_BITS)
    return set_error("level_host: nb_re must be 1..2^20");
  if (!chFext || !log2_maxh)
    return set_error("null argument");
  const uint32_t len = nr_rxf_level_len(nb_re), x = (uint32_t)nr_rxf_factor2(len);
  int32_t avgs = 0;
  for (uint32_t a = 0; a < n_rx; a++) {
    uint32_t sum = 0;
    for (uint32_t r = 0; r < nb_re; r++) {
      const int16_t *h = chFext + 2 * ((size_t)a * ant_stride + r);
      sum += (uint32_t)nr_rxf_level_term(nr_rxf_c16(h[0], h[1]), x);
    }
    const int32_t v = nr_rxf_level_avg((int32_t)sum, len);
    if (avg)
      avg[a] = v;
    avgs = std::max(avgs, v);
  }
  *log2_maxh = nr_rxf_log2_maxh(avgs, n_rx);
  return 0;
}

int32_t nrLDPC_hip_ulsch_channel_compensation(const int16_t *rxFext, const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride,
                                              const nrLDPC_hip_rx_seg_t *seg, uint32_t n_seg, const int32_t *shift, int16_t *records, int32_t mem,
                                              void *stream)
{
  if (rxf_check_common("channel_compensation", n_rx, mem) != 0)
    return -1;
  if (n_seg && (!rxFext || !chFext || !seg || !shift || !records))
    return set_error("null argument");
  RxFrontPlan p;
  if (rxf_plan_compensation(seg, n_seg, n_rx, ant_stride, p) != 0)
    return -1;
  const auto place = [&](uint64_t rx_bias, uint64_t ch_bias, uint64_t out_lo, uint64_t rec_word) {
    rxf_place(p, rx_bias, ch_bias, rxf_aligned_bias(out_lo), rec_word);
    return rxf_aligned_bias(out_lo);
  };
  const auto launch = [&](const rx_front_wg *wgs, uint32_t n_wg, const rx_front_seg_job *jobs, const uint32_t *rx, const uint32_t *ch, const void *const *per_tb,
                          uint32_t *rec, hipStream_t s) {
    return nr_launch_rx_compensation(wgs, n_wg, jobs, rx, ch, n_rx, ant_stride, static_cast<const int32_t *>(per_tb[0]), rec, s);
  };
  const auto scatter = [&](const uint8_t *bounce, uint64_t bias) { rxf_scatter(p, bounce, bias, records); };
  return rx_receiver_call("channel_compensation", p, p.jobs, n_seg, rxFext, chFext, {shift}, records, mem, stream, place, launch, scatter);
}

int32_t nrLDPC_hip_ulsch_channel_level(const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, const nrLDPC_hip_rx_seg_t *first_sym, uint32_t n_tb,
                                       int32_t *log2_maxh, int32_t mem, void *stream)
{
  if (rxf_check_common("channel_level", n_rx, mem) != 0)
    return -1;
  if (n_tb && (!chFext || !first_sym || !log2_maxh))
    return set_error("null argument");
  if (n_tb == 0)
    return 0;
  RxFrontPlan p;
  if (rxf_plan_level(first_sym, n_tb, n_rx, ant_stride, p) != 0)
    return -1;
  const auto launch = [&](const rx_front_lvl_job *jobs, const uint32_t *ch, const void *const *, int32_t *state, int32_t *out, hipStream_t s) {
    return nr_launch_rx_level(jobs, n_tb, ch, n_rx, ant_stride, state, out, s);
  };
  return rx_level_call("channel_level", p.lvl, p.ch_lo, p.ch_hi, chFext, {}, log2_maxh, mem, stream, launch);
}

} /* extern "C" */
