/*
 * rx_front_api.inc.cpp -- the UL receive front's entry points: channel level and channel compensation of the single-layer PUSCH
 * receiver (included into ldpc_api.cpp; uses the call scopes of slot_call.inc.cpp).  The arithmetic: nr_rx_front.h; the kernels:
 * tb_rx_front.hip.  Everything the kernels index with is checked before anything is enqueued: the checks, the plan and the
 * workgroup table are rx_plan.h's, which the CPU emulation of the kernels shares.
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
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    if (n_seg == 0)
      return 0;
    DeviceCall dc;
    if (dc.open("channel_compensation", {{records, 4}, {rxFext, 4}, {chFext, 4}, {shift, 4}}, DEV_NEEDS_ALIGNED, stream) != 0 ||
        dc.refuse_capture("channel_compensation") != 0)
      return -1;
    if (p.jobs.empty())
      return 0;
    rxf_place(p, 0, 0, 0, reinterpret_cast<uintptr_t>(records) >> 2);
    const auto tab = table2(p.wgs, p.jobs);
    uint8_t *base = dc.upload(tab);
    if (!base)
      return -1;
    HIP_TRY(nr_launch_rx_compensation(tab.first(base), (uint32_t)p.wgs.size(), tab.second(base), reinterpret_cast<const uint32_t *>(rxFext),
                                      reinterpret_cast<const uint32_t *>(chFext), n_rx, ant_stride, shift, reinterpret_cast<uint32_t *>(records), dc.s));
    return 0;
  }
  if (p.jobs.empty())
    return 0;
  StagedCall st;
  if (st.open() != 0)
    return -1;
  /* the device works on copies of the c16 ranges the segments reach; the output keeps the caller's alignment phase */
  const uint64_t out_pad = p.out_lo & 3u;
  rxf_place(p, p.rx_lo, p.ch_lo, p.out_lo - out_pad, 0);
  const auto tab = table2(p.wgs, p.jobs);
  const size_t rx_n = (size_t)(p.rx_hi - p.rx_lo) * 4u, ch_n = (size_t)(p.ch_hi - p.ch_lo) * 4u, out_b = (size_t)(p.out_hi - p.out_lo + out_pad) * 4u;
  const size_t tab_o = st.take(tab.bytes()), shift_o = st.take((size_t)p.n_shift * 4u), rx_o = st.take(rx_n), ch_o = st.take(ch_n);
  if (st.ensure(out_b) != 0)
    return -1;
  tab.write(st.h(tab_o));
  memcpy(st.h(shift_o), shift, (size_t)p.n_shift * 4u);
  memcpy(st.h(rx_o), rxFext + 2 * p.rx_lo, rx_n);
  memcpy(st.h(ch_o), chFext + 2 * p.ch_lo, ch_n);
  const auto launch = [&] {
    HIP_TRY(nr_launch_rx_compensation(tab.first(st.d(tab_o)), (uint32_t)p.wgs.size(), tab.second(st.d(tab_o)), reinterpret_cast<const uint32_t *>(st.d(rx_o)),
                                      reinterpret_cast<const uint32_t *>(st.d(ch_o)), n_rx, ant_stride, reinterpret_cast<const int32_t *>(st.d(shift_o)),
                                      reinterpret_cast<uint32_t *>(st.d_out()), st.stream()));
    return 0;
  };
  if (st.run(st.top, launch, out_b) != 0)
    return -1;
  rxf_scatter(p, st.h_out(), p.out_lo - out_pad, records);
  return 0;
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
  const auto tab = rxf_level_tables(p.lvl);
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    DeviceCall dc;
    if (dc.open("channel_level", {{log2_maxh, 4}, {chFext, 4}}, DEV_NEEDS_ALIGNED, stream) != 0 || dc.refuse_capture("channel_level") != 0)
      return -1;
    uint8_t *base = dc.upload(tab);
    if (!base)
      return -1;
    HIP_TRY(nr_launch_rx_level(tab.first(base), n_tb, reinterpret_cast<const uint32_t *>(chFext), n_rx, ant_stride, tab.second(base), log2_maxh, dc.s));
    return 0;
  }
  StagedCall st;
  if (st.open() != 0)
    return -1;
  for (rx_front_lvl_job &j : p.lvl)
    j.ch_off -= p.ch_lo;
  const size_t ch_n = (size_t)(p.ch_hi - p.ch_lo) * 4u, out_b = (size_t)n_tb * 4u;
  const size_t tab_o = st.take(tab.bytes()), ch_o = st.take(ch_n);
  if (st.ensure(out_b) != 0)
    return -1;
  tab.write(st.h(tab_o));
  memcpy(st.h(ch_o), chFext + 2 * p.ch_lo, ch_n);
  const auto launch = [&] {
    HIP_TRY(nr_launch_rx_level(tab.first(st.d(tab_o)), n_tb, reinterpret_cast<const uint32_t *>(st.d(ch_o)), n_rx, ant_stride, tab.second(st.d(tab_o)),
                               reinterpret_cast<int32_t *>(st.d_out()), st.stream()));
    return 0;
  };
  if (st.run(ch_o + ch_n, launch, out_b) != 0)
    return -1;
  memcpy(log2_maxh, st.h_out(), out_b);
  return 0;
}

} /* extern "C" */
