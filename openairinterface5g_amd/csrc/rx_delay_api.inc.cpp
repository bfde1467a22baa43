/*
 * rx_delay_api.inc.cpp -- the PUSCH delay search: the GPU call and its CPU check form (included into ldpc_api.cpp behind
 * rx_chest_api.inc.cpp, whose descriptor check it shares; uses rxf_check_common of rx_plan.h and the call scopes of
 * slot_call.inc.cpp).  The arithmetic: nr_delay.h; the kernels: tb_rx_delay.hip.  Everything the kernels index with is checked
 * before anything is enqueued: the checks, the twiddle table, the plan and the workgroup table are rx_delay_plan.h's, which the
 * CPU emulation of the kernels shares.
 */
#include "rx_delay_plan.h"

namespace {

/* the twiddles per fft_size, built once; their device copies per (HIP ordinal, fft_size), uploaded once */
std::mutex dly_mu;
std::map<uint32_t, std::vector<uint32_t>> dly_tab_host;
std::map<std::pair<int, uint32_t>, uint32_t *> dly_tab_dev;

const std::vector<uint32_t> &dly_table_locked(uint32_t N)
{
  std::vector<uint32_t> &t = dly_tab_host[N];
  if (t.empty())
    dly_fill_twiddles(N, t);
  return t;
}

/* on the current device (UseDevice); nullptr + error when the allocation or the copy fails */
const nr_dly_c *dly_table_device(int ordinal, uint32_t N)
{
  std::lock_guard<std::mutex> lk(dly_mu);
  uint32_t *&p = dly_tab_dev[std::make_pair(ordinal, N)];
  if (!p) {
    const std::vector<uint32_t> &t = dly_table_locked(N);
    uint32_t *d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d), t.size() * 4u);
    if (e == hipSuccess && (e = hipMemcpy(d, t.data(), t.size() * 4u, hipMemcpyHostToDevice)) != hipSuccess)
      (void)hipFree(d);
    if (e != hipSuccess) {
      set_error("est_delay: the twiddle table could not be uploaded", e);
      return nullptr;
    }
    p = d;
  }
  return reinterpret_cast<const nr_dly_c *>(p);
}

} // namespace

extern "C" {

int32_t nrLDPC_hip_pusch_est_delay(const int16_t *rxdataF, uint64_t rx_ant_stride, uint32_t n_rx, const nrLDPC_hip_chest_seg_t *seg, uint32_t n_seg,
                                   uint32_t flags, int32_t *est_delay, float *peak, int32_t mem, void *stream)
{
  if (rxf_check_common("est_delay", n_rx, mem) != 0)
    return -1;
  if (n_seg && (!rxdataF || !seg || !est_delay))
    return set_error("null argument");
  DelayPlan p;
  if (dly_check_flags(flags) != 0 || dly_plan(seg, n_seg, n_rx, rx_ant_stride, p) != 0)
    return -1;
  if (n_seg == 0)
    return 0;
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    DeviceCall dc;
    if (dc.open("est_delay", {{est_delay, 4}, {rxdataF, 4}, {peak, 4}}, DEV_NEEDS_ALIGNED, stream) != 0 || dc.refuse_capture("est_delay") != 0)
      return -1;
    for (uint32_t i = 0; i < n_seg; i++)
      if (!nr_che_is_avg(seg[i].mode) && !(p.jobs[i].tw = dly_table_device(dc.ord, seg[i].fft_size)))
        return -1;
    const DelayLayout dl(p);
    uint8_t *base = dc.upload(dl.lay);
    if (!base)
      return -1;
    return dly_launch(p, dl, base, reinterpret_cast<const uint32_t *>(rxdataF), rx_ant_stride, n_rx, flags, est_delay, peak, dc.s);
  }
  if (p.wgs.empty()) { /* averaging descriptors alone: 0 and 0, no GPU work */
    for (uint32_t i = 0; i < n_seg; i++)
      for (uint32_t a = 0; a < n_rx; a++) {
        est_delay[(size_t)seg[i].delay_off + a] = 0;
        if (peak)
          peak[(size_t)seg[i].delay_off + a] = 0.0f;
      }
    return 0;
  }
  StagedCall st;
  if (st.open() != 0)
    return -1;
  /* the device works on a copy of the c16 range of the grid the pilots lie in and writes the results of the call's (descriptor,
   * antenna) pairs one after another: the delays, then the peaks */
  for (uint32_t i = 0; i < n_seg; i++) {
    rx_delay_job &j = p.jobs[i];
    if (!nr_che_is_avg(seg[i].mode) && !(j.tw = dly_table_device(g.dev[0].id, seg[i].fft_size)))
      return -1;
    j.rx_off -= nr_che_is_avg(seg[i].mode) ? j.rx_off : p.rx_lo;
    j.delay_off = i * n_rx;
  }
  const DelayLayout dl(p);
  const size_t rx_n = (size_t)(p.rx_hi - p.rx_lo) * 4u, res_b = align_up((size_t)n_seg * n_rx * 4u, 16), out_b = 2u * res_b;
  const size_t tab_o = st.take(dl.lay.upload_bytes()), rx_o = st.take(rx_n);
  if (st.ensure(out_b) != 0)
    return -1;
  dl.lay.write(st.h(tab_o));
  memcpy(st.h(rx_o), rxdataF + 2 * p.rx_lo, rx_n);
  const auto launch = [&] {
    return dly_launch(p, dl, st.d(tab_o), reinterpret_cast<const uint32_t *>(st.d(rx_o)), rx_ant_stride, n_rx, flags,
                      reinterpret_cast<int32_t *>(st.d_out()), reinterpret_cast<float *>(st.d_out() + res_b), st.stream());
  };
  if (st.run(st.top, launch, out_b) != 0)
    return -1;
  for (uint32_t i = 0; i < n_seg; i++) {
    memcpy(est_delay + seg[i].delay_off, st.h_out() + (size_t)i * n_rx * 4u, (size_t)n_rx * 4u);
    if (peak)
      memcpy(peak + seg[i].delay_off, st.h_out() + res_b + (size_t)i * n_rx * 4u, (size_t)n_rx * 4u);
  }
  return 0;
}

int32_t nrLDPC_hip_pusch_est_delay_host(const int16_t *rxdataF, uint64_t rx_ant_stride, uint32_t n_rx, const nrLDPC_hip_chest_seg_t *seg, uint32_t flags,
                                        int32_t *est_delay, float *peak)
{
  if (!rxdataF || !seg || !est_delay)
    return set_error("null argument");
  if (rxf_check_common("est_delay_host", n_rx, NRLDPC_HIP_MEM_HOST) != 0 || dly_check_flags(flags) != 0 || che_check_seg("est_delay_host", *seg) != 0)
    return -1;
  std::vector<uint32_t> tw; /* a copy: the search runs outside the lock */
  if (!nr_che_is_avg(seg->mode)) {
    std::lock_guard<std::mutex> lk(dly_mu);
    tw = dly_table_locked(seg->fft_size);
  }
  return dly_host_seg(*seg, reinterpret_cast<const uint32_t *>(rxdataF), rx_ant_stride, n_rx, flags, tw.data(), est_delay, peak);
}

} /* extern "C" */
