/*
 * rx_ml_api.inc.cpp -- the two-layer PUSCH max-log ML receiver's entry points (QPSK, 16QAM): the channel level over the 2 n_rx
 * (layer, antenna) pairs, the receiver itself from the OFDM grid, and their CPU forms on extracted arrays (included into
 * ldpc_api.cpp behind rx_mmse_api.inc.cpp; uses the call scopes of slot_call.inc.cpp).  The arithmetic: nr_rx_ml.h; the kernels:
 * tb_rx_ml.hip.  Everything the kernels index with is checked before anything is enqueued: the checks, the plan and the
 * workgroup table are rx_plan.h's (rxl_*), which the CPU emulation of the kernels shares.
 */

namespace {

/* only the segments' words of the bounce that begins at word `bias` of the LLR array go to the caller's array */
void rxl_scatter(const std::vector<rx_front_grid_job> &gj, const uint8_t *bounce, uint64_t bias, int16_t *llr)
{
  for (const rx_front_grid_job &g : gj)
    memcpy(llr + 2 * (g.s.out_off + bias), bounce + 4u * g.s.out_off, (size_t)g.s.nb_re * g.s.Qm * 4u);
}

} // namespace

extern "C" {

int32_t nrLDPC_hip_ulsch_ml_2layers_host(const int16_t *rxFext, const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, uint32_t nb_re, uint8_t Qm,
                                         int32_t shift, int16_t *out)
{
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return set_error("ml_2layers_host: n_rx must be 1..8");
  if (Qm != 2 && Qm != 4)
    return set_error("ml_2layers_host: Qm must be 2 or 4");
  if (nb_re && (!rxFext || !chFext || !out))
    return set_error("null argument");
  const uint32_t s = nr_rxf_shift(shift);
  const int32_t amp[3] = {nr_rxf_amp(Qm, 0), 0, 0};
  for (size_t r = 0; r < nb_re; r++) {
    nr_rxl_re_t R = {};
    for (uint32_t a = 0; a < n_rx; a++)
      nr_rxl_mac(&R, rxm_c16_at(chFext, (size_t)a * ant_stride + r), rxm_c16_at(chFext, (size_t)(n_rx + a) * ant_stride + r),
                 rxm_c16_at(rxFext, (size_t)a * ant_stride + r), s, amp);
    for (uint32_t l = 0; l < 2; l++) {
      int32_t L[4];
      nr_rxl_llr(&R, Qm, l, L);
      for (uint32_t m = 0; m < Qm; m++)
        out[(size_t)Qm * (2u * r + l) + m] = (int16_t)L[m];
    }
  }
  return 0;
}

int32_t nrLDPC_hip_ulsch_level_ml_host(const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, uint32_t nb_re, int32_t max_ch, int32_t *avg,
                                       int32_t *log2_maxh)
{
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return set_error("level_ml_host: n_rx must be 1..8");
  if (nb_re == 0 || (uint64_t)nb_re * 2u > NR_SCR_MAX_BITS)
    return set_error("level_ml_host: nb_re must be 1..2^20");
  if (!chFext || !log2_maxh)
    return set_error("null argument");
  const uint32_t len = nr_rxf_level_len(nb_re), x = (uint32_t)nr_rxf_factor2(len), sce = nr_rxm_shift_ch_ext(max_ch);
  int32_t avgs = 0;
  for (uint32_t a = 0; a < 2u * n_rx; a++) {
    uint32_t sum = 0;
    for (uint32_t r = 0; r < nb_re; r++)
      sum += (uint32_t)nr_rxm_level_term(rxm_c16_at(chFext, (size_t)a * ant_stride + r), x, sce);
    const int32_t v = nr_rxf_level_avg((int32_t)sum, len);
    if (avg)
      avg[a] = v;
    avgs = std::max(avgs, v);
  }
  *log2_maxh = nr_rxl_log2_maxh(avgs);
  return 0;
}

int32_t nrLDPC_hip_ulsch_ml_2layers_grid(const int16_t *rxdataF, const int16_t *ul_ch, uint32_t n_rx, uint64_t rx_ant_stride, uint64_t ch_ant_stride,
                                         const nrLDPC_hip_rx_grid_seg_t *seg, uint32_t n_seg, const int32_t *shift, int16_t *llr, int32_t mem,
                                         void *stream)
{
  if (rxf_check_common("ml_2layers_grid", n_rx, mem) != 0)
    return -1;
  if (n_seg && (!rxdataF || !ul_ch || !seg || !shift || !llr))
    return set_error("null argument");
  RxFrontPlan p;
  std::vector<rx_front_grid_job> gj;
  if (rxl_plan(seg, n_seg, n_rx, rx_ant_stride, ch_ant_stride, p, gj) != 0)
    return -1;
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    if (n_seg == 0)
      return 0;
    DeviceCall dc;
    if (dc.open("ml_2layers_grid", {{llr, 4}, {rxdataF, 4}, {ul_ch, 4}, {shift, 4}}, DEV_NEEDS_ALIGNED, stream) != 0 ||
        dc.refuse_capture("ml_2layers_grid") != 0)
      return -1;
    if (gj.empty())
      return 0;
    rxl_place(p, gj, 0, 0, 0);
    const auto tab = table2(p.wgs, gj);
    uint8_t *base = dc.upload(tab);
    if (!base)
      return -1;
    HIP_TRY(nr_launch_rx_ml_grid(tab.first(base), (uint32_t)p.wgs.size(), tab.second(base), reinterpret_cast<const uint32_t *>(rxdataF),
                                 reinterpret_cast<const uint32_t *>(ul_ch), n_rx, rx_ant_stride, ch_ant_stride, shift,
                                 reinterpret_cast<uint32_t *>(llr), dc.s));
    return 0;
  }
  if (gj.empty())
    return 0;
  StagedCall st;
  if (st.open() != 0)
    return -1;
  /* the device works on copies of the ranges the segments reach */
  rxl_place(p, gj, p.rx_lo, p.ch_lo, p.out_lo);
  const auto tab = table2(p.wgs, gj);
  const size_t rx_n = (size_t)(p.rx_hi - p.rx_lo) * 4u, ch_n = (size_t)(p.ch_hi - p.ch_lo) * 4u, out_b = (size_t)(p.out_hi - p.out_lo) * 4u;
  const size_t tab_o = st.take(tab.bytes()), shift_o = st.take((size_t)p.n_shift * 4u), rx_o = st.take(rx_n), ch_o = st.take(ch_n);
  if (st.ensure(out_b) != 0)
    return -1;
  tab.write(st.h(tab_o));
  memcpy(st.h(shift_o), shift, (size_t)p.n_shift * 4u);
  memcpy(st.h(rx_o), rxdataF + 2 * p.rx_lo, rx_n);
  memcpy(st.h(ch_o), ul_ch + 2 * p.ch_lo, ch_n);
  const auto launch = [&] {
    HIP_TRY(nr_launch_rx_ml_grid(tab.first(st.d(tab_o)), (uint32_t)p.wgs.size(), tab.second(st.d(tab_o)), reinterpret_cast<const uint32_t *>(st.d(rx_o)),
                                 reinterpret_cast<const uint32_t *>(st.d(ch_o)), n_rx, rx_ant_stride, ch_ant_stride,
                                 reinterpret_cast<const int32_t *>(st.d(shift_o)), reinterpret_cast<uint32_t *>(st.d_out()), st.stream()));
    return 0;
  };
  if (st.run(st.top, launch, out_b) != 0)
    return -1;
  rxl_scatter(gj, st.h_out(), p.out_lo, llr);
  return 0;
}

int32_t nrLDPC_hip_ulsch_channel_level_grid_ml(const int16_t *ul_ch, uint32_t n_rx, uint64_t ch_ant_stride, const nrLDPC_hip_rx_grid_seg_t *first_sym,
                                               uint32_t n_tb, const int32_t *max_ch, int32_t *log2_maxh, int32_t mem, void *stream)
{
  if (rxf_check_common("channel_level_grid_ml", n_rx, mem) != 0)
    return -1;
  if (n_tb && (!ul_ch || !first_sym || !max_ch || !log2_maxh))
    return set_error("null argument");
  if (n_tb == 0)
    return 0;
  std::vector<rx_front_grid_lvl_job> lvl;
  uint64_t ch_lo, ch_hi;
  /* the estimates' range over 2 n_rx pairs */
  if (rxg_plan_level(first_sym, n_tb, 2u * n_rx, ch_ant_stride, lvl, ch_lo, ch_hi) != 0)
    return -1;
  const auto tab = rxf_level_tables(lvl);
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    DeviceCall dc;
    if (dc.open("channel_level_grid_ml", {{log2_maxh, 4}, {ul_ch, 4}, {max_ch, 4}}, DEV_NEEDS_ALIGNED, stream) != 0 ||
        dc.refuse_capture("channel_level_grid_ml") != 0)
      return -1;
    uint8_t *base = dc.upload(tab);
    if (!base)
      return -1;
    HIP_TRY(nr_launch_rx_level_grid_ml(tab.first(base), n_tb, reinterpret_cast<const uint32_t *>(ul_ch), n_rx, ch_ant_stride, max_ch, tab.second(base),
                                       log2_maxh, dc.s));
    return 0;
  }
  StagedCall st;
  if (st.open() != 0)
    return -1;
  for (rx_front_grid_lvl_job &j : lvl)
    j.ch_off -= ch_lo;
  const size_t ch_n = (size_t)(ch_hi - ch_lo) * 4u, out_b = (size_t)n_tb * 4u;
  const size_t tab_o = st.take(tab.bytes()), max_o = st.take((size_t)n_tb * 4u), ch_o = st.take(ch_n);
  if (st.ensure(out_b) != 0)
    return -1;
  tab.write(st.h(tab_o));
  memcpy(st.h(max_o), max_ch, (size_t)n_tb * 4u);
  memcpy(st.h(ch_o), ul_ch + 2 * ch_lo, ch_n);
  const auto launch = [&] {
    HIP_TRY(nr_launch_rx_level_grid_ml(tab.first(st.d(tab_o)), n_tb, reinterpret_cast<const uint32_t *>(st.d(ch_o)), n_rx, ch_ant_stride,
                                       reinterpret_cast<const int32_t *>(st.d(max_o)), tab.second(st.d(tab_o)),
                                       reinterpret_cast<int32_t *>(st.d_out()), st.stream()));
    return 0;
  };
  if (st.run(ch_o + ch_n, launch, out_b) != 0)
    return -1;
  memcpy(log2_maxh, st.h_out(), out_b);
  return 0;
}

} /* extern "C" */
