/*
 * rx_ml_api.inc.cpp -- the two-layer PUSCH max-log ML receiver's entry points (QPSK, 16QAM): the channel level over the 2 n_rx
 * (layer, antenna) pairs, the receiver itself from the OFDM grid, and their CPU forms on extracted arrays (included into
 * ldpc_api.cpp behind rx_mmse_api.inc.cpp; uses the two call bodies of rx_front_api.inc.cpp and rx2_level_host of
 * rx_mmse_api.inc.cpp).  The arithmetic: nr_rx_ml.h; the kernels: tb_rx_ml.hip.  Everything the kernels index with is checked
 * before anything is enqueued: the checks, the plan and the workgroup table are rx_plan.h's (rxl_plan), which the CPU
 * emulation of the kernels shares.
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
  return rx2_level_host("level_ml_host", chFext, n_rx, ant_stride, nb_re, max_ch, avg, log2_maxh, [](int32_t avgs) { return nr_rxl_log2_maxh(avgs); });
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
  const auto place = [&](uint64_t rx_bias, uint64_t ch_bias, uint64_t out_lo, uint64_t) {
    rxl_place(p, gj, rx_bias, ch_bias, out_lo);
    return out_lo;
  };
  const auto launch = [&](const rx_front_wg *wgs, uint32_t n_wg, const rx_front_grid_job *jobs, const uint32_t *rx, const uint32_t *ch,
                          const void *const *per_tb, uint32_t *out, hipStream_t s) {
    return nr_launch_rx_ml_grid(wgs, n_wg, jobs, rx, ch, n_rx, rx_ant_stride, ch_ant_stride, static_cast<const int32_t *>(per_tb[0]), out, s);
  };
  const auto scatter = [&](const uint8_t *bounce, uint64_t bias) { rxl_scatter(gj, bounce, bias, llr); };
  return rx_receiver_call("ml_2layers_grid", p, gj, n_seg, rxdataF, ul_ch, {shift}, llr, mem, stream, place, launch, scatter);
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
  const auto launch = [&](const rx_front_grid_lvl_job *jobs, const uint32_t *ch, const void *const *per_tb, int32_t *state, int32_t *out, hipStream_t s) {
    return nr_launch_rx_level_grid_ml(jobs, n_tb, ch, n_rx, ch_ant_stride, static_cast<const int32_t *>(per_tb[0]), state, out, s);
  };
  return rx_level_call("channel_level_grid_ml", lvl, ch_lo, ch_hi, ul_ch, {max_ch}, log2_maxh, mem, stream, launch);
}

} /* extern "C" */
