/*
 * rx_mmse_api.inc.cpp -- the two-layer PUSCH MMSE receiver's entry points: the channel level over the 2 n_rx (layer, antenna)
 * pairs, the receiver itself from the OFDM grid, and their CPU forms on extracted arrays (included into ldpc_api.cpp behind
 * rx_grid_api.inc.cpp; uses the two call bodies of rx_front_api.inc.cpp).  The arithmetic: nr_rx_mmse.h; the kernels: tb_rx_mmse.hip.
 * Everything the kernels index with is checked before anything is enqueued: the checks, the plan and the workgroup table are
 * rx_plan.h's (rxm_plan), which the CPU emulation of the kernels shares.  rx2_level_host, the CPU level of a two-layer
 * block, serves this file and rx_ml_api.inc.cpp.
 */

namespace {

/* only the segments' entries of the bounce that begins at c16 `bias` of the record array go to the caller's array */
void rxm_scatter(const std::vector<rx_front_grid_job> &gj, const uint8_t *bounce, uint64_t bias, int16_t *records)
{
  for (const rx_front_grid_job &g : gj)
    for (uint32_t k = 0; k < g.s.Qm / 2u; k++) {
      const uint64_t at = g.s.out_off + (uint64_t)k * g.s.plane;
      memcpy(records + 2 * (at + bias), bounce + 4u * at, (size_t)g.s.nb_re * 8u);
    }
}

uint32_t rxm_c16_at(const int16_t *p, size_t i) { return nr_rxf_c16(p[2 * i], p[2 * i + 1]); }

/* the channel level of one two-layer block's measurement symbol on the CPU, behind the caller's n_rx rule: the MMSE level's term
 * over the 2 n_rx pairs; final(avgs): the receiver's formula */
int rx2_level_host(const char *who, const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, uint32_t nb_re, int32_t max_ch, int32_t *avg,
                   int32_t *log2_maxh, int32_t (*final)(int32_t avgs))
{
  if (nb_re == 0 || (uint64_t)nb_re * 2u > NR_SCR_MAX_BITS)
    return set_error((std::string(who) + ": nb_re must be 1..2^20").c_str());
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
  *log2_maxh = final(avgs);
  return 0;
}

} // namespace

extern "C" {

int32_t nrLDPC_hip_ulsch_mmse_2layers_host(const int16_t *rxFext, const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, uint32_t nb_re,
                                           uint8_t Qm, int32_t shift, uint32_t nvar, int16_t *out)
{
  if (n_rx != 2 && n_rx != 4)
    return set_error("mmse_2layers_host: n_rx must be 2 or 4");
  if (Qm != 6 && Qm != 8)
    return set_error("mmse_2layers_host: Qm must be 6 or 8");
  if (nb_re && (!rxFext || !chFext || !out))
    return set_error("null argument");
  const uint32_t s = nr_rxf_shift(shift), np = Qm / 2u;
  for (uint32_t r0 = 0; r0 < nb_re; r0 += NR_RXM_QUAD) {
    nr_rxm_re_t R[NR_RXM_QUAD] = {};
    int32_t det[NR_RXM_QUAD];
    for (uint32_t u = 0; u < NR_RXM_QUAD; u++) {
      const size_t r = (size_t)r0 + u;
      if (r < nb_re) /* the lanes behind nb_re are the zero padding */
        for (uint32_t a = 0; a < n_rx; a++)
          nr_rxm_mac(&R[u], rxm_c16_at(chFext, (size_t)a * ant_stride + r), rxm_c16_at(chFext, (size_t)(n_rx + a) * ant_stride + r),
                     rxm_c16_at(rxFext, (size_t)a * ant_stride + r), s);
      det[u] = nr_rxm_det(&R[u], nvar);
    }
    const int32_t bm = nr_rxm_b_mag(det), bs = nr_rxm_b_sym(det);
    for (uint32_t u = 0; u < NR_RXM_QUAD && r0 + u < nb_re; u++) {
      const size_t r = (size_t)r0 + u;
      for (uint32_t l = 0; l < 2; l++)
        for (uint32_t k = 0; k < np; k++) {
          const uint32_t v = k == 0 ? (l == 0 ? nr_rxm_sym0(&R[u], bs) : nr_rxm_sym1(&R[u], bs)) : nr_rxm_mag(det[u], bm, nr_rxf_amp(Qm, k - 1u));
          int16_t *o = out + 2 * (((size_t)l * np + k) * nb_re + r);
          o[0] = (int16_t)nr_rxf_re(v);
          o[1] = (int16_t)nr_rxf_im(v);
        }
    }
  }
  return 0;
}

int32_t nrLDPC_hip_ulsch_level_mmse_host(const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, uint32_t nb_re, int32_t max_ch, int32_t *avg,
                                         int32_t *log2_maxh)
{
  if (n_rx != 2 && n_rx != 4)
    return set_error("level_mmse_host: n_rx must be 2 or 4");
  return rx2_level_host("level_mmse_host", chFext, n_rx, ant_stride, nb_re, max_ch, avg, log2_maxh, [](int32_t avgs) { return nr_rxm_log2_maxh(avgs); });
}

int32_t nrLDPC_hip_ulsch_mmse_2layers_grid(const int16_t *rxdataF, const int16_t *ul_ch, uint32_t n_rx, uint64_t rx_ant_stride, uint64_t ch_ant_stride,
                                           const nrLDPC_hip_rx_grid_seg_t *seg, uint32_t n_seg, const int32_t *shift, const uint32_t *nvar,
                                           int16_t *records, int32_t mem, void *stream)
{
  if (rxm_check_common("mmse_2layers_grid", n_rx, mem) != 0)
    return -1;
  if (n_seg && (!rxdataF || !ul_ch || !seg || !shift || !nvar || !records))
    return set_error("null argument");
  RxFrontPlan p;
  std::vector<rx_front_grid_job> gj;
  if (rxm_plan(seg, n_seg, n_rx, rx_ant_stride, ch_ant_stride, p, gj) != 0)
    return -1;
  const auto place = [&](uint64_t rx_bias, uint64_t ch_bias, uint64_t out_lo, uint64_t) {
    rxm_place(p, gj, rx_bias, ch_bias, out_lo);
    return out_lo;
  };
  const auto launch = [&](const rx_front_wg *wgs, uint32_t n_wg, const rx_front_grid_job *jobs, const uint32_t *rx, const uint32_t *ch,
                          const void *const *per_tb, uint32_t *rec, hipStream_t s) {
    return nr_launch_rx_mmse_grid(wgs, n_wg, jobs, rx, ch, n_rx, rx_ant_stride, ch_ant_stride, static_cast<const int32_t *>(per_tb[0]),
                                  static_cast<const uint32_t *>(per_tb[1]), rec, s);
  };
  const auto scatter = [&](const uint8_t *bounce, uint64_t bias) { rxm_scatter(gj, bounce, bias, records); };
  return rx_receiver_call("mmse_2layers_grid", p, gj, n_seg, rxdataF, ul_ch, {shift, nvar}, records, mem, stream, place, launch, scatter);
}

int32_t nrLDPC_hip_ulsch_channel_level_grid_mmse(const int16_t *ul_ch, uint32_t n_rx, uint64_t ch_ant_stride, const nrLDPC_hip_rx_grid_seg_t *first_sym,
                                                 uint32_t n_tb, const int32_t *max_ch, int32_t *log2_maxh, int32_t mem, void *stream)
{
  if (rxm_check_common("channel_level_grid_mmse", n_rx, mem) != 0)
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
    return nr_launch_rx_level_grid_mmse(jobs, n_tb, ch, n_rx, ch_ant_stride, static_cast<const int32_t *>(per_tb[0]), state, out, s);
  };
  return rx_level_call("channel_level_grid_mmse", lvl, ch_lo, ch_hi, ul_ch, {max_ch}, log2_maxh, mem, stream, launch);
}

} /* extern "C" */
