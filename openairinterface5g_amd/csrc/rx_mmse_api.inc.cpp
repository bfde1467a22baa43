/*
 * rx_mmse_api.inc.cpp -- the two-layer PUSCH MMSE receiver's entry points: the channel level over the 2 n_rx (layer, antenna)
 * pairs, the receiver itself from the OFDM grid, and their CPU forms on extracted arrays (included into ldpc_api.cpp behind
 * rx_grid_api.inc.cpp; uses the call scopes of slot_call.inc.cpp).  The arithmetic: nr_rx_mmse.h; the kernels: tb_rx_mmse.hip.
 * Everything the kernels index with is checked before anything is enqueued: the checks, the plan and the workgroup table are
 * rx_plan.h's (rxm_*), which the CPU emulation of the kernels shares.
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
  if (nb_re == 0 || (uint64_t)nb_re * 2u > NR_SCR_MAX_BITS)
    return set_error("level_mmse_host: nb_re must be 1..2^20");
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
  *log2_maxh = nr_rxm_log2_maxh(avgs);
  return 0;
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
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    if (n_seg == 0)
      return 0;
    DeviceCall dc;
    if (dc.open("mmse_2layers_grid", {{records, 4}, {rxdataF, 4}, {ul_ch, 4}, {shift, 4}, {nvar, 4}}, DEV_NEEDS_ALIGNED, stream) != 0 ||
        dc.refuse_capture("mmse_2layers_grid") != 0)
      return -1;
    if (gj.empty())
      return 0;
    rxm_place(p, gj, 0, 0, 0);
    const auto tab = table2(p.wgs, gj);
    uint8_t *base = dc.upload(tab);
    if (!base)
      return -1;
    HIP_TRY(nr_launch_rx_mmse_grid(tab.first(base), (uint32_t)p.wgs.size(), tab.second(base), reinterpret_cast<const uint32_t *>(rxdataF),
                                   reinterpret_cast<const uint32_t *>(ul_ch), n_rx, rx_ant_stride, ch_ant_stride, shift, nvar,
                                   reinterpret_cast<uint32_t *>(records), dc.s));
    return 0;
  }
  if (gj.empty())
    return 0;
  StagedCall st;
  if (st.open() != 0)
    return -1;
  /* the device works on copies of the c16 ranges the segments reach */
  rxm_place(p, gj, p.rx_lo, p.ch_lo, p.out_lo);
  const auto tab = table2(p.wgs, gj);
  const size_t rx_n = (size_t)(p.rx_hi - p.rx_lo) * 4u, ch_n = (size_t)(p.ch_hi - p.ch_lo) * 4u, out_b = (size_t)(p.out_hi - p.out_lo) * 4u;
  const size_t tab_o = st.take(tab.bytes()), shift_o = st.take((size_t)p.n_shift * 4u), nvar_o = st.take((size_t)p.n_shift * 4u), rx_o = st.take(rx_n),
               ch_o = st.take(ch_n);
  if (st.ensure(out_b) != 0)
    return -1;
  tab.write(st.h(tab_o));
  memcpy(st.h(shift_o), shift, (size_t)p.n_shift * 4u);
  memcpy(st.h(nvar_o), nvar, (size_t)p.n_shift * 4u);
  memcpy(st.h(rx_o), rxdataF + 2 * p.rx_lo, rx_n);
  memcpy(st.h(ch_o), ul_ch + 2 * p.ch_lo, ch_n);
  const auto launch = [&] {
    HIP_TRY(nr_launch_rx_mmse_grid(tab.first(st.d(tab_o)), (uint32_t)p.wgs.size(), tab.second(st.d(tab_o)), reinterpret_cast<const uint32_t *>(st.d(rx_o)),
                                   reinterpret_cast<const uint32_t *>(st.d(ch_o)), n_rx, rx_ant_stride, ch_ant_stride,
                                   reinterpret_cast<const int32_t *>(st.d(shift_o)), reinterpret_cast<const uint32_t *>(st.d(nvar_o)),
                                   reinterpret_cast<uint32_t *>(st.d_out()), st.stream()));
    return 0;
  };
  if (st.run(st.top, launch, out_b) != 0)
    return -1;
  rxm_scatter(gj, st.h_out(), p.out_lo, records);
  return 0;
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
  const auto tab = rxf_level_tables(lvl);
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    DeviceCall dc;
    if (dc.open("channel_level_grid_mmse", {{log2_maxh, 4}, {ul_ch, 4}, {max_ch, 4}}, DEV_NEEDS_ALIGNED, stream) != 0 ||
        dc.refuse_capture("channel_level_grid_mmse") != 0)
      return -1;
    uint8_t *base = dc.upload(tab);
    if (!base)
      return -1;
    HIP_TRY(nr_launch_rx_level_grid_mmse(tab.first(base), n_tb, reinterpret_cast<const uint32_t *>(ul_ch), n_rx, ch_ant_stride, max_ch, tab.second(base),
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
    HIP_TRY(nr_launch_rx_level_grid_mmse(tab.first(st.d(tab_o)), n_tb, reinterpret_cast<const uint32_t *>(st.d(ch_o)), n_rx, ch_ant_stride,
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
