/*
 * rx_grid_api.inc.cpp -- the UL receive front read from the OFDM grid: the _grid forms of the two calls of
 * rx_front_api.inc.cpp (they use its scatter and the call scopes of slot_call.inc.cpp), the CPU extraction for checking, and the
 * descriptors of a PUSCH allocation.  Where the REs lie: nr_rx_grid.h; the kernels: tb_rx_front.hip.  Everything the kernels
 * index with is checked before anything is enqueued: the grid checks, ranges and plan are rx_plan.h's.
 */

extern "C" {

int32_t nrLDPC_hip_ulsch_extract_host(const int16_t *rxdataF, const int16_t *ul_ch, uint32_t pattern, uint32_t fft_size, uint32_t start_re,
                                      uint32_t nb_re, int16_t *rxFext, int16_t *chFext)
{
  if (rxg_check_seg("extract_host", pattern, fft_size, start_re, nb_re) != 0)
    return -1;
  if (nb_re && (!rxdataF || !ul_ch || !rxFext || !chFext))
    return set_error("null argument");
  for (uint32_t j = 0; j < nb_re; j++) {
    const uint32_t p = nr_rxg_p(pattern, j), sc = nr_rxg_grid_sc(start_re, p, fft_size);
    rxFext[2 * (size_t)j] = rxdataF[2 * (size_t)sc];
    rxFext[2 * (size_t)j + 1] = rxdataF[2 * (size_t)sc + 1];
    chFext[2 * (size_t)j] = ul_ch[2 * (size_t)p];
    chFext[2 * (size_t)j + 1] = ul_ch[2 * (size_t)p + 1];
  }
  return 0;
}

int32_t nrLDPC_hip_pusch_grid_segments(const nrLDPC_hip_pusch_alloc_t *alloc, uint32_t n_alloc, nrLDPC_hip_rx_grid_seg_t *seg_out, uint32_t cap,
                                       nrLDPC_hip_rx_grid_seg_t *first_sym_out, uint32_t *n_seg_out)
{
  if (!n_seg_out || (n_alloc && (!alloc || !first_sym_out)) || (cap && !seg_out))
    return set_error("null argument");
  /* everything is checked and derived first: nothing is written when an allocation is refused */
  std::vector<nrLDPC_hip_rx_grid_seg_t> segs, first;
  for (uint32_t i = 0; i < n_alloc; i++) {
    const nrLDPC_hip_pusch_alloc_t &a = alloc[i];
    const uint32_t N = a.fft_size, type = a.dmrs_config_type, cdm = a.num_dmrs_cdm_grps_no_data;
    if (qam_check_qm(a.Qm) != 0)
      return set_error("pusch_grid_segments: Qm must be 2, 4, 6 or 8");
    if (alloc_check_symbols("pusch_grid_segments", a.start_symbol, a.nr_of_symbols) != 0 ||
        alloc_check_width("pusch_grid_segments", a.rb_size, N, a.first_carrier_offset) != 0)
      return -1;
    if (type > 1)
      return set_error("pusch_grid_segments: dmrs_config_type must be 0 (type 1) or 1 (type 2)");
    if (cdm < 1 || cdm > 2)
      return set_error("pusch_grid_segments: num_dmrs_cdm_grps_no_data must be 1 or 2");
    if (type == 1 && cdm == 2)
      return set_error("pusch_grid_segments: type 2 with two CDM groups without data is not supported (the level runs over extracted entries beyond nb_re)");
    const uint32_t start_re = nr_rxg_start_re(a.first_carrier_offset, a.bwp_start, a.rb_start, N);
    uint32_t off = 0;
    bool have_first = false;
    for (uint32_t sym = a.start_symbol; sym < a.start_symbol + a.nr_of_symbols; sym++) {
      if (nr_rxg_double_dmrs(a.ul_dmrs_symb_pos, sym))
        return set_error("pusch_grid_segments: two adjacent DMRS symbols are not supported");
      const uint32_t nb = nr_rxg_nb_re(a.ul_dmrs_symb_pos, sym, type, cdm, a.rb_size);
      if (nb == 0)
        continue;
      nrLDPC_hip_rx_grid_seg_t g;
      memset(&g, 0, sizeof g);
      g.tb = a.tb;
      g.Qm = a.Qm;
      g.pattern = (uint8_t)nr_rxg_symbol_pattern(a.ul_dmrs_symb_pos, sym, type);
      g.nb_re = nb;
      g.plane = a.plane;
      g.sym_off = off;
      g.fft_size = N;
      g.start_re = start_re;
      g.rx_off = a.rx_slot_off + (uint64_t)sym * N;
      g.ch_off = a.ch_off + (uint64_t)a.dmrs_symbol * N;
      g.rec_off = a.rec_off;
      off += nb;
      if (off > a.plane)
        return set_error("pusch_grid_segments: the symbols' REs add up to more than plane");
      segs.push_back(g);
      if (!have_first) {
        first.push_back(g);
        have_first = true;
      }
    }
    if (!have_first)
      return set_error("pusch_grid_segments: no symbol of the allocation has data REs");
  }
  if (emit_segments(segs, seg_out, cap, n_seg_out, "pusch_grid_segments: more segments than cap") != 0)
    return -1;
  if (!first.empty())
    memcpy(first_sym_out, first.data(), first.size() * sizeof first[0]);
  return 0;
}

int32_t nrLDPC_hip_ulsch_channel_compensation_grid(const int16_t *rxdataF, const int16_t *ul_ch, uint32_t n_rx, uint64_t rx_ant_stride,
                                                   uint64_t ch_ant_stride, const nrLDPC_hip_rx_grid_seg_t *seg, uint32_t n_seg, const int32_t *shift,
                                                   int16_t *records, int32_t mem, void *stream)
{
  if (rxf_check_common("channel_compensation_grid", n_rx, mem) != 0)
    return -1;
  if (n_seg && (!rxdataF || !ul_ch || !seg || !shift || !records))
    return set_error("null argument");
  RxFrontPlan p;
  std::vector<rx_front_grid_job> gj;
  if (rxg_plan_compensation(seg, n_seg, n_rx, rx_ant_stride, ch_ant_stride, p, gj) != 0)
    return -1;
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    if (n_seg == 0)
      return 0;
    DeviceCall dc;
    if (dc.open("channel_compensation_grid", {{records, 4}, {rxdataF, 4}, {ul_ch, 4}, {shift, 4}}, DEV_NEEDS_ALIGNED, stream) != 0 ||
        dc.refuse_capture("channel_compensation_grid") != 0)
      return -1;
    if (gj.empty())
      return 0;
    rxg_place(p, gj, 0, 0, 0, reinterpret_cast<uintptr_t>(records) >> 2);
    const auto tab = table2(p.wgs, gj);
    uint8_t *base = dc.upload(tab);
    if (!base)
      return -1;
    HIP_TRY(nr_launch_rx_compensation_grid(tab.first(base), (uint32_t)p.wgs.size(), tab.second(base), reinterpret_cast<const uint32_t *>(rxdataF),
                                           reinterpret_cast<const uint32_t *>(ul_ch), n_rx, rx_ant_stride, ch_ant_stride, shift,
                                           reinterpret_cast<uint32_t *>(records), dc.s));
    return 0;
  }
  if (gj.empty())
    return 0;
  StagedCall st;
  if (st.open() != 0)
    return -1;
  /* the device works on copies of the c16 ranges the segments reach; the output keeps the caller's alignment phase */
  const uint64_t out_pad = p.out_lo & 3u;
  rxg_place(p, gj, p.rx_lo, p.ch_lo, p.out_lo - out_pad, 0);
  const auto tab = table2(p.wgs, gj);
  const size_t rx_n = (size_t)(p.rx_hi - p.rx_lo) * 4u, ch_n = (size_t)(p.ch_hi - p.ch_lo) * 4u, out_b = (size_t)(p.out_hi - p.out_lo + out_pad) * 4u;
  const size_t tab_o = st.take(tab.bytes()), shift_o = st.take((size_t)p.n_shift * 4u), rx_o = st.take(rx_n), ch_o = st.take(ch_n);
  if (st.ensure(out_b) != 0)
    return -1;
  tab.write(st.h(tab_o));
  memcpy(st.h(shift_o), shift, (size_t)p.n_shift * 4u);
  memcpy(st.h(rx_o), rxdataF + 2 * p.rx_lo, rx_n);
  memcpy(st.h(ch_o), ul_ch + 2 * p.ch_lo, ch_n);
  const auto launch = [&] {
    HIP_TRY(nr_launch_rx_compensation_grid(tab.first(st.d(tab_o)), (uint32_t)p.wgs.size(), tab.second(st.d(tab_o)),
                                           reinterpret_cast<const uint32_t *>(st.d(rx_o)), reinterpret_cast<const uint32_t *>(st.d(ch_o)), n_rx, rx_ant_stride,
                                           ch_ant_stride, reinterpret_cast<const int32_t *>(st.d(shift_o)), reinterpret_cast<uint32_t *>(st.d_out()),
                                           st.stream()));
    return 0;
  };
  if (st.run(st.top, launch, out_b) != 0)
    return -1;
  rxf_scatter(p, st.h_out(), p.out_lo - out_pad, records);
  return 0;
}

int32_t nrLDPC_hip_ulsch_channel_level_grid(const int16_t *ul_ch, uint32_t n_rx, uint64_t ch_ant_stride, const nrLDPC_hip_rx_grid_seg_t *first_sym,
                                            uint32_t n_tb, int32_t *log2_maxh, int32_t mem, void *stream)
{
  if (rxf_check_common("channel_level_grid", n_rx, mem) != 0)
    return -1;
  if (n_tb && (!ul_ch || !first_sym || !log2_maxh))
    return set_error("null argument");
  if (n_tb == 0)
    return 0;
  std::vector<rx_front_grid_lvl_job> lvl;
  uint64_t ch_lo, ch_hi;
  if (rxg_plan_level(first_sym, n_tb, n_rx, ch_ant_stride, lvl, ch_lo, ch_hi) != 0)
    return -1;
  const auto tab = rxf_level_tables(lvl);
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    DeviceCall dc;
    if (dc.open("channel_level_grid", {{log2_maxh, 4}, {ul_ch, 4}}, DEV_NEEDS_ALIGNED, stream) != 0 || dc.refuse_capture("channel_level_grid") != 0)
      return -1;
    uint8_t *base = dc.upload(tab);
    if (!base)
      return -1;
    HIP_TRY(nr_launch_rx_level_grid(tab.first(base), n_tb, reinterpret_cast<const uint32_t *>(ul_ch), n_rx, ch_ant_stride, tab.second(base), log2_maxh,
                                    dc.s));
    return 0;
  }
  StagedCall st;
  if (st.open() != 0)
    return -1;
  for (rx_front_grid_lvl_job &j : lvl)
    j.ch_off -= ch_lo;
  const size_t ch_n = (size_t)(ch_hi - ch_lo) * 4u, out_b = (size_t)n_tb * 4u;
  const size_t tab_o = st.take(tab.bytes()), ch_o = st.take(ch_n);
  if (st.ensure(out_b) != 0)
    return -1;
  tab.write(st.h(tab_o));
  memcpy(st.h(ch_o), ul_ch + 2 * ch_lo, ch_n);
  const auto launch = [&] {
    HIP_TRY(nr_launch_rx_level_grid(tab.first(st.d(tab_o)), n_tb, reinterpret_cast<const uint32_t *>(st.d(ch_o)), n_rx, ch_ant_stride,
                                    tab.second(st.d(tab_o)), reinterpret_cast<int32_t *>(st.d_out()), st.stream()));
    return 0;
  };
  if (st.run(ch_o + ch_n, launch, out_b) != 0)
    return -1;
  memcpy(log2_maxh, st.h_out(), out_b);
  return 0;
}

} /* extern "C" */
