/*
 * rx_grid_api.inc.cpp -- the UL receive front read from the OFDM grid: the _grid forms of the two calls of
 * rx_front_api.inc.cpp (they use its scatter and its two call bodies, rx_level_call and rx_receiver_call), the CPU extraction for checking, and the
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
    /* whose estimates a symbol reads: an explicit symbol for the whole allocation, or the reference's own rule with chest_time = 0 --
     * dmrs_symbol starts as the allocation's first DMRS symbol (nr_ulsch_demodulation.c:1460, :1477-1478; the level reads that one,
     * :1606) and the symbol loop moves it to each DMRS symbol it reaches before that symbol's inner_rx (:1403-1408).  One deliberate
     * deviation: the reference runs that loop only for symbols with REs (:1666), so with two CDM groups without data its DMRS
     * symbols never move dmrs_symbol; here every DMRS symbol of the allocation does. */
    const bool follow = a.dmrs_symbol == NRLDPC_HIP_DMRS_SYMBOL_FOLLOW;
    if (!follow && a.dmrs_symbol >= 14)
      return set_error("pusch_grid_segments: dmrs_symbol must be 0..13 or 255 (NRLDPC_HIP_DMRS_SYMBOL_FOLLOW)");
    uint32_t first_dmrs = a.dmrs_symbol, cur_dmrs = a.dmrs_symbol;
    if (follow) {
      first_dmrs = a.start_symbol;
      while (first_dmrs < a.start_symbol + a.nr_of_symbols && !nr_rxg_is_dmrs(a.ul_dmrs_symb_pos, first_dmrs))
        first_dmrs++;
      if (first_dmrs == a.start_symbol + a.nr_of_symbols)
        return set_error("pusch_grid_segments: dmrs_symbol = 255 needs a DMRS symbol inside the allocation (the reference would read estimates at 255 fft_size)");
      cur_dmrs = first_dmrs;
    }
    const uint32_t start_re = nr_rxg_start_re(a.first_carrier_offset, a.bwp_start, a.rb_start, N);
    uint32_t off = 0;
    bool have_first = false;
    for (uint32_t sym = a.start_symbol; sym < a.start_symbol + a.nr_of_symbols; sym++) {
      if (nr_rxg_double_dmrs(a.ul_dmrs_symb_pos, sym))
        return set_error("pusch_grid_segments: two adjacent DMRS symbols are not supported");
      if (follow && nr_rxg_is_dmrs(a.ul_dmrs_symb_pos, sym))
        cur_dmrs = sym;
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
      g.ch_off = a.ch_off + (uint64_t)cur_dmrs * N;
      g.rec_off = a.rec_off;
      off += nb;
      if (off > a.plane)
        return set_error("pusch_grid_segments: the symbols' REs add up to more than plane");
      segs.push_back(g);
      if (!have_first) {
        g.ch_off = a.ch_off + (uint64_t)first_dmrs * N;
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
  const auto place = [&](uint64_t rx_bias, uint64_t ch_bias, uint64_t out_lo, uint64_t rec_word) {
    rxg_place(p, gj, rx_bias, ch_bias, rxf_aligned_bias(out_lo), rec_word);
    return rxf_aligned_bias(out_lo);
  };
  const auto launch = [&](const rx_front_wg *wgs, uint32_t n_wg, const rx_front_grid_job *jobs, const uint32_t *rx, const uint32_t *ch,
                          const void *const *per_tb, uint32_t *rec, hipStream_t s) {
    return nr_launch_rx_compensation_grid(wgs, n_wg, jobs, rx, ch, n_rx, rx_ant_stride, ch_ant_stride, static_cast<const int32_t *>(per_tb[0]), rec, s);
  };
  const auto scatter = [&](const uint8_t *bounce, uint64_t bias) { rxf_scatter(p, bounce, bias, records); };
  return rx_receiver_call("channel_compensation_grid", p, gj, n_seg, rxdataF, ul_ch, {shift}, records, mem, stream, place, launch, scatter);
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
  const auto launch = [&](const rx_front_grid_lvl_job *jobs, const uint32_t *ch, const void *const *, int32_t *state, int32_t *out, hipStream_t s) {
    return nr_launch_rx_level_grid(jobs, n_tb, ch, n_rx, ch_ant_stride, state, out, s);
  };
  return rx_level_call("channel_level_grid", lvl, ch_lo, ch_hi, ul_ch, {}, log2_maxh, mem, stream, launch);
}

} /* extern "C" */
