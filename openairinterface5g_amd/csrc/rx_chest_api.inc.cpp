/*
 * rx_chest_api.inc.cpp -- PUSCH DMRS channel estimation: the GPU call, its CPU check forms and the descriptors of a PUSCH
 * allocation (included into ldpc_api.cpp; uses rxf_check_common of rx_plan.h and the call scopes and the DMRS helpers of
 * slot_call.inc.cpp).  The arithmetic: nr_chest.h; the kernel: tb_rx_chest.hip.  Everything the kernel indexes with is checked
 * before anything is enqueued: the descriptor check, the delay table, the plan and the workgroup table are rx_chest_plan.h's,
 * which the CPU emulation of the kernel shares.
 */
#include "rx_chest_plan.h"

namespace {

/* the tables per fft_size, built once; their device copies per (HIP ordinal, fft_size), uploaded once */
std::mutex che_mu;
std::map<uint32_t, std::vector<uint32_t>> che_tab_host;
std::map<std::pair<int, uint32_t>, uint32_t *> che_tab_dev;

const std::vector<uint32_t> &che_table_locked(uint32_t N)
{
  std::vector<uint32_t> &t = che_tab_host[N];
  if (t.empty())
    che_fill_table(N, t);
  return t;
}

/* on the current device (UseDevice); nullptr + error when the allocation or the copy fails */
const uint32_t *che_table_device(int ordinal, uint32_t N)
{
  std::lock_guard<std::mutex> lk(che_mu);
  uint32_t *&p = che_tab_dev[std::make_pair(ordinal, N)];
  if (!p) {
    const std::vector<uint32_t> &t = che_table_locked(N);
    uint32_t *d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d), t.size() * 4u);
    if (e == hipSuccess && (e = hipMemcpy(d, t.data(), t.size() * 4u, hipMemcpyHostToDevice)) != hipSuccess)
      (void)hipFree(d);
    if (e != hipSuccess) {
      set_error("channel_estimation: the delay table could not be uploaded", e);
      return nullptr;
    }
    p = d;
  }
  return p;
}

/* one descriptor, one antenna on the CPU: rx = the symbol's subcarrier 0, out = 12 rb_size c16 */
int che_host_one(const nrLDPC_hip_chest_seg_t &g, const uint32_t *rx, int32_t d, uint32_t *out)
{
  std::vector<uint32_t> gold;
  uint32_t w0;
  if (!dmrs_gold_words(g.c_init, g.dmrs_offset, nr_che_pilots_per_rb(g.mode) * g.rb_size, gold, w0))
    return set_error("chest_host: the Gold sequence could not be generated");
  const uint32_t *fwd = nullptr, *inv = nullptr;
  {
    std::lock_guard<std::mutex> lk(che_mu);
    const std::vector<uint32_t> &t = che_table_locked(g.fft_size);
    fwd = t.data() + (size_t)nr_che_delay_idx(d) * g.fft_size;
    inv = t.data() + (size_t)nr_che_inv_delay_idx(d) * g.fft_size;
  }
  for (uint32_t u = 0; u < nr_che_units(g.mode, g.rb_size); u++) {
    const uint64_t bits = dmrs_bits(gold, w0, g.dmrs_offset + nr_che_unit_first_pilot(g.mode, u));
    if (g.mode == NR_CHE_TYPE1_INTERP)
      nr_che_t1_interp(rx, g.fft_size, g.start_re, g.rb_size, g.port, g.dmrs_offset, bits, fwd, inv, u, out + 4u * u);
    else if (g.mode == NR_CHE_TYPE2_INTERP)
      nr_che_t2_interp(rx, g.fft_size, g.start_re, g.port, g.dmrs_offset, bits, inv, u, out + 4u * u);
    else {
      const uint32_t v = nr_che_avg(g.mode, rx, g.fft_size, g.start_re, g.port, g.dmrs_offset, bits, u);
      for (uint32_t k = 0; k < 12u; k++)
        out[12u * u + k] = v;
    }
  }
  return 0;
}

/* the four launches over the tables' device copy */
int che_launch(const ChestPlan &p, const rx_chest_wg *wgs, const rx_chest_job *jobs, const uint32_t *rx, uint64_t rx_stride, uint32_t *ch,
               uint64_t ch_stride, const int32_t *delay, hipStream_t s)
{
  uint32_t first = 0;
  for (uint32_t mode = 0; mode < NR_CHE_MODES; mode++) {
    HIP_TRY(nr_launch_rx_chest(mode, wgs + first, p.n_wg[mode], jobs, rx, rx_stride, ch, ch_stride, delay, s));
    first += p.n_wg[mode];
  }
  return 0;
}

} // namespace

extern "C" {

int32_t nrLDPC_hip_delay_table_host(uint32_t fft_size, int32_t delay, int16_t *out)
{
  if (!out)
    return set_error("null argument");
  if (!che_fft_ok(fft_size))
    return set_error("delay_table_host: fft_size must be 128, 256, 512, 1024, 1536, 2048, 4096, 6144 or 8192");
  std::lock_guard<std::mutex> lk(che_mu);
  memcpy(out, che_table_locked(fft_size).data() + (size_t)nr_che_delay_idx(delay) * fft_size, (size_t)fft_size * 4u);
  return 0;
}

int32_t nrLDPC_hip_pusch_dmrs_host(uint32_t c_init, uint32_t dmrs_offset, uint32_t n, uint32_t port, uint32_t type, int16_t *out)
{
  if (n && !out)
    return set_error("null argument");
  if (type > 1)
    return set_error("pusch_dmrs_host: type must be 0 (type 1) or 1 (type 2)");
  if (port >= nr_che_ports(type))
    return set_error("pusch_dmrs_host: port must be 0..7 for type 1 and 0..11 for type 2");
  if (c_init >> 31)
    return set_error("pusch_dmrs_host: c_init must be below 2^31");
  if (dmrs_offset > (1u << 20) || n > (1u << 20))
    return set_error("pusch_dmrs_host: dmrs_offset or n above 2^20");
  if (n == 0)
    return 0;
  std::vector<uint32_t> gold;
  uint32_t w0;
  if (!dmrs_gold_words(c_init, dmrs_offset, n, gold, w0))
    return set_error("pusch_dmrs_host: the Gold sequence could not be generated");
  for (uint32_t k = 0; k < n; k++) {
    const nr_che_c c = nr_che_pilot((uint32_t)dmrs_bits(gold, w0, dmrs_offset + k) & 3u, dmrs_offset + k, port);
    out[2 * (size_t)k] = (int16_t)c.r;
    out[2 * (size_t)k + 1] = (int16_t)c.i;
  }
  return 0;
}

int32_t nrLDPC_hip_pusch_chest_host(const int16_t *rxdataF, const nrLDPC_hip_chest_seg_t *seg, int32_t est_delay, int16_t *ul_ch)
{
  if (!rxdataF || !seg || !ul_ch)
    return set_error("null argument");
  if (che_check_seg("chest_host", *seg) != 0)
    return -1;
  std::vector<uint32_t> out(12u * (size_t)seg->rb_size);
  if (che_host_one(*seg, reinterpret_cast<const uint32_t *>(rxdataF) + seg->rx_off, est_delay, out.data()) != 0)
    return -1;
  memcpy(ul_ch + 2 * seg->ch_off, out.data(), out.size() * 4u);
  return 0;
}

int32_t nrLDPC_hip_pusch_chest_segments(const nrLDPC_hip_pusch_alloc_t *alloc, const nrLDPC_hip_pusch_chest_cfg_t *cfg, uint32_t n_alloc, uint32_t n_rx,
                                        nrLDPC_hip_chest_seg_t *seg_out, uint32_t cap, uint32_t *n_seg_out)
{
  if (!n_seg_out || (n_alloc && (!alloc || !cfg)) || (cap && !seg_out))
    return set_error("null argument");
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return set_error("pusch_chest_segments: n_rx must be 1..8");
  std::vector<nrLDPC_hip_chest_seg_t> segs;
  for (uint32_t i = 0; i < n_alloc; i++) {
    const nrLDPC_hip_pusch_alloc_t &a = alloc[i];
    const nrLDPC_hip_pusch_chest_cfg_t &c = cfg[i];
    const uint32_t N = a.fft_size, type = a.dmrs_config_type;
    if (alloc_check_symbols("pusch_chest_segments", a.start_symbol, a.nr_of_symbols) != 0 ||
        alloc_check_width("pusch_chest_segments", a.rb_size, N, a.first_carrier_offset) != 0)
      return -1;
    if (type > 1)
      return set_error("pusch_chest_segments: dmrs_config_type must be 0 (type 1) or 1 (type 2)");
    if (c.chest_freq > 1)
      return set_error("pusch_chest_segments: chest_freq must be 0 (interpolation) or 1 (average per PRB)");
    if (c.scid > 1)
      return set_error("pusch_chest_segments: scid must be 0 or 1");
    if (c.dmrs_scrambling_id > 0xffffu)
      return set_error("pusch_chest_segments: dmrs_scrambling_id above 65535");
    if (c.slot >= 160)
      return set_error("pusch_chest_segments: slot must be below 160");
    if (c.port >= nr_che_ports(type))
      return set_error("pusch_chest_segments: port must be 0..7 for type 1 and 0..11 for type 2");
    if ((uint64_t)a.bwp_start + a.rb_start > (1u << 16))
      return set_error("pusch_chest_segments: bwp_start + rb_start above 2^16");
    for (uint32_t sym = a.start_symbol; sym < a.start_symbol + a.nr_of_symbols; sym++) {
      if (!nr_rxg_is_dmrs(a.ul_dmrs_symb_pos, sym))
        continue;
      nrLDPC_hip_chest_seg_t g;
      memset(&g, 0, sizeof g);
      g.mode = (uint8_t)(type + 2u * c.chest_freq);
      g.port = (uint8_t)c.port;
      g.fft_size = N;
      g.start_re = nr_rxg_start_re(a.first_carrier_offset, a.bwp_start, a.rb_start, N);
      g.rb_size = a.rb_size;
      g.dmrs_offset = 12u * (a.bwp_start + a.rb_start) / (type == 0 ? 2u : 3u); /* nr_dmrs_rx.c:84 */
      g.c_init = dmrs_c_init(c.slot, sym, c.dmrs_scrambling_id, c.scid);
      g.delay_off = (uint32_t)segs.size() * n_rx;
      g.rx_off = a.rx_slot_off + (uint64_t)sym * N;
      g.ch_off = a.ch_off + (uint64_t)sym * N;
      if (che_check_seg("pusch_chest_segments", g) != 0)
        return -1;
      segs.push_back(g);
    }
  }
  return emit_segments(segs, seg_out, cap, n_seg_out, "pusch_chest_segments: more descriptors than cap");
}

int32_t nrLDPC_hip_pusch_channel_estimation(const int16_t *rxdataF, uint64_t rx_ant_stride, int16_t *ul_ch, uint64_t ch_ant_stride, uint32_t n_rx,
                                            const nrLDPC_hip_chest_seg_t *seg, uint32_t n_seg, const int32_t *est_delay, int32_t mem, void *stream)
{
  if (rxf_check_common("channel_estimation", n_rx, mem) != 0)
    return -1;
  if (n_seg && (!rxdataF || !ul_ch || !seg))
    return set_error("null argument");
  ChestPlan p;
  if (che_plan(seg, n_seg, n_rx, rx_ant_stride, ch_ant_stride, p) != 0)
    return -1;
  const auto tab = table2(p.wgs, p.jobs);
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    if (n_seg == 0)
      return 0;
    DeviceCall dc;
    if (dc.open("channel_estimation", {{ul_ch, 4}, {rxdataF, 4}, {est_delay, 4}}, DEV_NEEDS_ALIGNED, stream) != 0 ||
        dc.refuse_capture("channel_estimation") != 0)
      return -1;
    for (uint32_t i = 0; i < n_seg; i++)
      if (!(p.jobs[i].tab = che_table_device(dc.ord, seg[i].fft_size)))
        return -1;
    uint8_t *base = dc.upload(tab);
    if (!base)
      return -1;
    return che_launch(p, tab.first(base), tab.second(base), reinterpret_cast<const uint32_t *>(rxdataF), rx_ant_stride, reinterpret_cast<uint32_t *>(ul_ch),
                      ch_ant_stride, est_delay, dc.s);
  }
  if (n_seg == 0)
    return 0;
  StagedCall st;
  if (st.open() != 0)
    return -1;
  /* the device works on a copy of the c16 range of the grid the pilots lie in and on the delays of the call's (descriptor,
   * antenna) pairs; the output keeps the caller's alignment phase */
  const uint64_t out_bias = p.out_lo - (p.out_lo & 3u);
  for (uint32_t i = 0; i < n_seg; i++) {
    rx_chest_job &j = p.jobs[i];
    if (!(j.tab = che_table_device(g.dev[0].id, seg[i].fft_size)))
      return -1;
    j.rx_off -= p.rx_lo;
    j.ch_off -= out_bias;
    j.delay_off = i * n_rx;
  }
  const size_t rx_n = (size_t)(p.rx_hi - p.rx_lo) * 4u, out_b = (size_t)(p.out_hi - out_bias) * 4u;
  const size_t tab_o = st.take(tab.bytes()), delay_o = st.take((size_t)n_seg * n_rx * 4u), rx_o = st.take(rx_n);
  if (st.ensure(out_b) != 0)
    return -1;
  tab.write(st.h(tab_o));
  int32_t *dl = reinterpret_cast<int32_t *>(st.h(delay_o));
  for (uint32_t i = 0; i < n_seg; i++)
    for (uint32_t a = 0; a < n_rx; a++)
      dl[(size_t)i * n_rx + a] = est_delay ? est_delay[(size_t)seg[i].delay_off + a] : 0;
  memcpy(st.h(rx_o), rxdataF + 2 * p.rx_lo, rx_n);
  const auto launch = [&] {
    return che_launch(p, tab.first(st.d(tab_o)), tab.second(st.d(tab_o)), reinterpret_cast<const uint32_t *>(st.d(rx_o)), rx_ant_stride,
                      reinterpret_cast<uint32_t *>(st.d_out()), ch_ant_stride, reinterpret_cast<const int32_t *>(st.d(delay_o)), st.stream());
  };
  if (st.run(st.top, launch, out_b) != 0)
    return -1;
  /* only the write set goes to the caller's array */
  for (uint32_t i = 0; i < n_seg; i++)
    for (uint32_t a = 0; a < n_rx; a++) {
      const uint64_t at = seg[i].ch_off + (uint64_t)a * ch_ant_stride;
      memcpy(ul_ch + 2 * at, st.h_out() + 4u * (at - out_bias), (size_t)seg[i].rb_size * 48u);
    }
  return 0;
}

} /* extern "C" */
