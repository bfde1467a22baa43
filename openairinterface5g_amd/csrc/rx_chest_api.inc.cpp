/*
 * rx_chest_api.inc.cpp -- PUSCH DMRS channel estimation: the GPU call, its CPU check forms and the descriptors of a PUSCH
 * allocation (included into ldpc_api.cpp; uses rxf_check_common of rx_plan.h and the call scopes and the DMRS helpers of
 * slot_call.inc.cpp).  The arithmetic: nr_chest.h; the kernel: tb_rx_chest.hip.  Everything the kernel indexes with is checked
 * before anything is enqueued: the descriptor check, the delay table, the plan and the workgroup table are rx_chest_plan.h's,
 * which the CPU emulation of the kernel shares.  pusch_channel_estimation and pusch_channel_estimation_meas (the same estimates plus
 * the reference's max_ch / nvar per block) are one call body, che_call; the measuring kernels, their finishing launch and the time
 * average of the estimates (pusch_chest_time_avg) are tb_rx_chest_meas.hip's, their plans rx_chest_meas_plan.h's.
 */
#include "rx_chest_plan.h"
#include "rx_chest_meas_plan.h"

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

/* the measurements of one descriptor's antenna on the CPU behind che_host_one: out = its 12 rb_size estimates */
void che_host_meas_one(const nrLDPC_hip_chest_seg_t &g, const uint32_t *rx, const uint32_t *out, int32_t &max_ch, uint64_t &noise)
{
  std::vector<uint32_t> gold;
  uint32_t w0;
  (void)dmrs_gold_words(g.c_init, g.dmrs_offset, nr_che_pilots_per_rb(g.mode) * g.rb_size, gold, w0); /* che_host_one has generated them */
  for (uint32_t u = 0; u < nr_che_units(g.mode, g.rb_size); u++) {
    const uint64_t bits = dmrs_bits(gold, w0, g.dmrs_offset + nr_che_unit_first_pilot(g.mode, u));
    if (g.mode == NR_CHE_TYPE1_INTERP)
      noise += nr_che_t1_meas(rx, g.fft_size, g.start_re, g.port, g.dmrs_offset, bits, u, out + 4u * u, &max_ch);
    else if (g.mode == NR_CHE_TYPE2_INTERP)
      noise += nr_che_t2_meas(rx, g.fft_size, g.start_re, g.port, g.dmrs_offset, bits, u, &max_ch);
    else
      max_ch = nr_che_avg_meas(g.rb_size, u, out[12u * u], max_ch);
  }
}

/* what the measuring call has besides: the blocks of the descriptors and the two result arrays */
struct CheMeasArgs {
  const uint32_t *seg_tb, *nvar_div;
  uint32_t n_tb;
  int32_t *max_ch;
  uint32_t *nvar;
};
/* the four launches over the tables' device copy; md: with the measurements and their finishing launch */
int che_launch(const ChestPlan &p, const rx_chest_wg *wgs, const rx_chest_job *jobs, const uint32_t *rx, uint64_t rx_stride, uint32_t *ch,
               uint64_t ch_stride, const int32_t *delay, hipStream_t s, const CheMeasDev *md = nullptr, uint32_t n_tb = 0)
{
  uint32_t first = 0;
  for (uint32_t mode = 0; mode < NR_CHE_MODES; mode++) {
    if (md)
      HIP_TRY(nr_launch_rx_chest_meas(mode, wgs + first, p.n_wg[mode], jobs, md->mjobs, rx, rx_stride, ch, ch_stride, delay, md->mx, md->noise, s));
    else
      HIP_TRY(nr_launch_rx_chest(mode, wgs + first, p.n_wg[mode], jobs, rx, rx_stride, ch, ch_stride, delay, s));
    first += p.n_wg[mode];
  }
  if (md)
    HIP_TRY(nr_launch_rx_chest_finish(md->tbs, n_tb, md->list, md->mjobs, md->mx, md->noise, md->max_ch, md->nvar, s));
  return 0;
}

/* the body of pusch_channel_estimation (ma == nullptr) and of pusch_channel_estimation_meas: checks, plan, one of the two scopes,
 * launches, scatter */
int che_call(const char *who, const int16_t *rxdataF, uint64_t rx_ant_stride, int16_t *ul_ch, uint64_t ch_ant_stride, uint32_t n_rx,
             const nrLDPC_hip_chest_seg_t *seg, uint32_t n_seg, const int32_t *est_delay, const CheMeasArgs *ma, int32_t mem, void *stream)
{
  if (rxf_check_common(who, n_rx, mem) != 0)
    return -1;
  if (n_seg && (!rxdataF || !ul_ch || !seg))
    return set_error("null argument");
  if (ma && ((n_seg && !ma->seg_tb) || (ma->n_tb && (!ma->nvar_div || !ma->max_ch || !ma->nvar))))
    return set_error("null argument");
  ChestPlan p;
  ChestMeasPlan m;
  if (che_plan(seg, n_seg, n_rx, rx_ant_stride, ch_ant_stride, p) != 0 ||
      (ma && che_meas_plan(seg, n_seg, n_rx, ma->seg_tb, ma->nvar_div, ma->n_tb, m) != 0))
    return -1;
  const uint32_t n_tb = ma ? ma->n_tb : 0;
  if (n_seg == 0 && n_tb == 0)
    return 0;
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    DeviceCall dc;
    const DevArray plain[] = {{ul_ch, 4}, {rxdataF, 4}, {est_delay, 4}};
    const DevArray meas[] = {{ma ? ma->max_ch : nullptr, 4}, {ma ? ma->nvar : nullptr, 4}, {ul_ch, 4}, {rxdataF, 4}, {est_delay, 4}};
    if ((ma ? dc.open(who, meas, DEV_NEEDS_ALIGNED, stream) : dc.open(who, plain, DEV_NEEDS_ALIGNED, stream)) != 0 || dc.refuse_capture(who) != 0)
      return -1;
    for (uint32_t i = 0; i < n_seg; i++)
      if (!(p.jobs[i].tab = che_table_device(dc.ord, seg[i].fft_size)))
        return -1;
    const CheLayout cl(p, ma ? &m : nullptr);
    uint8_t *base = dc.upload(cl.lay);
    if (!base)
      return -1;
    const CheMeasDev md = ma ? cl.meas(base, ma->max_ch, ma->nvar) : CheMeasDev{};
    return che_launch(p, cl.at<rx_chest_wg>(base, cl.wg), cl.at<rx_chest_job>(base, cl.job), reinterpret_cast<const uint32_t *>(rxdataF), rx_ant_stride,
                      reinterpret_cast<uint32_t *>(ul_ch), ch_ant_stride, est_delay, dc.s, ma ? &md : nullptr, n_tb);
  }
  if (n_seg == 0) { /* blocks without a descriptor: 0 / 0, no GPU work */
    for (uint32_t t = 0; t < n_tb; t++)
      ma->max_ch[t] = 0, ma->nvar[t] = 0;
    return 0;
  }
  StagedCall st;
  if (st.open() != 0)
    return -1;
  /* the device works on a copy of the c16 range of the grid the pilots lie in and on the delays of the call's (descriptor,
   * antenna) pairs; the output keeps the caller's alignment phase; the two result arrays follow the estimates' bounce */
  const uint64_t out_bias = p.out_lo - (p.out_lo & 3u);
  for (uint32_t i = 0; i < n_seg; i++) {
    rx_chest_job &j = p.jobs[i];
    if (!(j.tab = che_table_device(g.dev[0].id, seg[i].fft_size)))
      return -1;
    j.rx_off -= p.rx_lo;
    j.ch_off -= out_bias;
    j.delay_off = i * n_rx;
  }
  const CheLayout cl(p, ma ? &m : nullptr);
  const size_t rx_n = (size_t)(p.rx_hi - p.rx_lo) * 4u, ch_b = (size_t)(p.out_hi - out_bias) * 4u, res_o = align_up(ch_b, 16),
               out_b = res_o + 2u * align_up((size_t)n_tb * 4u, 16);
  const size_t tab_o = st.take(cl.lay.upload_bytes()), delay_o = st.take((size_t)n_seg * n_rx * 4u), rx_o = st.take(rx_n);
  if (st.ensure(out_b) != 0)
    return -1;
  cl.lay.write(st.h(tab_o));
  int32_t *dl = reinterpret_cast<int32_t *>(st.h(delay_o));
  for (uint32_t i = 0; i < n_seg; i++)
    for (uint32_t a = 0; a < n_rx; a++)
      dl[(size_t)i * n_rx + a] = est_delay ? est_delay[(size_t)seg[i].delay_off + a] : 0;
  memcpy(st.h(rx_o), rxdataF + 2 * p.rx_lo, rx_n);
  const size_t nvar_o = res_o + align_up((size_t)n_tb * 4u, 16);
  const auto launch = [&] {
    uint8_t *base = st.d(tab_o);
    const CheMeasDev md = ma ? cl.meas(base, reinterpret_cast<int32_t *>(st.d_out() + res_o), reinterpret_cast<uint32_t *>(st.d_out() + nvar_o)) : CheMeasDev{};
    return che_launch(p, cl.at<rx_chest_wg>(base, cl.wg), cl.at<rx_chest_job>(base, cl.job), reinterpret_cast<const uint32_t *>(st.d(rx_o)), rx_ant_stride,
                      reinterpret_cast<uint32_t *>(st.d_out()), ch_ant_stride, reinterpret_cast<const int32_t *>(st.d(delay_o)), st.stream(),
                      ma ? &md : nullptr, n_tb);
  };
  if (st.run(st.top, launch, out_b) != 0)
    return -1;
  /* only the write set goes to the caller's array */
  for (uint32_t i = 0; i < n_seg; i++)
    for (uint32_t a = 0; a < n_rx; a++) {
      const uint64_t at = seg[i].ch_off + (uint64_t)a * ch_ant_stride;
      memcpy(ul_ch + 2 * at, st.h_out() + 4u * (at - out_bias), (size_t)seg[i].rb_size * 48u);
    }
  if (ma && n_tb) {
    memcpy(ma->max_ch, st.h_out() + res_o, (size_t)n_tb * 4u);
    memcpy(ma->nvar, st.h_out() + nvar_o, (size_t)n_tb * 4u);
  }
  return 0;
}

/* only the first symbol's entries of the (descriptor, plane) pairs go back to the caller from a staged span that begins at lo */
void che_avg_scatter(const nrLDPC_hip_chest_avg_seg_t *seg, uint32_t n_seg, uint32_t n_plane, uint64_t ch_stride, const uint8_t *span, uint64_t lo,
                     int16_t *ul_ch)
{
  for (uint32_t i = 0; i < n_seg; i++)
    for (uint32_t q = 0; seg[i].n_sym > 1 && q < n_plane; q++) {
      const uint64_t at = seg[i].ch_off[0] + (uint64_t)q * ch_stride;
      memcpy(ul_ch + 2 * at, span + 4u * (at - lo), (size_t)seg[i].rb_size * 48u);
    }
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
  return che_call("channel_estimation", rxdataF, rx_ant_stride, ul_ch, ch_ant_stride, n_rx, seg, n_seg, est_delay, nullptr, mem, stream);
}

int32_t nrLDPC_hip_pusch_channel_estimation_meas(const int16_t *rxdataF, uint64_t rx_ant_stride, int16_t *ul_ch, uint64_t ch_ant_stride, uint32_t n_rx,
                                                 const nrLDPC_hip_chest_seg_t *seg, uint32_t n_seg, const int32_t *est_delay, const uint32_t *seg_tb,
                                                 const uint32_t *nvar_div, uint32_t n_tb, int32_t *max_ch, uint32_t *nvar, int32_t mem, void *stream)
{
  const CheMeasArgs ma{seg_tb, nvar_div, n_tb, max_ch, nvar};
  return che_call("channel_estimation_meas", rxdataF, rx_ant_stride, ul_ch, ch_ant_stride, n_rx, seg, n_seg, est_delay, &ma, mem, stream);
}

int32_t nrLDPC_hip_pusch_chest_meas_host(const int16_t *rxdataF, uint64_t rx_ant_stride, uint32_t n_rx, const nrLDPC_hip_chest_seg_t *seg,
                                         const int32_t *est_delay, int32_t *max_ch, uint64_t *noise_amp2, uint32_t *nest_count)
{
  if (!rxdataF || !seg || !max_ch || !noise_amp2 || !nest_count)
    return set_error("null argument");
  if (rxf_check_common("chest_meas_host", n_rx, NRLDPC_HIP_MEM_HOST) != 0 || che_check_seg("chest_meas_host", *seg) != 0)
    return -1;
  std::vector<uint32_t> out(12u * (size_t)seg->rb_size);
  int32_t mx = 0;
  uint64_t noise = 0;
  for (uint32_t a = 0; a < n_rx; a++) {
    const uint32_t *rx = reinterpret_cast<const uint32_t *>(rxdataF) + seg->rx_off + (uint64_t)a * rx_ant_stride;
    if (che_host_one(*seg, rx, est_delay ? est_delay[(size_t)seg->delay_off + a] : 0, out.data()) != 0)
      return -1;
    che_host_meas_one(*seg, rx, out.data(), mx, noise);
  }
  *max_ch = mx;
  *noise_amp2 = noise;
  *nest_count = nr_che_nest_per_antenna(seg->mode, seg->rb_size) * n_rx;
  return 0;
}

int32_t nrLDPC_hip_pusch_chest_time_avg_host(int16_t *ul_ch, const nrLDPC_hip_chest_avg_seg_t *seg)
{
  if (!ul_ch || !seg)
    return set_error("null argument");
  ChestAvgPlan p;
  if (che_avg_plan(seg, 1, 1, 0, p) != 0)
    return -1;
  uint32_t *ch = reinterpret_cast<uint32_t *>(ul_ch);
  for (uint32_t k = 0; seg->n_sym > 1 && k < 12u * seg->rb_size; k++) {
    uint32_t w[NR_CHE_AVG_MAX_SYM];
    for (uint32_t s = 0; s < seg->n_sym; s++)
      w[s] = ch[seg->ch_off[s] + k];
    ch[seg->ch_off[0] + k] = nr_che_tavg(w, seg->n_sym);
  }
  return 0;
}

int32_t nrLDPC_hip_pusch_chest_avg_segments(const nrLDPC_hip_pusch_alloc_t *alloc, uint32_t n_alloc, nrLDPC_hip_chest_avg_seg_t *out, uint32_t cap,
                                            uint32_t *n_out, uint8_t *first_dmrs_out)
{
  if (!n_out || (n_alloc && (!alloc || !first_dmrs_out)) || (cap && !out))
    return set_error("null argument");
  std::vector<nrLDPC_hip_chest_avg_seg_t> segs;
  std::vector<uint8_t> first;
  for (uint32_t i = 0; i < n_alloc; i++) {
    const nrLDPC_hip_pusch_alloc_t &a = alloc[i];
    if (alloc_check_symbols("pusch_chest_avg_segments", a.start_symbol, a.nr_of_symbols) != 0 ||
        alloc_check_width("pusch_chest_avg_segments", a.rb_size, a.fft_size, a.first_carrier_offset) != 0)
      return -1;
    nrLDPC_hip_chest_avg_seg_t g;
    memset(&g, 0, sizeof g);
    g.rb_size = a.rb_size;
    for (uint32_t sym = a.start_symbol; sym < a.start_symbol + a.nr_of_symbols; sym++) {
      if (!nr_rxg_is_dmrs(a.ul_dmrs_symb_pos, sym))
        continue;
      if (g.n_sym == NR_CHE_AVG_MAX_SYM)
        return set_error("pusch_chest_avg_segments: more than four DMRS symbols in the allocation (the reference asserts)");
      if (g.n_sym == 0)
        first.push_back((uint8_t)sym);
      g.ch_off[g.n_sym++] = a.ch_off + (uint64_t)sym * a.fft_size;
    }
    if (g.n_sym == 0)
      return set_error("pusch_chest_avg_segments: no DMRS symbol in the allocation (the reference asserts)");
    segs.push_back(g);
  }
  if (emit_segments(segs, out, cap, n_out, "pusch_chest_avg_segments: more descriptors than cap") != 0)
    return -1;
  if (!first.empty())
    memcpy(first_dmrs_out, first.data(), first.size());
  return 0;
}

int32_t nrLDPC_hip_pusch_chest_time_avg(int16_t *ul_ch, uint64_t ch_ant_stride, uint32_t n_plane, const nrLDPC_hip_chest_avg_seg_t *seg, uint32_t n_seg,
                                        int32_t mem, void *stream)
{
  if (check_mem("chest_time_avg", mem) != 0)
    return -1;
  if (n_seg && (!ul_ch || !seg))
    return set_error("null argument");
  ChestAvgPlan p;
  if (che_avg_plan(seg, n_seg, n_plane, ch_ant_stride, p) != 0)
    return -1;
  const auto tab = table2(p.wgs, p.jobs);
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    if (n_seg == 0)
      return 0;
    DeviceCall dc;
    if (dc.open("chest_time_avg", {{ul_ch, 4}}, DEV_NEEDS_ALIGNED, stream) != 0 || dc.refuse_capture("chest_time_avg") != 0)
      return -1;
    if (p.wgs.empty())
      return 0;
    uint8_t *base = dc.upload(tab);
    if (!base)
      return -1;
    HIP_TRY(nr_launch_rx_chest_time_avg(tab.first(base), (uint32_t)p.wgs.size(), tab.second(base), reinterpret_cast<uint32_t *>(ul_ch), ch_ant_stride, dc.s));
    return 0;
  }
  if (p.wgs.empty())
    return 0;
  StagedCall st;
  if (st.open() != 0)
    return -1;
  /* the device works in place on a copy of the span from the lowest to the highest c16 read or written, which keeps the caller's
   * alignment phase; only the write set comes back */
  const uint64_t bias = p.lo - (p.lo & 3u);
  for (rx_chest_avg_job &j : p.jobs)
    for (uint32_t s = 0; s < j.n_sym; s++)
      j.ch_off[s] -= bias;
  const size_t span_b = (size_t)(p.hi - bias) * 4u;
  const size_t tab_o = st.take(tab.bytes()), ch_o = st.take(span_b);
  if (st.ensure(16) != 0)
    return -1;
  tab.write(st.h(tab_o));
  memcpy(st.h(ch_o) + 4u * (p.lo - bias), ul_ch + 2 * p.lo, (size_t)(p.hi - p.lo) * 4u);
  const auto launch = [&] {
    HIP_TRY(nr_launch_rx_chest_time_avg(tab.first(st.d(tab_o)), (uint32_t)p.wgs.size(), tab.second(st.d(tab_o)), reinterpret_cast<uint32_t *>(st.d(ch_o)),
                                        ch_ant_stride, st.stream()));
    return 0;
  };
  if (st.run(st.top, launch, st.top, true) != 0)
    return -1;
  che_avg_scatter(seg, n_seg, n_plane, ch_ant_stride, st.h(ch_o), bias, ul_ch);
  return 0;
}

} /* extern "C" */
