/*
 * rx_chest_api.inc.cpp -- PUSCH DMRS channel estimation: the GPU call, its CPU check forms and the descriptors of a PUSCH
 * allocation (included into ldpc_api.cpp; uses rxf_check_common of rx_front_api.inc.cpp and the call scopes, the table layout, the
 * overlap check and the DMRS helpers of slot_call.inc.cpp).  The arithmetic: nr_chest.h; the kernel: tb_rx_chest.hip.  Everything
 * the kernel indexes with is checked here, before anything is enqueued.
 */

namespace {

bool che_fft_ok(uint32_t N)
{
  /* freq2time (common/utils/nr/nr_common.c:934-961) */
  static const uint32_t sizes[] = {128, 256, 512, 1024, 1536, 2048, 4096, 6144, 8192};
  for (uint32_t s : sizes)
    if (s == N)
      return true;
  return false;
}

/* init_delay_table (nr_common.c:916-928), one row */
void che_delay_row(uint32_t N, int32_t d, uint32_t *out)
{
  for (uint32_t k = 0; k < N; k++) {
    const double a = 2.0 * M_PI * (double)k * (double)d / (double)N;
    nr_che_c c;
    c.r = (int16_t)round(256.0 * cos(a));
    c.i = (int16_t)round(256.0 * sin(a));
    out[k] = nr_che_pack(c);
  }
}

/* the tables per fft_size, built once; their device copies per (HIP ordinal, fft_size), uploaded once */
std::mutex che_mu;
std::map<uint32_t, std::vector<uint32_t>> che_tab_host;
std::map<std::pair<int, uint32_t>, uint32_t *> che_tab_dev;

const std::vector<uint32_t> &che_table_locked(uint32_t N)
{
  std::vector<uint32_t> &t = che_tab_host[N];
  if (t.empty()) {
    t.resize((size_t)NR_CHE_DELAY_ROWS * N);
    for (int32_t d = -NR_CHE_MAX_DELAY; d <= NR_CHE_MAX_DELAY; d++)
      che_delay_row(N, d, t.data() + (size_t)nr_che_delay_idx(d) * N);
  }
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

int che_check_seg(const char *who, const nrLDPC_hip_chest_seg_t &g)
{
  const std::string w(who);
  if (g.mode >= NR_CHE_MODES)
    return set_error((w + ": mode must be TYPE1_INTERP, TYPE2_INTERP, TYPE1_AVG or TYPE2_AVG").c_str());
  if (g.port >= nr_che_ports(g.mode))
    return set_error((w + ": port must be 0..7 for type 1 and 0..11 for type 2").c_str());
  if (!che_fft_ok(g.fft_size))
    return set_error((w + ": fft_size must be 128, 256, 512, 1024, 1536, 2048, 4096, 6144 or 8192").c_str());
  if (g.rb_size == 0)
    return set_error((w + ": rb_size is 0").c_str());
  if ((uint64_t)g.rb_size * 12u > g.fft_size)
    return set_error((w + ": the allocation is wider than fft_size").c_str());
  if (g.start_re >= g.fft_size)
    return set_error((w + ": start_re must be below fft_size").c_str());
  if (g.c_init >> 31)
    return set_error((w + ": c_init must be below 2^31").c_str());
  if (g.dmrs_offset > (1u << 20))
    return set_error((w + ": dmrs_offset above 2^20").c_str());
  if (nr_che_reaches_n(g.mode, g.port, g.fft_size, g.start_re, g.rb_size))
    return set_error((w + ": a pilot RE at subcarrier fft_size - 1 with nushift 1 would be read at index fft_size").c_str());
  return 0;
}

/* the c16 range [lo, hi) of the symbol that a descriptor's pilots lie in */
void che_rx_range(const nrLDPC_hip_chest_seg_t &g, uint32_t &lo, uint32_t &hi)
{
  lo = UINT32_MAX;
  hi = 0;
  const uint32_t nu = g.mode == NR_CHE_TYPE1_INTERP ? 0u : nr_che_nushift(g.port), delta = g.mode == NR_CHE_TYPE1_INTERP ? nr_che_delta1(g.port) : 0u;
  for (uint32_t t = 0; t < 12u * g.rb_size; t++) {
    const bool used = nr_che_is_type2(g.mode) ? t % 6u < 2u : !(t & 1u);
    if (!used)
      continue;
    const uint32_t at = nr_che_wrap(g.start_re, t + delta, g.fft_size) + nu;
    lo = std::min(lo, at);
    hi = std::max(hi, at + 1u);
  }
}

const nr_gold_tables_t &che_gold_tables()
{
  static const nr_gold_tables_t t = nr_gold_make_tables();
  return t;
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

struct ChestPlan {
  std::vector<rx_chest_job> jobs;
  std::vector<rx_chest_wg> wgs; /* sorted by mode */
  uint32_t n_wg[NR_CHE_MODES] = {0, 0, 0, 0};
  uint64_t rx_lo = UINT64_MAX, rx_hi = 0, out_lo = UINT64_MAX, out_hi = 0;
};

int che_plan(const nrLDPC_hip_chest_seg_t *seg, uint32_t n_seg, uint32_t n_rx, uint64_t rx_stride, uint64_t ch_stride, ChestPlan &p)
{
  std::vector<Range64> out;
  p.jobs.resize(n_seg);
  for (uint32_t i = 0; i < n_seg; i++) {
    const nrLDPC_hip_chest_seg_t &g = seg[i];
    if (che_check_seg("channel_estimation", g) != 0)
      return -1;
    uint32_t lo, hi;
    che_rx_range(g, lo, hi);
    p.rx_lo = std::min(p.rx_lo, g.rx_off + lo);
    p.rx_hi = std::max(p.rx_hi, g.rx_off + hi + (uint64_t)(n_rx - 1) * rx_stride);
    for (uint32_t a = 0; a < n_rx; a++)
      out.push_back(Range64{g.ch_off + (uint64_t)a * ch_stride, g.ch_off + (uint64_t)a * ch_stride + 12u * g.rb_size});
    rx_chest_job &j = p.jobs[i];
    memset(&j, 0, sizeof j);
    j.rx_off = g.rx_off;
    j.ch_off = g.ch_off;
    j.fft_size = g.fft_size;
    j.start_re = g.start_re;
    j.rb_size = g.rb_size;
    j.dmrs_offset = g.dmrs_offset;
    j.port = g.port;
    j.delay_off = g.delay_off;
  }
  if (ranges_overlap(out, p.out_lo, p.out_hi))
    return set_error("channel_estimation: the output ranges of two (descriptor, antenna) pairs overlap");
  /* the workgroup table, mode by mode; the Gold registers of a piece are the same for every antenna */
  for (uint32_t mode = 0; mode < NR_CHE_MODES; mode++)
    for (uint32_t i = 0; i < n_seg; i++) {
      if (seg[i].mode != mode)
        continue;
      const uint32_t units = nr_che_units(mode, seg[i].rb_size);
      for (uint32_t q = 0; q * NR_CHE_THREADS < units; q++) {
        rx_chest_wg w{};
        w.job = i;
        w.piece = q;
        w.w0 = (2u * (seg[i].dmrs_offset + nr_che_unit_first_pilot(mode, q * NR_CHE_THREADS))) >> 5;
        nr_gold_jump(&che_gold_tables(), seg[i].c_init, w.w0, &w.x1, &w.x2);
        for (uint32_t a = 0; a < n_rx; a++) {
          w.ant = a;
          p.wgs.push_back(w);
          p.n_wg[mode]++;
        }
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
