/*
 * rx_front_api.inc.cpp -- the UL receive front's entry points: channel level and channel compensation of the single-layer PUSCH
 * receiver (included at the end of ldpc_api.cpp, behind qam_api.inc.cpp whose checks it shares).  The arithmetic: nr_rx_front.h;
 * the kernels: tb_rx_front.hip.  Everything the kernels index with is checked here, before anything is enqueued.
 */

namespace {

/* what a call's descriptors come to: the job lists and the c16 ranges of the caller's arrays they reach */
struct RxFrontPlan {
  std::vector<rx_front_seg_job> jobs;
  std::vector<rx_front_wg> wgs;
  std::vector<rx_front_lvl_job> lvl;
  uint64_t rx_lo = UINT64_MAX, rx_hi = 0, ch_lo = UINT64_MAX, ch_hi = 0, out_lo = UINT64_MAX, out_hi = 0;
  uint32_t n_shift = 0; /* 1 + the largest tb */
};

int rxf_check_common(const char *who, uint32_t n_rx, int32_t mem)
{
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return set_error((std::string(who) + ": n_rx must be 1..8").c_str());
  if (mem != NRLDPC_HIP_MEM_HOST && mem != NRLDPC_HIP_MEM_DEVICE)
    return set_error((std::string(who) + ": mem must be NRLDPC_HIP_MEM_HOST or NRLDPC_HIP_MEM_DEVICE").c_str());
  return 0;
}

/* graph capture of the two calls is not supported: they upload their descriptors through the thread's page-locked area */
int rxf_check_stream(const char *who, hipStream_t s)
{
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    return set_error((std::string(who) + ": the stream is being captured (graph capture of this call is not supported)").c_str());
  }
  return 0;
}

/* the segments of a compensation call, without the workgroup table (that needs the address the records are written at) */
int rxf_plan_compensation(const nrLDPC_hip_rx_seg_t *seg, uint32_t n_seg, uint32_t n_rx, uint64_t ant_stride, RxFrontPlan &p)
{
  struct Range { uint64_t lo, hi; };
  std::vector<Range> out;
  p.jobs.reserve(n_seg);
  for (uint32_t i = 0; i < n_seg; i++) {
    const nrLDPC_hip_rx_seg_t &g = seg[i];
    if (qam_check_qm(g.Qm) != 0)
      return set_error("channel_compensation: Qm must be 2, 4, 6 or 8");
    if (g.rec_off & 1u)
      return set_error("channel_compensation: rec_off must be even");
    if ((uint64_t)g.sym_off + g.nb_re > g.plane)
      return set_error("channel_compensation: sym_off + nb_re above plane");
    if ((uint64_t)g.nb_re * g.Qm > NR_SCR_MAX_BITS)
      return set_error("channel_compensation: nb_re * Qm above 2^21");
    p.n_shift = std::max(p.n_shift, g.tb + 1u);
    if (g.nb_re == 0)
      continue;
    const uint64_t first = g.rec_off / 2u + g.sym_off, reach = (uint64_t)(n_rx - 1) * ant_stride + g.nb_re;
    for (uint32_t k = 0; k < g.Qm / 2u; k++)
      out.push_back(Range{first + (uint64_t)k * g.plane, first + (uint64_t)k * g.plane + g.nb_re});
    p.rx_lo = std::min(p.rx_lo, g.rx_off);
    p.rx_hi = std::max(p.rx_hi, g.rx_off + reach);
    p.ch_lo = std::min(p.ch_lo, g.ch_off);
    p.ch_hi = std::max(p.ch_hi, g.ch_off + reach);
    p.out_lo = std::min(p.out_lo, first);
    p.out_hi = std::max(p.out_hi, out.back().hi);
    rx_front_seg_job j{};
    j.rx_off = g.rx_off;
    j.ch_off = g.ch_off;
    j.out_off = first;
    j.plane = g.plane;
    j.nb_re = g.nb_re;
    j.tb = g.tb;
    j.Qm = g.Qm;
    p.jobs.push_back(j);
  }
  std::sort(out.begin(), out.end(), [](const Range &a, const Range &b) { return a.lo < b.lo; });
  for (size_t i = 1; i < out.size(); i++)
    if (out[i].lo < out[i - 1].hi)
      return set_error("channel_compensation: the output ranges of two segments overlap");
  return 0;
}

/* offsets relative to the copies' starts (staged) and the workgroup table for records written at word address rec_word */
void rxf_place(RxFrontPlan &p, uint64_t rx_bias, uint64_t ch_bias, uint64_t out_bias, uint64_t rec_word)
{
  for (size_t i = 0; i < p.jobs.size(); i++) {
    rx_front_seg_job &j = p.jobs[i];
    j.rx_off -= rx_bias;
    j.ch_off -= ch_bias;
    j.out_off -= out_bias;
    j.phase = (uint32_t)((rec_word + j.out_off) & 3u);
    const uint32_t groups = (j.nb_re + j.phase + NR_RXF_GROUP - 1u) / NR_RXF_GROUP;
    for (uint32_t q = 0; q * NR_RXF_THREADS < groups; q++)
      p.wgs.push_back(rx_front_wg{(uint32_t)i, q});
  }
}

size_t rxf_jobs_bytes(const RxFrontPlan &p) { return align_up(p.wgs.size() * sizeof(rx_front_wg), 16) + align_up(p.jobs.size() * sizeof(rx_front_seg_job), 16); }
void rxf_write_jobs(const RxFrontPlan &p, uint8_t *dst)
{
  memcpy(dst, p.wgs.data(), p.wgs.size() * sizeof(rx_front_wg));
  memcpy(dst + align_up(p.wgs.size() * sizeof(rx_front_wg), 16), p.jobs.data(), p.jobs.size() * sizeof(rx_front_seg_job));
}

int rxf_plan_level(const nrLDPC_hip_rx_seg_t *fs, uint32_t n_tb, uint32_t n_rx, uint64_t ant_stride, RxFrontPlan &p)
{
  std::vector<uint8_t> seen(n_tb, 0);
  p.lvl.resize(n_tb);
  for (uint32_t i = 0; i < n_tb; i++) {
    if (fs[i].tb >= n_tb || seen[fs[i].tb])
      return set_error("channel_level: every tb below n_tb must be named once");
    seen[fs[i].tb] = 1;
    if (fs[i].nb_re == 0)
      return set_error("channel_level: the measurement symbol has no REs");
    if ((uint64_t)fs[i].nb_re * 2u > NR_SCR_MAX_BITS)
      return set_error("channel_level: nb_re above 2^20");
    p.lvl[i] = rx_front_lvl_job{fs[i].ch_off, fs[i].nb_re, fs[i].tb};
    p.ch_lo = std::min(p.ch_lo, fs[i].ch_off);
    p.ch_hi = std::max(p.ch_hi, fs[i].ch_off + (uint64_t)(n_rx - 1) * ant_stride + fs[i].nb_re);
  }
  return 0;
}

bool rxf_dev_ok(const void *p, int ord) { return scr_device_ordinal(p) == ord && (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

} // namespace

extern "C" {

int32_t nrLDPC_hip_ulsch_compensate_host(const int16_t *rxFext, const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, uint32_t nb_re,
                                         uint8_t Qm, int32_t shift, int16_t *out)
{
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return set_error("compensate_host: n_rx must be 1..8");
  if (qam_check_qm(Qm) != 0)
    return -1;
  if (nb_re && (!rxFext || !chFext || !out))
    return set_error("null argument");
  const uint32_t s = nr_rxf_shift(shift), np = Qm / 2u;
  const int32_t amp[3] = {nr_rxf_amp(Qm, 0), nr_rxf_amp(Qm, 1), nr_rxf_amp(Qm, 2)};
  for (uint32_t r = 0; r < nb_re; r++) {
    nr_rxf_acc_t acc = {{0, 0, 0, 0}};
    for (uint32_t a = 0; a < n_rx; a++) {
      const int16_t *h = chFext + 2 * ((size_t)a * ant_stride + r), *y = rxFext + 2 * ((size_t)a * ant_stride + r);
      nr_rxf_mac(&acc, nr_rxf_c16(h[0], h[1]), nr_rxf_c16(y[0], y[1]), s, amp);
    }
    for (uint32_t k = 0; k < np; k++) {
      out[2 * ((size_t)k * nb_re + r)] = (int16_t)nr_rxf_re(acc.w[k]);
      out[2 * ((size_t)k * nb_re + r) + 1] = (int16_t)nr_rxf_im(acc.w[k]);
    }
  }
  return 0;
}

int32_t nrLDPC_hip_ulsch_level_host(const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, uint32_t nb_re, int32_t *avg, int32_t *log2_maxh)
{
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return set_error("level_host: n_rx must be 1..8");
  if (nb_re == 0 || (uint64_t)nb_re * 2u > NR_SCR_MAX_BITS)
    return set_error("level_host: nb_re must be 1..2^20");
  if (!chFext || !log2_maxh)
    return set_error("null argument");
  const uint32_t len = nr_rxf_level_len(nb_re), x = (uint32_t)nr_rxf_factor2(len);
  int32_t avgs = 0;
  for (uint32_t a = 0; a < n_rx; a++) {
    uint32_t sum = 0;
    for (uint32_t r = 0; r < nb_re; r++) {
      const int16_t *h = chFext + 2 * ((size_t)a * ant_stride + r);
      sum += (uint32_t)nr_rxf_level_term(nr_rxf_c16(h[0], h[1]), x);
    }
    const int32_t v = nr_rxf_level_avg((int32_t)sum, len);
    if (avg)
      avg[a] = v;
    avgs = std::max(avgs, v);
  }
  *log2_maxh = nr_rxf_log2_maxh(avgs, n_rx);
  return 0;
}

int32_t nrLDPC_hip_ulsch_channel_compensation(const int16_t *rxFext, const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride,
                                              const nrLDPC_hip_rx_seg_t *seg, uint32_t n_seg, const int32_t *shift, int16_t *records, int32_t mem,
                                              void *stream)
{
  if (rxf_check_common("channel_compensation", n_rx, mem) != 0)
    return -1;
  if (n_seg && (!rxFext || !chFext || !seg || !shift || !records))
    return set_error("null argument");
  RxFrontPlan p;
  if (rxf_plan_compensation(seg, n_seg, n_rx, ant_stride, p) != 0)
    return -1;
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    if (n_seg == 0)
      return 0;
    const int ord = scr_device_ordinal(records);
    if (ord < 0 || !rxf_dev_ok(records, ord) || !rxf_dev_ok(rxFext, ord) || !rxf_dev_ok(chFext, ord) || !rxf_dev_ok(shift, ord))
      return set_error("channel_compensation: DEVICE mem needs every array in device memory of one GPU, 4-byte aligned");
    Device *dv = device_for_ordinal(ord);
    if (!dv)
      return -1;
    UseDevice use(*dv);
    if (rxf_check_stream("channel_compensation", static_cast<hipStream_t>(stream)) != 0)
      return -1;
    if (p.jobs.empty())
      return 0;
    rxf_place(p, 0, 0, 0, reinterpret_cast<uintptr_t>(records) >> 2);
    TbCtx &c = tls_tb;
    hipStream_t s;
    const size_t bytes = rxf_jobs_bytes(p);
    if (tb_begin(s, static_cast<hipStream_t>(stream), false) != 0 || tb_wait_upload(c) != 0 || c.jobs_h.ensure(bytes) != 0 ||
        c.jobs_d.ensure(bytes) != 0)
      return -1;
    rxf_write_jobs(p, c.jobs_h.p);
    if (tb_upload_jobs(c, c.jobs_d.p, bytes, s) != 0)
      return -1;
    HIP_TRY(nr_launch_rx_compensation(reinterpret_cast<const rx_front_wg *>(c.jobs_d.p), (uint32_t)p.wgs.size(),
                                      reinterpret_cast<const rx_front_seg_job *>(c.jobs_d.p + align_up(p.wgs.size() * sizeof(rx_front_wg), 16)),
                                      reinterpret_cast<const uint32_t *>(rxFext), reinterpret_cast<const uint32_t *>(chFext), n_rx, ant_stride, shift,
                                      reinterpret_cast<uint32_t *>(records), s));
    return 0;
  }
  if (p.jobs.empty())
    return 0;
  if (ensure_ready() != 0)
    return -1;
  UseDevice use(g.dev[0]);
  ThreadCtx &c = tls_ctx;
  /* the device works on copies of the c16 ranges the segments reach; the output keeps the caller's alignment phase */
  const uint64_t out_pad = p.out_lo & 3u;
  rxf_place(p, p.rx_lo, p.ch_lo, p.out_lo - out_pad, 0);
  const size_t jobs_b = rxf_jobs_bytes(p), shift_b = align_up((size_t)p.n_shift * 4u, 16), rx_b = align_up((size_t)(p.rx_hi - p.rx_lo) * 4u, 16),
               ch_b = align_up((size_t)(p.ch_hi - p.ch_lo) * 4u, 16), out_b = (size_t)(p.out_hi - p.out_lo + out_pad) * 4u;
  if (c.ensure(jobs_b + shift_b + rx_b + ch_b, out_b) != 0)
    return -1;
  rxf_write_jobs(p, c.h_in);
  memcpy(c.h_in + jobs_b, shift, (size_t)p.n_shift * 4u);
  memcpy(c.h_in + jobs_b + shift_b, rxFext + 2 * p.rx_lo, (size_t)(p.rx_hi - p.rx_lo) * 4u);
  memcpy(c.h_in + jobs_b + shift_b + rx_b, chFext + 2 * p.ch_lo, (size_t)(p.ch_hi - p.ch_lo) * 4u);
  HIP_TRY(hipMemcpyAsync(c.d_in, c.h_in, jobs_b + shift_b + rx_b + ch_b, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(nr_launch_rx_compensation(reinterpret_cast<const rx_front_wg *>(c.d_in), (uint32_t)p.wgs.size(),
                                    reinterpret_cast<const rx_front_seg_job *>(c.d_in + align_up(p.wgs.size() * sizeof(rx_front_wg), 16)),
                                    reinterpret_cast<const uint32_t *>(c.d_in + jobs_b + shift_b),
                                    reinterpret_cast<const uint32_t *>(c.d_in + jobs_b + shift_b + rx_b), n_rx, ant_stride,
                                    reinterpret_cast<const int32_t *>(c.d_in + jobs_b), reinterpret_cast<uint32_t *>(c.d_out), c.stream));
  HIP_TRY(hipMemcpyAsync(c.h_out, c.d_out, out_b, hipMemcpyDeviceToHost, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  /* only the segments' entries go to the caller's array */
  for (const rx_front_seg_job &j : p.jobs)
    for (uint32_t k = 0; k < j.Qm / 2u; k++) {
      const uint64_t at = j.out_off + (uint64_t)k * j.plane;
      memcpy(records + 2 * (at + p.out_lo - out_pad), c.h_out + 4u * at, (size_t)j.nb_re * 4u);
    }
  return 0;
}

int32_t nrLDPC_hip_ulsch_channel_level(const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, const nrLDPC_hip_rx_seg_t *first_sym, uint32_t n_tb,
                                       int32_t *log2_maxh, int32_t mem, void *stream)
{
  if (rxf_check_common("channel_level", n_rx, mem) != 0)
    return -1;
  if (n_tb && (!chFext || !first_sym || !log2_maxh))
    return set_error("null argument");
  if (n_tb == 0)
    return 0;
  RxFrontPlan p;
  if (rxf_plan_level(first_sym, n_tb, n_rx, ant_stride, p) != 0)
    return -1;
  /* the blocks' jobs, then their zeroed state (maxima, counters) */
  const size_t jobs_b = align_up((size_t)n_tb * sizeof(rx_front_lvl_job), 16), state_b = align_up((size_t)n_tb * 8u, 16);
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    const int ord = scr_device_ordinal(log2_maxh);
    if (ord < 0 || !rxf_dev_ok(log2_maxh, ord) || !rxf_dev_ok(chFext, ord))
      return set_error("channel_level: DEVICE mem needs every array in device memory of one GPU, 4-byte aligned");
    Device *dv = device_for_ordinal(ord);
    if (!dv)
      return -1;
    UseDevice use(*dv);
    if (rxf_check_stream("channel_level", static_cast<hipStream_t>(stream)) != 0)
      return -1;
    TbCtx &c = tls_tb;
    hipStream_t s;
    if (tb_begin(s, static_cast<hipStream_t>(stream), false) != 0 || tb_wait_upload(c) != 0 || c.jobs_h.ensure(jobs_b + state_b) != 0 ||
        c.jobs_d.ensure(jobs_b + state_b) != 0)
      return -1;
    memcpy(c.jobs_h.p, p.lvl.data(), (size_t)n_tb * sizeof(rx_front_lvl_job));
    memset(c.jobs_h.p + jobs_b, 0, state_b);
    if (tb_upload_jobs(c, c.jobs_d.p, jobs_b + state_b, s) != 0)
      return -1;
    HIP_TRY(nr_launch_rx_level(reinterpret_cast<const rx_front_lvl_job *>(c.jobs_d.p), n_tb, reinterpret_cast<const uint32_t *>(chFext), n_rx,
                               ant_stride, reinterpret_cast<int32_t *>(c.jobs_d.p + jobs_b), log2_maxh, s));
    return 0;
  }
  if (ensure_ready() != 0)
    return -1;
  UseDevice use(g.dev[0]);
  ThreadCtx &c = tls_ctx;
  for (rx_front_lvl_job &j : p.lvl)
    j.ch_off -= p.ch_lo;
  const size_t ch_b = (size_t)(p.ch_hi - p.ch_lo) * 4u;
  if (c.ensure(jobs_b + state_b + align_up(ch_b, 16), (size_t)n_tb * 4u) != 0)
    return -1;
  memcpy(c.h_in, p.lvl.data(), (size_t)n_tb * sizeof(rx_front_lvl_job));
  memset(c.h_in + jobs_b, 0, state_b);
  memcpy(c.h_in + jobs_b + state_b, chFext + 2 * p.ch_lo, ch_b);
  HIP_TRY(hipMemcpyAsync(c.d_in, c.h_in, jobs_b + state_b + ch_b, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(nr_launch_rx_level(reinterpret_cast<const rx_front_lvl_job *>(c.d_in), n_tb, reinterpret_cast<const uint32_t *>(c.d_in + jobs_b + state_b),
                             n_rx, ant_stride, reinterpret_cast<int32_t *>(c.d_in + jobs_b), reinterpret_cast<int32_t *>(c.d_out), c.stream));
  HIP_TRY(hipMemcpyAsync(c.h_out, c.d_out, (size_t)n_tb * 4u, hipMemcpyDeviceToHost, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  memcpy(log2_maxh, c.h_out, (size_t)n_tb * 4u);
  return 0;
}

} /* extern "C" */
