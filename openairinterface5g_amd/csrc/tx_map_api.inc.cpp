/*
 * tx_map_api.inc.cpp -- PDSCH resource mapping with DMRS onto the transmit grid: the GPU call, its CPU check forms and the
 * descriptors of a PDSCH allocation (included into ldpc_api.cpp; uses the call scopes and the DMRS helpers of slot_call.inc.cpp).
 * The arithmetic: nr_pdsch_map.h; the kernel: tb_tx_map.hip.  Everything the kernel indexes with is checked before anything is
 * enqueued: the descriptor check, the plan and the workgroup table are tx_map_plan.h's, which the CPU emulation of the kernels
 * shares.
 */
#include "tx_map_plan.h"

namespace {

/* one descriptor, one antenna on the CPU: lay = the symbol's stretch of the layer's plane (NULL: zeros), sym = the symbol's
 * subcarrier 0 */
int txm_host_one(const nrLDPC_hip_pdsch_map_seg_t &g, const uint32_t *lay, uint32_t layer, uint32_t *sym)
{
  const uint32_t n_re = 12u * g.rb_size;
  if (!lay) {
    for (uint32_t i = 0; i < n_re; i++)
      sym[nr_pdm_wrap(g.start_re, i, g.fft_size)] = 0u;
    return 0;
  }
  const nr_pdm_sym s = nr_pdm_sym_make(g.pattern, g.ncdm, g.l_prime, g.port[layer], g.amp);
  std::vector<uint32_t> gold;
  uint32_t w0 = 0;
  /* an RE behind the last pilot asks for the bits of the symbol behind the last one */
  if (g.pattern != NR_PDM_FULL && !dmrs_gold_words(g.c_init, g.dmrs_offset, nr_pdm_count(s.pmask, n_re) + 1u, gold, w0))
    return set_error("pdsch_map_host: the Gold sequence could not be generated");
  for (uint32_t i = 0; i < n_re; i++) {
    uint64_t bits = 0;
    const uint32_t jlo = nr_pdm_count(s.pmask, i);
    if (g.pattern != NR_PDM_FULL)
      bits = dmrs_bits(gold, w0, g.dmrs_offset + jlo);
    sym[nr_pdm_wrap(g.start_re, i, g.fft_size)] = nr_pdm_re(&s, lay, i, bits, jlo);
  }
  return 0;
}

/* the launches over the tables' device copy */
int txm_launch(const TxMapPlan &p, const tx_map_wg *wgs, const tx_map_job *jobs, const uint32_t *lay, uint32_t *tx, uint64_t tx_stride, hipStream_t s)
{
  uint32_t first = 0;
  for (uint32_t pattern = 0; pattern < NR_PDM_PATTERNS; pattern++) {
    HIP_TRY(nr_launch_tx_map(pattern, wgs + first, p.n_wg[pattern], jobs, lay, tx, tx_stride, s));
    first += p.n_wg[pattern];
  }
  return 0;
}

/* HOST mem: the workgroup table at its largest, one piece more per (descriptor, antenna) than the REs alone need */
size_t txm_max_wg(const nrLDPC_hip_pdsch_map_seg_t *seg, uint32_t n_seg, uint32_t n_tx)
{
  size_t max_wg = 0;
  for (uint32_t i = 0; i < n_seg; i++)
    max_wg += (size_t)n_tx * ((12u * (size_t)seg[i].rb_size + 3u) / (NR_TXM_THREADS * NR_TXM_GROUP) + 1u);
  return max_wg;
}
/* HOST mem: only the write set goes from the bounce (its c16 0 = out_lo of the grid) to the caller's array */
void txm_scatter(const nrLDPC_hip_pdsch_map_seg_t *seg, uint32_t n_seg, uint32_t n_tx, uint64_t tx_ant_stride, const uint8_t *bounce, uint64_t out_lo,
                 int16_t *txdataF)
{
  for (uint32_t i = 0; i < n_seg; i++) {
    const uint32_t n_re = 12u * seg[i].rb_size, first = std::min(n_re, seg[i].fft_size - seg[i].start_re);
    for (uint32_t a = 0; a < n_tx; a++) {
      const uint64_t base = seg[i].tx_off + (uint64_t)a * tx_ant_stride;
      memcpy(txdataF + 2 * (base + seg[i].start_re), bounce + 4u * (base + seg[i].start_re - out_lo), (size_t)first * 4u);
      if (first < n_re)
        memcpy(txdataF + 2 * base, bounce + 4u * (base - out_lo), (size_t)(n_re - first) * 4u);
    }
  }
}

} // namespace

extern "C" {

int32_t nrLDPC_hip_pdsch_dmrs_host(uint32_t c_init, uint32_t dmrs_offset, uint32_t n, int16_t *out)
{
  if (n && !out)
    return set_error("null argument");
  if (c_init >> 31)
    return set_error("pdsch_dmrs_host: c_init must be below 2^31");
  if (dmrs_offset > (1u << 20) || n > (1u << 20))
    return set_error("pdsch_dmrs_host: dmrs_offset or n above 2^20");
  if (n == 0)
    return 0;
  std::vector<uint32_t> gold;
  uint32_t w0;
  if (!dmrs_gold_words(c_init, dmrs_offset, n, gold, w0))
    return set_error("pdsch_dmrs_host: the Gold sequence could not be generated");
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t c = nr_qam_point(2u, (uint32_t)dmrs_bits(gold, w0, dmrs_offset + k) & 3u);
    out[2 * (size_t)k] = (int16_t)(c & 0xffffu);
    out[2 * (size_t)k + 1] = (int16_t)(c >> 16);
  }
  return 0;
}

int32_t nrLDPC_hip_pdsch_map_host(const int16_t *layers, const nrLDPC_hip_pdsch_map_seg_t *seg, int32_t layer, int16_t *txdataF)
{
  if (!seg || !txdataF || (layer >= 0 && !layers))
    return set_error("null argument");
  if (txm_check_seg("pdsch_map_host", *seg) != 0)
    return -1;
  if (layer >= (int32_t)seg->Nl)
    return set_error("pdsch_map_host: layer must be below Nl, or negative for an antenna behind the layers");
  const uint32_t *lay = layer < 0 ? nullptr : reinterpret_cast<const uint32_t *>(layers) + seg->lay_off / 2u + (uint64_t)layer * seg->plane + seg->sym_off;
  return txm_host_one(*seg, lay, layer < 0 ? 0u : (uint32_t)layer, reinterpret_cast<uint32_t *>(txdataF) + seg->tx_off);
}

int32_t nrLDPC_hip_pdsch_map_segments(const nrLDPC_hip_pdsch_alloc_t *alloc, uint32_t n_alloc, nrLDPC_hip_pdsch_map_seg_t *seg_out, uint32_t cap,
                                      uint32_t *n_seg_out)
{
  if (!n_seg_out || (n_alloc && !alloc) || (cap && !seg_out))
    return set_error("null argument");
  std::vector<nrLDPC_hip_pdsch_map_seg_t> segs;
  for (uint32_t i = 0; i < n_alloc; i++) {
    const nrLDPC_hip_pdsch_alloc_t &a = alloc[i];
    const uint32_t N = a.fft_size, type = a.dmrs_config_type;
    if (alloc_check_symbols("pdsch_map_segments", a.start_symbol, a.nr_of_symbols) != 0)
      return -1;
    if (a.Nl < 1 || a.Nl > NR_PDM_MAX_LAYERS)
      return set_error("pdsch_map_segments: Nl must be 1..4");
    if (type > 1)
      return set_error("pdsch_map_segments: dmrs_config_type must be 0 (type 1) or 1 (type 2)");
    if (a.amp < 1 || a.amp > 32767)
      return set_error("pdsch_map_segments: amp must be 1..32767");
    if (alloc_check_width("pdsch_map_segments", a.rb_size, N, a.first_carrier_offset) != 0)
      return -1;
    if (a.scid > 1)
      return set_error("pdsch_map_segments: scid must be 0 or 1");
    if (a.dl_dmrs_scrambling_id > 0xffffu)
      return set_error("pdsch_map_segments: dl_dmrs_scrambling_id above 65535");
    if (a.slot >= 160)
      return set_error("pdsch_map_segments: slot must be below 160");
    if ((uint64_t)a.bwp_start + a.rb_start > (1u << 16))
      return set_error("pdsch_map_segments: bwp_start + rb_start above 2^16");
    /* get_dmrs_port (nr_common.c:494-511): layer l takes the l-th set bit; an empty bitmap (DCI 1_0) is port 0 */
    uint8_t port[NR_PDM_MAX_LAYERS] = {0, 0, 0, 0};
    for (uint32_t l = 0; l < a.Nl; l++) {
      int32_t found = -1, p = a.dmrs_ports == 0 ? 0 : -1;
      for (uint32_t b = 0; b < 12u && p < 0; b++)
        if (((a.dmrs_ports >> b) & 1u) && ++found == (int32_t)l)
          p = (int32_t)b;
      if (p < 0)
        return set_error("pdsch_map_segments: dmrs_ports has no port for a layer");
      port[l] = (uint8_t)p;
    }
    uint32_t l_overline = 0; /* get_l0 (nr_sch_dmrs.c:89-98) */
    while (l_overline < 14u && !((a.dl_dmrs_symb_pos >> l_overline) & 1u))
      l_overline++;
    uint32_t l_prime = 0, m = 0;
    for (uint32_t sym = a.start_symbol; sym < a.start_symbol + a.nr_of_symbols; sym++) {
      nrLDPC_hip_pdsch_map_seg_t g;
      memset(&g, 0, sizeof g);
      const bool dmrs = (a.dl_dmrs_symb_pos >> sym) & 1u;
      g.pattern = (uint8_t)(dmrs ? (type == 0 ? NR_PDM_DMRS1 : NR_PDM_DMRS2) : NR_PDM_FULL);
      g.Nl = (uint8_t)a.Nl;
      g.amp = (int16_t)a.amp;
      g.fft_size = N;
      g.start_re = nr_rxg_start_re(a.first_carrier_offset, a.bwp_start, a.rb_start, N);
      g.rb_size = a.rb_size;
      g.plane = a.plane;
      g.sym_off = m;
      g.tx_off = a.tx_slot_off + (uint64_t)sym * N;
      g.lay_off = a.lay_off;
      if (dmrs) {
        if (a.num_dmrs_cdm_grps_no_data > 255u)
          return set_error("pdsch_map_segments: num_dmrs_cdm_grps_no_data must be 1..2 for type 1 and 1..3 for type 2");
        g.ncdm = (uint8_t)a.num_dmrs_cdm_grps_no_data;
        if (sym == l_overline + 1u) /* :264-269 */
          l_prime = 1;
        else if (sym > l_overline + 1u) {
          l_overline = sym;
          l_prime = 0;
        }
        g.l_prime = (uint8_t)l_prime;
        memcpy(g.port, port, sizeof port);
        g.dmrs_offset = (a.rb_start + (a.si_rnti ? 0u : a.bwp_start)) * (type == 0 ? 6u : 4u); /* :260-263 */
        g.c_init = dmrs_c_init(a.slot, sym, a.dl_dmrs_scrambling_id, a.scid);
      }
      uint32_t pm, dm;
      nr_pdm_masks(g.pattern, g.ncdm, nr_pdm_delta(g.pattern, port[0] < nr_pdm_ports(g.pattern) ? port[0] : 0u), &pm, &dm);
      g.nb_re = a.rb_size * nr_pdm_popc(dm);
      if ((uint64_t)m + g.nb_re > a.plane)
        return set_error("pdsch_map_segments: the data REs of the symbols add up to more than plane");
      if (txm_check_seg("pdsch_map_segments", g) != 0)
        return -1;
      m += g.nb_re;
      segs.push_back(g);
    }
    if (m != a.plane)
      return set_error("pdsch_map_segments: the data REs of the symbols do not add up to plane");
  }
  return emit_segments(segs, seg_out, cap, n_seg_out, "pdsch_map_segments: more descriptors than cap");
}

int32_t nrLDPC_hip_pdsch_resource_mapping(const int16_t *layers, int16_t *txdataF, uint64_t tx_ant_stride, uint32_t n_tx,
                                          const nrLDPC_hip_pdsch_map_seg_t *seg, uint32_t n_seg, int32_t mem, void *stream)
{
  if (n_tx < 1 || n_tx > NR_PDM_MAX_TX)
    return set_error("pdsch_resource_mapping: n_tx must be 1..8");
  if (check_mem("pdsch_resource_mapping", mem) != 0)
    return -1;
  if (n_seg && (!layers || !txdataF || !seg))
    return set_error("null argument");
  TxMapPlan p;
  if (txm_plan("pdsch_resource_mapping", seg, n_seg, n_tx, tx_ant_stride, p) != 0)
    return -1;
  if (n_seg == 0)
    return 0;
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    DeviceCall dc;
    if (dc.open("pdsch_resource_mapping", {{txdataF, 4}, {layers, 4}}, DEV_NEEDS_ALIGNED, stream) != 0 ||
        dc.refuse_capture("pdsch_resource_mapping") != 0)
      return -1;
    txm_plan_wgs(seg, n_seg, n_tx, tx_ant_stride, txdataF, p);
    const auto tab = table2(p.wgs, p.jobs);
    uint8_t *base = dc.upload(tab);
    if (!base)
      return -1;
    return txm_launch(p, tab.first(base), tab.second(base), reinterpret_cast<const uint32_t *>(layers), reinterpret_cast<uint32_t *>(txdataF),
                      tx_ant_stride, dc.s);
  }
  StagedCall st;
  if (st.open() != 0)
    return -1;
  /* the device reads a copy of the span of the layer planes the descriptors reach and works on a bounce of the span of the grid
   * from the lowest to the highest c16 written */
  for (uint32_t i = 0; i < n_seg; i++) {
    p.jobs[i].tx_off -= p.out_lo;
    p.jobs[i].lay_off -= p.lay_lo;
  }
  const size_t lay_n = (size_t)(p.lay_hi - p.lay_lo) * 4u, out_b = (size_t)(p.out_hi - p.out_lo) * 4u;
  /* the workgroup table's phases depend on where the bounce lies, so the buffers come first, for a table of the largest size:
   * one piece more per (descriptor, antenna) at the most */
  const size_t max_wg = txm_max_wg(seg, n_seg, n_tx);
  if (st.ensure(out_b, Table2<tx_map_wg, const tx_map_job>::bytes(max_wg, p.jobs.size()) + align_up(lay_n, 16)) != 0)
    return -1;
  txm_plan_wgs(seg, n_seg, n_tx, tx_ant_stride, st.d_out(), p);
  const auto tab = table2(p.wgs, p.jobs);
  const size_t tab_o = st.take(tab.bytes()), lay_o = st.take(lay_n);
  tab.write(st.h(tab_o));
  memcpy(st.h(lay_o), layers + 2 * p.lay_lo, lay_n);
  const auto launch = [&] {
    return txm_launch(p, tab.first(st.d(tab_o)), tab.second(st.d(tab_o)), reinterpret_cast<const uint32_t *>(st.d(lay_o)),
                      reinterpret_cast<uint32_t *>(st.d_out()), tx_ant_stride, st.stream());
  };
  if (st.run(st.top, launch, out_b) != 0)
    return -1;
  txm_scatter(seg, n_seg, n_tx, tx_ant_stride, st.h_out(), p.out_lo, txdataF);
  return 0;
}

} /* extern "C" */
