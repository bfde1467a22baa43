/*
 * tx_precode_api.inc.cpp -- PDSCH resource mapping with precoding, layers to antenna ports through per-PRG matrices: the GPU
 * call, its CPU check form and the descriptor builder (included into ldpc_api.cpp behind tx_map_api.inc.cpp, whose scatter it
 * uses).  The arithmetic: nr_pdsch_map.h; the kernel: tb_tx_map.hip.  The caller's PMI lists are resolved against the matrix
 * table before the launch (txp_plan of tx_map_plan.h), so the device searches nothing; the resolved lists and the matrices in use
 * travel with the descriptors in the call's one upload (job_layout.h).
 */

namespace {

/* one descriptor, one antenna on the CPU: lay = the symbol's stretch of layer 0's plane, sym = the symbol's subcarrier 0 */
int txp_host_one(const nrLDPC_hip_pdsch_map_seg_t &g, const tx_map_prg &pg, const TxPrecodePlan &pp, const uint32_t *lay, uint32_t ant, uint32_t *sym)
{
  const uint32_t n_re = 12u * g.rb_size, last = nr_pdm_last_pmask(g.pattern);
  nr_pdm_sym s[NR_PDM_MAX_LAYERS];
  for (uint32_t l = 0; l < g.Nl; l++)
    s[l] = nr_pdm_sym_make(g.pattern, g.ncdm, g.l_prime, g.port[l], g.amp);
  std::vector<uint32_t> gold;
  uint32_t w0 = 0;
  if (g.pattern != NR_PDM_FULL && !dmrs_gold_words(g.c_init, g.dmrs_offset, nr_pdm_count(last, n_re) + 1u, gold, w0))
    return set_error("pdsch_precode_host: the Gold sequence could not be generated");
  for (uint32_t i = 0; i < n_re; i++) {
    uint64_t bits = 0;
    const uint32_t jlo = nr_pdm_count(last, i);
    if (g.pattern != NR_PDM_FULL)
      bits = dmrs_bits(gold, w0, g.dmrs_offset + jlo);
    const uint32_t pmx = pp.pmx[pg.pmx_off + (i / 12u) / pg.prg_size];
    uint32_t m[NR_PDM_MAX_LAYERS] = {0, 0, 0, 0}, wt[NR_PDM_MAX_LAYERS] = {0, 0, 0, 0};
    for (uint32_t l = 0; l < g.Nl; l++) {
      m[l] = nr_pdm_re(&s[l], lay + (uint64_t)l * g.plane, i, bits, jlo);
      if (pmx)
        wt[l] = pp.mats[pmx - 1u].w[l][ant];
    }
    sym[nr_pdm_wrap(g.start_re, i, g.fft_size)] = nr_pdm_antenna(m, wt, g.Nl, ant, pmx);
  }
  return 0;
}

/* the launches over the tables' device copy at base */
int txp_launch(const TxMapPlan &p, const TxPrecodeTables &t, const uint8_t *base, const uint32_t *lay, uint32_t *tx, uint64_t tx_stride, hipStream_t s)
{
  const tx_map_wg *wgs = reinterpret_cast<const tx_map_wg *>(base + t.wgs);
  for (uint32_t pattern = 0; pattern < NR_PDM_PATTERNS; pattern++) {
    HIP_TRY(nr_launch_tx_precode(pattern, wgs, p.n_wg[pattern], reinterpret_cast<const tx_map_job *>(base + t.jobs),
                                 reinterpret_cast<const tx_map_prg *>(base + t.prgs), reinterpret_cast<const uint16_t *>(base + t.pmx),
                                 reinterpret_cast<const tx_map_pm *>(base + t.mats), lay, tx, tx_stride, s));
    wgs += p.n_wg[pattern];
  }
  return 0;
}

} // namespace

extern "C" {

int32_t nrLDPC_hip_pdsch_precode_host(const int16_t *layers, const nrLDPC_hip_pdsch_map_seg_t *seg, const nrLDPC_hip_pdsch_prg_t *prg,
                                      const uint16_t *pmi_list, uint32_t n_pmi, const nrLDPC_hip_pm_pdu_t *pm, uint32_t n_pm, uint32_t n_tx, uint32_t ant,
                                      int16_t *txdataF)
{
  if (!layers || !seg || !prg || !txdataF)
    return set_error("null argument");
  if (n_tx < 1 || n_tx > NR_PDM_MAX_TX)
    return set_error("pdsch_precode_host: n_tx must be 1..8");
  if (ant >= n_tx)
    return set_error("pdsch_precode_host: ant must be below n_tx");
  if (txm_check_seg("pdsch_precode_host", *seg) != 0)
    return -1;
  if (n_tx < seg->Nl)
    return set_error("pdsch_precode_host: n_tx is below a descriptor's Nl");
  TxPrecodePlan pp;
  if (txp_plan("pdsch_precode_host", seg, prg, 1, n_tx, pmi_list, n_pmi, pm, n_pm, pp) != 0)
    return -1;
  return txp_host_one(*seg, pp.prgs[0], pp, reinterpret_cast<const uint32_t *>(layers) + seg->lay_off / 2u + seg->sym_off, ant,
                      reinterpret_cast<uint32_t *>(txdataF) + seg->tx_off);
}

int32_t nrLDPC_hip_pdsch_precode_segments(const nrLDPC_hip_pdsch_alloc_t *alloc, const nrLDPC_hip_pdsch_prg_t *alloc_prg, uint32_t n_alloc, uint32_t n_pmi,
                                          nrLDPC_hip_pdsch_map_seg_t *seg_out, nrLDPC_hip_pdsch_prg_t *prg_out, uint32_t cap, uint32_t *n_seg_out)
{
  if (!n_seg_out || (n_alloc && (!alloc || !alloc_prg)) || (cap && (!seg_out || !prg_out)))
    return set_error("null argument");
  std::vector<nrLDPC_hip_pdsch_map_seg_t> segs;
  std::vector<nrLDPC_hip_pdsch_prg_t> prgs;
  for (uint32_t i = 0; i < n_alloc; i++) {
    /* the unit builder's checks and descriptors, allocation by allocation; its refusals keep its name */
    nrLDPC_hip_pdsch_map_seg_t sym[NR_RXG_SYMBOLS];
    uint32_t n = 0;
    if (nrLDPC_hip_pdsch_map_segments(alloc + i, 1, sym, NR_RXG_SYMBOLS, &n) != 0)
      return -1;
    const nrLDPC_hip_pdsch_prg_t &r = alloc_prg[i];
    if (r.prg_size) {
      if (r.pmi_count < (alloc[i].rb_size + r.prg_size - 1u) / r.prg_size)
        return set_error("pdsch_precode_segments: an allocation's PMI range is shorter than ceil(rb_size / prg_size)");
      if ((uint64_t)r.pmi_off + r.pmi_count > n_pmi)
        return set_error("pdsch_precode_segments: an allocation's PMI range reaches outside the PMI list");
    }
    segs.insert(segs.end(), sym, sym + n);
    prgs.insert(prgs.end(), n, r); /* every symbol of the allocation shares the range */
  }
  if (segs.size() > cap)
    return set_error("pdsch_precode_segments: more descriptors than cap");
  if (!prgs.empty())
    memcpy(prg_out, prgs.data(), prgs.size() * sizeof prgs[0]);
  return emit_segments(segs, seg_out, cap, n_seg_out, "pdsch_precode_segments: more descriptors than cap");
}

int32_t nrLDPC_hip_pdsch_resource_mapping_precoded(const int16_t *layers, int16_t *txdataF, uint64_t tx_ant_stride, uint32_t n_tx,
                                                   const nrLDPC_hip_pdsch_map_seg_t *seg, const nrLDPC_hip_pdsch_prg_t *prg, uint32_t n_seg,
                                                   const uint16_t *pmi_list, uint32_t n_pmi, const nrLDPC_hip_pm_pdu_t *pm, uint32_t n_pm, int32_t mem,
                                                   void *stream)
{
  const char *const who = "pdsch_resource_mapping_precoded";
  if (n_tx < 1 || n_tx > NR_PDM_MAX_TX)
    return set_error("pdsch_resource_mapping_precoded: n_tx must be 1..8");
  if (check_mem(who, mem) != 0)
    return -1;
  if (n_seg && (!layers || !txdataF || !seg || !prg))
    return set_error("null argument");
  TxMapPlan p;
  TxPrecodePlan pp;
  if (txm_plan(who, seg, n_seg, n_tx, tx_ant_stride, p) != 0 || txp_plan(who, seg, prg, n_seg, n_tx, pmi_list, n_pmi, pm, n_pm, pp) != 0)
    return -1;
  if (n_seg == 0)
    return 0;
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    DeviceCall dc;
    if (dc.open(who, {{txdataF, 4}, {layers, 4}}, DEV_NEEDS_ALIGNED, stream) != 0 || dc.refuse_capture(who) != 0)
      return -1;
    txm_plan_wgs(seg, n_seg, n_tx, tx_ant_stride, txdataF, p, true);
    const TxPrecodeTables tab(p, pp);
    const uint8_t *base = dc.upload(tab.lay);
    if (!base)
      return -1;
    return txp_launch(p, tab, base, reinterpret_cast<const uint32_t *>(layers), reinterpret_cast<uint32_t *>(txdataF), tx_ant_stride, dc.s);
  }
  StagedCall st;
  if (st.open() != 0)
    return -1;
  /* as the unit call: a copy of the span of the layer planes, a bounce of the span of the grid, the buffers ahead of the table */
  for (uint32_t i = 0; i < n_seg; i++) {
    p.jobs[i].tx_off -= p.out_lo;
    p.jobs[i].lay_off -= p.lay_lo;
  }
  const size_t lay_n = (size_t)(p.lay_hi - p.lay_lo) * 4u, out_b = (size_t)(p.out_hi - p.out_lo) * 4u;
  if (st.ensure(out_b, TxPrecodeTables::bytes(txm_max_wg(seg, n_seg, n_tx), p, pp) + align_up(lay_n, 16)) != 0)
    return -1;
  txm_plan_wgs(seg, n_seg, n_tx, tx_ant_stride, st.d_out(), p, true);
  const TxPrecodeTables tab(p, pp);
  const size_t tab_o = st.take(tab.lay.upload_bytes()), lay_o = st.take(lay_n);
  tab.lay.write(st.h(tab_o));
  memcpy(st.h(lay_o), layers + 2 * p.lay_lo, lay_n);
  const auto launch = [&] {
    return txp_launch(p, tab, st.d(tab_o), reinterpret_cast<const uint32_t *>(st.d(lay_o)), reinterpret_cast<uint32_t *>(st.d_out()), tx_ant_stride,
                      st.stream());
  };
  if (st.run(st.top, launch, out_b) != 0)
    return -1;
  txm_scatter(seg, n_seg, n_tx, tx_ant_stride, st.h_out(), p.out_lo, txdataF);
  return 0;
}

} /* extern "C" */
