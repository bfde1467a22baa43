/*
 * tx_map_plan.h -- what the PDSCH resource mapping calls (unit and precoded) derive from their descriptors before anything is
 * enqueued: the descriptor check, the job list, the ranges of the layer planes and of the grid they reach, the workgroup table of
 * tb_tx_map.hip with its jumped Gold registers, and for the precoded call the resolved PMI lists, the matrices in use and the
 * layout of the call's one job buffer.  Plain arithmetic (slot_plan.h): tx_map_api.inc.cpp and tx_precode_api.inc.cpp run it in
 * front of their DEVICE and HOST scopes, and the CPU emulation of the kernels (tests/emul/) runs the same code.
 */
#ifndef TX_MAP_PLAN_H
#define TX_MAP_PLAN_H
#include <map>
#include "slot_plan.h"
#include "rx_chest_plan.h" /* che_fft_ok, che_gold_tables */
#include "job_layout.h"
#include "nr_pdsch_map.h"
#include "nr_gold.h"
#include "tb_tx_map.h"

namespace {

/* ---- the unit call (tx_map_api.inc.cpp) ---- */
int txm_check_seg(const char *who, const nrLDPC_hip_pdsch_map_seg_t &g)
{
  const std::string w(who);
  if (g.pattern >= NR_PDM_PATTERNS)
    return set_error((w + ": pattern must be FULL, DMRS1 or DMRS2").c_str());
  if (g.Nl < 1 || g.Nl > NR_PDM_MAX_LAYERS)
    return set_error((w + ": Nl must be 1..4").c_str());
  if (g.amp <= 0)
    return set_error((w + ": amp must be positive").c_str());
  if (!che_fft_ok(g.fft_size))
    return set_error((w + ": fft_size must be 128, 256, 512, 1024, 1536, 2048, 4096, 6144 or 8192").c_str());
  if (g.rb_size == 0)
    return set_error((w + ": rb_size is 0").c_str());
  if ((uint64_t)g.rb_size * 12u > g.fft_size)
    return set_error((w + ": the allocation is wider than fft_size").c_str());
  if (g.start_re >= g.fft_size)
    return set_error((w + ": start_re must be below fft_size").c_str());
  if (g.lay_off & 1u)
    return set_error((w + ": lay_off must be even").c_str());
  if (g.pattern != NR_PDM_FULL) {
    if (g.ncdm < 1 || g.ncdm > nr_pdm_max_ncdm(g.pattern))
      return set_error((w + ": ncdm must be 1..2 for type 1 and 1..3 for type 2").c_str());
    if (g.l_prime > 1)
      return set_error((w + ": l_prime must be 0 or 1").c_str());
    for (uint32_t l = 0; l < g.Nl; l++)
      if (g.port[l] >= nr_pdm_ports(g.pattern))
        return set_error((w + ": port must be 0..7 for type 1 and 0..11 for type 2").c_str());
    if (g.c_init >> 31)
      return set_error((w + ": c_init must be below 2^31").c_str());
    if (g.dmrs_offset > (1u << 20))
      return set_error((w + ": dmrs_offset above 2^20").c_str());
  }
  for (uint32_t l = 0; l < g.Nl; l++) {
    uint32_t pm, dm;
    nr_pdm_masks(g.pattern, g.ncdm, nr_pdm_delta(g.pattern, g.port[l]), &pm, &dm);
    if (g.nb_re != g.rb_size * nr_pdm_popc(dm))
      return set_error((w + ": nb_re is not the number of data REs of the pattern (for every layer's port)").c_str());
  }
  if ((uint64_t)g.sym_off + g.nb_re > g.plane)
    return set_error((w + ": sym_off + nb_re is above plane").c_str());
  return 0;
}

struct TxMapPlan {
  std::vector<tx_map_job> jobs;
  std::vector<tx_map_wg> wgs; /* sorted by pattern */
  uint32_t n_wg[NR_PDM_PATTERNS] = {0, 0, 0};
  uint64_t lay_lo = UINT64_MAX, lay_hi = 0, out_lo = UINT64_MAX, out_hi = 0; /* c16 */
};

/* checks and ranges; the workgroup table needs the address the grid is written at (txm_plan_wgs) */
int txm_plan(const char *who, const nrLDPC_hip_pdsch_map_seg_t *seg, uint32_t n_seg, uint32_t n_tx, uint64_t tx_stride, TxMapPlan &p)
{
  std::vector<Range64> out;
  p.jobs.resize(n_seg);
  for (uint32_t i = 0; i < n_seg; i++) {
    const nrLDPC_hip_pdsch_map_seg_t &g = seg[i];
    if (txm_check_seg(who, g) != 0)
      return -1;
    if (n_tx < g.Nl)
      return set_error((std::string(who) + ": n_tx is below a descriptor's Nl").c_str());
    const uint64_t lay0 = g.lay_off / 2u + g.sym_off;
    p.lay_lo = std::min(p.lay_lo, lay0);
    p.lay_hi = std::max(p.lay_hi, lay0 + (uint64_t)(g.Nl - 1u) * g.plane + g.nb_re);
    const uint32_t n_re = 12u * g.rb_size, first = std::min(n_re, g.fft_size - g.start_re);
    for (uint32_t a = 0; a < n_tx; a++) {
      const uint64_t base = g.tx_off + (uint64_t)a * tx_stride;
      out.push_back(Range64{base + g.start_re, base + g.start_re + first});
      if (first < n_re)
        out.push_back(Range64{base, base + (n_re - first)});
    }
    tx_map_job &j = p.jobs[i];
    memset(&j, 0, sizeof j);
    j.tx_off = g.tx_off;
    j.lay_off = lay0;
    j.plane = g.plane;
    j.fft_size = g.fft_size;
    j.start_re = g.start_re;
    j.n_re = n_re;
    j.dmrs_offset = g.dmrs_offset;
    j.Nl = g.Nl;
    j.ncdm = g.ncdm;
    j.l_prime = g.l_prime;
    j.amp = g.amp;
    for (uint32_t l = 0; l < g.Nl; l++)
      j.ports |= (uint32_t)g.port[l] << (8u * l);
  }
  if (ranges_overlap(out, p.out_lo, p.out_hi))
    return set_error((std::string(who) + ": the output ranges of two (descriptor, antenna) pairs overlap").c_str());
  return 0;
}

/* the workgroup table, pattern by pattern; tx = the address the kernel is given, the jobs' tx_off as they will be launched.
 * precoded: every antenna needs the pilots of every layer, so its Gold registers stand where the port with the latest pilots is */
void txm_plan_wgs(const nrLDPC_hip_pdsch_map_seg_t *seg, uint32_t n_seg, uint32_t n_tx, uint64_t tx_stride, const void *tx, TxMapPlan &p,
                  bool precoded = false)
{
  const uint64_t word0 = (uint64_t)(reinterpret_cast<uintptr_t>(tx) >> 2);
  for (uint32_t pattern = 0; pattern < NR_PDM_PATTERNS; pattern++)
    for (uint32_t i = 0; i < n_seg; i++) {
      const nrLDPC_hip_pdsch_map_seg_t &g = seg[i];
      if (g.pattern != pattern)
        continue;
      const tx_map_job &j = p.jobs[i];
      for (uint32_t a = 0; a < n_tx; a++) {
        tx_map_wg w{};
        w.job = i;
        w.ant = a;
        w.phase = (uint32_t)((word0 + j.tx_off + (uint64_t)a * tx_stride + j.start_re) & 3u);
        uint32_t pm = 0, dm = 0;
        if (precoded)
          pm = nr_pdm_last_pmask(pattern);
        else if (a < g.Nl)
          nr_pdm_masks(pattern, g.ncdm, nr_pdm_delta(pattern, g.port[a]), &pm, &dm);
        for (uint32_t q = 0; (uint64_t)q * NR_TXM_THREADS * NR_TXM_GROUP < (uint64_t)j.n_re + w.phase; q++) {
          w.piece = q;
          if (pm) {
            const uint32_t i_first = q ? q * NR_TXM_THREADS * NR_TXM_GROUP - w.phase : 0u;
            w.w0 = (2u * (g.dmrs_offset + nr_pdm_count(pm, i_first))) >> 5;
            nr_gold_jump(&che_gold_tables(), g.c_init, w.w0, &w.x1, &w.x2);
          }
          p.wgs.push_back(w);
          p.n_wg[pattern]++;
        }
      }
    }
}

/* ---- the precoded call (tx_precode_api.inc.cpp) ---- */
struct TxPrecodePlan {
  std::vector<tx_map_prg> prgs; /* parallel to the descriptors */
  std::vector<uint16_t> pmx;    /* per PRG: 0 = unit, else 1 + index into mats */
  std::vector<tx_map_pm> mats;  /* the matrices in use */
};

int txp_plan(const char *who, const nrLDPC_hip_pdsch_map_seg_t *seg, const nrLDPC_hip_pdsch_prg_t *prg, uint32_t n_seg, uint32_t n_tx,
             const uint16_t *pmi_list, uint32_t n_pmi, const nrLDPC_hip_pm_pdu_t *pm, uint32_t n_pm, TxPrecodePlan &pp)
{
  const std::string w(who);
  std::map<uint16_t, uint32_t> by_idx;
  for (uint32_t t = 0; pm && t < n_pm; t++) {
    if (pm[t].pm_idx == 0)
      return set_error((w + ": pm_idx 0 in the precoding-matrix table (0 is the unit matrix)").c_str());
    if (!by_idx.emplace(pm[t].pm_idx, t).second)
      return set_error((w + ": a pm_idx appears twice in the precoding-matrix table").c_str());
  }
  std::vector<int32_t> slot_of(pm ? n_pm : 0u, -1); /* table entry -> index into mats */
  pp.prgs.resize(n_seg);
  for (uint32_t i = 0; i < n_seg; i++) {
    const nrLDPC_hip_pdsch_map_seg_t &g = seg[i];
    const nrLDPC_hip_pdsch_prg_t &r = prg[i];
    tx_map_prg &o = pp.prgs[i];
    if (r.prg_size == 0) { /* unit precoding: one PRG as wide as the allocation */
      o.prg_size = g.rb_size;
      o.pmx_off = (uint32_t)pp.pmx.size();
      pp.pmx.push_back(0);
      continue;
    }
    const uint32_t need = (g.rb_size + r.prg_size - 1u) / r.prg_size;
    if (r.pmi_count < need)
      return set_error((w + ": a descriptor's PMI range is shorter than ceil(rb_size / prg_size)").c_str());
    if (!pmi_list || (uint64_t)r.pmi_off + r.pmi_count > n_pmi)
      return set_error((w + ": a descriptor's PMI range reaches outside the PMI list").c_str());
    /* the symbols of an allocation share their range: resolved once */
    if (i > 0 && prg[i - 1].prg_size == r.prg_size && prg[i - 1].pmi_off == r.pmi_off && prg[i - 1].pmi_count == r.pmi_count &&
        seg[i - 1].rb_size == g.rb_size && seg[i - 1].Nl == g.Nl) {
      o = pp.prgs[i - 1];
      continue;
    }
    o.prg_size = r.prg_size;
    o.pmx_off = (uint32_t)pp.pmx.size();
    for (uint32_t q = 0; q < need; q++) {
      const uint16_t pmi = pmi_list[r.pmi_off + q];
      if (pmi == 0) {
        pp.pmx.push_back(0);
        continue;
      }
      if (n_tx < 2)
        return set_error((w + ": n_tx must be at least 2 when a PMI is not 0 (no precoding with a single antenna port)").c_str());
      if (!pm)
        return set_error((w + ": a PMI that is not 0 needs the precoding-matrix table").c_str());
      const auto it = by_idx.find(pmi);
      if (it == by_idx.end())
        return set_error((w + ": a PMI that no entry of the precoding-matrix table carries").c_str());
      const nrLDPC_hip_pm_pdu_t &m = pm[it->second];
      if (m.numLayers != g.Nl)
        return set_error((w + ": numLayers of a precoding matrix is not the descriptor's Nl").c_str());
      if (m.num_ant_ports < n_tx || m.num_ant_ports > NR_PDM_MAX_TX)
        return set_error((w + ": num_ant_ports of a precoding matrix must be n_tx..8").c_str());
      if (slot_of[it->second] < 0) {
        if (pp.mats.size() >= 0xffffu)
          return set_error((w + ": more than 65534 precoding matrices in use").c_str());
        slot_of[it->second] = (int32_t)pp.mats.size();
        tx_map_pm d;
        for (uint32_t l = 0; l < NR_PDM_MAX_LAYERS; l++)
          for (uint32_t a = 0; a < NR_PDM_MAX_TX; a++)
            d.w[l][a] = nr_pdm_pack(m.weights[l][a][0], m.weights[l][a][1]);
        pp.mats.push_back(d);
      }
      pp.pmx.push_back((uint16_t)(slot_of[it->second] + 1));
    }
  }
  return 0;
}

/* the call's tables in one job buffer: the workgroup table, the jobs, their PRG records, the resolved PMIs, the matrices */
struct TxPrecodeTables {
  JobLayout lay;
  size_t wgs, jobs, prgs, pmx, mats;
  TxPrecodeTables(const TxMapPlan &p, const TxPrecodePlan &pp)
      : wgs(lay.add(p.wgs)), jobs(lay.add(p.jobs)), prgs(lay.add(pp.prgs)), pmx(lay.add(pp.pmx)), mats(lay.add(pp.mats))
  {
  }
  /* what a table of n_wg workgroups takes at the most */
  static size_t bytes(size_t n_wg, const TxMapPlan &p, const TxPrecodePlan &pp)
  {
    return align_up(n_wg * sizeof(tx_map_wg), 16) + align_up(p.jobs.size() * sizeof(tx_map_job), 16) + align_up(pp.prgs.size() * sizeof(tx_map_prg), 16) +
           align_up(pp.pmx.size() * sizeof(uint16_t), 16) + align_up(pp.mats.size() * sizeof(tx_map_pm), 16);
  }
};

} // namespace
#endif
