/*
 * slot_tx_emul.cpp -- the DL transmit side's slot-level kernels and the standalone QAM passes on the CPU (test infrastructure):
 * tb_tx_map.hip and tb_qam.hip are #included as they are and read against the host shim (hip_host/); see slot_rx_emul.cpp for
 * the idea.  The mapping plans are the library's own (tx_map_plan.h); the QAM passes have no plan, their launchers take the
 * caller's arrays.  An entry point is the DEVICE mem branch of the library call of the same name, in place on the caller's arrays.
 */
#include "slot_emul_common.h"
#include "tx_map_plan.h"
#include "tb_tx_map.hip"
#include "tb_qam.hip"

namespace {

int txm_check_call(const char *who, const int16_t *layers, const int16_t *txdataF, uint32_t n_tx)
{
  if (n_tx < 1 || n_tx > NR_PDM_MAX_TX)
    return set_error((std::string(who) + ": n_tx must be 1..8").c_str());
  if ((reinterpret_cast<uintptr_t>(layers) | reinterpret_cast<uintptr_t>(txdataF)) & 3u)
    return set_error((std::string(who) + ": every array 4-byte aligned").c_str());
  return 0;
}

} // namespace

extern "C" {

int32_t slot_emul_pdsch_resource_mapping(const int16_t *layers, int16_t *txdataF, uint64_t tx_ant_stride, uint32_t n_tx,
                                         const nrLDPC_hip_pdsch_map_seg_t *seg, uint32_t n_seg)
{
  if (txm_check_call("pdsch_resource_mapping", layers, txdataF, n_tx) != 0)
    return -1;
  TxMapPlan p;
  if (txm_plan("pdsch_resource_mapping", seg, n_seg, n_tx, tx_ant_stride, p) != 0)
    return -1;
  if (n_seg == 0)
    return 0;
  txm_plan_wgs(seg, n_seg, n_tx, tx_ant_stride, txdataF, p);
  const auto tab = table2(p.wgs, p.jobs);
  const auto base = tables_copy(tab);
  /* the library's loop (txm_launch of tx_map_api.inc.cpp): one launch a pattern over its part of the workgroup table */
  const tx_map_wg *wgs = tab.first(base.get());
  for (uint32_t pattern = 0; pattern < NR_PDM_PATTERNS; wgs += p.n_wg[pattern++])
    if (launched(nr_launch_tx_map(pattern, wgs, p.n_wg[pattern], tab.second(base.get()), c16(layers), c16(txdataF), tx_ant_stride, nullptr)) != 0)
      return -1;
  return 0;
}

int32_t slot_emul_pdsch_resource_mapping_precoded(const int16_t *layers, int16_t *txdataF, uint64_t tx_ant_stride, uint32_t n_tx,
                                                  const nrLDPC_hip_pdsch_map_seg_t *seg, const nrLDPC_hip_pdsch_prg_t *prg, uint32_t n_seg,
                                                  const uint16_t *pmi_list, uint32_t n_pmi, const nrLDPC_hip_pm_pdu_t *pm, uint32_t n_pm)
{
  const char *const who = "pdsch_resource_mapping_precoded";
  if (txm_check_call(who, layers, txdataF, n_tx) != 0)
    return -1;
  TxMapPlan p;
  TxPrecodePlan pp;
  if (txm_plan(who, seg, n_seg, n_tx, tx_ant_stride, p) != 0 || txp_plan(who, seg, prg, n_seg, n_tx, pmi_list, n_pmi, pm, n_pm, pp) != 0)
    return -1;
  if (n_seg == 0)
    return 0;
  txm_plan_wgs(seg, n_seg, n_tx, tx_ant_stride, txdataF, p, true);
  const TxPrecodeTables tab(p, pp);
  const auto base = tables_copy(tab.lay, tab.lay.upload_bytes());
  /* the library's loop (txp_launch of tx_precode_api.inc.cpp) */
  const uint8_t *b = base.get();
  const tx_map_wg *wgs = reinterpret_cast<const tx_map_wg *>(b + tab.wgs);
  for (uint32_t pattern = 0; pattern < NR_PDM_PATTERNS; wgs += p.n_wg[pattern++])
    if (launched(nr_launch_tx_precode(pattern, wgs, p.n_wg[pattern], reinterpret_cast<const tx_map_job *>(b + tab.jobs),
                                      reinterpret_cast<const tx_map_prg *>(b + tab.prgs), reinterpret_cast<const uint16_t *>(b + tab.pmx),
                                      reinterpret_cast<const tx_map_pm *>(b + tab.mats), c16(layers), c16(txdataF), tx_ant_stride, nullptr)) != 0)
      return -1;
  return 0;
}

/* in: ceil(length / 32) words; out: length / Qm points, 2-byte aligned at the least */
int32_t slot_emul_modulation(const uint32_t *in, uint32_t length, uint32_t Qm, int16_t *out)
{
  if (qam_check_qm(Qm) != 0)
    return -1;
  if (length % Qm)
    return set_error("modulation: length must be a multiple of Qm");
  return launched(nr_launch_modulation(in, length, Qm, out, nullptr));
}

/* the planes beyond Qm / 2 may be null; llr: nb_re Qm int16 */
int32_t slot_emul_ulsch_llr(const int32_t *rxdataF_comp, const int32_t *ul_ch_mag, const int32_t *ul_ch_magb, const int32_t *ul_ch_magc, uint32_t nb_re,
                            uint32_t Qm, int16_t *llr)
{
  if (qam_check_qm(Qm) != 0)
    return -1;
  const int32_t *in[4] = {rxdataF_comp, ul_ch_mag, ul_ch_magb, ul_ch_magc};
  const uint32_t *pl[4] = {nullptr, nullptr, nullptr, nullptr};
  for (uint32_t k = 0; k < Qm / 2u; k++)
    pl[k] = reinterpret_cast<const uint32_t *>(in[k]);
  return launched(nr_launch_ulsch_llr(pl, nb_re, Qm, llr, nullptr));
}

int32_t slot_emul_layer_mapping(const int16_t *in, uint32_t n_symbs, uint32_t Nl, int16_t *out, uint32_t layer_stride)
{
  if (Nl < 1 || Nl > 4 || n_symbs % Nl || layer_stride < n_symbs / Nl)
    return set_error("layer_mapping: Nl 1..4, n_symbs a multiple of it, layer_stride at least n_symbs / Nl");
  return launched(nr_launch_layer_mapping(in, n_symbs, Nl, out, layer_stride, nullptr));
}

/* the symbol encode's scrambling + mapping + layer mapping launch over n_tb job records (tb_chain.h) */
int32_t slot_emul_scramble_map_tb(const tb_sym_tb_job *jobs, uint32_t n_tb, uint32_t max_s, const uint8_t *in, uint8_t *out)
{
  WithThreads t;
  return launched(nr_launch_scramble_map_tb(jobs, n_tb, max_s, in, out, nullptr));
}

} /* extern "C" */
