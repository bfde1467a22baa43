/*
 * slot_rx_emul.cpp -- the UL receive front's kernels on the CPU (test infrastructure): tb_rx_front.hip, tb_rx_mmse.hip and
 * tb_rx_chest.hip are #included as they are and read against the host shim (hip_host/), so every work-item's decomposition --
 * which elements it loads 16 bytes at a time, which word by word, where a quad meets the grid's wrap or the segment's end -- runs as
 * the GPU compiles it.  The plans are the library's own (rx_plan.h, rx_chest_plan.h), the launchers the .hip files' own
 * (the shim's hipLaunchKernelGGL runs the grid).  An entry point is the DEVICE mem branch of the library call of the same name:
 * checks, plan, place at bias 0, tables, launch, in place on the caller's arrays.
 *
 * The arrays are used exactly as given: a caller that passes arrays of the documented extents (include/nrLDPC_hip.h) and runs
 * under AddressSanitizer sees every read or write beyond them (slot_emul_san.cpp).
 */
#include "slot_emul_common.h"
#include <map>
#include "rx_plan.h"
#include "rx_chest_plan.h"
#include "tb_rx_front.hip"
#include "tb_rx_mmse.hip"
#include "tb_rx_chest.hip"

extern "C" {

const char *slot_emul_last_error() { return slot_emul_error.c_str(); }

int32_t slot_emul_channel_compensation(const int16_t *rxFext, const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, const nrLDPC_hip_rx_seg_t *seg,
                                       uint32_t n_seg, const int32_t *shift, int16_t *records)
{
  if (rxf_check_common("channel_compensation", n_rx, NRLDPC_HIP_MEM_DEVICE) != 0)
    return -1;
  if (!aligned4({rxFext, chFext, shift, records}))
    return set_error("channel_compensation: every array 4-byte aligned");
  RxFrontPlan p;
  if (rxf_plan_compensation(seg, n_seg, n_rx, ant_stride, p) != 0)
    return -1;
  if (p.jobs.empty())
    return 0;
  rxf_place(p, 0, 0, 0, reinterpret_cast<uintptr_t>(records) >> 2);
  const auto tab = table2(p.wgs, p.jobs);
  const auto base = tables_copy(tab);
  return launched(nr_launch_rx_compensation(tab.first(base.get()), (uint32_t)p.wgs.size(), tab.second(base.get()), c16(rxFext), c16(chFext), n_rx, ant_stride,
                                            shift, c16(records), nullptr));
}

int32_t slot_emul_channel_level(const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, const nrLDPC_hip_rx_seg_t *first_sym, uint32_t n_tb,
                                int32_t *log2_maxh)
{
  if (rxf_check_common("channel_level", n_rx, NRLDPC_HIP_MEM_DEVICE) != 0)
    return -1;
  if (n_tb == 0)
    return 0;
  RxFrontPlan p;
  if (rxf_plan_level(first_sym, n_tb, n_rx, ant_stride, p) != 0)
    return -1;
  const auto tab = rxf_level_tables(p.lvl);
  const auto base = tables_copy(tab);
  WithThreads t;
  return launched(nr_launch_rx_level(tab.first(base.get()), n_tb, c16(chFext), n_rx, ant_stride, tab.second(base.get()), log2_maxh, nullptr));
}

int32_t slot_emul_channel_compensation_grid(const int16_t *rxdataF, const int16_t *ul_ch, uint32_t n_rx, uint64_t rx_ant_stride, uint64_t ch_ant_stride,
                                            const nrLDPC_hip_rx_grid_seg_t *seg, uint32_t n_seg, const int32_t *shift, int16_t *records)
{
  if (rxf_check_common("channel_compensation_grid", n_rx, NRLDPC_HIP_MEM_DEVICE) != 0)
    return -1;
  if (!aligned4({rxdataF, ul_ch, shift, records}))
    return set_error("channel_compensation_grid: every array 4-byte aligned");
  RxFrontPlan p;
  std::vector<rx_front_grid_job> gj;
  if (rxg_plan_compensation(seg, n_seg, n_rx, rx_ant_stride, ch_ant_stride, p, gj) != 0)
    return -1;
  if (gj.empty())
    return 0;
  rxg_place(p, gj, 0, 0, 0, reinterpret_cast<uintptr_t>(records) >> 2);
  const auto tab = table2(p.wgs, gj);
  const auto base = tables_copy(tab);
  return launched(nr_launch_rx_compensation_grid(tab.first(base.get()), (uint32_t)p.wgs.size(), tab.second(base.get()), c16(rxdataF), c16(ul_ch), n_rx,
                                                 rx_ant_stride, ch_ant_stride, shift, c16(records), nullptr));
}

int32_t slot_emul_channel_level_grid(const int16_t *ul_ch, uint32_t n_rx, uint64_t ch_ant_stride, const nrLDPC_hip_rx_grid_seg_t *first_sym, uint32_t n_tb,
                                     int32_t *log2_maxh)
{
  if (rxf_check_common("channel_level_grid", n_rx, NRLDPC_HIP_MEM_DEVICE) != 0)
    return -1;
  if (n_tb == 0)
    return 0;
  std::vector<rx_front_grid_lvl_job> lvl;
  uint64_t ch_lo, ch_hi;
  if (rxg_plan_level(first_sym, n_tb, n_rx, ch_ant_stride, lvl, ch_lo, ch_hi) != 0)
    return -1;
  const auto tab = rxf_level_tables(lvl);
  const auto base = tables_copy(tab);
  WithThreads t;
  return launched(nr_launch_rx_level_grid(tab.first(base.get()), n_tb, c16(ul_ch), n_rx, ch_ant_stride, tab.second(base.get()), log2_maxh, nullptr));
}

int32_t slot_emul_mmse_2layers_grid(const int16_t *rxdataF, const int16_t *ul_ch, uint32_t n_rx, uint64_t rx_ant_stride, uint64_t ch_ant_stride,
                                    const nrLDPC_hip_rx_grid_seg_t *seg, uint32_t n_seg, const int32_t *shift, const uint32_t *nvar, int16_t *records)
{
  if (rxm_check_common("mmse_2layers_grid", n_rx, NRLDPC_HIP_MEM_DEVICE) != 0)
    return -1;
  if (!aligned4({rxdataF, ul_ch, shift, nvar, records}))
    return set_error("mmse_2layers_grid: every array 4-byte aligned");
  RxFrontPlan p;
  std::vector<rx_front_grid_job> gj;
  if (rxm_plan(seg, n_seg, n_rx, rx_ant_stride, ch_ant_stride, p, gj) != 0)
    return -1;
  if (gj.empty())
    return 0;
  rxm_place(p, gj, 0, 0, 0);
  const auto tab = table2(p.wgs, gj);
  const auto base = tables_copy(tab);
  return launched(nr_launch_rx_mmse_grid(tab.first(base.get()), (uint32_t)p.wgs.size(), tab.second(base.get()), c16(rxdataF), c16(ul_ch), n_rx,
                                         rx_ant_stride, ch_ant_stride, shift, nvar, c16(records), nullptr));
}

int32_t slot_emul_channel_level_grid_mmse(const int16_t *ul_ch, uint32_t n_rx, uint64_t ch_ant_stride, const nrLDPC_hip_rx_grid_seg_t *first_sym,
                                          uint32_t n_tb, const int32_t *max_ch, int32_t *log2_maxh)
{
  if (rxm_check_common("channel_level_grid_mmse", n_rx, NRLDPC_HIP_MEM_DEVICE) != 0)
    return -1;
  if (n_tb == 0)
    return 0;
  std::vector<rx_front_grid_lvl_job> lvl;
  uint64_t ch_lo, ch_hi;
  if (rxg_plan_level(first_sym, n_tb, 2u * n_rx, ch_ant_stride, lvl, ch_lo, ch_hi) != 0)
    return -1;
  const auto tab = rxf_level_tables(lvl);
  const auto base = tables_copy(tab);
  WithThreads t;
  return launched(nr_launch_rx_level_grid_mmse(tab.first(base.get()), n_tb, c16(ul_ch), n_rx, ch_ant_stride, max_ch, tab.second(base.get()), log2_maxh,
                                               nullptr));
}

/* est_delay may be null (no delay compensation), as in the library */
int32_t slot_emul_pusch_channel_estimation(const int16_t *rxdataF, uint64_t rx_ant_stride, int16_t *ul_ch, uint64_t ch_ant_stride, uint32_t n_rx,
                                           const nrLDPC_hip_chest_seg_t *seg, uint32_t n_seg, const int32_t *est_delay)
{
  if (rxf_check_common("channel_estimation", n_rx, NRLDPC_HIP_MEM_DEVICE) != 0)
    return -1;
  if (!aligned4({rxdataF, ul_ch, est_delay}))
    return set_error("channel_estimation: every array 4-byte aligned");
  ChestPlan p;
  if (che_plan(seg, n_seg, n_rx, rx_ant_stride, ch_ant_stride, p) != 0)
    return -1;
  if (n_seg == 0)
    return 0;
  /* the delay tables, each in an allocation of exactly NR_CHE_DELAY_ROWS fft_size words as the library's device copies are */
  std::map<uint32_t, std::unique_ptr<uint32_t[]>> tabs;
  for (uint32_t i = 0; i < n_seg; i++) {
    std::unique_ptr<uint32_t[]> &d = tabs[seg[i].fft_size];
    if (!d) {
      std::vector<uint32_t> t;
      che_fill_table(seg[i].fft_size, t);
      d.reset(new uint32_t[t.size()]);
      memcpy(d.get(), t.data(), t.size() * 4u);
    }
    p.jobs[i].tab = d.get();
  }
  const auto tab = table2(p.wgs, p.jobs);
  const auto base = tables_copy(tab);
  /* the library's loop (che_launch of rx_chest_api.inc.cpp): one launch a mode over its part of the workgroup table */
  const rx_chest_wg *wgs = tab.first(base.get());
  for (uint32_t mode = 0; mode < NR_CHE_MODES; wgs += p.n_wg[mode++])
    if (launched(nr_launch_rx_chest(mode, wgs, p.n_wg[mode], tab.second(base.get()), c16(rxdataF), rx_ant_stride, c16(ul_ch), ch_ant_stride, est_delay,
                                    nullptr)) != 0)
      return -1;
  return 0;
}

} /* extern "C" */
