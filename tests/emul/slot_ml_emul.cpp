/*
 * slot_ml_emul.cpp -- the two-layer ML receiver's kernels on the CPU as a shared library (test infrastructure), for the descriptor
 * sweep of tests/test_slot_sweep_host.py: the DEVICE mem branches of ml_emul_san.cpp (tb_rx_ml.hip itself against the host shim, over
 * the library's own plan), exported.  ml_emul_san.cpp is #included as it is, so there is one copy of them; its main is renamed and
 * never called.
 */
#define main ml_emul_san_main
#include "ml_emul_san.cpp"
#undef main

extern "C" {

const char *slot_ml_emul_last_error() { return slot_emul_error.c_str(); }

int32_t slot_emul_ml_2layers_grid(const int16_t *rxdataF, const int16_t *ul_ch, uint32_t n_rx, uint64_t rx_ant_stride, uint64_t ch_ant_stride,
                                  const nrLDPC_hip_rx_grid_seg_t *seg, uint32_t n_seg, const int32_t *shift, int16_t *llr)
{
  return emul_ml_2layers_grid(rxdataF, ul_ch, n_rx, rx_ant_stride, ch_ant_stride, seg, n_seg, shift, llr);
}

int32_t slot_emul_channel_level_grid_ml(const int16_t *ul_ch, uint32_t n_rx, uint64_t ch_ant_stride, const nrLDPC_hip_rx_grid_seg_t *first_sym, uint32_t n_tb,
                                        const int32_t *max_ch, int32_t *log2_maxh)
{
  return emul_channel_level_grid_ml(ul_ch, n_rx, ch_ant_stride, first_sym, n_tb, max_ch, log2_maxh);
}

} /* extern "C" */
