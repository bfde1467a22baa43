/*
 * tb_rx_ml.h -- launch functions of the two-layer max-log ML receiver (tb_rx_ml.hip).  The job records are those of the grid
 * source of the single-layer front (tb_rx_front.h): rx_front_grid_job with s.out_off = the 32-bit word index of the segment's
 * first LLR pair in the LLR array, rec_off / 2 + Qm sym_off (s.plane and s.phase are not used), s.ch_off = pair 0's estimate of
 * PUSCH subcarrier 0; rx_front_wg.piece counts NR_RXF_THREADS groups of NR_RXF_GROUP REs; rx_front_grid_lvl_job as it is.
 */
#ifndef TB_RX_ML_H
#define TB_RX_ML_H
#include "tb_rx_front.h"

/* n_wg workgroups; wgs[n_wg], jobs[] and shift[] in device memory; rx / ch / llr 4-byte aligned; n_rx = 1..8 */
hipError_t nr_launch_rx_ml_grid(const rx_front_wg *wgs, uint32_t n_wg, const rx_front_grid_job *jobs, const uint32_t *rx, const uint32_t *ch,
                                uint32_t n_rx, uint64_t rx_ant_stride, uint64_t ch_ant_stride, const int32_t *shift, uint32_t *llr, hipStream_t s);
/* n_tb blocks, one workgroup per (block, pair), 2 n_rx pairs; state = 2 n_tb zeroed int32 (the blocks' maxima, then their counters) */
hipError_t nr_launch_rx_level_grid_ml(const rx_front_grid_lvl_job *jobs, uint32_t n_tb, const uint32_t *ch, uint32_t n_rx, uint64_t ch_ant_stride,
                                      const int32_t *max_ch, int32_t *state, int32_t *log2_maxh, hipStream_t s);
#endif
