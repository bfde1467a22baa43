/*
 * tb_rx_mmse.h -- launch functions of the two-layer MMSE receiver (tb_rx_mmse.hip).  The job records are those of the grid
 * source of the single-layer front (tb_rx_front.h): rx_front_grid_job with s.out_off = the c16 index of codeword symbol
 * 2 sym_off of plane 0 (s.phase is not used), s.ch_off = pair 0's estimate of PUSCH subcarrier 0; rx_front_wg.piece counts
 * NR_RXF_THREADS quads; rx_front_grid_lvl_job as it is.
 */
#ifndef TB_RX_MMSE_H
#define TB_RX_MMSE_H
#include "tb_rx_front.h"

/* n_wg workgroups; wgs[n_wg], jobs[], shift[] and nvar[] in device memory; rx / ch / rec 4-byte aligned; n_rx = 2 or 4 */
hipError_t nr_launch_rx_mmse_grid(const rx_front_wg *wgs, uint32_t n_wg, const rx_front_grid_job *jobs, const uint32_t *rx, const uint32_t *ch,
                                  uint32_t n_rx, uint64_t rx_ant_stride, uint64_t ch_ant_stride, const int32_t *shift, const uint32_t *nvar,
                                  uint32_t *rec, hipStream_t s);
/* n_tb blocks, one workgroup per (block, pair), 2 n_rx pairs; state = 2 n_tb zeroed int32 (the blocks' maxima, then their counters) */
hipError_t nr_launch_rx_level_grid_mmse(const rx_front_grid_lvl_job *jobs, uint32_t n_tb, const uint32_t *ch, uint32_t n_rx, uint64_t ch_ant_stride,
                                        const int32_t *max_ch, int32_t *state, int32_t *log2_maxh, hipStream_t s);
#endif
