/*
 * tb_rx_front.h -- job records and launch functions of the UL receive front (tb_rx_front.hip): what rx_front_api.inc.cpp
 * derives from the caller's nrLDPC_hip_rx_seg_t descriptors after it has checked them, and what rx_grid_api.inc.cpp derives from
 * nrLDPC_hip_rx_grid_seg_t descriptors for the grid source (nr_rx_grid.h).  Offsets are in c16 words.
 */
#ifndef TB_RX_FRONT_H
#define TB_RX_FRONT_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NR_RXF_THREADS 256
#define NR_RXF_GROUP 4 /* REs per thread: one 16-byte load per antenna and array, one 16-byte store per plane */

/* one segment of the compensation launch = one OFDM symbol's data REs of one transport block */
typedef struct rx_front_seg_job {
  uint64_t rx_off, ch_off; /* antenna 0's first RE in rxFext / chFext; antenna a at + a ant_stride */
  uint64_t out_off;        /* plane 0's first entry of the segment in the record array; plane k at + k plane */
  uint32_t plane, nb_re;
  uint32_t tb;             /* index into shift[] */
  uint32_t Qm;
  uint32_t phase;          /* (word address of the segment's first output) & 3: thread group g takes REs 4g - phase .. + 3 */
  uint32_t pad;
} rx_front_seg_job;

/* workgroup w of the compensation launch works on thread groups piece * NR_RXF_THREADS .. of segment seg */
typedef struct rx_front_wg {
  uint32_t seg, piece;
} rx_front_wg;

/* one block of the level launch: its measurement symbol */
typedef struct rx_front_lvl_job {
  uint64_t ch_off;
  uint32_t nb_re;
  uint32_t tb; /* index into log2_maxh[] */
} rx_front_lvl_job;

/* the grid source: the same segment, read from the OFDM grid and the full-width channel estimates.  s.rx_off = antenna 0's
 * subcarrier 0 of the OFDM symbol in the grid, s.ch_off = antenna 0's estimate of PUSCH subcarrier 0 */
typedef struct rx_front_grid_job {
  rx_front_seg_job s;
  uint32_t pattern, fft_size, start_re; /* NR_RXG_*; N; start_re < N; p(nb_re - 1) < N */
  uint32_t pad;
} rx_front_grid_job;

typedef struct rx_front_grid_lvl_job {
  uint64_t ch_off; /* antenna 0's estimate of PUSCH subcarrier 0 */
  uint32_t nb_re;
  uint32_t tb;
  uint32_t pattern;
  uint32_t pad;
} rx_front_grid_lvl_job;

/* n_wg workgroups; wgs[n_wg], jobs[] and shift[] in device memory; rx / ch / rec 4-byte aligned */
hipError_t nr_launch_rx_compensation(const rx_front_wg *wgs, uint32_t n_wg, const rx_front_seg_job *jobs, const uint32_t *rx, const uint32_t *ch,
                                     uint32_t n_rx, uint64_t ant_stride, const int32_t *shift, uint32_t *rec, hipStream_t s);
/* n_tb blocks, one workgroup per (block, antenna); state = 2 n_tb zeroed int32 (the blocks' maxima, then their counters) */
hipError_t nr_launch_rx_level(const rx_front_lvl_job *jobs, uint32_t n_tb, const uint32_t *ch, uint32_t n_rx, uint64_t ant_stride, int32_t *state,
                              int32_t *log2_maxh, hipStream_t s);
/* the same two launches with the grid source; the grid and the estimates have an antenna stride each */
hipError_t nr_launch_rx_compensation_grid(const rx_front_wg *wgs, uint32_t n_wg, const rx_front_grid_job *jobs, const uint32_t *rx, const uint32_t *ch,
                                          uint32_t n_rx, uint64_t rx_ant_stride, uint64_t ch_ant_stride, const int32_t *shift, uint32_t *rec,
                                          hipStream_t s);
hipError_t nr_launch_rx_level_grid(const rx_front_grid_lvl_job *jobs, uint32_t n_tb, const uint32_t *ch, uint32_t n_rx, uint64_t ch_ant_stride,
                                   int32_t *state, int32_t *log2_maxh, hipStream_t s);
#endif
