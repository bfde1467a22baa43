/*
 * tb_rx_chest.h -- job records and the launch function of the PUSCH channel estimation kernel (tb_rx_chest.hip): what
 * rx_chest_api.inc.cpp derives from the caller's nrLDPC_hip_chest_seg_t descriptors after it has checked them.  Offsets are in
 * c16 words.  The arithmetic: nr_chest.h.
 */
#ifndef TB_RX_CHEST_H
#define TB_RX_CHEST_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NR_CHE_THREADS 256 /* output units (4-RE groups or PRBs) per workgroup */

/* one descriptor = one DMRS symbol of one allocation */
typedef struct rx_chest_job {
  uint64_t rx_off, ch_off;   /* antenna 0's subcarrier 0 of the symbol in the grid; antenna 0's first output entry */
  const uint32_t *tab;       /* the delay table of fft_size in device memory: NR_CHE_DELAY_ROWS rows of fft_size c16 */
  uint32_t fft_size, start_re, rb_size, dmrs_offset;
  uint32_t port, delay_off;
} rx_chest_job;

/* workgroup w works on units piece * NR_CHE_THREADS .. of antenna ant of descriptor job; x1 / x2 = the Gold registers at
 * sequence word w0, the word of the first pilot bit of the workgroup's first unit */
typedef struct rx_chest_wg {
  uint32_t job, ant, piece, w0;
  uint32_t x1, x2;
} rx_chest_wg;

/* n_wg workgroups of one mode (NR_CHE_*); wgs[n_wg] and jobs[] in device memory; rx / ch 4-byte aligned; est_delay may be
 * NULL (delay 0 everywhere) */
hipError_t nr_launch_rx_chest(uint32_t mode, const rx_chest_wg *wgs, uint32_t n_wg, const rx_chest_job *jobs, const uint32_t *rx, uint64_t rx_ant_stride,
                              uint32_t *ch, uint64_t ch_ant_stride, const int32_t *est_delay, hipStream_t s);
#endif
