/*
 * tb_rx_delay.h -- job records and the launch functions of the PUSCH delay search (tb_rx_delay.hip): what rx_delay_api.inc.cpp
 * derives from the caller's nrLDPC_hip_chest_seg_t descriptors after it has checked them.  Offsets are in c16 words.  The
 * arithmetic: nr_delay.h.
 */
#ifndef TB_RX_DELAY_H
#define TB_RX_DELAY_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nr_delay.h"

#define NR_DLY_THREADS 1024

/* a kernel's dynamic LDS (the launch's lds_bytes); the CPU emulation of the kernels (tests/emul/) supplies a meaning of its own */
#ifndef NR_DLY_DYNAMIC_LDS
#define NR_DLY_DYNAMIC_LDS(type, name) extern __shared__ __attribute__((aligned(16))) type name[]
#endif

/* one descriptor = one DMRS symbol of one allocation, the averaging ones included (they get delay 0) */
typedef struct rx_delay_job {
  uint64_t rx_off;     /* antenna 0's subcarrier 0 of the symbol in the grid */
  const nr_dly_c *tw;  /* the twiddles of fft_size in device memory: fft_size of them, then NR_DLY_ONE_WORDS c16 (256, 0) */
  uint32_t fft_size, start_re, rb_size, dmrs_offset;
  uint32_t port, mode;
  uint32_t delay_off;  /* antenna 0's entry in est_delay / peak */
  uint32_t first_res;  /* antenna 0's entry in the search results (interpolating modes) */
} rx_delay_job;

/* workgroup w transforms antenna ant of descriptor job; x1 / x2 = the Gold registers at sequence word w0, the word of the first
 * pilot's bits */
typedef struct rx_delay_wg {
  uint32_t job, ant, w0;
  uint32_t x1, x2, pad;
} rx_delay_wg;

/* what a workgroup found: the largest P and the lowest n that has it (0, 0 for an all-zero symbol) */
typedef struct rx_delay_res {
  float peak;
  uint32_t pos;
} rx_delay_res;

/* n_wg workgroups whose descriptors all have fft_size; res[n_wg] receives one result a workgroup.  wgs, jobs, res in device
 * memory; rx 4-byte aligned */
hipError_t nr_launch_rx_delay_search(uint32_t fft_size, const rx_delay_wg *wgs, uint32_t n_wg, const rx_delay_job *jobs, const uint32_t *rx,
                                     uint64_t rx_ant_stride, rx_delay_res *res, hipStream_t s);
/* behind the searches on the same stream: est_delay[delay_off + a] and, where peak is given, peak[delay_off + a] of every
 * descriptor, a < n_rx; flags = NR_DLY_RUNNING_MAX or NR_DLY_PER_ANTENNA */
hipError_t nr_launch_rx_delay_combine(const rx_delay_job *jobs, uint32_t n_job, uint32_t n_rx, uint32_t flags, const rx_delay_res *res,
                                      int32_t *est_delay, float *peak, hipStream_t s);
#endif
