/*
 * tb_tx_map.h -- job records and the launch function of the PDSCH resource mapping kernel (tb_tx_map.hip): what
 * tx_map_api.inc.cpp derives from the caller's nrLDPC_hip_pdsch_map_seg_t descriptors after it has checked them.  Offsets are in
 * c16 words.  The arithmetic: nr_pdsch_map.h.
 */
#ifndef TB_TX_MAP_H
#define TB_TX_MAP_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NR_TXM_THREADS 256 /* 4-RE groups per workgroup */
#define NR_TXM_GROUP 4u

/* one descriptor = one OFDM symbol of one allocation */
typedef struct tx_map_job {
  uint64_t tx_off;  /* antenna 0's subcarrier 0 of the symbol in txdataF */
  uint64_t lay_off; /* layer 0's first entry of this symbol in layers */
  uint32_t plane, fft_size, start_re, n_re; /* n_re = 12 rb_size */
  uint32_t dmrs_offset, Nl, ncdm, l_prime;
  int32_t amp;
  uint32_t ports; /* layer l's port in byte l */
} tx_map_job;

/* workgroup w works on REs (piece * NR_TXM_THREADS + thread) * 4 - phase .. + 3 of antenna ant of descriptor job; phase = the
 * word address of the antenna's first RE mod 4, so that a thread's four REs start on a 16-byte boundary; x1 / x2 = the Gold
 * registers at sequence word w0, the word of the first pilot bit of the workgroup's first RE (unused for FULL and for the
 * antennas behind the layers) */
typedef struct tx_map_wg {
  uint32_t job, ant, piece, phase;
  uint32_t w0, x1, x2, pad;
} tx_map_wg;

/* precoding (nr_tx_precode_kernel), per descriptor: RB b of the allocation belongs to PRG b / prg_size (never 0 here: unit
 * precoding of a whole descriptor is one PRG as wide as the allocation), whose matrix is pmx[pmx_off + PRG]: 0 = unit, otherwise 1 +
 * the index into the call's matrices -- resolved on the host, nothing is searched on the device */
typedef struct tx_map_prg {
  uint32_t prg_size, pmx_off;
} tx_map_prg;
/* one precoding matrix: the weight of layer l for antenna a as a c16 word */
typedef struct tx_map_pm {
  uint32_t w[4][8];
} tx_map_pm;

/* n_wg workgroups of one pattern (NR_PDM_*); wgs[n_wg] and jobs[] in device memory; lay / tx 4-byte aligned */
hipError_t nr_launch_tx_map(uint32_t pattern, const tx_map_wg *wgs, uint32_t n_wg, const tx_map_job *jobs, const uint32_t *lay, uint32_t *tx,
                            uint64_t tx_ant_stride, hipStream_t s);
/* the same with precoding: prgs[] parallel to jobs[]; a workgroup's Gold registers stand at the word of the pilot number that
 * nr_pdm_last_pmask has reached at its first RE, for every antenna */
hipError_t nr_launch_tx_precode(uint32_t pattern, const tx_map_wg *wgs, uint32_t n_wg, const tx_map_job *jobs, const tx_map_prg *prgs, const uint16_t *pmx,
                                const tx_map_pm *mats, const uint32_t *lay, uint32_t *tx, uint64_t tx_ant_stride, hipStream_t s);
#endif
