/*
 * tb_rx_chest_meas.h -- job records and launch functions of the measuring PUSCH channel estimation and of the time average of
 * its estimates (tb_rx_chest_meas.hip).  The estimation runs on tb_rx_chest.h's workgroup table and job records unchanged; what
 * the measurements need in addition is a table of its own, parallel to the jobs.  Offsets are in c16 words.  The arithmetic:
 * nr_chest.h.
 */
#ifndef TB_RX_CHEST_MEAS_H
#define TB_RX_CHEST_MEAS_H
#include "tb_rx_chest.h"

/* parallel to rx_chest_job: the block the descriptor belongs to and the call's nest_count, which the host knows */
typedef struct rx_chest_meas_job {
  uint32_t tb, nest_count;
} rx_chest_meas_job;

/* block tb's descriptors are list[first .. first + count - 1] of the call's descriptor list; div = nvar_div[tb] > 0 */
typedef struct rx_chest_meas_tb {
  uint32_t first, count, div, pad;
} rx_chest_meas_tb;

/* n_wg workgroups of one mode as nr_launch_rx_chest, which besides add their shares to mx[tb] (int32, n_tb of them) and
 * noise[descriptor] (uint64), both zero before the call's first launch */
hipError_t nr_launch_rx_chest_meas(uint32_t mode, const rx_chest_wg *wgs, uint32_t n_wg, const rx_chest_job *jobs, const rx_chest_meas_job *mjobs,
                                   const uint32_t *rx, uint64_t rx_ant_stride, uint32_t *ch, uint64_t ch_ant_stride, const int32_t *est_delay, int32_t *mx,
                                   uint64_t *noise, hipStream_t s);
/* behind the call's last estimation launch on the same stream: one thread a block forms max_ch[tb] and nvar[tb] */
hipError_t nr_launch_rx_chest_finish(const rx_chest_meas_tb *tbs, uint32_t n_tb, const uint32_t *list, const rx_chest_meas_job *mjobs, const int32_t *mx,
                                     const uint64_t *noise, int32_t *max_ch, uint32_t *nvar, hipStream_t s);

#define NR_CHE_AVG_MAX_SYM 4u
/* one descriptor of the time average: the first symbol's entries are replaced by the average of the n_sym symbols' */
typedef struct rx_chest_avg_job {
  uint64_t ch_off[NR_CHE_AVG_MAX_SYM];
  uint32_t n_sym, rb_size;
} rx_chest_avg_job;
/* workgroup w: 4-c16 units piece * NR_CHE_THREADS .. of plane `plane` of descriptor job */
typedef struct rx_chest_avg_wg {
  uint32_t job, plane, piece, pad;
} rx_chest_avg_wg;
hipError_t nr_launch_rx_chest_time_avg(const rx_chest_avg_wg *wgs, uint32_t n_wg, const rx_chest_avg_job *jobs, uint32_t *ch, uint64_t ch_ant_stride,
                                       hipStream_t s);
#endif
