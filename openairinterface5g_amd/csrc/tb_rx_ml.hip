/*
 * tb_rx_ml.hip -- the two-layer PUSCH max-log ML receiver for QPSK and 16QAM on gfx950 (nr_rx_ml.h): the reference's channel
 * compensation with rho (openair1/PHY/NR_TRANSPORT/nr_ulsch_demodulation.c:505-571), nr_ulsch_compute_ML_llr
 * (nr_ulsch_llr_computation.c:2100-2129) and the layer de-mapping (nr_ulsch_demodulation.c:1431-1438) over every OFDM symbol of
 * every two-layer transport block of a slot in one launch, from the FFT grid and the per-layer channel estimates straight into
 * the LLR array nrLDPC_hip_ulsch_decode_scrambled reads; and the channel level of the blocks' measurement symbols over the 2 n_rx
 * (layer, antenna) pairs (:1612-1647).
 *
 * A thread takes a group of four REs counted from the segment's RE 0, so every array is read with 16-byte loads (the group and
 * its loader: tb_rx_group.h, shared with the MMSE receiver).  Bit m of layer
 * l of RE r is int16 rec_off + Qm (2 (sym_off + r) + l) + m: an RE's two layers are Qm 32-bit words side by side, a group's
 * four REs 32 (QPSK) or 64 (16QAM) contiguous bytes, stored as 16-byte stores at a 4-byte aligned address.  Per RE 4 n_rx bytes
 * of grid and 8 n_rx bytes of estimates come in and 4 Qm bytes go out; no LDS.  Qm is uniform per segment: the QPSK / 16QAM
 * choice is a scalar branch.
 */
#include <hip/hip_runtime.h>
#include "nr_rx_ml.h"
#include "nr_rx_grid.h"
#include "tb_rx_ml.h"
#include "tb_rx_group.h"
#include "tb_rx_level.h"

/* NRX = 2, 4: the antennas unrolled; NRX = 0: any n_rx, one antenna's loads at a time */
template <int NRX>
__global__ void __launch_bounds__(NR_RXF_THREADS)
nr_rx_ml_grid_kernel(const rx_front_wg *__restrict__ wgs, const rx_front_grid_job *__restrict__ jobs, const uint32_t *__restrict__ rx,
                     const uint32_t *__restrict__ ch, uint32_t n_rx, uint64_t rx_stride, uint64_t ch_stride, const int32_t *__restrict__ shift,
                     uint32_t *__restrict__ llr)
{
  const rx_front_wg w = wgs[blockIdx.x];
  const rx_front_grid_job J = jobs[w.seg];
  const rx_front_seg_job &j = J.s;
  const uint32_t r0 = (w.piece * NR_RXF_THREADS + threadIdx.x) * NR_RXF_GROUP;
  if (r0 >= j.nb_re)
    return;
  const uint32_t s = nr_rxf_shift(shift[j.tb]);
  const int32_t amp[3] = {nr_rxf_amp(j.Qm, 0), 0, 0};
  const uint32_t *y0 = rx + j.rx_off, *h0 = ch + j.ch_off, *h1 = h0 + (size_t)(NRX > 0 ? NRX : n_rx) * ch_stride;
  const rx_group G = rx_group_locate(J, r0);

  nr_rxl_re_t R[4] = {};
  if constexpr (NRX > 0) {
    uint32_t yv[NRX][4], h0v[NRX][4], h1v[NRX][4];
    rx_group_load<NRX>(G, y0, rx_stride, h0, h1, ch_stride, yv, h0v, h1v);
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int a = 0; a < NRX; a++)
        nr_rxl_mac(&R[u], h0v[a][u], h1v[a][u], yv[a][u], s, amp);
  } else {
    for (uint32_t a = 0; a < n_rx; a++) { /* in order: the sums of rho saturate */
      uint32_t yv[1][4], h0v[1][4], h1v[1][4];
      rx_group_load<1>(G, y0 + (size_t)a * rx_stride, rx_stride, h0 + (size_t)a * ch_stride, h1 + (size_t)a * ch_stride, ch_stride, yv, h0v, h1v);
#pragma unroll
      for (int u = 0; u < 4; u++)
        nr_rxl_mac(&R[u], h0v[0][u], h1v[0][u], yv[0][u], s, amp);
    }
  }

  /* layer de-mapping (:1431-1438) is the store: RE r0 + u, layer l at word Qm (r0 + u) + (Qm / 2) l of the segment */
  uint32_t *o = llr + j.out_off + (size_t)j.Qm * r0;
  if (j.Qm == 2) { /* scalar */
    uint32_t v[8];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int l = 0; l < 2; l++) {
        int32_t L[2];
        nr_rxl_llr(&R[u], 2, l, L);
        v[2 * u + l] = nr_rxf_c16(L[0], L[1]);
      }
    if (G.whole) {
      rx_store4(o, v[0], v[1], v[2], v[3]);
      rx_store4(o + 4, v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (r0 + u < j.nb_re) {
          o[2 * u] = v[2 * u];
          o[2 * u + 1] = v[2 * u + 1];
        }
    }
  } else {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      uint32_t v[4];
#pragma unroll
      for (int l = 0; l < 2; l++) {
        int32_t L[4];
        nr_rxl_llr(&R[u], 4, l, L);
        v[2 * l] = nr_rxf_c16(L[0], L[1]);
        v[2 * l + 1] = nr_rxf_c16(L[2], L[3]);
      }
      if (G.whole)
        rx_store4(o + 4 * u, v[0], v[1], v[2], v[3]);
      else if (r0 + u < j.nb_re) {
#pragma unroll
        for (int k = 0; k < 4; k++)
          o[4 * u + k] = v[k];
      }
    }
  }
}

hipError_t nr_launch_rx_ml_grid(const rx_front_wg *wgs, uint32_t n_wg, const rx_front_grid_job *jobs, const uint32_t *rx, const uint32_t *ch,
                                uint32_t n_rx, uint64_t rx_ant_stride, uint64_t ch_ant_stride, const int32_t *shift, uint32_t *llr, hipStream_t s)
{
  if (n_wg == 0)
    return hipSuccess;
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return hipErrorInvalidValue;
#define RXL_LAUNCH(N) hipLaunchKernelGGL(nr_rx_ml_grid_kernel<N>, dim3(n_wg), dim3(NR_RXF_THREADS), 0, s, wgs, jobs, rx, ch, n_rx, rx_ant_stride, ch_ant_stride, shift, llr)
  switch (n_rx) {
    case 2: RXL_LAUNCH(2); break;
    case 4: RXL_LAUNCH(4); break;
    default: RXL_LAUNCH(0); break;
  }
#undef RXL_LAUNCH
  return hipGetLastError();
}

/* ---- channel level: the two-layer body (tb_rx_level.h) with the ML branch's formula at the end ---- */
__global__ void __launch_bounds__(NR_RXF_THREADS)
nr_rx_level_grid_ml_kernel(const rx_front_grid_lvl_job *__restrict__ jobs, const uint32_t *__restrict__ ch, uint32_t n_pair, uint64_t ant_stride,
                           const int32_t *__restrict__ max_ch, int32_t *mx, int32_t *cnt, int32_t *__restrict__ log2_maxh)
{
  rx2_level_body(jobs, ch, n_pair, ant_stride, max_ch, [](int32_t avgs) { return nr_rxl_log2_maxh(avgs); }, mx, cnt, log2_maxh);
}

hipError_t nr_launch_rx_level_grid_ml(const rx_front_grid_lvl_job *jobs, uint32_t n_tb, const uint32_t *ch, uint32_t n_rx, uint64_t ch_ant_stride,
                                      const int32_t *max_ch, int32_t *state, int32_t *log2_maxh, hipStream_t s)
{
  if (n_tb == 0)
    return hipSuccess;
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(nr_rx_level_grid_ml_kernel, dim3(n_tb * 2u * n_rx), dim3(NR_RXF_THREADS), 0, s, jobs, ch, 2u * n_rx, ch_ant_stride, max_ch,
                     state, state + n_tb, log2_maxh);
  return hipGetLastError();
}
