/*
 * tb_rx_mmse.hip -- the two-layer PUSCH MMSE receiver for gfx950 (nr_rx_mmse.h): the reference's matched filter per layer,
 * nr_ulsch_mmse_2layers() (openair1/PHY/NR_TRANSPORT/nr_ulsch_demodulation.c:869-1260) and the layer de-mapping (:1431-1438) over
 * every OFDM symbol of every two-layer transport block of a slot in one launch, from the FFT grid and the per-layer channel
 * estimates straight into the planar symbol records nrLDPC_hip_ulsch_decode_symbols reads with Nl = 2; and the channel level of
 * the blocks' measurement symbols over the 2 n_rx (layer, antenna) pairs (:1612-1647).
 *
 * A thread takes one quad of the reference: REs 4q .. 4q + 3 counted from the segment's RE 0, the four lanes of one 128-bit
 * vector.  The quad shares the shift b = log2_approx(sum of the lanes' det >> 2) - 8, so the quads cannot be moved against the
 * segment: the `phase` of the single-layer kernel, which lays its groups for 16-byte aligned stores, cannot be carried over.
 * The stores here are 16 bytes at a 4-byte aligned address.  Per RE 4 n_rx bytes of grid and 8 n_rx bytes of estimates come in
 * and 2 Qm bytes go out; no LDS.
 *
 * The 16-byte load and store and the DMRS1 pick are tb_rx_group.h's.  The loader of a quad is written out here and not taken
 * from that header: with the shared one (the estimates as two arrays of n_rx, layer 0's and layer 1's loads interleaved) the
 * n_rx = 4 kernel measured 0.5 .. 1 % slower than with this one (one array of 2 n_rx pairs, loaded in order), outside the spread of
 * repeated runs.  What it does and why is said once, at rx_group_load.
 */
#include <hip/hip_runtime.h>
#include "nr_rx_mmse.h"
#include "nr_rx_grid.h"
#include "tb_rx_mmse.h"
#include "tb_rx_group.h"
#include "tb_rx_level.h"

static_assert(NR_RXM_QUAD == NR_RXF_GROUP, "a thread's group of four REs is the quad that shares the shift b");

template <int NRX>
__global__ void __launch_bounds__(NR_RXF_THREADS)
nr_rx_mmse_grid_kernel(const rx_front_wg *__restrict__ wgs, const rx_front_grid_job *__restrict__ jobs, const uint32_t *__restrict__ rx,
                       const uint32_t *__restrict__ ch, uint64_t rx_stride, uint64_t ch_stride, const int32_t *__restrict__ shift,
                       const uint32_t *__restrict__ nvar, uint32_t *__restrict__ rec)
{
  const rx_front_wg w = wgs[blockIdx.x];
  const rx_front_grid_job J = jobs[w.seg];
  const rx_front_seg_job &j = J.s;
  const uint32_t r0 = (w.piece * NR_RXF_THREADS + threadIdx.x) * NR_RXM_QUAD;
  if (r0 >= j.nb_re)
    return;
  const uint32_t s = nr_rxf_shift(shift[j.tb]), nv = nvar[j.tb], np = j.Qm >> 1;
  const uint32_t *y0 = rx + j.rx_off, *h0 = ch + j.ch_off;

  /* the quad's REs of the n_rx antennas and of the 2 n_rx pairs, every load issued before the first use (rx_group_load of
   * tb_rx_group.h: the pattern tested once around all loads, DMRS1's two loads within the segment's own range) */
  uint32_t yv[NRX][4], hv[2 * NRX][4];
  const uint32_t pa = nr_rxg_p(J.pattern, r0), span = nr_rxg_p(J.pattern, r0 + 3u) - pa, g = J.start_re + pa;
  const bool whole = r0 + NR_RXM_QUAD <= j.nb_re;
  if (whole && !(g < J.fft_size && g + span >= J.fft_size)) {
    const uint32_t ga = g >= J.fft_size ? g - J.fft_size : g;
    if (J.pattern == NR_RXG_DMRS1) { /* wave-uniform */
      uint32_t yA[NRX][4], yB[NRX][4], hA[2 * NRX][4], hB[2 * NRX][4];
#pragma unroll
      for (int a = 0; a < NRX; a++) {
        rx_load4(yA[a], y0 + (size_t)a * rx_stride + ga);
        rx_load4(yB[a], y0 + (size_t)a * rx_stride + ga + 3);
      }
#pragma unroll
      for (int a = 0; a < 2 * NRX; a++) {
        rx_load4(hA[a], h0 + (size_t)a * ch_stride + pa);
        rx_load4(hB[a], h0 + (size_t)a * ch_stride + pa + 3);
      }
#pragma unroll
      for (int a = 0; a < NRX; a++)
        rx_pick_dmrs1(yv[a], yA[a], yB[a]);
#pragma unroll
      for (int a = 0; a < 2 * NRX; a++)
        rx_pick_dmrs1(hv[a], hA[a], hB[a]);
    } else {
#pragma unroll
      for (int a = 0; a < NRX; a++)
        rx_load4(yv[a], y0 + (size_t)a * rx_stride + ga);
#pragma unroll
      for (int a = 0; a < 2 * NRX; a++)
        rx_load4(hv[a], h0 + (size_t)a * ch_stride + pa);
    }
  } else {
    /* the grid wraps inside the quad, or the segment ends inside it: RE by RE; the lanes behind nb_re are the reference's zero
     * padding (:1284-1285) and still enter the quad's sum of determinants */
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const bool in = r0 + u < j.nb_re;
      const uint32_t p = nr_rxg_p(J.pattern, r0 + u), sc = nr_rxg_grid_sc(J.start_re, p, J.fft_size);
#pragma unroll
      for (int a = 0; a < NRX; a++)
        yv[a][u] = in ? y0[(size_t)a * rx_stride + sc] : 0u;
#pragma unroll
      for (int a = 0; a < 2 * NRX; a++)
        hv[a][u] = in ? h0[(size_t)a * ch_stride + p] : 0u;
    }
  }

  nr_rxm_re_t R[4] = {};
  int32_t det[4];
#pragma unroll
  for (int u = 0; u < 4; u++) {
#pragma unroll
    for (int a = 0; a < NRX; a++)
      nr_rxm_mac(&R[u], hv[a][u], hv[NRX + a][u], yv[a][u], s);
    det[u] = nr_rxm_det(&R[u], nv);
  }
  const int32_t bm = nr_rxm_b_mag(det), bs = nr_rxm_b_sym(det);

  /* codeword symbol 2 (sym_off + r) + l (:1431-1438): the quad's eight entries of a plane lie side by side */
  uint32_t *o = rec + j.out_off + 2u * (size_t)r0;
  uint32_t v[8];
#pragma unroll
  for (int u = 0; u < 4; u++) {
    v[2 * u] = nr_rxm_sym0(&R[u], bs);
    v[2 * u + 1] = nr_rxm_sym1(&R[u], bs);
  }
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    if (k >= np)
      break;
    if (k > 0) {
      const int32_t amp = nr_rxf_amp(j.Qm, k - 1u);
#pragma unroll
      for (int u = 0; u < 4; u++)
        v[2 * u] = v[2 * u + 1] = nr_rxm_mag(det[u], bm, amp);
    }
    uint32_t *ok = o + (size_t)k * j.plane;
    if (whole) {
      rx_store4(ok, v[0], v[1], v[2], v[3]);
      rx_store4(ok + 4, v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (r0 + u < j.nb_re) {
          ok[2 * u] = v[2 * u];
          ok[2 * u + 1] = v[2 * u + 1];
        }
    }
  }
}

hipError_t nr_launch_rx_mmse_grid(const rx_front_wg *wgs, uint32_t n_wg, const rx_front_grid_job *jobs, const uint32_t *rx, const uint32_t *ch,
                                  uint32_t n_rx, uint64_t rx_ant_stride, uint64_t ch_ant_stride, const int32_t *shift, const uint32_t *nvar,
                                  uint32_t *rec, hipStream_t s)
{
  if (n_wg == 0)
    return hipSuccess;
#define RXM_LAUNCH(N) hipLaunchKernelGGL(nr_rx_mmse_grid_kernel<N>, dim3(n_wg), dim3(NR_RXF_THREADS), 0, s, wgs, jobs, rx, ch, rx_ant_stride, ch_ant_stride, shift, nvar, rec)
  switch (n_rx) {
    case 2: RXM_LAUNCH(2); break;
    case 4: RXM_LAUNCH(4); break;
    default: return hipErrorInvalidValue;
  }
#undef RXM_LAUNCH
  return hipGetLastError();
}

/* ---- channel level: the two-layer body (tb_rx_level.h) with the MMSE formula at the end ---- */
__global__ void __launch_bounds__(NR_RXF_THREADS)
nr_rx_level_grid_mmse_kernel(const rx_front_grid_lvl_job *__restrict__ jobs, const uint32_t *__restrict__ ch, uint32_t n_pair, uint64_t ant_stride,
                             const int32_t *__restrict__ max_ch, int32_t *mx, int32_t *cnt, int32_t *__restrict__ log2_maxh)
{
  rx2_level_body(jobs, ch, n_pair, ant_stride, max_ch, [](int32_t avgs) { return nr_rxm_log2_maxh(avgs); }, mx, cnt, log2_maxh);
}

hipError_t nr_launch_rx_level_grid_mmse(const rx_front_grid_lvl_job *jobs, uint32_t n_tb, const uint32_t *ch, uint32_t n_rx, uint64_t ch_ant_stride,
                                        const int32_t *max_ch, int32_t *state, int32_t *log2_maxh, hipStream_t s)
{
  if (n_tb == 0)
    return hipSuccess;
  if (n_rx != 2 && n_rx != 4)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(nr_rx_level_grid_mmse_kernel, dim3(n_tb * 2u * n_rx), dim3(NR_RXF_THREADS), 0, s, jobs, ch, 2u * n_rx, ch_ant_stride, max_ch,
                     state, state + n_tb, log2_maxh);
  return hipGetLastError();
}
