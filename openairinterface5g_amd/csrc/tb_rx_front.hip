/*
 * tb_rx_front.hip -- the UL receive front for gfx950 (nr_rx_front.h): the reference's nr_ulsch_channel_compensation() for one
 * layer (openair1/PHY/NR_TRANSPORT/nr_ulsch_demodulation.c:468-577) over every OFDM symbol of every transport block of a slot in
 * one launch, writing straight into the planar symbol records nrLDPC_hip_ulsch_decode_symbols reads, and the channel level of the
 * blocks' first symbols with the shift log2_maxh it gives (:434-466, :1612-1647).
 *
 * Compensation is memory bound by construction: 8 n_rx bytes in and 2 Qm bytes out per RE, a handful of integer operations
 * between them.  A thread takes NR_RXF_GROUP consecutive REs; the groups of a segment are laid so that plane 0's stores are 16-byte
 * aligned (the segment's first RE rarely is: nb_re per symbol is 12, 6 or 8 per RB), with a short head and tail stored word by word.
 */
#include <hip/hip_runtime.h>
#include "nr_rx_front.h"
#include "nr_rx_grid.h"
#include "tb_rx_front.h"
#include "tb_rx_group.h"
#include "tb_rx_level.h"

/* ---- the grid source (nr_rx_grid.h): the segment's REs are read from the OFDM grid and the full-width channel estimates ----
 * A thread group's four REs r0 .. r0 + 3 are PUSCH subcarriers p(r0) .. p(r0 + 3): 4 consecutive c16 for FULL (and for DMRS2
 * when r0 % 4 == 0), 7 for DMRS1, 6 for DMRS2 otherwise.  Load A takes the four c16 from p(r0), load B the four that end at
 * p(r0 + 3); together they cover exactly [p(r0), p(r0 + 3)], so nothing outside the segment's own range is read.  r0 % 4 is the
 * same for every group of a segment (r0 = 4g - phase), so whether B is needed and which words are taken are wave-uniform. */
struct rxf_grid_group {
  uint32_t pa, ga; /* load A: offset behind the estimate of subcarrier 0 / behind the grid's subcarrier 0 */
  uint32_t db;     /* load B lies db c16 behind load A (3 for DMRS1, 2 for DMRS2) */
  uint32_t q;      /* r0 % 4 */
  bool dmrs1, two, straddle; /* straddle: the group's grid range runs over the wrap at N -> RE by RE */
};
__device__ __forceinline__ rxf_grid_group rxf_grid_locate(const rx_front_grid_job &J, int32_t r0)
{
  rxf_grid_group G;
  G.q = (4u - J.s.phase) & 3u;
  G.dmrs1 = J.pattern == NR_RXG_DMRS1;
  G.two = G.dmrs1 || (J.pattern == NR_RXG_DMRS2 && G.q != 0);
  G.pa = nr_rxg_p(J.pattern, (uint32_t)r0);
  const uint32_t span = nr_rxg_p(J.pattern, (uint32_t)r0 + NR_RXF_GROUP - 1u) - G.pa;
  G.db = span - (NR_RXF_GROUP - 1u);
  const uint32_t g = J.start_re + G.pa;
  G.straddle = g < J.fft_size && g + span >= J.fft_size;
  G.ga = g >= J.fft_size ? g - J.fft_size : g;
  return G;
}
/* the group's four REs out of loads A and B.  DMRS1: p = pa, pa + 2, pa + 4, pa + 6 = A[0], A[2], B[1], B[3];
 * DMRS2 with q = r0 % 4 > 0: REs u < 4 - q are A[u], the others (behind the two pilot subcarriers) B[u] */
__device__ __forceinline__ void rxf_grid_pick(uint32_t (&v)[NR_RXF_GROUP], const uint32_t (&A)[NR_RXF_GROUP], const uint32_t (&B)[NR_RXF_GROUP],
                                              const rxf_grid_group &G)
{
  v[0] = A[0];
  v[1] = G.dmrs1 ? A[2] : (G.q > 2 ? B[1] : A[1]);
  v[2] = G.dmrs1 ? B[1] : (G.q > 1 ? B[2] : A[2]);
  v[3] = B[3];
}

__device__ __forceinline__ const rx_front_seg_job &rxf_seg(const rx_front_seg_job &j) { return j; }
__device__ __forceinline__ const rx_front_seg_job &rxf_seg(const rx_front_grid_job &j) { return j.s; }

/* NRX > 0: that many antennas, every load issued before the first use; NRX = 0: n_rx antennas one after another.
 * GRID: Job = rx_front_grid_job and the inputs are the grid and the estimates, else rx_front_seg_job and extracted arrays
 * (rx_stride == ch_stride) */
template <int NRX, bool GRID, typename Job>
__device__ __forceinline__ void rx_compensation_body(const rx_front_wg *__restrict__ wgs, const Job *__restrict__ jobs, const uint32_t *__restrict__ rx,
                                                     const uint32_t *__restrict__ ch, uint32_t n_rx, uint64_t rx_stride, uint64_t ch_stride,
                                                     const int32_t *__restrict__ shift, uint32_t *__restrict__ rec)
{
  const rx_front_wg w = wgs[blockIdx.x];
  const Job J = jobs[w.seg];
  const rx_front_seg_job &j = rxf_seg(J);
  const int32_t nb_re = (int32_t)j.nb_re;
  const int32_t r0 = (int32_t)((w.piece * NR_RXF_THREADS + threadIdx.x) * NR_RXF_GROUP) - (int32_t)j.phase;
  if (r0 >= nb_re)
    return;
  const uint32_t s = nr_rxf_shift(shift[j.tb]), np = j.Qm >> 1;
  const int32_t amp[3] = {nr_rxf_amp(j.Qm, 0), nr_rxf_amp(j.Qm, 1), nr_rxf_amp(j.Qm, 2)};
  const uint32_t *y0 = rx + j.rx_off, *h0 = ch + j.ch_off;
  uint32_t *o = rec + j.out_off;
  const uint32_t nrx = NRX ? (uint32_t)NRX : n_rx;

  bool whole = r0 >= 0 && r0 + NR_RXF_GROUP <= nb_re;
  uint32_t hoff = (uint32_t)r0, yoff = (uint32_t)r0;
  [[maybe_unused]] rxf_grid_group G;
  if constexpr (GRID) {
    if (whole) {
      G = rxf_grid_locate(J, r0);
      hoff = G.pa;
      yoff = G.ga;
      whole = !G.straddle;
    }
  }
  if (whole) {
    nr_rxf_acc_t acc[NR_RXF_GROUP] = {};
    bool done = false;
    if constexpr (GRID) {
      if (G.two) { /* wave-uniform */
        if constexpr (NRX > 0) {
          uint32_t hA[NRX][NR_RXF_GROUP], hB[NRX][NR_RXF_GROUP], yA[NRX][NR_RXF_GROUP], yB[NRX][NR_RXF_GROUP];
#pragma unroll
          for (int a = 0; a < NRX; a++) {
            rx_load4(hA[a], h0 + (size_t)a * ch_stride + hoff);
            rx_load4(hB[a], h0 + (size_t)a * ch_stride + hoff + G.db);
            rx_load4(yA[a], y0 + (size_t)a * rx_stride + yoff);
            rx_load4(yB[a], y0 + (size_t)a * rx_stride + yoff + G.db);
          }
#pragma unroll
          for (int a = 0; a < NRX; a++) {
            uint32_t hv[NR_RXF_GROUP], yv[NR_RXF_GROUP];
            rxf_grid_pick(hv, hA[a], hB[a], G);
            rxf_grid_pick(yv, yA[a], yB[a], G);
#pragma unroll
            for (int u = 0; u < NR_RXF_GROUP; u++)
              nr_rxf_mac(&acc[u], hv[u], yv[u], s, amp);
          }
        } else {
          for (uint32_t a = 0; a < nrx; a++) {
            uint32_t hA[NR_RXF_GROUP], hB[NR_RXF_GROUP], yA[NR_RXF_GROUP], yB[NR_RXF_GROUP], hv[NR_RXF_GROUP], yv[NR_RXF_GROUP];
            rx_load4(hA, h0 + (size_t)a * ch_stride + hoff);
            rx_load4(hB, h0 + (size_t)a * ch_stride + hoff + G.db);
            rx_load4(yA, y0 + (size_t)a * rx_stride + yoff);
            rx_load4(yB, y0 + (size_t)a * rx_stride + yoff + G.db);
            rxf_grid_pick(hv, hA, hB, G);
            rxf_grid_pick(yv, yA, yB, G);
#pragma unroll
            for (int u = 0; u < NR_RXF_GROUP; u++)
              nr_rxf_mac(&acc[u], hv[u], yv[u], s, amp);
          }
        }
        done = true;
      }
    }
    if (!done) {
      if constexpr (NRX > 0) {
        uint32_t hv[NRX][NR_RXF_GROUP], yv[NRX][NR_RXF_GROUP];
#pragma unroll
        for (int a = 0; a < NRX; a++) {
          rx_load4(hv[a], h0 + (size_t)a * ch_stride + hoff);
          rx_load4(yv[a], y0 + (size_t)a * rx_stride + yoff);
        }
#pragma unroll
        for (int a = 0; a < NRX; a++)
#pragma unroll
          for (int u = 0; u < NR_RXF_GROUP; u++)
            nr_rxf_mac(&acc[u], hv[a][u], yv[a][u], s, amp);
      } else {
        for (uint32_t a = 0; a < nrx; a++) {
          uint32_t hv[NR_RXF_GROUP], yv[NR_RXF_GROUP];
          rx_load4(hv, h0 + (size_t)a * ch_stride + hoff);
          rx_load4(yv, y0 + (size_t)a * rx_stride + yoff);
#pragma unroll
          for (int u = 0; u < NR_RXF_GROUP; u++)
            nr_rxf_mac(&acc[u], hv[u], yv[u], s, amp);
        }
      }
    }
    /* plane 0 at r0 is 16-byte aligned: that is what `phase` was chosen for */
    *reinterpret_cast<rx_u32x4 *>(o + r0) = (rx_u32x4){acc[0].w[0], acc[1].w[0], acc[2].w[0], acc[3].w[0]};
#pragma unroll
    for (uint32_t k = 1; k < 4; k++)
      if (k < np)
        rx_store4(o + (size_t)k * j.plane + r0, acc[0].w[k], acc[1].w[k], acc[2].w[k], acc[3].w[k]);
    return;
  }
  /* head (REs before the first aligned group) and tail; with the grid source also a group that straddles the wrap */
  const int32_t hi = r0 + NR_RXF_GROUP < nb_re ? r0 + NR_RXF_GROUP : nb_re;
  for (int32_t r = r0 < 0 ? 0 : r0; r < hi; r++) {
    nr_rxf_acc_t acc = {};
    uint32_t hr = (uint32_t)r, yr = (uint32_t)r;
    if constexpr (GRID) {
      hr = nr_rxg_p(J.pattern, (uint32_t)r);
      yr = nr_rxg_grid_sc(J.start_re, hr, J.fft_size);
    }
    for (uint32_t a = 0; a < nrx; a++)
      nr_rxf_mac(&acc, h0[(size_t)a * ch_stride + hr], y0[(size_t)a * rx_stride + yr], s, amp);
    o[r] = acc.w[0];
#pragma unroll
    for (uint32_t k = 1; k < 4; k++)
      if (k < np)
        o[(size_t)k * j.plane + r] = acc.w[k];
  }
}

template <int NRX>
__global__ void __launch_bounds__(NR_RXF_THREADS)
nr_rx_compensation_kernel(const rx_front_wg *__restrict__ wgs, const rx_front_seg_job *__restrict__ jobs, const uint32_t *__restrict__ rx,
                          const uint32_t *__restrict__ ch, uint32_t n_rx, uint64_t ant_stride, const int32_t *__restrict__ shift,
                          uint32_t *__restrict__ rec)
{
  rx_compensation_body<NRX, false>(wgs, jobs, rx, ch, n_rx, ant_stride, ant_stride, shift, rec);
}

template <int NRX>
__global__ void __launch_bounds__(NR_RXF_THREADS)
nr_rx_compensation_grid_kernel(const rx_front_wg *__restrict__ wgs, const rx_front_grid_job *__restrict__ jobs, const uint32_t *__restrict__ rx,
                               const uint32_t *__restrict__ ch, uint32_t n_rx, uint64_t rx_ant_stride, uint64_t ch_ant_stride,
                               const int32_t *__restrict__ shift, uint32_t *__restrict__ rec)
{
  rx_compensation_body<NRX, true>(wgs, jobs, rx, ch, n_rx, rx_ant_stride, ch_ant_stride, shift, rec);
}

hipError_t nr_launch_rx_compensation(const rx_front_wg *wgs, uint32_t n_wg, const rx_front_seg_job *jobs, const uint32_t *rx, const uint32_t *ch,
                                     uint32_t n_rx, uint64_t ant_stride, const int32_t *shift, uint32_t *rec, hipStream_t s)
{
  if (n_wg == 0)
    return hipSuccess;
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return hipErrorInvalidValue;
#define RXF_LAUNCH(N) hipLaunchKernelGGL(nr_rx_compensation_kernel<N>, dim3(n_wg), dim3(NR_RXF_THREADS), 0, s, wgs, jobs, rx, ch, n_rx, ant_stride, shift, rec)
  switch (n_rx) {
    case 1: RXF_LAUNCH(1); break;
    case 2: RXF_LAUNCH(2); break;
    case 4: RXF_LAUNCH(4); break;
    case 8: RXF_LAUNCH(8); break;
    default: RXF_LAUNCH(0); break;
  }
#undef RXF_LAUNCH
  return hipGetLastError();
}

hipError_t nr_launch_rx_compensation_grid(const rx_front_wg *wgs, uint32_t n_wg, const rx_front_grid_job *jobs, const uint32_t *rx, const uint32_t *ch,
                                          uint32_t n_rx, uint64_t rx_ant_stride, uint64_t ch_ant_stride, const int32_t *shift, uint32_t *rec,
                                          hipStream_t s)
{
  if (n_wg == 0)
    return hipSuccess;
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return hipErrorInvalidValue;
#define RXF_LAUNCH(N) hipLaunchKernelGGL(nr_rx_compensation_grid_kernel<N>, dim3(n_wg), dim3(NR_RXF_THREADS), 0, s, wgs, jobs, rx, ch, n_rx, rx_ant_stride, ch_ant_stride, shift, rec)
  switch (n_rx) {
    case 1: RXF_LAUNCH(1); break;
    case 2: RXF_LAUNCH(2); break;
    case 4: RXF_LAUNCH(4); break;
    case 8: RXF_LAUNCH(8); break;
    default: RXF_LAUNCH(0); break;
  }
#undef RXF_LAUNCH
  return hipGetLastError();
}

/* ---- channel level: workgroup (block b, antenna a) sums the terms of b's measurement symbol on antenna a; the block's maximum
 * and the count of antennas done are device-scope atomics, and the last antenna to arrive writes log2_maxh (tb_rx_level.h) ---- */
/* GRID: Job = rx_front_grid_lvl_job, term r is the estimate of PUSCH subcarrier p(r) */
template <bool GRID, typename Job>
__device__ __forceinline__ void rx_level_body(const Job *__restrict__ jobs, const uint32_t *__restrict__ ch, uint32_t n_rx, uint64_t ant_stride, int32_t *mx,
                                              int32_t *cnt, int32_t *__restrict__ log2_maxh)
{
  const uint32_t b = blockIdx.x / n_rx, a = blockIdx.x % n_rx;
  const Job j = jobs[b];
  const uint32_t len = nr_rxf_level_len(j.nb_re), x = (uint32_t)nr_rxf_factor2(len);
  const uint32_t *h = ch + j.ch_off + (size_t)a * ant_stride;
  const auto term = [&](uint32_t r) {
    if constexpr (GRID)
      return nr_rxf_level_term(h[nr_rxg_p(j.pattern, r)], x);
    else
      return nr_rxf_level_term(h[r], x);
  };
  rx_level_sum(b, n_rx, j.nb_re, len, term, [&](int32_t avgs) { return nr_rxf_log2_maxh(avgs, n_rx); }, mx, cnt, &log2_maxh[j.tb]);
}

__global__ void __launch_bounds__(NR_RXF_THREADS)
nr_rx_level_kernel(const rx_front_lvl_job *__restrict__ jobs, const uint32_t *__restrict__ ch, uint32_t n_rx, uint64_t ant_stride, int32_t *mx,
                   int32_t *cnt, int32_t *__restrict__ log2_maxh)
{
  rx_level_body<false>(jobs, ch, n_rx, ant_stride, mx, cnt, log2_maxh);
}

__global__ void __launch_bounds__(NR_RXF_THREADS)
nr_rx_level_grid_kernel(const rx_front_grid_lvl_job *__restrict__ jobs, const uint32_t *__restrict__ ch, uint32_t n_rx, uint64_t ant_stride, int32_t *mx,
                        int32_t *cnt, int32_t *__restrict__ log2_maxh)
{
  rx_level_body<true>(jobs, ch, n_rx, ant_stride, mx, cnt, log2_maxh);
}

hipError_t nr_launch_rx_level(const rx_front_lvl_job *jobs, uint32_t n_tb, const uint32_t *ch, uint32_t n_rx, uint64_t ant_stride, int32_t *state,
                              int32_t *log2_maxh, hipStream_t s)
{
  if (n_tb == 0)
    return hipSuccess;
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(nr_rx_level_kernel, dim3(n_tb * n_rx), dim3(NR_RXF_THREADS), 0, s, jobs, ch, n_rx, ant_stride, state, state + n_tb, log2_maxh);
  return hipGetLastError();
}

hipError_t nr_launch_rx_level_grid(const rx_front_grid_lvl_job *jobs, uint32_t n_tb, const uint32_t *ch, uint32_t n_rx, uint64_t ch_ant_stride,
                                   int32_t *state, int32_t *log2_maxh, hipStream_t s)
{
  if (n_tb == 0)
    return hipSuccess;
  if (n_rx < 1 || n_rx > NR_RXF_MAX_RX)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(nr_rx_level_grid_kernel, dim3(n_tb * n_rx), dim3(NR_RXF_THREADS), 0, s, jobs, ch, n_rx, ch_ant_stride, state, state + n_tb,
                     log2_maxh);
  return hipGetLastError();
}
