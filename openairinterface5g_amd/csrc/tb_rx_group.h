/*
 * tb_rx_group.h -- what the receive front's kernels share in reading a thread's four REs (NR_RXF_GROUP) from the OFDM grid and the
 * full-width channel estimates: the 16-byte load and store at a 4-byte aligned address and the DMRS1 pick (tb_rx_front.hip,
 * tb_rx_mmse.hip, tb_rx_ml.hip), and, for the two-layer receivers, where a group lies and the loader of its REs.  The groups of
 * the two-layer receivers are counted from the segment's RE 0 (r0 % 4 == 0); the single-layer kernel lays its groups by `phase`
 * and keeps its own locate and pick (tb_rx_front.hip).  The ML kernels load through rx_group_load; the MMSE kernel carries the
 * same steps written out for its one array of 2 n_rx pairs (tb_rx_mmse.hip says why), so what the steps are for is said here.
 */
#ifndef TB_RX_GROUP_H
#define TB_RX_GROUP_H
#include <hip/hip_runtime.h>
#include "nr_rx_grid.h"
#include "tb_rx_front.h"

typedef uint32_t rx_u32x4 __attribute__((ext_vector_type(4)));

/* 16 bytes at a 4-byte aligned address (the inputs' offsets and strides are the caller's; the outputs of the two-layer receivers
 * and planes 1.. of the single-layer one begin at any word) */
__device__ __forceinline__ void rx_load4(uint32_t (&w)[4], const uint32_t *p)
{
  rx_u32x4 v;
  __builtin_memcpy(&v, p, sizeof v);
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}
__device__ __forceinline__ void rx_store4(uint32_t *p, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
  const rx_u32x4 v = {a, b, c, d};
  __builtin_memcpy(p, &v, sizeof v);
}
/* DMRS1, a group's four REs out of one array: PUSCH subcarriers p(r0), + 2, + 4, + 6 = A[0], A[2], B[1], B[3] of load A at p(r0)
 * and load B three c16 behind it; together they cover exactly [p(r0), p(r0 + 3)], nothing outside the segment's own range is
 * read */
__device__ __forceinline__ void rx_pick_dmrs1(uint32_t (&v)[4], const uint32_t (&A)[4], const uint32_t (&B)[4])
{
  v[0] = A[0]; v[1] = A[2]; v[2] = B[1]; v[3] = B[3];
}

/* where a thread's group of a two-layer receiver lies */
struct rx_group {
  uint32_t pattern, start_re, fft_size, r0, nb_re;
  uint32_t pa, ga; /* PUSCH subcarrier of RE r0; its grid subcarrier (fast only) */
  bool whole;      /* all four REs lie within nb_re */
  bool fast;       /* ... and the grid does not wrap inside the group */
};
__device__ __forceinline__ rx_group rx_group_locate(const rx_front_grid_job &J, uint32_t r0)
{
  rx_group G;
  G.pattern = J.pattern;
  G.start_re = J.start_re;
  G.fft_size = J.fft_size;
  G.r0 = r0;
  G.nb_re = J.s.nb_re;
  G.pa = nr_rxg_p(J.pattern, r0);
  const uint32_t span = nr_rxg_p(J.pattern, r0 + 3u) - G.pa, g = J.start_re + G.pa;
  G.whole = r0 + NR_RXF_GROUP <= J.s.nb_re;
  G.fast = G.whole && !(g < J.fft_size && g + span >= J.fft_size);
  G.ga = g >= J.fft_size ? g - J.fft_size : g;
  return G;
}

/* The group's REs of N antennas (y, rx_stride apart) and of their 2 N pairs (h0 / h1 = layer 0's / layer 1's, ch_stride apart),
 * every load issued before the first use.  r0 % 4 == 0, so the four REs are PUSCH subcarriers p(r0) .. p(r0) + 3 for FULL and
 * DMRS2: one load per array; DMRS1: two (rx_pick_dmrs1).  The pattern is tested once around the loads of all arrays, not per
 * array: a branch per array puts a wait for the load in front of the next one.  A group that the grid's wrap cuts, and a partial
 * last group, go RE by RE; the REs behind nb_re read nothing and are zero -- the reference's zero padding
 * (nr_ulsch_demodulation.c:1284-1285), which still enters the sum of determinants that an MMSE quad's shift is taken from. */
template <int N>
__device__ __forceinline__ void rx_group_load(const rx_group &G, const uint32_t *y, uint64_t rx_stride, const uint32_t *h0, const uint32_t *h1,
                                              uint64_t ch_stride, uint32_t (&yv)[N][4], uint32_t (&h0v)[N][4], uint32_t (&h1v)[N][4])
{
  if (G.fast) {
    if (G.pattern == NR_RXG_DMRS1) { /* wave-uniform */
      uint32_t yA[N][4], yB[N][4], gA[N][4], gB[N][4], kA[N][4], kB[N][4];
#pragma unroll
      for (int a = 0; a < N; a++) {
        rx_load4(yA[a], y + (size_t)a * rx_stride + G.ga);
        rx_load4(yB[a], y + (size_t)a * rx_stride + G.ga + 3);
      }
#pragma unroll
      for (int a = 0; a < N; a++) {
        rx_load4(gA[a], h0 + (size_t)a * ch_stride + G.pa);
        rx_load4(gB[a], h0 + (size_t)a * ch_stride + G.pa + 3);
        rx_load4(kA[a], h1 + (size_t)a * ch_stride + G.pa);
        rx_load4(kB[a], h1 + (size_t)a * ch_stride + G.pa + 3);
      }
#pragma unroll
      for (int a = 0; a < N; a++) {
        rx_pick_dmrs1(yv[a], yA[a], yB[a]);
        rx_pick_dmrs1(h0v[a], gA[a], gB[a]);
        rx_pick_dmrs1(h1v[a], kA[a], kB[a]);
      }
    } else {
#pragma unroll
      for (int a = 0; a < N; a++)
        rx_load4(yv[a], y + (size_t)a * rx_stride + G.ga);
#pragma unroll
      for (int a = 0; a < N; a++) {
        rx_load4(h0v[a], h0 + (size_t)a * ch_stride + G.pa);
        rx_load4(h1v[a], h1 + (size_t)a * ch_stride + G.pa);
      }
    }
  } else {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const bool in = G.r0 + u < G.nb_re;
      const uint32_t p = nr_rxg_p(G.pattern, G.r0 + u), sc = nr_rxg_grid_sc(G.start_re, p, G.fft_size);
#pragma unroll
      for (int a = 0; a < N; a++) {
        yv[a][u] = in ? y[(size_t)a * rx_stride + sc] : 0u;
        h0v[a][u] = in ? h0[(size_t)a * ch_stride + p] : 0u;
        h1v[a][u] = in ? h1[(size_t)a * ch_stride + p] : 0u;
      }
    }
  }
}
#endif
