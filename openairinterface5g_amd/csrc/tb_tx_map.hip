/*
 * tb_tx_map.hip -- PDSCH resource mapping with DMRS onto the transmit grid for gfx950: one launch per symbol pattern over a
 * host-built workgroup table (descriptor, antenna, piece), nothing searched on the device.  The kernel is memory bound by
 * construction: at most 4 bytes in and 4 bytes out per RE.  A thread owns four consecutive grid REs, laid so that its store is
 * 16-byte aligned (the antenna's first RE rarely is); the head and the tail of an antenna's range and the one group that runs
 * over the wrap at fft_size are written word by word.  The antennas behind the layers receive zeros.  What an RE is, which
 * plane entry or pilot it takes and its value are nr_pdsch_map.h's alone; the host check form runs the same functions.
 * nr_tx_precode_kernel is the same launch structure with precoding: all layers of an RE, then the antenna's sum (further down).
 *
 * Pilot bits: the workgroup's Gold registers stand at the word of its first pilot; a thread steps them serially to its own word
 * (at most 33 steps: 1024 REs hold at most 512 pilots) and needs at most 4 pilots = 8 bits.
 */
#include "tb_tx_map.h"
#include "nr_pdsch_map.h"
#include "nr_gold.h"

namespace {

typedef uint32_t txm_u32x4 __attribute__((ext_vector_type(4)));

/* 16 bytes at a 4-byte aligned address: the layer planes keep the caller's offsets */
__device__ __forceinline__ void txm_load4(uint32_t (&w)[NR_TXM_GROUP], const uint32_t *p)
{
  txm_u32x4 v;
  __builtin_memcpy(&v, p, sizeof v);
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}

/* sequence bit first_bit in bit 0; two words hold what a group reads */
__device__ __forceinline__ uint64_t txm_bits(const tx_map_wg &w, uint32_t first_bit)
{
  uint32_t a = w.x1, b = w.x2;
  for (uint32_t n = (first_bit >> 5) - w.w0; n != 0; n--) {
    a = nr_gold_step1(a);
    b = nr_gold_step2(b);
  }
  const uint64_t lo = a ^ b, hi = nr_gold_step1(a) ^ nr_gold_step2(b);
  return (lo | (hi << 32)) >> (first_bit & 31u);
}

template <uint32_t PATTERN>
__global__ void __launch_bounds__(NR_TXM_THREADS)
nr_tx_map_kernel(const tx_map_wg *__restrict__ wgs, const tx_map_job *__restrict__ jobs, const uint32_t *__restrict__ layers, uint32_t *__restrict__ tx,
                 uint64_t tx_ant_stride)
{
  const tx_map_wg w = wgs[blockIdx.x];
  const tx_map_job j = jobs[w.job];
  const int32_t n_re = (int32_t)j.n_re;
  const int32_t i0 = (int32_t)((w.piece * NR_TXM_THREADS + threadIdx.x) * NR_TXM_GROUP) - (int32_t)w.phase;
  if (i0 >= n_re)
    return;
  const uint32_t N = j.fft_size, k0 = j.start_re;
  const int32_t at_wrap = (int32_t)(N - k0); /* the allocation subcarrier that lands on grid subcarrier 0 */
  uint32_t *sym = tx + j.tx_off + (uint64_t)w.ant * tx_ant_stride;
  const bool whole = i0 >= 0 && i0 + (int32_t)NR_TXM_GROUP <= n_re && !(i0 < at_wrap && i0 + (int32_t)NR_TXM_GROUP > at_wrap);
  const int32_t lo = i0 < 0 ? 0 : i0, hi = i0 + (int32_t)NR_TXM_GROUP < n_re ? i0 + (int32_t)NR_TXM_GROUP : n_re;

  if (w.ant >= j.Nl) { /* unit precoding: zeros over the same REs */
    if (whole)
      *reinterpret_cast<uint4 *>(sym + nr_pdm_wrap(k0, (uint32_t)i0, N)) = make_uint4(0u, 0u, 0u, 0u);
    else
      for (int32_t i = lo; i < hi; i++)
        sym[nr_pdm_wrap(k0, (uint32_t)i, N)] = 0u;
    return;
  }

  const nr_pdm_sym s = nr_pdm_sym_make(PATTERN, j.ncdm, j.l_prime, (j.ports >> (8u * w.ant)) & 0xffu, j.amp);
  const uint32_t *lay = layers + j.lay_off + (uint64_t)w.ant * j.plane;
  uint64_t bits = 0;
  uint32_t jlo = 0;
  if constexpr (PATTERN != NR_PDM_FULL) {
    jlo = nr_pdm_count(s.pmask, (uint32_t)lo);
    bits = txm_bits(w, 2u * (j.dmrs_offset + jlo));
  }
  if (whole) {
    uint32_t o[NR_TXM_GROUP];
    if constexpr (PATTERN == NR_PDM_FULL) {
      uint32_t x[NR_TXM_GROUP];
      txm_load4(x, lay + i0);
#pragma unroll
      for (uint32_t u = 0; u < NR_TXM_GROUP; u++)
        o[u] = nr_pdm_mulhrs(x[u], s.amp);
    } else {
#pragma unroll
      for (uint32_t u = 0; u < NR_TXM_GROUP; u++)
        o[u] = nr_pdm_re(&s, lay, (uint32_t)i0 + u, bits, jlo);
    }
    *reinterpret_cast<uint4 *>(sym + nr_pdm_wrap(k0, (uint32_t)i0, N)) = make_uint4(o[0], o[1], o[2], o[3]);
  } else {
    for (int32_t i = lo; i < hi; i++)
      sym[nr_pdm_wrap(k0, (uint32_t)i, N)] = nr_pdm_re(&s, lay, (uint32_t)i, bits, jlo);
  }
}

/* The same mapping followed by precoding: a thread forms the values of all Nl layers of its four REs (one run of Gold bits, one
 * 16-byte plane load per layer in a FULL symbol) and from them the value of its one antenna.  Its REs lie in at most two RBs, so in
 * at most two PRGs: the weights of both are read once, an RE selects by its index.  Where both PRGs are unit only the antenna's own
 * layer is formed, and none behind the layers. */
template <uint32_t PATTERN>
__global__ void __launch_bounds__(NR_TXM_THREADS)
nr_tx_precode_kernel(const tx_map_wg *__restrict__ wgs, const tx_map_job *__restrict__ jobs, const tx_map_prg *__restrict__ prgs,
                     const uint16_t *__restrict__ pmx, const tx_map_pm *__restrict__ mats, const uint32_t *__restrict__ layers, uint32_t *__restrict__ tx,
                     uint64_t tx_ant_stride)
{
  const tx_map_wg w = wgs[blockIdx.x];
  const tx_map_job j = jobs[w.job];
  const int32_t n_re = (int32_t)j.n_re;
  const int32_t i0 = (int32_t)((w.piece * NR_TXM_THREADS + threadIdx.x) * NR_TXM_GROUP) - (int32_t)w.phase;
  if (i0 >= n_re)
    return;
  const uint32_t N = j.fft_size, k0 = j.start_re, Nl = j.Nl, ant = w.ant;
  const int32_t at_wrap = (int32_t)(N - k0);
  uint32_t *sym = tx + j.tx_off + (uint64_t)ant * tx_ant_stride;
  const bool whole = i0 >= 0 && i0 + (int32_t)NR_TXM_GROUP <= n_re && !(i0 < at_wrap && i0 + (int32_t)NR_TXM_GROUP > at_wrap);
  const int32_t lo = i0 < 0 ? 0 : i0, hi = i0 + (int32_t)NR_TXM_GROUP < n_re ? i0 + (int32_t)NR_TXM_GROUP : n_re;

  /* the PRGs of the first and of the last RE; REs from i_split on belong to the second */
  const tx_map_prg g = prgs[w.job];
  const uint32_t q_lo = ((uint32_t)lo / 12u) / g.prg_size, q_hi = ((uint32_t)(hi - 1) / 12u) / g.prg_size;
  const uint32_t pm_lo = pmx[g.pmx_off + q_lo], pm_hi = pmx[g.pmx_off + q_hi];
  const uint32_t i_split = q_hi * g.prg_size * 12u;
  const bool all_unit = (pm_lo | pm_hi) == 0u;
  uint32_t w_lo[NR_PDM_MAX_LAYERS], w_hi[NR_PDM_MAX_LAYERS];
#pragma unroll
  for (uint32_t l = 0; l < NR_PDM_MAX_LAYERS; l++) {
    w_lo[l] = pm_lo && l < Nl ? mats[pm_lo - 1u].w[l][ant] : 0u;
    w_hi[l] = pm_hi && l < Nl ? mats[pm_hi - 1u].w[l][ant] : 0u;
  }

  nr_pdm_sym s[NR_PDM_MAX_LAYERS];
  const uint32_t *lay[NR_PDM_MAX_LAYERS];
  bool need[NR_PDM_MAX_LAYERS];
#pragma unroll
  for (uint32_t l = 0; l < NR_PDM_MAX_LAYERS; l++) {
    s[l] = nr_pdm_sym_make(PATTERN, j.ncdm, j.l_prime, (j.ports >> (8u * l)) & 0xffu, j.amp);
    lay[l] = layers + j.lay_off + (uint64_t)l * j.plane;
    need[l] = l < Nl && (!all_unit || l == ant);
  }
  uint64_t bits = 0;
  uint32_t jlo = 0;
  if constexpr (PATTERN != NR_PDM_FULL) {
    jlo = nr_pdm_count(nr_pdm_last_pmask(PATTERN), (uint32_t)lo);
    bits = txm_bits(w, 2u * (j.dmrs_offset + jlo));
  }
  if (whole) {
    uint32_t m[NR_PDM_MAX_LAYERS][NR_TXM_GROUP], o[NR_TXM_GROUP];
#pragma unroll
    for (uint32_t l = 0; l < NR_PDM_MAX_LAYERS; l++) {
#pragma unroll
      for (uint32_t u = 0; u < NR_TXM_GROUP; u++)
        m[l][u] = 0u;
      if (need[l]) {
        if constexpr (PATTERN == NR_PDM_FULL) {
          uint32_t x[NR_TXM_GROUP];
          txm_load4(x, lay[l] + i0);
#pragma unroll
          for (uint32_t u = 0; u < NR_TXM_GROUP; u++)
            m[l][u] = nr_pdm_mulhrs(x[u], s[l].amp);
        } else {
#pragma unroll
          for (uint32_t u = 0; u < NR_TXM_GROUP; u++)
            m[l][u] = nr_pdm_re(&s[l], lay[l], (uint32_t)i0 + u, bits, jlo);
        }
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < NR_TXM_GROUP; u++) {
      const bool second = (uint32_t)i0 + u >= i_split;
      uint32_t mu[NR_PDM_MAX_LAYERS], wu[NR_PDM_MAX_LAYERS];
#pragma unroll
      for (uint32_t l = 0; l < NR_PDM_MAX_LAYERS; l++) {
        mu[l] = m[l][u];
        wu[l] = second ? w_hi[l] : w_lo[l];
      }
      o[u] = nr_pdm_antenna(mu, wu, Nl, ant, second ? pm_hi : pm_lo);
    }
    *reinterpret_cast<uint4 *>(sym + nr_pdm_wrap(k0, (uint32_t)i0, N)) = make_uint4(o[0], o[1], o[2], o[3]);
  } else {
    for (int32_t i = lo; i < hi; i++) {
      const bool second = (uint32_t)i >= i_split;
      uint32_t mu[NR_PDM_MAX_LAYERS], wu[NR_PDM_MAX_LAYERS];
#pragma unroll
      for (uint32_t l = 0; l < NR_PDM_MAX_LAYERS; l++) {
        mu[l] = need[l] ? nr_pdm_re(&s[l], lay[l], (uint32_t)i, bits, jlo) : 0u;
        wu[l] = second ? w_hi[l] : w_lo[l];
      }
      sym[nr_pdm_wrap(k0, (uint32_t)i, N)] = nr_pdm_antenna(mu, wu, Nl, ant, second ? pm_hi : pm_lo);
    }
  }
}

} // namespace

hipError_t nr_launch_tx_precode(uint32_t pattern, const tx_map_wg *wgs, uint32_t n_wg, const tx_map_job *jobs, const tx_map_prg *prgs, const uint16_t *pmx,
                                const tx_map_pm *mats, const uint32_t *lay, uint32_t *tx, uint64_t tx_ant_stride, hipStream_t s)
{
  if (n_wg == 0)
    return hipSuccess;
#define TXP_LAUNCH(P) \
  hipLaunchKernelGGL(nr_tx_precode_kernel<P>, dim3(n_wg), dim3(NR_TXM_THREADS), 0, s, wgs, jobs, prgs, pmx, mats, lay, tx, tx_ant_stride)
  switch (pattern) {
    case NR_PDM_FULL: TXP_LAUNCH(NR_PDM_FULL); break;
    case NR_PDM_DMRS1: TXP_LAUNCH(NR_PDM_DMRS1); break;
    case NR_PDM_DMRS2: TXP_LAUNCH(NR_PDM_DMRS2); break;
    default: return hipErrorInvalidValue;
  }
#undef TXP_LAUNCH
  return hipGetLastError();
}

hipError_t nr_launch_tx_map(uint32_t pattern, const tx_map_wg *wgs, uint32_t n_wg, const tx_map_job *jobs, const uint32_t *lay, uint32_t *tx,
                            uint64_t tx_ant_stride, hipStream_t s)
{
  if (n_wg == 0)
    return hipSuccess;
#define TXM_LAUNCH(P) hipLaunchKernelGGL(nr_tx_map_kernel<P>, dim3(n_wg), dim3(NR_TXM_THREADS), 0, s, wgs, jobs, lay, tx, tx_ant_stride)
  switch (pattern) {
    case NR_PDM_FULL: TXM_LAUNCH(NR_PDM_FULL); break;
    case NR_PDM_DMRS1: TXM_LAUNCH(NR_PDM_DMRS1); break;
    case NR_PDM_DMRS2: TXM_LAUNCH(NR_PDM_DMRS2); break;
    default: return hipErrorInvalidValue;
  }
#undef TXM_LAUNCH
  return hipGetLastError();
}
