/*
 * tb_tx_map.hip -- PDSCH resource mapping with DMRS onto the transmit grid for gfx950: one launch per symbol pattern over a
 * host-built workgroup table (descriptor, antenna, piece), nothing searched on the device.  The kernel is memory bound by
 * construction: at most 4 bytes in and 4 bytes out per RE.  A thread owns four consecutive grid REs, laid so that its store is
 * 16-byte aligned (the antenna's first RE rarely is); the head and the tail of an antenna's range and the one group that runs
 * over the wrap at fft_size are written word by word.  The antennas behind the layers receive zeros.  What an RE is, which
 * plane entry or pilot it takes and its value are nr_pdsch_map.h's alone; the host check form runs the same functions.
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

} // namespace

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
