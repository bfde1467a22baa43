/*
 * nr_chest.h -- PUSCH DMRS channel estimation of one OFDM symbol, one output unit at a time: nr_pusch_channel_estimation()
 * (openair1/PHY/NR_ESTIMATION/nr_ul_channel_estimation.c:67-473) with the pilots of nr_pusch_dmrs_rx()
 * (openair1/PHY/NR_REFSIG/nr_dmrs_rx.c:67-116) and the helper semantics of openair1/PHY/TOOLS/tools_defs.h:182-329.  Plain C (no
 * HIP headers): the host check form (rx_chest_api.inc.cpp) and the kernel (tb_rx_chest.hip) compute with the same definitions.
 *
 * A c16 is one 32-bit word, r in the low half.  rx points at subcarrier 0 of the symbol of one antenna, k0 =
 * bwp_start_subcarrier (:93, the allocation's start_re), N = ofdm_symbol_size.  Every read is relative to the symbol.
 *
 * Pilots (nr_dmrs_rx.c:84-99): pilot k of the allocation is sequence symbol i = dmrs_offset + k of the Gold sequence of
 * c_init (nr_gold.c:107-108); idx = (bit(2i) << 1) ^ bit(2i + 1) picks the conjugated QPSK point (nr_dmrs_rx.c:54-57: r =
 * -23170 when bit(2i), i = +23170 when bit(2i + 1)), negated when wf[p][i & 1] == -1, that is for odd ports at odd i (:45, :48);
 * lp = 0 (nr_ul_channel_estimation.c:119) so wt = 1.  A unit receives its pilots' bits as one 64-bit value, pilot plo's first.
 *
 * The four estimators, and the unit each is computed in:
 *   TYPE1_INTERP (:167-257)  4-RE group g of the 3 rb_size groups.  LS value of pilot pair n (:176-192): the two products at
 *     shift 16 added in int32, cast to int16; read at (k0 + 4n + 2 k_line + delta) % N (:181).  Pilot pc = 2n + k_line is that value
 *     rotated by delay_table[idx(d)][2 pc] at shift 8 (:209-210).  The window filters (:219-230, filt16a_32.h:242-249) are constant
 *     over groups of four REs; with the running ul_ch pointer resolved, pilot pc adds weight w(pc, g) to group g:
 *        pc = 0                  4096 to g = 0, 1                         (p0)
 *        pc = 1, 2               4096 to g = 0, 2048 to g = 1, 2          (p1p2)
 *        pc = 6 rb_size - 1      4096 to g = gs, 8192 to g = gs + 1       (last)
 *        every other pc          2048 to g = gs .. gs + 3                 (middle),  gs = (pc - 3) >> 1
 *     (the pointer advances by 4 after an even middle pilot, :227-229).  Each addition is c16multaddVectRealComplex
 *     (tools_defs.h:266-298): m = mulhrs(value, w) = (value w + 2^14) >> 15, t = adds(m, m), y = adds(t, y), saturating, so
 *     the order of the pilots is observable and is kept: ascending pc.  Group g receives pilots max(0, 2g - 3) .. min(6 rb_size
 *     - 1, 2g + 4) and no others, all four REs of it the same sum; RE 4g + j is then rotated by delay_table[idx(-d)][4g + j]
 *     (:243-245).  The accumulation starts from the reference's memset zeros (:159).
 *   TYPE2_INTERP (:259-283)  4-RE group; RE n lies in 6-RE block m = n / 6: ch0, ch1 = pilot x rx at shift 15, cast (:264-266),
 *     ch = (ch0 + ch1) >> 1 (:268); REs 0..3 of the block take mulhi_s1 (tools_defs.h:47: mulhi << 2) of ch and 16384, that is
 *     ch & ~3, through two saturating adds to zero (:270); REs 4, 5 take ch (:271-272); then delay_table[idx(-d)][n % 6] (:279-282).
 *     Reads at ((k0 + 6m + {0,1}) % N) + nushift: the wrap comes before nushift (:262-266).
 *   TYPE1_AVG (:287-343, the NO_INTERP build)  PRB b: six products at shift 15 summed in int32, / 6 towards zero, cast
 *     (:45-65), pilots 6b .. 6b + 5 at ((k0 + 12b + 2t) % N) + nushift, replicated over the PRB.
 *   TYPE2_AVG (:344-450)  PRB b: four products, / 4; pilots 4b .. 4b + 3 at ((k0 + 12b + 6m + {0,1}) % N) + nushift.  Two defects
 *     of the reference are not reproduced: its reads without soffset (:355-368, :388-435) and its first PRB
 *     using pilot 2 twice, which leaves every later PRB one pilot behind (:361-370).
 * nushift = (p >> 1) & 1 for both types (:89), delta = delta1[p] (nr_dmrs_rx.c:44).
 *
 * The delay is an input.  nr_est_delay (common/utils/nr/nr_common.c:968-990) finds it with a fixed-point IDFT that is not
 * rebuilt here; the caller passes est_delay per antenna, from nr_delay.h's fp32 search of the same LS values or from anywhere
 * else.  Note that the reference clears delay_t once per call and not per
 * antenna (:152-153): its delay_max_val is a running maximum, so antenna a's delay there depends on antennas 0 .. a.
 * Delay tables (nr_common.c:906-928): row get_delay_idx(d) = clamp(20 + d, 0, 40), entry k = round(256 cexp(i 2 pi k d / N)).
 */
#ifndef NR_CHEST_H
#define NR_CHEST_H
#include <stdint.h>

#if defined(__HIPCC__)
#define NR_CHE_HD __host__ __device__ static inline
#else
#define NR_CHE_HD static inline
#endif

#define NR_CHE_TYPE1_INTERP 0u
#define NR_CHE_TYPE2_INTERP 1u
#define NR_CHE_TYPE1_AVG 2u
#define NR_CHE_TYPE2_AVG 3u
#define NR_CHE_MODES 4u
#define NR_CHE_MAX_DELAY 20 /* MAX_DELAY_COMP */
#define NR_CHE_DELAY_ROWS (2 * NR_CHE_MAX_DELAY + 1)

typedef struct nr_che_c {
  int32_t r, i;
} nr_che_c;

NR_CHE_HD uint32_t nr_che_is_type2(uint32_t mode) { return mode & 1u; }
NR_CHE_HD uint32_t nr_che_is_avg(uint32_t mode) { return mode >> 1; }
NR_CHE_HD uint32_t nr_che_ports(uint32_t mode) { return nr_che_is_type2(mode) ? 12u : 8u; } /* nr_dmrs_rx.c:89 */
NR_CHE_HD uint32_t nr_che_nushift(uint32_t port) { return (port >> 1) & 1u; }                /* :89 */
NR_CHE_HD uint32_t nr_che_delta1(uint32_t port) { return (port >> 1) & 1u; }                 /* nr_dmrs_rx.c:44 */
/* pilots per PRB and output units of an allocation */
NR_CHE_HD uint32_t nr_che_pilots_per_rb(uint32_t mode) { return nr_che_is_type2(mode) ? 4u : 6u; }
NR_CHE_HD uint32_t nr_che_units(uint32_t mode, uint32_t rb_size) { return nr_che_is_avg(mode) ? rb_size : 3u * rb_size; }
NR_CHE_HD uint32_t nr_che_unit_res(uint32_t mode) { return nr_che_is_avg(mode) ? 12u : 4u; }
/* get_delay_idx (nr_common.c:906-914) */
NR_CHE_HD uint32_t nr_che_delay_idx(int32_t d)
{
  const int32_t c = d < -NR_CHE_MAX_DELAY ? -NR_CHE_MAX_DELAY : (d > NR_CHE_MAX_DELAY ? NR_CHE_MAX_DELAY : d);
  return (uint32_t)(NR_CHE_MAX_DELAY + c);
}
NR_CHE_HD uint32_t nr_che_inv_delay_idx(int32_t d) { return 2u * NR_CHE_MAX_DELAY - nr_che_delay_idx(d); }

NR_CHE_HD nr_che_c nr_che_unpack(uint32_t w)
{
  nr_che_c c;
  c.r = (int16_t)(w & 0xffffu);
  c.i = (int16_t)(w >> 16);
  return c;
}
NR_CHE_HD uint32_t nr_che_pack(nr_che_c c) { return ((uint32_t)c.r & 0xffffu) | ((uint32_t)c.i << 16); }
NR_CHE_HD int32_t nr_che_cast16(int32_t x) { return (int16_t)x; }
NR_CHE_HD int32_t nr_che_sat16(int32_t x) { return x > 32767 ? 32767 : (x < -32768 ? -32768 : x); }
/* (a b) >> s in int32 (c32x16mulShift, tools_defs.h:233-238); one factor is a pilot or a table entry, so nothing overflows */
NR_CHE_HD nr_che_c nr_che_mul_shift(nr_che_c a, nr_che_c b, int s)
{
  nr_che_c c;
  c.r = (a.r * b.r - a.i * b.i) >> s;
  c.i = (a.r * b.i + a.i * b.r) >> s;
  return c;
}
/* c16mulShift (tools_defs.h:207-212) */
NR_CHE_HD nr_che_c nr_che_mul_shift16(nr_che_c a, nr_che_c b, int s)
{
  nr_che_c c = nr_che_mul_shift(a, b, s);
  c.r = nr_che_cast16(c.r);
  c.i = nr_che_cast16(c.i);
  return c;
}
/* one term of c16multaddVectRealComplex (tools_defs.h:289-294) */
NR_CHE_HD int32_t nr_che_madd(int32_t y, int32_t alpha, int32_t w)
{
  const int32_t m = nr_che_cast16((alpha * w + 16384) >> 15);
  return nr_che_sat16(y + nr_che_sat16(m + m));
}

/* first pilot of the allocation that unit u reads, and how many it reads at the most (10) */
NR_CHE_HD uint32_t nr_che_unit_first_pilot(uint32_t mode, uint32_t u)
{
  if (mode == NR_CHE_TYPE1_INTERP)
    return u >= 2u ? ((2u * u - 3u) >> 1) << 1 : 0u;
  if (mode == NR_CHE_TYPE2_INTERP)
    return 2u * ((4u * u) / 6u);
  return nr_che_pilots_per_rb(mode) * u;
}
/* the conjugated pilot: sequence symbol i, its two bits in the low bits of b (nr_dmrs_rx.c:94-99) */
NR_CHE_HD nr_che_c nr_che_pilot(uint32_t b, uint32_t i, uint32_t port)
{
  nr_che_c c;
  c.r = (b & 1u) ? -23170 : 23170;
  c.i = (b & 2u) ? 23170 : -23170;
  if (port & i & 1u) {
    c.r = -c.r;
    c.i = -c.i;
  }
  return c;
}
/* pilot k of the allocation from the unit's bits */
NR_CHE_HD nr_che_c nr_che_unit_pilot(uint64_t bits, uint32_t plo, uint32_t k, uint32_t dmrs_offset, uint32_t port)
{
  return nr_che_pilot((uint32_t)(bits >> (2u * (k - plo))) & 3u, dmrs_offset + k, port);
}
/* (k0 + off) % N for k0 < N, off < N */
NR_CHE_HD uint32_t nr_che_wrap(uint32_t k0, uint32_t off, uint32_t N) { return k0 + off >= N ? k0 + off - N : k0 + off; }

/* the largest grid index an allocation reads; the descriptor is refused when it reaches N (the wrap precedes nushift) */
NR_CHE_HD uint32_t nr_che_reaches_n(uint32_t mode, uint32_t port, uint32_t N, uint32_t k0, uint32_t rb_size)
{
  if (mode == NR_CHE_TYPE1_INTERP || !nr_che_nushift(port))
    return 0;
  /* some pilot RE at grid index N - 1 before the shift */
  for (uint32_t b = 0; b < rb_size; b++)
    for (uint32_t t = 0; t < 12u; t++) {
      const uint32_t used = mode == NR_CHE_TYPE1_AVG ? !(t & 1u) : (t % 6u < 2u);
      if (used && nr_che_wrap(k0, 12u * b + t, N) == N - 1u)
        return 1;
    }
  return 0;
}

/* TYPE1_INTERP, group g: out[4] */
NR_CHE_HD void nr_che_t1_interp(const uint32_t *rx, uint32_t N, uint32_t k0, uint32_t rb_size, uint32_t port, uint32_t dmrs_offset, uint64_t bits,
                                const uint32_t *fwd, const uint32_t *inv, uint32_t g, uint32_t *out)
{
  const uint32_t P = 6u * rb_size, delta = nr_che_delta1(port);
  const uint32_t lo = g >= 2u ? 2u * g - 3u : 0u, hi = 2u * g + 4u < P - 1u ? 2u * g + 4u : P - 1u;
  const uint32_t plo = nr_che_unit_first_pilot(NR_CHE_TYPE1_INTERP, g);
  nr_che_c acc = {0, 0};
  for (uint32_t n = lo >> 1; n <= hi >> 1; n++) {
    /* LS estimate of the pair (:178-186) */
    nr_che_c ls = {0, 0};
    for (uint32_t kl = 0; kl < 2u; kl++) {
      const nr_che_c x = nr_che_unpack(rx[nr_che_wrap(k0, 4u * n + 2u * kl + delta, N)]);
      const nr_che_c t = nr_che_mul_shift(nr_che_unit_pilot(bits, plo, 2u * n + kl, dmrs_offset, port), x, 16);
      ls.r += t.r;
      ls.i += t.i;
    }
    ls.r = nr_che_cast16(ls.r);
    ls.i = nr_che_cast16(ls.i);
    for (uint32_t pc = 2u * n; pc <= 2u * n + 1u; pc++) {
      if (pc < lo || pc > hi)
        continue;
      int32_t w;
      const uint32_t gs = (pc - 3u) >> 1; /* pc >= 3 where it is used */
      if (pc == 0u)
        w = g < 2u ? 4096 : 0;
      else if (pc <= 2u)
        w = g == 0u ? 4096 : (g <= 2u ? 2048 : 0);
      else if (pc == P - 1u)
        w = g == gs ? 4096 : (g == gs + 1u ? 8192 : 0);
      else
        w = (g >= gs && g <= gs + 3u) ? 2048 : 0;
      if (w == 0)
        continue; /* adds 0: no effect */
      const nr_che_c ch = nr_che_mul_shift16(ls, nr_che_unpack(fwd[2u * pc]), 8);
      acc.r = nr_che_madd(acc.r, ch.r, w);
      acc.i = nr_che_madd(acc.i, ch.i, w);
    }
  }
  for (uint32_t j = 0; j < 4u; j++)
    out[j] = nr_che_pack(nr_che_mul_shift16(acc, nr_che_unpack(inv[4u * g + j]), 8));
}

/* TYPE2_INTERP: the pair value of 6-RE block m (:264-268) */
NR_CHE_HD nr_che_c nr_che_t2_block(const uint32_t *rx, uint32_t N, uint32_t k0, uint32_t port, uint32_t dmrs_offset, uint64_t bits, uint32_t plo,
                                   uint32_t m)
{
  const uint32_t nu = nr_che_nushift(port);
  const nr_che_c c0 = nr_che_mul_shift16(nr_che_unit_pilot(bits, plo, 2u * m, dmrs_offset, port), nr_che_unpack(rx[nr_che_wrap(k0, 6u * m, N) + nu]), 15);
  const nr_che_c c1 =
      nr_che_mul_shift16(nr_che_unit_pilot(bits, plo, 2u * m + 1u, dmrs_offset, port), nr_che_unpack(rx[nr_che_wrap(k0, 6u * m + 1u, N) + nu]), 15);
  nr_che_c c;
  c.r = nr_che_cast16((c0.r + c1.r) >> 1);
  c.i = nr_che_cast16((c0.i + c1.i) >> 1);
  return c;
}
/* TYPE2_INTERP, group g: out[4]; inv = row idx(-d) */
NR_CHE_HD void nr_che_t2_interp(const uint32_t *rx, uint32_t N, uint32_t k0, uint32_t port, uint32_t dmrs_offset, uint64_t bits, const uint32_t *inv,
                                uint32_t g, uint32_t *out)
{
  const uint32_t m0 = (4u * g) / 6u, m1 = (4u * g + 3u) / 6u, plo = 2u * m0;
  const nr_che_c a = nr_che_t2_block(rx, N, k0, port, dmrs_offset, bits, plo, m0);
  const nr_che_c b = m1 != m0 ? nr_che_t2_block(rx, N, k0, port, dmrs_offset, bits, plo, m1) : a;
  for (uint32_t j = 0; j < 4u; j++) {
    const uint32_t n = 4u * g + j, r = n % 6u;
    nr_che_c c = n / 6u == m0 ? a : b;
    if (r < 4u) { /* mulhi_s1 with 16384: (x >> 2) << 2; the two saturating adds to zero change nothing */
      c.r = nr_che_sat16(nr_che_sat16(nr_che_cast16((c.r >> 2) * 4)));
      c.i = nr_che_sat16(nr_che_sat16(nr_che_cast16((c.i >> 2) * 4)));
    }
    out[j] = nr_che_pack(nr_che_mul_shift16(c, nr_che_unpack(inv[r]), 8));
  }
}

/* TYPE1_AVG / TYPE2_AVG, PRB b: the one value of its 12 REs */
NR_CHE_HD uint32_t nr_che_avg(uint32_t mode, const uint32_t *rx, uint32_t N, uint32_t k0, uint32_t port, uint32_t dmrs_offset, uint64_t bits,
                              uint32_t b)
{
  const uint32_t nu = nr_che_nushift(port), np = nr_che_pilots_per_rb(mode), plo = np * b;
  nr_che_c s = {0, 0};
  for (uint32_t t = 0; t < np; t++) {
    const uint32_t off = mode == NR_CHE_TYPE1_AVG ? 12u * b + 2u * t : 12u * b + 6u * (t >> 1) + (t & 1u);
    const nr_che_c p = nr_che_mul_shift(nr_che_unit_pilot(bits, plo, plo + t, dmrs_offset, port), nr_che_unpack(rx[nr_che_wrap(k0, off, N) + nu]), 15);
    s.r += p.r;
    s.i += p.i;
  }
  s.r = nr_che_cast16(s.r / (int32_t)np);
  s.i = nr_che_cast16(s.i / (int32_t)np);
  return nr_che_pack(s);
}

/*
 * The measurements of a call, max_ch and nvar (:187, :246-247, :269, :273, :311, :405, :468-469), one output unit at a time next
 * to the unit's estimates.  A call's results are max_ch, an int32 maximum, and noise_amp2, a uint64 sum, over all antennas; both
 * are order-free, so each unit hands back its own share:
 *   TYPE1_INTERP  group g holds REs 4g .. 4g + 3, whose ul_ls_est is the cast LS value of pair g (:188-190).  Its share: the
 *     maximum over |r|, |i| of pair g's int32 LS value BEFORE the cast (:186-187), and c16amp2(c16sub(ls16, ul_ch[k])) of its four
 *     REs (:246-247) against the estimates the unit stores; c16sub wraps to int16, c16amp2 is a uint32.  nest_count: 12 rb_size
 *     per antenna (:255).
 *   TYPE2_INTERP  pair m (6-RE block m) belongs to the group that holds RE 6m, g = 6m / 4, and to no other: its share is the
 *     maximum over ch (:269) and c16amp2(c16sub(ch0, ch)) (:273).  nest_count: 2 rb_size per antenna (:274).
 *   TYPE1_AVG / TYPE2_AVG  PRB b counts for the maximum when 1 <= b <= rb_size - 2 (:309-311, :386-405: the first and the last
 *     PRB's code has no max_ch line); no noise term, nest_count 0.
 * |x| is taken in int32: an int16 -32768 gives 32768.
 */
NR_CHE_HD int32_t nr_che_abs_max(int32_t m, nr_che_c c)
{
  const int32_t r = c.r < 0 ? -c.r : c.r, i = c.i < 0 ? -c.i : c.i;
  const int32_t v = r > i ? r : i;
  return m > v ? m : v;
}
/* c16amp2(c16sub(a, b)) (tools_defs.h:182-191) */
NR_CHE_HD uint32_t nr_che_sub_amp2(nr_che_c a, nr_che_c b)
{
  const int32_t r = nr_che_cast16(a.r - b.r), i = nr_che_cast16(a.i - b.i);
  return (uint32_t)(r * r) + (uint32_t)(i * i);
}
/* calls per antenna of nest_count's increments */
NR_CHE_HD uint32_t nr_che_nest_per_antenna(uint32_t mode, uint32_t rb_size)
{
  return mode == NR_CHE_TYPE1_INTERP ? 12u * rb_size : (mode == NR_CHE_TYPE2_INTERP ? 2u * rb_size : 0u);
}
/* TYPE1_INTERP: the int32 LS value of pair n before the cast (:178-185); bits from pilot plo on */
NR_CHE_HD nr_che_c nr_che_t1_ls32(const uint32_t *rx, uint32_t N, uint32_t k0, uint32_t port, uint32_t dmrs_offset, uint64_t bits, uint32_t plo, uint32_t n)
{
  const uint32_t delta = nr_che_delta1(port);
  nr_che_c ls = {0, 0};
  for (uint32_t kl = 0; kl < 2u; kl++) {
    const nr_che_c x = nr_che_unpack(rx[nr_che_wrap(k0, 4u * n + 2u * kl + delta, N)]);
    const nr_che_c t = nr_che_mul_shift(nr_che_unit_pilot(bits, plo, 2u * n + kl, dmrs_offset, port), x, 16);
    ls.r += t.r;
    ls.i += t.i;
  }
  return ls;
}
/* TYPE1_INTERP, group g with its stored estimates out[4]: max_ch = max(max_ch, ...), the group's four noise terms */
NR_CHE_HD uint64_t nr_che_t1_meas(const uint32_t *rx, uint32_t N, uint32_t k0, uint32_t port, uint32_t dmrs_offset, uint64_t bits, uint32_t g,
                                  const uint32_t *out, int32_t *max_ch)
{
  nr_che_c ls = nr_che_t1_ls32(rx, N, k0, port, dmrs_offset, bits, nr_che_unit_first_pilot(NR_CHE_TYPE1_INTERP, g), g);
  *max_ch = nr_che_abs_max(*max_ch, ls);
  ls.r = nr_che_cast16(ls.r);
  ls.i = nr_che_cast16(ls.i);
  uint64_t noise = 0;
  for (uint32_t j = 0; j < 4u; j++)
    noise += nr_che_sub_amp2(ls, nr_che_unpack(out[j]));
  return noise;
}
/* TYPE2_INTERP: ch0 of 6-RE block m (:264) */
NR_CHE_HD nr_che_c nr_che_t2_ch0(const uint32_t *rx, uint32_t N, uint32_t k0, uint32_t port, uint32_t dmrs_offset, uint64_t bits, uint32_t plo, uint32_t m)
{
  return nr_che_mul_shift16(nr_che_unit_pilot(bits, plo, 2u * m, dmrs_offset, port), nr_che_unpack(rx[nr_che_wrap(k0, 6u * m, N) + nr_che_nushift(port)]),
                            15);
}
/* TYPE2_INTERP, group g: the share of the pair it owns, if it owns one (blocks < n_blocks = 2 rb_size) */
NR_CHE_HD uint64_t nr_che_t2_meas(const uint32_t *rx, uint32_t N, uint32_t k0, uint32_t port, uint32_t dmrs_offset, uint64_t bits, uint32_t g,
                                  int32_t *max_ch)
{
  const uint32_t m0 = (4u * g) / 6u, m = (4u * g + 3u) / 6u, plo = 2u * m0;
  if ((6u * m) / 4u != g) /* RE 6m lies in another group (m0 < m: in the one before) */
    return 0;
  const nr_che_c ch = nr_che_t2_block(rx, N, k0, port, dmrs_offset, bits, plo, m);
  *max_ch = nr_che_abs_max(*max_ch, ch);
  return nr_che_sub_amp2(nr_che_t2_ch0(rx, N, k0, port, dmrs_offset, bits, plo, m), ch);
}
/* TYPE1_AVG / TYPE2_AVG, PRB b with its value v */
NR_CHE_HD int32_t nr_che_avg_meas(uint32_t rb_size, uint32_t b, uint32_t v, int32_t max_ch)
{
  return (b >= 1u && b + 2u <= rb_size) ? nr_che_abs_max(max_ch, nr_che_unpack(v)) : max_ch;
}
/* the call's nvar_tmp (:468-469; the caller's variable starts at 0, nr_ulsch_demodulation.c:1481) */
NR_CHE_HD uint32_t nr_che_nvar_tmp(uint64_t noise_amp2, uint32_t nest_count) { return nest_count ? (uint32_t)(noise_amp2 / nest_count) : 0u; }

/*
 * nr_chest_time_domain_avg (openair1/PHY/NR_REFSIG/dmrs_nr.c:343-417), one c16: w[0 .. n - 1] = the entry in the n DMRS symbols
 * in symbol order.  The later symbols are added to the first with adds_epi16, saturating per component and one after the other
 * (:358-370); then >> 1 for two symbols (:372-378), >> 2 for four (:379-385), C's / 3 for three (:386-414: towards zero).
 */
NR_CHE_HD int32_t nr_che_tavg16(int32_t acc, uint32_t n)
{
  return n == 2u ? acc >> 1 : (n == 4u ? acc >> 2 : (n == 3u ? acc / 3 : acc));
}
/* one later symbol's entry added to the running sum; the sum divided */
NR_CHE_HD uint32_t nr_che_tavg_add(uint32_t acc, uint32_t x)
{
  nr_che_c a = nr_che_unpack(acc);
  const nr_che_c b = nr_che_unpack(x);
  a.r = nr_che_sat16(a.r + b.r);
  a.i = nr_che_sat16(a.i + b.i);
  return nr_che_pack(a);
}
NR_CHE_HD uint32_t nr_che_tavg_div(uint32_t acc, uint32_t n)
{
  nr_che_c a = nr_che_unpack(acc);
  a.r = nr_che_tavg16(a.r, n);
  a.i = nr_che_tavg16(a.i, n);
  return nr_che_pack(a);
}
NR_CHE_HD uint32_t nr_che_tavg(const uint32_t *w, uint32_t n)
{
  uint32_t acc = w[0];
  for (uint32_t s = 1; s < n; s++)
    acc = nr_che_tavg_add(acc, w[s]);
  return nr_che_tavg_div(acc, n);
}
#endif
