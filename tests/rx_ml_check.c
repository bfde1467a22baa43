/* The arithmetic of csrc/nr_rx_ml.h as plain C under the host sanitizers: every function over random and full-scale values
 * (components -32768, 32767, 0), every shift 0..31, 1..8 antennas, both modulations and both layers.  No signed overflow, no shift
 * out of range, no index outside the local arrays.  Prints a checksum; test_rx_ml_host.py compiles and runs it. */
#include <stdio.h>
#include "nr_rx_ml.h"

static uint32_t rnd(void)
{
  static uint64_t s = 88172645463325252ull;
  s ^= s << 13;
  s ^= s >> 7;
  s ^= s << 17;
  return (uint32_t)(s >> 16);
}
static uint32_t pick(void)
{
  static const uint32_t c[4] = {0x80008000u, 0x7fff7fffu, 0x80007fffu, 0};
  const uint32_t r = rnd();
  return (r & 3) ? c[(r >> 2) & 3] ^ (((r >> 4) & 1) ? 0 : (rnd() & 0xffff0000u)) : rnd();
}

int main(void)
{
  uint64_t acc = 0;
  for (int it = 0; it < 100000; it++) {
    const uint32_t n_rx = 1 + rnd() % 8, s = rnd() % 32, Qm = (it & 1) ? 2 : 4;
    const int32_t amp[3] = {nr_rxf_amp(Qm, 0), 0, 0};
    nr_rxl_re_t R = {{{{0, 0, 0, 0}}, {{0, 0, 0, 0}}}, 0, 0};
    for (uint32_t a = 0; a < n_rx; a++)
      nr_rxl_mac(&R, pick(), pick(), pick(), s, amp);
    if (it & 2) { /* the LLR functions alone on full-scale streams, magnitudes and rho */
      R.l[0].w[0] = pick();
      R.l[1].w[0] = pick();
      R.l[0].w[1] = pick();
      R.l[1].w[1] = pick();
      R.rho01 = pick();
      R.rho10 = pick();
    }
    for (uint32_t l = 0; l < 2; l++) {
      int32_t L[4] = {0, 0, 0, 0};
      nr_rxl_llr(&R, Qm, l, L);
      for (uint32_t m = 0; m < Qm; m++) {
        if (L[m] < -32768 || L[m] > 32767)
          return 1;
        acc = acc * 31u + (uint32_t)L[m];
      }
    }
    const uint32_t sce = nr_rxm_shift_ch_ext((int32_t)rnd());
    acc += (uint32_t)nr_rxm_level_term(pick(), rnd() % 13, sce) + (uint32_t)nr_rxl_log2_maxh((int32_t)rnd());
  }
  printf("%llu\n", (unsigned long long)acc);
  return 0;
}
