/* The arithmetic of csrc/nr_rx_mmse.h as plain C under the host sanitizers: every function over random and full-scale values
 * (components -32768, 32767, 0), every shift 0..31, nvar up to 2^32 - 1, quads with a lane of zero padding.  No signed overflow,
 * no shift out of range.  Prints a checksum; test_rx_mmse_host.py compiles and runs it. */
#include <stdio.h>
#include "nr_rx_mmse.h"

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
  const uint32_t nvars[5] = {0, 1, 37, 70000, 0xffffffffu};
  for (int it = 0; it < 100000; it++) {
    const uint32_t n_rx = (it & 1) ? 2 : 4, s = rnd() % 32, nv = nvars[rnd() % 5];
    nr_rxm_re_t R[4] = {{{0, 0}, 0, 0, 0, 0}};
    int32_t det[4];
    for (int u = 0; u < 4; u++) {
      if (!(u == 3 && (it & 4)))
        for (uint32_t a = 0; a < n_rx; a++)
          nr_rxm_mac(&R[u], pick(), pick(), pick(), s);
      det[u] = nr_rxm_det(&R[u], nv);
    }
    const int32_t bm = nr_rxm_b_mag(det), bs = nr_rxm_b_sym(det);
    for (int u = 0; u < 4; u++) {
      acc += nr_rxm_sym0(&R[u], bs) ^ nr_rxm_sym1(&R[u], bs);
      for (uint32_t k = 0; k < 3; k++)
        acc += nr_rxm_mag(det[u], bm, nr_rxf_amp(8, k));
    }
    const uint32_t sce = nr_rxm_shift_ch_ext((int32_t)rnd());
    acc += (uint32_t)nr_rxm_level_term(pick(), rnd() % 13, sce) + (uint32_t)nr_rxm_log2_maxh((int32_t)rnd());
  }
  printf("%llu\n", (unsigned long long)acc);
  return 0;
}
