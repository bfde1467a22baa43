/*
 * nr_gold.h -- the length-31 Gold sequence of 38.211 section 5.2.1 (data scrambling: sections 6.3.1.1 and 7.3.1.1),
 * 32 bits at a time, with jump-ahead to any word.  Plain C (no HIP headers), so that the host code (nr_coding_host.c)
 * and the HIP kernels (tb_scrambling.hip) generate the sequence from the same definitions.
 *
 *   c(n) = x1(n + Nc) ^ x2(n + Nc), Nc = 1600
 *   x1(n + 31) = x1(n + 3) ^ x1(n),                    x1(0) = 1, x1(1 .. 30) = 0
 *   x2(n + 31) = x2(n + 3) ^ x2(n + 2) ^ x2(n + 1) ^ x2(n), x2(0 .. 30) = the bits of c_init, bit 0 first
 *
 * Word w of the sequence holds c(32w + k) in bit k (least significant bit first), the layout of the reference's
 * lte_gold_generic().  A register is kept as the 32-bit word of its bits x(32m .. 32m + 31); one step (nr_gold_step1 /
 * nr_gold_step2) gives the next word, and is a linear map over GF(2): a 32 x 32 matrix T.  The register word that
 * belongs to sequence word w is number w + Nc/32, reached from word 0 by T^(w + 50) = the product of the tables'
 * T^(2^i) over the set bits of w + 50 -- NR_GOLD_JUMPS of them cover every word a transport block can have
 * (G <= 1.5 Mbit: w < 2^16).
 */
#ifndef NR_GOLD_H
#define NR_GOLD_H
#include <stdint.h>

#if defined(__HIPCC__)
#define NR_GOLD_HD __host__ __device__ static inline constexpr
#elif defined(__cplusplus)
#define NR_GOLD_HD static inline constexpr
#else
#define NR_GOLD_HD static inline
#endif

#define NR_GOLD_NC_WORDS 50u /* Nc = 1600 bits */
#define NR_GOLD_JUMPS 17     /* T^(2^i), i < 17 */
/* first_word of a jump must stay below this: w + 50 < 2^17 */
#define NR_GOLD_MAX_FIRST_WORD ((1u << NR_GOLD_JUMPS) - NR_GOLD_NC_WORDS)

/* one step of 32 bits: t holds the bits whose two taps lie inside the old word; the top four bits of the new word take
 * taps from its own bottom four, which t already has right */
NR_GOLD_HD uint32_t nr_gold_step1(uint32_t x)
{
  const uint32_t t = (x >> 1) ^ (x >> 4);
  return t ^ (t << 31) ^ (t << 28);
}
NR_GOLD_HD uint32_t nr_gold_step2(uint32_t x)
{
  const uint32_t t = (x >> 1) ^ (x >> 2) ^ (x >> 3) ^ (x >> 4);
  return t ^ (t << 31) ^ (t << 30) ^ (t << 29) ^ (t << 28);
}
/* register words 0: bits 0 .. 30 as defined above, bit 31 by the recurrence */
NR_GOLD_HD uint32_t nr_gold_x1_init(void) { return 0x80000001u; }
NR_GOLD_HD uint32_t nr_gold_x2_init(uint32_t c_init)
{
  const uint32_t x = c_init & 0x7fffffffu;
  return x | (((x ^ (x >> 1) ^ (x >> 2) ^ (x >> 3)) & 1u) << 31);
}

/* T^(2^i) of both registers, in the two forms the kernels use.  row[i][j]: row j of the x1 matrix (j < 32) or row j - 32
 * of the x2 matrix (j >= 32) -- lane j of a wave forms bit j of the product by a parity (nr_gold_jump_wave).  col[i][b]:
 * column b of the x1 (b < 32) / x2 (b >= 32) matrix -- the product = the XOR of the columns of the set bits. */
typedef struct nr_gold_tables {
  uint32_t row[NR_GOLD_JUMPS][64];
  uint32_t col[NR_GOLD_JUMPS][64];
} nr_gold_tables_t;

/* M x (columns form) */
NR_GOLD_HD uint32_t nr_gold_apply_cols(const uint32_t *col, uint32_t x)
{
  uint32_t y = 0;
  for (int b = 0; b < 32; b++)
    y ^= col[b] & (0u - ((x >> b) & 1u));
  return y;
}

NR_GOLD_HD nr_gold_tables_t nr_gold_make_tables(void)
{
  nr_gold_tables_t t = {{{0}}, {{0}}};
  for (int b = 0; b < 32; b++) {
    t.col[0][b] = nr_gold_step1(1u << b);
    t.col[0][32 + b] = nr_gold_step2(1u << b);
  }
  for (int i = 1; i < NR_GOLD_JUMPS; i++) /* M^2: column b = M (column b of M) */
    for (int r = 0; r < 2; r++)
      for (int b = 0; b < 32; b++)
        t.col[i][32 * r + b] = nr_gold_apply_cols(&t.col[i - 1][32 * r], t.col[i - 1][32 * r + b]);
  for (int i = 0; i < NR_GOLD_JUMPS; i++)
    for (int r = 0; r < 2; r++)
      for (int j = 0; j < 32; j++) {
        uint32_t v = 0;
        for (int b = 0; b < 32; b++)
          v |= ((t.col[i][32 * r + b] >> j) & 1u) << b;
        t.row[i][32 * r + j] = v;
      }
  return t;
}

/* register words of sequence word w (w < NR_GOLD_MAX_FIRST_WORD), one matrix product per set bit of w + 50 */
NR_GOLD_HD void nr_gold_jump(const nr_gold_tables_t *t, uint32_t c_init, uint32_t w, uint32_t *x1, uint32_t *x2)
{
  uint32_t a = nr_gold_x1_init(), b = nr_gold_x2_init(c_init);
  const uint32_t n = w + NR_GOLD_NC_WORDS;
  for (int i = 0; i < NR_GOLD_JUMPS; i++)
    if ((n >> i) & 1u) {
      a = nr_gold_apply_cols(&t->col[i][0], a);
      b = nr_gold_apply_cols(&t->col[i][32], b);
    }
  *x1 = a;
  *x2 = b;
}

/* c_init of PDSCH / PUSCH data scrambling (38.211 7.3.1.1 / 6.3.1.1): n_RNTI 2^15 + q 2^14 + n_ID */
NR_GOLD_HD uint32_t nr_gold_c_init(uint32_t n_rnti, uint32_t q, uint32_t n_id) { return (n_rnti << 15) + (q << 14) + n_id; }
#endif
