/*
 * abi_cases.h -- what the C harnesses of the per-segment plugin entry points share (abi_threads.c, abi_lifecycle.c): the
 * table of decoder cases, their deterministic LLRs and parameter blocks, and the dump file in which a harness hands the
 * calls it compares everything else with -- inputs, outputs, pass counts -- to the Python side, which runs the oracle on
 * the same inputs (tests/abi_dump.py).  Test infrastructure.
 */
#ifndef ABI_CASES_H
#define ABI_CASES_H
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nrLDPC_hip.h"

#define NCASE 12
static const int cases[NCASE][4] = { /* BG, Z, R, numMaxIter */
  {1, 384, 13, 8}, {1, 384, 13, 8}, {1, 384, 23, 8}, {1, 352, 89, 5}, {2, 64, 15, 8}, {2, 208, 13, 8},
  {1, 96, 13, 8},  {1, 384, 13, 2}, {2, 6, 15, 8},   {1, 18, 13, 8},  {2, 384, 23, 8}, {1, 384, 13, 8}};
static int ncols(int BG, int R) { return BG == 1 ? (R == 13 ? 68 : R == 23 ? 35 : 27) : (R == 15 ? 52 : R == 13 ? 32 : 17); }
typedef int (*crc_t)(uint8_t *, uint32_t, uint8_t);

/* LLRs of case c (*s is the generator's state, carried from case to case: start it at ABI_LLR_SEED and go through the cases
 * in order); returns the number of values.  Odd cases: noisy all-zero code word, even: noise. */
#define ABI_LLR_SEED 12345u
static int abi_case_llr(int c, unsigned *s, int8_t **llr_out)
{
  const int BG = cases[c][0], Z = cases[c][1], R = cases[c][2], n = ncols(BG, R) * Z;
  int8_t *llr = aligned_alloc(64, (n + 63) / 64 * 64);
  for (int i = 0; i < n; i++) {
    *s = *s * 1664525u + 1013904223u;
    const int r = (int)((*s >> 16) % 41) - 20;            /* -20..20 */
    llr[i] = (int8_t)(i < 2 * Z ? 0 : (c & 1) ? 14 + r / 2 : r);
  }
  *llr_out = llr;
  return n;
}

/* parameter block of case c; crc_cb: the library's nrLDPC_hip_check_crc -- the CRC stop that is evaluated on the GPU (a
 * caller's own predicate would be called on the host) */
static void abi_case_params(int c, crc_t crc_cb, t_nrLDPC_dec_params *p)
{
  memset(p, 0, sizeof(*p));
  p->BG = cases[c][0]; p->Z = cases[c][1]; p->R = cases[c][2]; p->numMaxIter = cases[c][3]; p->outMode = nrLDPC_outMode_BIT;
  if (c == 11) { p->check_crc = crc_cb; p->E = 22 * 384; p->crc_type = 1; } /* CRC-stop mode in the mix */
}
static int abi_case_out_len(int c) { return (ncols(cases[c][0], cases[c][2]) * cases[c][1] + 31) / 32 * 4; }

/* build every case's code descriptor before the first per-segment call (batch = the library's LDPCdecoder_batch) */
typedef int32_t (*abi_batch_t)(const nrLDPC_hip_dec_batch_t *);
static void abi_warm_code(abi_batch_t batch, int BG, int Z, int R)
{
  nrLDPC_hip_dec_batch_t b;
  int8_t dummy[16];
  int32_t it;
  memset(&b, 0, sizeof(b));
  b.params.BG = BG; b.params.Z = Z; b.params.R = R; b.params.numMaxIter = 1;
  b.llr = dummy; b.out = dummy; b.n_iter = &it; b.llr_stride = 68 * 384; b.out_stride = 68 * 384;
  batch(&b);
}
static void abi_warm_cases(abi_batch_t batch)
{
  for (int c = 0; c < NCASE; c++)
    abi_warm_code(batch, cases[c][0], cases[c][1], cases[c][2]);
}

/* Dump file: records back to back, each 16 int32 {magic, kind, BG, Z, R or Kb, numMaxIter, CRC stop, E, crc_type, byte p_out
 * was filled with before the call, returned pass count, input bytes, output bytes, 0, 0, 0} followed by the input and the
 * output bytes.  kind 0: one LDPCdecoder call; 1: one segment of an LDPCencoder call. */
#define ABI_DUMP_MAGIC 0x41424944
static void abi_dump_record(FILE *f, int kind, int BG, int Z, int R_or_Kb, int max_iter, int use_crc, int E, int crc_type, int out_init,
                            int n_iter, const void *in, int in_len, const void *out, int out_len)
{
  const int32_t h[16] = {ABI_DUMP_MAGIC, kind, BG, Z, R_or_Kb, max_iter, use_crc, E, crc_type, out_init, n_iter, in_len, out_len, 0, 0, 0};
  if (!f)
    return;
  fwrite(h, sizeof(h), 1, f);
  fwrite(in, 1, (size_t)in_len, f);
  fwrite(out, 1, (size_t)out_len, f);
}
static void abi_dump_dec(FILE *f, int c, const t_nrLDPC_dec_params *p, int out_init, int n_iter, const int8_t *llr, const uint8_t *out)
{
  abi_dump_record(f, 0, p->BG, p->Z, p->R, p->numMaxIter, p->check_crc != NULL, p->E, p->crc_type, out_init, n_iter, llr,
                  ncols(cases[c][0], cases[c][2]) * cases[c][1], out, abi_case_out_len(c));
}
#endif
