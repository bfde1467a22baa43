/*
 * dec_emul_san.cpp -- the decoder kernels (dec_fast_emul.cpp, rx_fused_emul.cpp: ldpc_decoder.hip, ldpc_decoder_fast.hip and
 * tb_rx_fused.hip on the CPU) on arrays of
 * exactly the documented extents.  A stand-alone program, built with -fsanitize=address,undefined by
 * tests/test_dec_kernels_san.py: every array is a heap allocation of its own -- num_llr input bytes per block with the rows
 * num_llr apart, out_bytes per output row, the workgroup's LDS exactly the f_lds_total (lds_total) its launch asks for
 * (hip_host_run.h) -- so a read or a write in front of the first byte a launch may touch or behind the last one is a report, and so
 * is a misaligned vector access or an arithmetic overflow.
 *
 * The program has no oracle: every launch is compared with the generic kernel (ldpc_dec_generic_block.h, another work
 * decomposition of the same contract) on the same inputs, pass counts and output rows.  Inputs: the all-zero code word behind
 * noise (block 0 of a case has no sign errors and stops early, block 1 fails), a saturated block and one with a few errors; every case
 * checks that its reference has both a block that stops early and one that runs every pass.  A launch of jobs of
 * four codes with a shared transport-block flag is checked against the abort rule as ldpc_dec_fast_block.h states it.  Built
 * without optimisation and with one lifting size's own instantiations (-D'LDPC_FAST_ZC_LIST(X)=X(208)': the bodies with
 * compile-time row strides, which the Zc = 208 cases run): with all of them and -O1 the compiler takes most of a minute.
 * Exit status 0 and nothing on stderr: clean.
 */
#include "dec_emul_common.h"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

extern "C" {
int dec_emul_fast_info(int kernel, int BG, int Z, int R, int shape, int mb, int32_t *info);
int dec_emul_decode(const int32_t *p, const int8_t *llr, uint32_t llr_stride, int8_t *out, uint32_t out_stride, int32_t *n_iter,
                    const int8_t *pull, uint32_t pull_stride, unsigned long long *trace);
int rx_fused_emul_run(int n_tb, int32_t *tb, const int32_t *opt, uint32_t harq_stride, const int16_t *llr, int16_t *harq, uint8_t *payload,
                      uint8_t *ack, int32_t *iter_max, uint32_t *gen, int32_t *seg, int8_t *l_rows, uint32_t l_stride, int32_t *info);
int dec_emul_decode_jobs(int fast, int n_jobs, const int32_t *spec, const uint64_t *llr_off, const uint64_t *out_off, int shape, int out_mode,
                         int use_crc, int zc, const int8_t *llr, int8_t *out, int32_t *n_iter, int32_t *tb_abort);
}

namespace {
long n_calls = 0, n_bad = 0;
bool verbose = false; /* argv[1] = -v: the reference's pass counts per case */
uint32_t lcg_state = 12345u;
uint32_t lcg()
{
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return lcg_state >> 8;
}

/* block b of a case: the all-zero code word (LLR > 0) behind noise, or saturation values */
void fill_block(int8_t *llr, int num_llr, int Z, int b)
{
  static const int8_t sat[6] = {-128, -127, 127, 0, 1, -1};
  static const int spread[4] = {6, 60, 0, 14}; /* noise amplitude around the mean 12: no sign errors, hopeless, (saturated), a few */
  for (int i = 0; i < num_llr; i++) {
    if ((b & 3) == 2)
      llr[i] = sat[lcg() % 6];
    else if (i < 2 * Z)
      llr[i] = 0; /* the punctured columns */
    else {
      const int s = spread[b & 3];
      int v = 12 + (int)(lcg() % (uint32_t)(2 * s + 1)) - s + (int)(lcg() % (uint32_t)(2 * s + 1)) - s;
      llr[i] = (int8_t)(v > 127 ? 127 : (v < -128 ? -128 : v));
    }
  }
}

struct Case {
  int kernel, BG, Z, R, shape, n, mode, crc, mb, jobs, misalign, stagger, trace;
};

void run_case(const Case &c)
{
  int32_t info[DEC_I_COUNT];
  if (dec_emul_fast_info(c.kernel, c.BG, c.Z, c.R, c.shape, c.mb, info) != 0 || (c.kernel != 3 && !info[DEC_I_F_OK])) {
    n_bad++;
    fprintf(stderr, "no descriptor: kernel %d BG %d Z %d R %d\n", c.kernel, c.BG, c.Z, c.R);
    return;
  }
  const int num_llr = info[DEC_I_NUM_LLR], ob = c.mode == 0 ? (num_llr + 31) / 32 * 4 : num_llr;
  const int K = (c.BG == 1 ? 22 : 10) * c.Z;
  const size_t n = (size_t)c.n;
  std::unique_ptr<int8_t[]> llr(new int8_t[n * num_llr]), out(new int8_t[n * ob]), ref(new int8_t[n * ob]);
  std::unique_ptr<int32_t[]> it(new int32_t[n]), it_ref(new int32_t[n]);
  for (size_t b = 0; b < n; b++)
    fill_block(llr.get() + b * num_llr, num_llr, c.Z, (int)b);
  for (size_t i = 0; i < n * ob; i++)
    out[i] = ref[i] = 0x3c;
  int32_t p[DEC_P_COUNT] = {0};
  p[DEC_P_BG] = c.BG; p[DEC_P_Z] = c.Z; p[DEC_P_R] = c.R; p[DEC_P_SHAPE] = c.shape; p[DEC_P_N_BLOCKS] = c.n;
  p[DEC_P_MAX_ITER] = 8; p[DEC_P_OUT_MODE] = c.mode; p[DEC_P_USE_CRC] = c.crc; p[DEC_P_E] = c.crc ? K : 0; p[DEC_P_CRC_TYPE] = 1;
  p[DEC_P_ZC] = -1;
  /* the reference: the generic kernel, rows exactly num_llr apart (any alignment) */
  p[DEC_P_KERNEL] = 3;
  int rc = dec_emul_decode(p, llr.get(), (uint32_t)num_llr, ref.get(), (uint32_t)ob, it_ref.get(), nullptr, 0, nullptr);
  p[DEC_P_KERNEL] = c.kernel; p[DEC_P_MB] = c.mb; p[DEC_P_JOBS] = c.jobs;
  if (c.kernel == 2) {
    /* the pull kernel: the source rows in an array of their own, c.misalign bytes behind a 16-byte boundary (the allocation
     * then has that many bytes in front: the rows themselves end with it); the device rows exact */
    const uint32_t stride = (uint32_t)((num_llr + 15) / 16 * 16);
    std::unique_ptr<int8_t[]> src(new int8_t[c.misalign + (n - 1) * stride + num_llr]), dev(new int8_t[(n - 1) * stride + num_llr]);
    for (size_t b = 0; b < n; b++)
      memcpy(src.get() + c.misalign + b * stride, llr.get() + b * num_llr, (size_t)num_llr);
    p[DEC_P_PULL_STAGGER] = c.stagger; p[DEC_P_PULL_FIRST_ROUND] = c.n;
    rc |= dec_emul_decode(p, dev.get(), stride, out.get(), (uint32_t)ob, it.get(), src.get() + c.misalign, stride, nullptr);
    for (size_t b = 0; b < n; b++)
      rc |= memcmp(dev.get() + b * stride, llr.get() + b * num_llr, (size_t)num_llr) != 0;
  } else if (c.trace) {
    /* the diagnostic instantiation: 32 words of stamps per block, exactly; word 4 is the pass count */
    std::unique_ptr<unsigned long long[]> tr(new unsigned long long[n * 32]());
    rc |= dec_emul_decode(p, llr.get(), (uint32_t)num_llr, out.get(), (uint32_t)ob, it.get(), nullptr, 0, tr.get());
    for (size_t b = 0; b < n; b++)
      rc |= tr[b * 32 + 4] != (unsigned long long)it[b];
  } else {
    rc |= dec_emul_decode(p, llr.get(), (uint32_t)num_llr, out.get(), (uint32_t)ob, it.get(), nullptr, 0, nullptr);
  }
  n_calls++;
  bool same = rc == 0 && memcmp(out.get(), ref.get(), n * ob) == 0;
  for (size_t b = 0; b < n && same; b++)
    same = it[b] == it_ref[b];
  if (!same) {
    n_bad++;
    fprintf(stderr, "mismatch: kernel %d BG %d Z %d R %d shape %d n %d mode %d crc %d mb %d jobs %d rc %d\n", c.kernel, c.BG, c.Z, c.R, c.shape, c.n,
            c.mode, c.crc, c.mb, c.jobs, rc);
  }
  /* the inputs must give the cases something to tell apart: a block that stops early and one that runs every pass */
  bool early = false, full = false;
  for (size_t b = 0; b < n; b++) {
    early |= it_ref[b] >= 2 && it_ref[b] <= 8;
    full |= it_ref[b] == 9;
  }
  if (verbose) {
    static auto t0 = std::chrono::steady_clock::now();
    printf("%6.2f s  kernel %d BG %d Z %d R %d crc %d:", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), c.kernel, c.BG, c.Z,
           c.R, c.crc);
    for (size_t b = 0; b < n; b++)
      printf(" %d", it_ref[b]);
    printf("\n");
  }
  if (!early || !full) {
    n_bad++;
    fprintf(stderr, "vacuous inputs: kernel %d BG %d Z %d R %d crc %d\n", c.kernel, c.BG, c.Z, c.R, c.crc);
  }
}
/* four jobs of different codes in one launch of the jobs kernel, the rows packed end to end in one allocation each; jobs 0 and 1
 * share a transport-block flag, job 0 fails, so job 1 (workgroups run in order) gives up at its second pass: numMaxIter + 2 and an
 * untouched row (ldpc_dec_fast_block.h).  The others equal the generic kernel on the same rows. */
void run_mixed_jobs(int crc)
{
  static const int codes[4][3] = {{1, 16, 13}, {2, 64, 15}, {1, 44, 23}, {2, 8, 13}};
  static const int kind[4] = {1, 3, 0, 2}; /* fill_block: fails, a few sign errors, none, saturated */
  int32_t spec[4 * DEC_J_COUNT], info[DEC_I_COUNT];
  uint64_t llr_off[4], out_off[4];
  int nl[4], ob[4];
  size_t lo = 0, oo = 0;
  for (int k = 0; k < 4; k++) {
    if (dec_emul_fast_info(0, codes[k][0], codes[k][1], codes[k][2], 0, 0, info) != 0) {
      n_bad++;
      return;
    }
    nl[k] = info[DEC_I_NUM_LLR];
    ob[k] = (nl[k] + 31) / 32 * 4;
    llr_off[k] = lo; out_off[k] = oo;
    lo += (size_t)nl[k]; oo += (size_t)ob[k];
    int32_t *j = spec + k * DEC_J_COUNT;
    j[DEC_J_BG] = codes[k][0]; j[DEC_J_Z] = codes[k][1]; j[DEC_J_R] = codes[k][2]; j[DEC_J_MAX_ITER] = 8;
    j[DEC_J_E] = crc ? (codes[k][0] == 1 ? 22 : 10) * codes[k][1] : 0; j[DEC_J_CRC_TYPE] = 1; j[DEC_J_ITER_IDX] = 3 - k;
    j[DEC_J_ABORT_IDX] = k < 2 ? 0 : -1;
  }
  std::unique_ptr<int8_t[]> llr(new int8_t[lo]), out(new int8_t[oo]), ref(new int8_t[oo]);
  std::unique_ptr<int32_t[]> it(new int32_t[4]), flags(new int32_t[1]());
  int32_t it_ref[4];
  memset(out.get(), 0x3c, oo);
  memset(ref.get(), 0x3c, oo);
  int rc = 0;
  for (int k = 0; k < 4; k++) {
    fill_block(llr.get() + llr_off[k], nl[k], codes[k][1], kind[k]);
    int32_t p[DEC_P_COUNT] = {0};
    p[DEC_P_KERNEL] = 3; p[DEC_P_BG] = codes[k][0]; p[DEC_P_Z] = codes[k][1]; p[DEC_P_R] = codes[k][2]; p[DEC_P_N_BLOCKS] = 1;
    p[DEC_P_MAX_ITER] = 8; p[DEC_P_USE_CRC] = crc; p[DEC_P_E] = spec[k * DEC_J_COUNT + DEC_J_E]; p[DEC_P_CRC_TYPE] = 1; p[DEC_P_ZC] = -1;
    if (k != 1) /* (job 1's row stays untouched) */
      rc |= dec_emul_decode(p, llr.get() + llr_off[k], (uint32_t)nl[k], ref.get() + out_off[k], (uint32_t)ob[k], &it_ref[k], nullptr, 0, nullptr);
  }
  it_ref[1] = 8 + 2;
  rc |= dec_emul_decode_jobs(1, 4, spec, llr_off, out_off, 0, 0, crc, 0, llr.get(), out.get(), it.get(), flags.get());
  n_calls++;
  bool same = rc == 0 && memcmp(out.get(), ref.get(), oo) == 0 && flags[0] == 1 && it_ref[0] == 9;
  for (int k = 0; k < 4 && same; k++)
    same = it[3 - k] == it_ref[k];
  if (!same) {
    n_bad++;
    fprintf(stderr, "mismatch: mixed jobs, crc %d rc %d: %d %d %d %d\n", crc, rc, it[3], it[2], it[1], it[0]);
  }
}
/* one launch of the fused UL segment kernel (rx_fused_emul.cpp: tb_rx_fused.hip) over two transport blocks -- one BG2 segment of
 * Zc = 52, two of Zc = 208 -- of the all-zero payload (its CRCs are zero: the all-zero code word) behind noise, rate 0.8: G LLRs per
 * block and no more, soft-buffer rows of exactly the larger block's N = 50 Zc values, A / 8 payload bytes, the decoder input rows
 * (when they live in memory) exactly num_llr bytes each, the LDS exactly what the plan's rule gives.  Both blocks must decode. */
void run_fused(int lrow, int round, int rv)
{
  enum { N_TB = 2, N_SEG = 3 };
  static const int A[N_TB] = {400, 3912}, G[N_TB] = {500, 4888};
  const uint32_t stride = 50 * 208;
  int32_t tb[N_TB * RXF_T_COUNT] = {0}, opt[RXF_O_COUNT] = {0}, info[RXF_I_COUNT] = {0};
  for (int i = 0; i < N_TB; i++) {
    int32_t *t = tb + i * RXF_T_COUNT;
    t[RXF_T_A] = A[i]; t[RXF_T_G] = G[i]; t[RXF_T_BG] = 2; t[RXF_T_QM] = 2; t[RXF_T_NL] = 1; t[RXF_T_RV] = rv; t[RXF_T_ROUND] = round;
    t[RXF_T_MAX_ITER] = 8;
  }
  opt[RXF_O_LROW] = lrow; opt[RXF_O_MUTE] = 1; opt[RXF_O_TRUNC] = 1; opt[RXF_O_ABORT] = 1; opt[RXF_O_INTERLEAVE] = 1;
  std::unique_ptr<int16_t[]> llr(new int16_t[G[0] + G[1]]), harq(new int16_t[N_SEG * stride]());
  std::unique_ptr<uint8_t[]> pay(new uint8_t[(A[0] + A[1]) / 8]), ack(new uint8_t[N_TB]);
  std::unique_ptr<int32_t[]> itm(new int32_t[N_TB]), seg(new int32_t[N_SEG * RXF_S_COUNT]());
  std::unique_ptr<uint32_t[]> gen(new uint32_t[N_TB]());
  for (int i = 0; i < G[0] + G[1]; i++)
    llr[i] = (int16_t)(40 + (int)(lcg() % 45u) - 22 + (int)(lcg() % 45u) - 22); /* -4 .. 84: a sign error here and there */
  memset(pay.get(), 0xa5, (size_t)(A[0] + A[1]) / 8);
  const int rc = rx_fused_emul_run(N_TB, tb, opt, stride, llr.get(), harq.get(), pay.get(), ack.get(), itm.get(), gen.get(), seg.get(), nullptr, 0, info);
  n_calls++;
  bool ok = rc == 0 && (info[RXF_I_LROW_OFF] != 0) == (lrow != 0) && info[RXF_I_N_SEG] == N_SEG && gen[0] == 1 && gen[1] == 1;
  for (int i = 0; i < N_TB && ok; i++)
    ok = ack[i] == 1 && itm[i] >= 1 && itm[i] <= 8;
  for (int i = 0; i < (A[0] + A[1]) / 8 && ok; i++)
    ok = pay[i] == 0;
  if (!ok) {
    n_bad++;
    fprintf(stderr, "mismatch: fused launch, lrow %d round %d: rc %d ack %d %d iter_max %d %d\n", lrow, round, rc, ack[0], ack[1], itm[0], itm[1]);
  }
}
} // namespace

int main(int argc, char **argv)
{
  verbose = argc > 1 && argv[1][0] == '-' && argv[1][1] == 'v';
  static const Case cases[] = {
      /* kernel BG   Z   R shape n mode crc mb jobs misalign stagger */
      {0, 1, 8, 13, 0, 3, 0, 0, 0, 0, 0, 0},    /* one-block fast kernel: single tasks, pair19 rows, syndrome */
      {0, 1, 8, 13, 1, 2, 1, 0, 0, 0, 0, 0},    /* latency shape, a byte per bit */
      {0, 2, 44, 15, 0, 2, 0, 1, 0, 0, 0, 0},   /* a partial last wave per task, CRC stop */
      {0, 2, 44, 13, 1, 2, 0, 1, 0, 1, 0, 0},   /* the jobs kernel */
      {0, 1, 44, 23, 1, 2, 0, 0, 0, 0, 0, 0, 1}, /* the diagnostic instantiation, the eager sweep */
      {0, 2, 64, 15, 0, 2, 0, 0, 0, 0, 0, 0},   /* extension LLRs read from the block's row */
      {0, 1, 208, 89, 0, 2, 0, 0, 0, 0, 0, 0},  /* the lifting size's own instantiation (compile-time strides), grouped tickets */
      {0, 1, 208, 89, 0, 2, 0, 1, 0, 1, 0, 0},  /* ... of the jobs kernel, CRC stop */
      {0, 2, 256, 15, 0, 2, 0, 0, 0, 0, 0, 0},  /* double tasks, one of them short */
      {1, 2, 8, 15, 0, 5, 0, 0, 4, 0, 0, 0},    /* four blocks per workgroup and a second workgroup of one */
      {1, 2, 8, 15, 0, 5, 0, 1, 4, 1, 0, 0},    /* ... through job groups */
      {1, 2, 2, 15, 0, 9, 0, 0, 2, 0, 0, 0},    /* four interleaved blocks per group, two groups per workgroup */
      {1, 1, 4, 23, 0, 7, 0, 1, 2, 1, 0, 0},
      {1, 2, 3, 13, 0, 5, 1, 0, 1, 0, 0, 0},
      {2, 2, 16, 13, 0, 2, 0, 0, 0, 0, 0, 0},   /* the pull prologue: 16-byte units */
      {2, 2, 16, 13, 0, 2, 0, 1, 0, 0, 4, 3},   /* ... dwords, staggered */
      {3, 1, 6, 23, 0, 3, 0, 0, 0, 1, 0, 0},    /* the generic kernel through its jobs launcher */
  };
  for (const Case &c : cases)
    run_case(c);
  run_mixed_jobs(0);
  run_mixed_jobs(1);
  run_fused(1, 0, 0); /* a first transmission on the cut graph, the decoder input in LDS */
  run_fused(0, 0, 0); /* ... in memory */
  run_fused(1, 1, 2); /* an rv 2 round (on cleared soft buffers): the whole rate mode, the mute-item instantiation */
  printf("%ld calls, %ld mismatches or refusals\n", n_calls, n_bad);
  return n_bad == 0 && n_calls > 0 ? 0 : 1;
}
