/*
 * abi_lifecycle.c -- the plugin life cycle of libldpc_hip.so from a C caller: loaded the way the reference's loader loads
 * it (common/utils/load_module_shlib.c:160-191, nrLDPC_load.c:45-75), LDPCshutdown() before the first call, between calls,
 * twice in a row and under the feet of calling threads, and process exit with the resident server kernels still up.
 * Every result is compared with the harness's own first answers, which go into a dump file for the oracle (abi_cases.h,
 * tests/abi_dump.py).  Reports one JSON line; what the numbers must be is decided in tests/test_gpu_lifecycle.py.
 * Test infrastructure.
 *
 *   gcc -O2 -I include tests/abi_lifecycle.c -o abi_lifecycle -ldl -lpthread
 *   ./abi_lifecycle <path/libldpc_hip.so> <dump file> [threads [calls per thread]]
 * Meant to run with NRLDPC_HIP_SRV_IDLE_US set to seconds: no generation of the server then leaves on its own, so the
 * launch counts are exact and a stop request that is not seen shows as a wait of that length.
 */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <pthread.h>
#include <sched.h>
#include <time.h>
#include <unistd.h>
#include "abi_cases.h"

typedef int32_t (*init_t)(void);
typedef int32_t (*stats_t)(int64_t *);
typedef int32_t (*dec_t)(t_nrLDPC_dec_params *, uint8_t, uint8_t, uint8_t, int8_t *, int8_t *, t_nrLDPC_time_stats *, decode_abort_t *);
typedef int32_t (*enc_t)(uint8_t **, uint8_t **, encoder_implemparams_t *);
typedef int32_t (*ver_t)(char *, char **);
typedef int32_t (*auto_t)(void *);

#define OUT_INIT 0x33
static init_t lib_init, lib_shutdown;
static dec_t dec;
static enc_t enc;
static stats_t stats;

static int8_t *llr[NCASE];
static uint8_t *expect[NCASE];
static int expect_iter[NCASE], out_len[NCASE];
static t_nrLDPC_dec_params prm[NCASE];

/* encoder calls: 1, 3 and 8 segments of BG1 Zc=384 and BG2 Zc=208 */
#define NENC 6
static const int enc_cases[NENC][3] = {{1, 384, 1}, {1, 384, 3}, {1, 384, 8}, {2, 208, 1}, {2, 208, 3}, {2, 208, 8}}; /* BG, Zc, segments */
static uint8_t *enc_in[NENC][8], *enc_expect[NENC][8];
#define ENC_OUT_MAX (68 * 384)

static double now_us(void)
{
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return t.tv_sec * 1e6 + t.tv_nsec / 1e3;
}

/* one LDPCdecoder call of case c into `out`; 0: pass count and bytes are the baseline's */
static int dec_call(int c, uint8_t *out, int *n_ret)
{
  t_nrLDPC_dec_params p = prm[c];
  memset(out, OUT_INIT, out_len[c]);
  const int n = dec(&p, 0, 0, 0, llr[c], (int8_t *)out, NULL, NULL);
  if (n_ret)
    *n_ret = n;
  return !(n == expect_iter[c] && memcmp(out, expect[c], out_len[c]) == 0);
}

/* one LDPCencoder call of encoder case e, parameters as the reference's caller sets them (nr_dlsch_coding.c:366); the
 * outputs land in out[0..n) */
static int enc_call(int e, uint8_t **out)
{
  const int BG = enc_cases[e][0], Zc = enc_cases[e][1], n = enc_cases[e][2], K = (BG == 1 ? 22 : 10) * Zc;
  encoder_implemparams_t ip;
  memset(&ip, 0, sizeof(ip));
  ip.n_segments = n; ip.macro_num = 0; ip.gen_code = 0; ip.Kr = K; ip.Kb = BG == 1 ? 22 : 10; ip.Zc = Zc; ip.BG = BG; ip.K = K; ip.E = K;
  for (int j = 0; j < n; j++)
    memset(out[j], OUT_INIT, ENC_OUT_MAX);
  return enc(enc_in[e], out, &ip);
}
static int enc_check(int e, uint8_t **out)
{
  const int BG = enc_cases[e][0], Zc = enc_cases[e][1], n = enc_cases[e][2], N = (BG == 1 ? 66 : 50) * Zc;
  int bad = enc_call(e, out) != 0;
  for (int j = 0; j < n; j++)
    bad |= memcmp(out[j], enc_expect[e][j], N) != 0;
  return bad;
}

static int status_max;
static int64_t gen_now(int64_t *served)
{
  int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  stats(st);
  if (st[0] > status_max)
    status_max = (int)st[0];
  if (served)
    *served = st[3];
  return st[2];
}

/* phase d */
static int calls_per_thread;
static volatile int completed, failures, nacked;
static void *worker(void *arg)
{
  const int tid = (int)(long)arg;
  uint8_t *out = malloc(68 * 384);
  for (int i = 0; i < calls_per_thread; i++) {
    const int c = (tid * 7 + i) % NCASE;
    int n = 0;
    if (dec_call(c, out, &n) != 0) {
      int touched = 0;
      for (int k = 0; k < out_len[c]; k++) touched |= out[k] != OUT_INIT;
      if (n == prm[c].numMaxIter + 1 && !touched) /* "not decoded": the library's answer when a call failed inside */
        __sync_fetch_and_add(&nacked, 1);
      __sync_fetch_and_add(&failures, 1);
      fprintf(stderr, "thread %d call %d case %d: n %d (expected %d)\n", tid, i, c, n, expect_iter[c]);
    }
    __sync_fetch_and_add(&completed, 1);
  }
  free(out);
  return NULL;
}

int main(int argc, char **argv)
{
  if (argc < 3) { fprintf(stderr, "usage: %s lib dump [threads [calls]]\n", argv[0]); return 2; }
  const int T = argc > 3 ? atoi(argv[3]) : 8;
  calls_per_thread = argc > 4 ? atoi(argv[4]) : 150;
  /* load_module_shlib.c:160, then the two optional hooks (:174-191), then the four names and LDPCinit (nrLDPC_load.c:55-70) */
  void *h = dlopen(argv[1], RTLD_LAZY | RTLD_NODELETE | RTLD_GLOBAL);
  if (!h) { fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
  ver_t ver = (ver_t)dlsym(h, "ldpc_checkbuildver");
  char build[] = "Branch: develop Abrev. Hash: 0123abc Date: x", *shlib_ver = NULL;
  if (ver && ver(build, &shlib_ver) < 0) { fprintf(stderr, "ldpc_checkbuildver refused\n"); return 2; }
  auto_t autoinit = (auto_t)dlsym(h, "ldpc_autoinit");
  if (autoinit && autoinit(NULL) != 0) { fprintf(stderr, "ldpc_autoinit failed\n"); return 2; }
  lib_init = (init_t)dlsym(h, "LDPCinit");
  lib_shutdown = (init_t)dlsym(h, "LDPCshutdown");
  dec = (dec_t)dlsym(h, "LDPCdecoder");
  enc = (enc_t)dlsym(h, "LDPCencoder");
  if (!ver || !autoinit || !lib_init || !lib_shutdown || !dec || !enc) { fprintf(stderr, "missing symbol\n"); return 2; }
  if (lib_init() != 0) { fprintf(stderr, "LDPCinit failed\n"); return 2; }

  /* a. before anything */
  int pre[4];
  pre[0] = lib_shutdown();
  pre[1] = lib_shutdown();
  pre[2] = lib_shutdown();
  pre[3] = lib_init();

  stats = (stats_t)dlsym(h, "nrLDPC_hip_server_stats");
  crc_t crc_cb = (crc_t)dlsym(h, "nrLDPC_hip_check_crc");
  abi_batch_t batch = (abi_batch_t)dlsym(h, "LDPCdecoder_batch");
  if (!stats || !crc_cb || !batch) { fprintf(stderr, "missing symbol\n"); return 2; }
  /* every code's descriptor now: set-up work (allocations, copies) must not meet a generation that stays for seconds */
  abi_warm_cases(batch);
  abi_warm_code(batch, 2, 208, 15); /* the encoder's BG2 code */

  /* b. baseline */
  FILE *dump = fopen(argv[2], "wb");
  if (!dump) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  unsigned s = ABI_LLR_SEED;
  for (int c = 0; c < NCASE; c++) {
    abi_case_llr(c, &s, &llr[c]);
    abi_case_params(c, crc_cb, &prm[c]);
    out_len[c] = abi_case_out_len(c);
    expect[c] = malloc(out_len[c]);
    memset(expect[c], OUT_INIT, out_len[c]);
    t_nrLDPC_dec_params p = prm[c];
    expect_iter[c] = dec(&p, 0, 0, 0, llr[c], (int8_t *)expect[c], NULL, NULL);
    if (expect_iter[c] < 0) { fprintf(stderr, "case %d failed\n", c); return 1; }
    abi_dump_dec(dump, c, &prm[c], OUT_INIT, expect_iter[c], llr[c], expect[c]);
  }
  uint8_t *enc_out[8];
  for (int j = 0; j < 8; j++)
    enc_out[j] = malloc(ENC_OUT_MAX);
  for (int e = 0; e < NENC; e++) {
    const int BG = enc_cases[e][0], Zc = enc_cases[e][1], n = enc_cases[e][2], K = (BG == 1 ? 22 : 10) * Zc, N = (BG == 1 ? 66 : 50) * Zc;
    for (int j = 0; j < n; j++) {
      enc_in[e][j] = calloc(1, K / 8 + 8);
      for (int i = 0; i < K / 8; i++) {
        s = s * 1664525u + 1013904223u;
        enc_in[e][j][i] = (uint8_t)(s >> 16);
      }
      enc_expect[e][j] = malloc(ENC_OUT_MAX);
    }
    if (enc_call(e, enc_expect[e]) != 0) { fprintf(stderr, "encoder case %d failed\n", e); return 1; }
    for (int j = 0; j < n; j++)
      abi_dump_record(dump, 1, BG, Zc, BG == 1 ? 22 : 10, 0, 0, 0, 0, OUT_INIT, 0, enc_in[e][j], K / 8, enc_expect[e][j], N);
  }
  fclose(dump);

  /* c. stop and relaunch */
  uint8_t *out = malloc(68 * 384);
  int bad_c = 0, bad_enc = 0;
  double shut_us[3], t0;
  const int64_t g0 = gen_now(NULL);
  bad_c += dec_call(5, out, NULL);
  t0 = now_us();
  bad_c += dec_call(1, out, NULL); /* (the case that is timed again below, as the first call after the shutdown) */
  const double warm_call_us = now_us() - t0;
  bad_enc += enc_check(1, enc_out);
  const int64_t g_control = gen_now(NULL);
  t0 = now_us();
  int shut_rc = lib_shutdown();
  shut_us[0] = now_us() - t0;
  t0 = now_us();
  bad_c += dec_call(1, out, NULL);
  const double relaunch_call_us = now_us() - t0;
  const int64_t g_after1 = gen_now(NULL);
  t0 = now_us();
  bad_enc += enc_check(2, enc_out);
  const double enc_relaunch_call_us = now_us() - t0;
  t0 = now_us();
  shut_rc |= lib_shutdown();
  shut_us[1] = now_us() - t0;
  t0 = now_us();
  shut_rc |= lib_shutdown();
  shut_us[2] = now_us() - t0;
  bad_c += dec_call(11, out, NULL);
  const int64_t g_after2 = gen_now(NULL);
  for (int e = 0; e < NENC; e++)
    bad_enc += enc_check(e, enc_out);
  for (int c = 0; c < NCASE; c++)
    bad_c += dec_call(c, out, NULL);

  /* d. shutdown under the callers' feet: one per 100 completed calls, however fast they complete */
  int64_t served0 = 0, served1 = 0;
  const int64_t launches0 = gen_now(&served0);
  pthread_t th[64];
  const int total = T * calls_per_thread;
  int shutdowns = 0;
  double shut_d_max_us = 0;
  for (long t = 0; t < T && t < 64; t++) pthread_create(&th[t], NULL, worker, (void *)t);
  for (int next = 100; next <= total; next += 100) {
    while (completed < next)
      usleep(20);
    t0 = now_us();
    shut_rc |= lib_shutdown();
    const double dt = now_us() - t0;
    if (dt > shut_d_max_us)
      shut_d_max_us = dt;
    shutdowns++;
  }
  for (int t = 0; t < T && t < 64; t++) pthread_join(th[t], NULL);
  const int64_t launches1 = gen_now(&served1);

  /* e. exit with a resident generation: one last call of each kind, the stamp, and out through main's return */
  bad_c += dec_call(0, out, NULL);
  bad_enc += enc_check(0, enc_out);
  const int64_t g_exit = gen_now(NULL);
  struct timespec rt;
  clock_gettime(CLOCK_REALTIME, &rt);
  printf("{\"pre\": [%d, %d, %d, %d], \"g0\": %lld, \"g_control\": %lld, \"g_after_shutdown\": %lld, \"g_after_two_shutdowns\": %lld, "
         "\"g_exit\": %lld, \"shutdown_rc\": %d, \"shutdown_us\": [%.1f, %.1f, %.1f], \"warm_call_us\": %.1f, \"relaunch_call_us\": %.1f, "
         "\"enc_relaunch_call_us\": %.1f, \"mismatches\": %d, \"enc_mismatches\": %d, \"status\": %d, \"threads\": %d, \"calls\": %d, "
         "\"failures\": %d, \"nacked\": %d, \"served\": %lld, \"server_launches\": %lld, \"shutdowns\": %d, \"shutdown_under_load_max_us\": %.1f, "
         "\"exit_stamp\": %.6f, \"iters\": [",
         pre[0], pre[1], pre[2], pre[3], (long long)g0, (long long)g_control, (long long)g_after1, (long long)g_after2, (long long)g_exit,
         shut_rc, shut_us[0], shut_us[1], shut_us[2], warm_call_us, relaunch_call_us, enc_relaunch_call_us, bad_c, bad_enc, status_max, T, total,
         failures, nacked, (long long)(served1 - served0), (long long)(launches1 - launches0), shutdowns, shut_d_max_us,
         rt.tv_sec + rt.tv_nsec / 1e9);
  for (int c = 0; c < NCASE; c++) printf("%d%s", expect_iter[c], c + 1 < NCASE ? ", " : "]}\n");
  fflush(stdout);
  return (failures || bad_c || bad_enc) ? 1 : 0;
}
