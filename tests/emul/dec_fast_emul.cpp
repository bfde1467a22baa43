/*
 * dec_fast_emul.cpp -- the decoder kernels on the CPU as they are written (test infrastructure; tests/test_dec_kernels_emul.py,
 * and with sanitizers dec_emul_san.cpp).
 *
 * Includes ldpc_decoder.hip and ldpc_decoder_fast.hip themselves against the host shim (hip_host/): every kernel, the block bodies
 * ldpc_dec_fast_block.h / ldpc_dec_fast_mblock.h / ldpc_dec_generic_block.h with their queues, barriers and votes, and the
 * launchers with their dispatch run with one real thread per work-item.  Descriptors come from ldpc_graph.c, the source the
 * library uses; no record layout is restated (ldpc_kernels.h).  The caller's arrays are handed to the kernels as they are: rows
 * of exactly num_llr input bytes and out_bytes output bytes when the strides say so.
 */
#include "dec_emul_common.h"
#include <memory>
#include <vector>
#include "../../openairinterface5g_amd/csrc/ldpc_decoder.hip"
#include "../../openairinterface5g_amd/csrc/ldpc_decoder_fast.hip"

namespace {
struct CrcTables {
  std::vector<uint32_t> t[4];
  CrcTables()
  {
    /* x^j * x^deg mod g, left aligned (ldpc_api.cpp fill_crc_pow): CRC24A, CRC24B, CRC16, CRC8 */
    static const uint32_t polys[4] = {0x864cfb00u, 0x80006300u, 0x10210000u, 0x9B000000u};
    for (int i = 0; i < 4; i++) {
      t[i].resize(LDPC_CRC_POW_LEN);
      uint32_t r = polys[i];
      for (int j = 0; j < LDPC_CRC_POW_LEN; j++) {
        t[i][j] = r;
        r = (r & 0x80000000u) ? ((r << 1) ^ polys[i]) : (r << 1);
      }
    }
  }
};
const CrcTables &crc_tables()
{
  static const CrcTables c;
  return c;
}

typedef std::unique_ptr<ldpc_code_desc_t> desc_ptr;

/* the descriptor a launch of `kernel` takes: the shape's, or the several-blocks-per-workgroup one (ldpc_api.cpp code_entry) */
int build_desc(int kernel, int BG, int Z, int R, int shape, int mb, ldpc_code_desc_t *d)
{
  if (kernel != 1)
    return ldpc_build_code_desc_shape(BG, Z, R, shape, d);
  if ((Z & 3) == 0 && Z >= 8)
    return ldpc_build_code_desc_multi(BG, Z, R, mb > 0 ? mb : ldpc_multi_blocks_for(Z), d);
  if (mb <= 0)
    mb = 64 / Z < 1 ? 1 : (64 / Z > 16 ? 16 : 64 / Z);
  return ldpc_build_code_desc_interleaved(BG, Z, R, mb, d);
}

void fill_crc(ldpc_dec_args &a, int crc_type)
{
  const CrcTables &c = crc_tables();
  a.crc_pow = c.t[crc_type & 3].data();
  for (int i = 0; i < 4; i++)
    a.crc_pow_tbl[i] = c.t[i].data();
}

struct WithThreads {
  WithThreads() { hip_host::launch_with_threads = true; }
  ~WithThreads() { hip_host::launch_with_threads = false; }
};
} // namespace

extern "C" int dec_emul_fast_info(int kernel, int BG, int Z, int R, int shape, int mb, int32_t *info)
{
  desc_ptr d(new ldpc_code_desc_t);
  if (build_desc(kernel, BG, Z, R, shape, mb, d.get()) != 0)
    return -1;
  info[DEC_I_F_OK] = d->f_ok;
  info[DEC_I_THREADS] = d->f_n_threads;
  info[DEC_I_LDS] = d->f_lds_total;
  info[DEC_I_NUM_LLR] = d->num_llr;
  info[DEC_I_CN_TASKS] = d->f_n_cn_tasks;
  int n2 = 0, n2short = 0, tmax = 0;
  if (d->f_ok) {
    for (int t = 0; t < d->f_n_cn_tasks; t++)
      if (d->f_cn_task[t][0] & 0x100) {
        n2++;
        n2short += d->f_cn_task[t][4] - d->f_cn_task[t][2] < 128;
      }
    for (int t = 0; t < d->f_n_bn_tickets; t++)
      tmax = d->f_bn_ticket[t][1] > tmax ? d->f_bn_ticket[t][1] : tmax;
  }
  info[DEC_I_DOUBLE_TASKS] = n2;
  info[DEC_I_SHORT_DOUBLE_TASKS] = n2short;
  info[DEC_I_PAIR19] = d->f_pair19;
  info[DEC_I_EXT_GLOBAL] = d->f_ext_global;
  info[DEC_I_BN_TICKETS] = d->f_n_bn_tickets;
  info[DEC_I_BN_TICKET_MAX] = tmax;
  info[DEC_I_BN_GROUP] = d->f_bn_group;
  info[DEC_I_MB] = d->f_mb;
  info[DEC_I_SUB] = d->f_sub;
  info[DEC_I_ZQ] = d->f_zq;
  info[DEC_I_GENERIC_THREADS] = d->n_threads;
  info[DEC_I_GENERIC_LDS] = d->lds_total;
  return 0;
}

/* does ldpc_launch_dec_fast take the lifting size's own instantiation (ldpc_launch_zc) for this descriptor? */
extern "C" int dec_emul_takes_zc_kernel(int BG, int Z, int R, int shape)
{
  desc_ptr d(new ldpc_code_desc_t);
  if (ldpc_build_code_desc_shape(BG, Z, R, shape, d.get()) != 0 || !d->f_ok)
    return -1;
  return ldpc_fast_zc_enabled(Z) && d->f_mb == 1 && d->f_rstride == Z + 4 && d->f_astride == 2 * Z;
}

/* n blocks of one code.  llr: rows of num_llr bytes llr_stride apart (kernel 2: the device row the workgroup fills from `pull`,
 * rows pull_stride apart); out: rows out_stride apart; n_iter: one pass count per block; trace: NULL, or 32 zeroed words per block
 * for the diagnostic instantiation's stamps (ldpc_dec_fast_block.h pass_stamps).  0, or a negative error. */
extern "C" int dec_emul_decode(const int32_t *p, const int8_t *llr, uint32_t llr_stride, int8_t *out, uint32_t out_stride, int32_t *n_iter,
                               const int8_t *pull, uint32_t pull_stride, unsigned long long *trace)
{
  const int kernel = p[DEC_P_KERNEL];
  const uint32_t n = (uint32_t)p[DEC_P_N_BLOCKS];
  desc_ptr d(new ldpc_code_desc_t);
  if (build_desc(kernel, p[DEC_P_BG], p[DEC_P_Z], p[DEC_P_R], p[DEC_P_SHAPE], p[DEC_P_MB], d.get()) != 0)
    return -1;
  if (kernel != 3 && !d->f_ok)
    return -2;
  ldpc_dec_args a;
  memset(&a, 0, sizeof a);
  a.code = d.get();
  a.llr = llr;
  a.llr_stride = llr_stride;
  a.out = out;
  a.out_stride = out_stride;
  a.n_iter = n_iter;
  a.num_max_iter = p[DEC_P_MAX_ITER];
  a.out_mode = p[DEC_P_OUT_MODE];
  a.use_crc = p[DEC_P_USE_CRC];
  a.E = p[DEC_P_E];
  fill_crc(a, p[DEC_P_CRC_TYPE]);
  a.pull = pull;
  a.pull_stride = pull_stride;
  a.pull_stagger_ticks = (uint32_t)p[DEC_P_PULL_STAGGER];
  a.pull_first_round = (uint32_t)p[DEC_P_PULL_FIRST_ROUND];
  a.trace = trace;
  std::vector<ldpc_dec_job> jobs;
  std::vector<ldpc_dec_mgroup> groups;
  std::vector<int32_t> scattered;
  if (p[DEC_P_JOBS]) { /* one job per block; block i reports at n - 1 - i */
    jobs.resize(n);
    scattered.assign(n, -1);
    for (uint32_t i = 0; i < n; i++) {
      ldpc_dec_job &j = jobs[i];
      memset(&j, 0, sizeof j);
      j.code = d.get();
      j.llr_off = (uint64_t)i * llr_stride;
      j.out_off = (uint64_t)i * out_stride;
      j.num_max_iter = a.num_max_iter;
      j.E = a.E;
      j.crc_type = p[DEC_P_CRC_TYPE];
      j.iter_idx = (int32_t)(n - 1 - i);
      j.abort_idx = -1;
      j.seg_idx = -1;
    }
    a.jobs = jobs.data();
    a.n_iter = scattered.data();
  }
  WithThreads threads;
  hipError_t e = hipSuccess;
  if (ldpc_kernels_init() != hipSuccess || ldpc_fast_kernel_init() != hipSuccess)
    return -3;
  if (kernel == 0 && p[DEC_P_JOBS])
    e = ldpc_launch_dec_fast_jobs(a, d->f_n_threads, d->f_lds_total, n, nullptr,
                                  p[DEC_P_ZC] >= 0 ? p[DEC_P_ZC] : (d->f_mb == 1 && d->f_rstride == d->Z + 4 && d->f_astride == 2 * d->Z ? d->Z : 0));
  else if (kernel == 0)
    e = ldpc_launch_dec_fast(a, *d, n, nullptr);
  else if (kernel == 1 && p[DEC_P_JOBS]) {
    const uint32_t per_wg = (uint32_t)d->f_mb * (uint32_t)d->f_sub;
    for (uint32_t first = 0; first < n; first += per_wg) {
      ldpc_dec_mgroup g;
      memset(&g, 0, sizeof g);
      g.code = d.get();
      g.first_job = first;
      g.n_valid = n - first < per_wg ? n - first : per_wg;
      g.num_max_iter = a.num_max_iter;
      g.E = a.E;
      g.crc_type = p[DEC_P_CRC_TYPE];
      groups.push_back(g);
    }
    a.mgroups = groups.data();
    e = ldpc_launch_dec_fast_multi_jobs(a, d->f_sub, d->f_n_threads, d->f_lds_total, (uint32_t)groups.size(), nullptr);
  } else if (kernel == 1)
    e = ldpc_launch_dec_fast_multi(a, *d, n, nullptr);
  else if (kernel == 2)
    e = ldpc_launch_dec_fast_pull(a, *d, n, nullptr);
  else if (kernel == 3 && p[DEC_P_JOBS])
    e = ldpc_launch_dec_generic_jobs(a, d->n_threads, d->lds_total, n, nullptr);
  else if (kernel == 3)
    e = ldpc_launch_dec_generic(a, *d, n, nullptr);
  else
    return -4;
  if (e != hipSuccess)
    return -5;
  if (p[DEC_P_JOBS])
    for (uint32_t i = 0; i < n; i++)
      n_iter[i] = scattered[n - 1 - i];
  return 0;
}

/* a launch of jobs of different codes (the transport-block chain's job launches): spec = DEC_J_COUNT ints per job, llr_off /
 * out_off its rows in llr / out, tb_abort the launch's flags (zero on entry) or NULL; fast = 1: ldpc_launch_dec_fast_jobs, 0:
 * ldpc_launch_dec_generic_jobs; zc as the launcher takes it.  n_iter[iter_idx] = the job's pass count. */
extern "C" int dec_emul_decode_jobs(int fast, int n_jobs, const int32_t *spec, const uint64_t *llr_off, const uint64_t *out_off, int shape,
                                    int out_mode, int use_crc, int zc, const int8_t *llr, int8_t *out, int32_t *n_iter, int32_t *tb_abort)
{
  std::vector<desc_ptr> descs;
  std::vector<ldpc_dec_job> jobs((size_t)n_jobs);
  int threads = 0, lds = 0;
  for (int i = 0; i < n_jobs; i++) {
    const int32_t *s = spec + (size_t)i * DEC_J_COUNT;
    descs.emplace_back(new ldpc_code_desc_t);
    ldpc_code_desc_t *d = descs.back().get();
    if (ldpc_build_code_desc_shape(s[DEC_J_BG], s[DEC_J_Z], s[DEC_J_R], shape, d) != 0)
      return -1;
    if (fast && !d->f_ok)
      return -2;
    const int t = fast ? d->f_n_threads : d->n_threads, l = fast ? d->f_lds_total : d->lds_total;
    threads = t > threads ? t : threads;
    lds = l > lds ? l : lds;
    ldpc_dec_job &j = jobs[(size_t)i];
    memset(&j, 0, sizeof j);
    j.code = d;
    j.llr_off = llr_off[i];
    j.out_off = out_off[i];
    j.num_max_iter = s[DEC_J_MAX_ITER];
    j.E = s[DEC_J_E];
    j.crc_type = s[DEC_J_CRC_TYPE];
    j.iter_idx = s[DEC_J_ITER_IDX];
    j.abort_idx = s[DEC_J_ABORT_IDX];
    j.seg_idx = -1;
  }
  ldpc_dec_args a;
  memset(&a, 0, sizeof a);
  a.llr = llr;
  a.out = out;
  a.n_iter = n_iter;
  a.out_mode = out_mode;
  a.use_crc = use_crc;
  fill_crc(a, 0);
  a.jobs = jobs.data();
  a.tb_abort = tb_abort;
  WithThreads threads_on;
  const hipError_t e = fast ? ldpc_launch_dec_fast_jobs(a, threads, lds, (uint32_t)n_jobs, nullptr, zc)
                            : ldpc_launch_dec_generic_jobs(a, threads, lds, (uint32_t)n_jobs, nullptr);
  return e == hipSuccess ? 0 : -5;
}
