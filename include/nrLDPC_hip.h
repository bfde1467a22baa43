/*
 * nrLDPC_hip.h -- C ABI of libldpc_hip.so, the MI355X (gfx950) drop-in for OAI's NR LDPC coding library.
 *
 * Part 1 is the reference's own plugin ABI: the four symbols load_LDPClib() resolves from
 * "libldpc<version>.so" (reference openair1/PHY/CODING/nrLDPC_load.c:45-75, nrLDPC_extern.h:27-45) with
 * the reference's parameter structures restated field for field, so that `ldpctest -v _hip`,
 * `nr_ulsim --loader.ldpc.shlibversion _hip` or the gNB softmodem can load this library unchanged.
 * A translation unit that already includes the reference's nrLDPC_defs.h must define
 * NRLDPC_HIP_NO_REFERENCE_TYPES before including this header.
 *
 * Part 2 adds batched entry points (many code blocks per call, device- or host-resident buffers, caller
 * stream) -- the form in which a GPU is actually fed -- plus the TB-level helpers around the codec.
 *
 * Plain pointers and sizes only; no C++/torch types.  All functions are thread safe.
 */
#ifndef NRLDPC_HIP_H
#define NRLDPC_HIP_H
#include <stdint.h>
#include <stdbool.h>
#include <pthread.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ===================================================================================================
 * Part 1 -- reference plugin ABI
 * =================================================================================================== */
#ifndef NRLDPC_HIP_NO_REFERENCE_TYPES

/* nrLDPC_decoder/nrLDPC_types.h:75-79 */
typedef enum nrLDPC_outMode {
  nrLDPC_outMode_BIT,     /* 32 bits per uint32_t output, MSB-first inside each byte */
  nrLDPC_outMode_BITINT8, /* 1 bit per int8_t output */
  nrLDPC_outMode_LLRINT8  /* reference quirk: delivers the BITINT8 result at this revision (decoder.c:866-877) */
} e_nrLDPC_outMode;

/* nrLDPC_decoder/nrLDPC_types.h:84-97 */
typedef struct nrLDPC_dec_params {
  uint8_t BG;         /* base graph 1 / 2 */
  uint16_t Z;         /* lifting size */
  uint8_t R;          /* decoder rate mode: 13, 23, 89 (BG1) / 15, 13, 23 (BG2) */
  uint16_t F;         /* filler bits (offload back ends only) */
  uint8_t Qm;         /* modulation (offload back ends only) */
  uint8_t rv;         /* (offload back ends only) */
  uint8_t numMaxIter; /* iteration cap; up to numMaxIter+1 CN/BN passes run (decoder.c:552-558) */
  int E;              /* number of leading output bits covered by the CRC check */
  e_nrLDPC_outMode outMode;
  int crc_type;       /* CRC24_A 0, CRC24_B 1, CRC16 2, CRC8 3 (coding_defs.h:33-36) */
  /* NULL: stop on parity check.  Non-NULL: stop on CRC from pass 3 on, the predicate applied to (p_out, E, crc_type) after
   * every such pass exactly as nrLDPC_decoder.c:849-861 applies it.
   *   - The library's own nrLDPC_hip_check_crc, or the host executable's `check_crc` (looked up once with
   *     dlsym(RTLD_DEFAULT) -- what nr_ulsch_decoding.c:216 / nr_dlsch_decoding.c:253 pass): the same CRC
   *     (crc_byte.c:314-380) is evaluated ON THE GPU from crc_type / E; the pointer is not called.  Needs outMode BIT,
   *     E % 8 == 0, 0 < E <= K; any other combination takes the next path.
   *   - Any other pointer (LDPCdecoder and host-memory LDPCdecoder_batch): it IS called on the host, on p_out, after every
   *     pass >= 3 in order until it returns non-zero -- the decoder runs all its passes without stopping and keeps every
   *     pass' output, so this path costs the full iteration count (slow, exact).
   *   - Device-memory batches, LDPCdecoder_jobs and the transport-block chain evaluate the CRC on the GPU whatever the
   *     pointer (there it is a mode flag) and refuse the combinations the GPU cannot serve. */
  int (*check_crc)(uint8_t *decoded_bytes, uint32_t n, uint8_t crc_type);
  uint8_t setCombIn;
} t_nrLDPC_dec_params;

/* common/utils/time_meas.h:61-74 (oai_cputime_t = long long on x86-64, :39).  The encoder's four optional meters
 * (tinput, tprep, tparity, toutput) and the decoder's `total` are filled the way start_meas()/stop_meas() (:148-176) fill
 * them, gated by the host executable's `opp_enabled` when it exports one. */
typedef struct time_stats {
  long long in;        /* time stamp of the running measurement */
  long long diff;      /* accumulated ticks */
  long long p_time;    /* last duration */
  double diff_square;
  long long max;
  int trials;
  int meas_flag;
  char *meas_name;
  int meas_index;
  int meas_enabled;
  void *tpoolmsg;
  void *tstatptr;
} time_stats_t;
/* nrLDPC_decoder/nrLDPC_types.h:115-127.  Only `total` is written (the reference's per-function split -- cnProc,
 * bnProc, the buffer copies -- has no counterpart in a kernel that keeps a block in LDS from LLR load to bit store). */
typedef struct nrLDPC_time_stats {
  time_stats_t llr2llrProcBuf, llr2CnProcBuf, cnProc, cnProcPc, bnProcPc, bnProc, cn2bnProcBuf, bn2cnProcBuf, llrRes2llrOut,
      llr2bit, total;
} t_nrLDPC_time_stats;

/* openair1/PHY/defs_common.h:998-1027 -- transport-block wide "stop decoding" flag shared by the segments */
typedef struct {
  pthread_mutex_t mutex_failure;
  bool failed;
} decode_abort_t;

/* nrLDPC_defs.h:40-66 */
typedef struct {
  unsigned int n_segments; /* number of segments in input[]/output[] */
  unsigned int macro_num;  /* this call encodes segments 8*macro_num .. min(n_segments, 8*macro_num+8) */
  unsigned char gen_code;
  time_stats_t *tinput;
  time_stats_t *tprep;
  time_stats_t *tparity;
  time_stats_t *toutput;
  int Kr;
  uint32_t Kb;  /* information columns entering the parity (22; 10/9/8/6 for BG2) */
  uint32_t Zc;
  void *harq;
  uint8_t BG;
  unsigned char *output;
  uint32_t K;   /* bits per segment incl. fillers = 22*Zc / 10*Zc */
  uint32_t F;
  uint8_t Qm;
  uint32_t E;
  unsigned int G;
  uint8_t rv;
} encoder_implemparams_t;

#endif /* NRLDPC_HIP_NO_REFERENCE_TYPES */

/* nrLDPC_defs.h:68-87.  LDPCinit: 0 on success (the loader asserts on anything else, nrLDPC_load.c:67);
 * here it selects the GPU (env NRLDPC_HIP_DEVICE, default 0) and fails (-1) when no gfx950-capable HIP
 * device is usable -- there is no CPU fallback. */
int32_t LDPCinit(void);
int32_t LDPCshutdown(void);
/* Optional loader hook (common/utils/load_module_shlib.c:174-185, checkverfunc_t): called by load_module_version_shlib()
 * right after dlopen() with the executable's build string; reports this library's and returns 0.  With
 * NRLDPC_HIP_REQUIRE_BUILD=<text> in the environment it returns -1 -- the loader then refuses the library -- unless the
 * executable's build string contains <text>. */
int32_t ldpc_checkbuildver(char *mainexec_buildversion, char **shlib_buildversion);
int32_t nrLDPC_hip_checkbuildver(char *mainexec_buildversion, char **shlib_buildversion); /* (what the offload-slot library forwards to) */
/* Optional loader hook (common/utils/load_module_shlib.c:186-191, initfunc_t): called by load_module_version_shlib() after the
 * version hook with the `initfunc_arg` of its caller -- NULL from load_LDPClib (nrLDPC_load.c:61).  NULL: nothing to do,
 * returns 0 (the GPU is taken by LDPCinit, which the loader's caller runs next: nrLDPC_load.c:66-67).  A maintainer who passes
 * an argument passes a C string with the GPU list in NRLDPC_HIP_DEVICES' format ("0", "2,3"): it is put into the environment
 * for LDPCinit unless the variable is already set.  The loader ignores the return value. */
int32_t ldpc_autoinit(void *arg);
/* One code block, synchronous, host buffers.  p_llr: int8[ncols(BG,R)*Z] in base-graph column order, the two
 * punctured columns 0 and fillers +127 (callers: nr_ulsch_decoding.c:195-219, ldpctest.c:294-332).
 * Returns the number of passes executed; > numMaxIter means "not decoded" and sets *ab (decoder.c:190-193);
 * numMaxIter+2 when *ab was already set on entry or is raised by another thread while the call is running (looked at
 * once per pass, decoder.c:556-559; p_out is then left as it was).  Never negative, like the reference: an internal error (bad
 * parameters, HIP failure) is reported as numMaxIter+1 with *ab set, so that callers which only test
 * `<= numMaxIter` (nr_ulsch_decoding.c:219-222) NACK; nrLDPC_hip_last_error() tells why.
 * Calls are served by a resident GPU kernel through per-thread mailboxes (no HIP runtime call per segment); see
 * csrc/ldpc_server.h for NRLDPC_HIP_SERVER / _SRV_SLOTS / _SRV_IDLE_US.
 * With check_crc set and whole columns of zeros at the end of p_llr (a high-rate first transmission), the call is decoded
 * without the rows that close on those columns: they send zeros in every pass (nrLDPC_cnProc.h:105-114), so p_out and the
 * return value are those of the whole rate mode (NRLDPC_HIP_CUT=0: off). */
int32_t LDPCdecoder(t_nrLDPC_dec_params *p_decParams, uint8_t harq_pid, uint8_t ulsch_id, uint8_t C, int8_t *p_llr,
                    int8_t *p_out, t_nrLDPC_time_stats *p_profiler, decode_abort_t *ab);
/* Up to 8 segments per call (ldpc_encoder_optim8segmulti.c:46-213): input[j] K/8 bytes MSB first,
 * output[j] one bit per byte, (BG1 ? 66 : 50)*Zc bytes = c[2Zc..K) || parity.  Return value: that of the DEFAULT reference
 * library, ldpc_encoder_optim8segmulti.c:213 -- 0, and -1 on bad parameters (:88-100 there) -- not the output length that
 * ldpc_encoder.c:251 (`libldpc_orig.so`) returns; the reference's callers ignore the value (nr_dlsch_coding.c:171,
 * nr_ulsch_coding.c:167, ldpctest.c:265-282), tests/test_gpu_encoder.py asserts the 0.  Served by a resident kernel of its own, like the decoder
 * (NRLDPC_HIP_ENC_SERVER=0: one launch per call). */
int32_t LDPCencoder(uint8_t **input, uint8_t **output, encoder_implemparams_t *impp);

/* ===================================================================================================
 * Part 2 -- batched / device-resident entry points
 * =================================================================================================== */
#define NRLDPC_HIP_MEM_HOST 0   /* pointers are host memory: staged through pinned buffers, call is synchronous */
#define NRLDPC_HIP_MEM_DEVICE 1 /* pointers are device memory on the library's GPU: call only enqueues on `stream` */
/* nrLDPC_hip_ulsch_decode only, OR-ed into `mem`: where the HARQ soft buffers d[r] live, independently of the other buffers.
 * The reference keeps them per HARQ process for the life of the process (NR_TRANSPORT/nr_ulsch_decoding.c:168,
 * harq_process->d[r]) while the LLRs of a slot arrive in host memory (nr_ulsch_decoding(..., short *ulsch_llr, ...), :320):
 * with NRLDPC_HIP_MEM_HOST | NRLDPC_HIP_MEM_HARQ_DEVICE or ..._HARQ_LIBRARY a call moves the slot's LLRs over the link once
 * and nothing else -- the soft buffers never leave the GPU. */
#define NRLDPC_HIP_MEM_HARQ_DEVICE 2  /* b->harq is device memory (hipMalloc, or hipMallocManaged) on the library's GPU whatever bit 0 says */
#define NRLDPC_HIP_MEM_HARQ_LIBRARY 4 /* b->harq is ignored: the library keeps the soft buffers in GPU memory of its own, one
                                       * set of C x harq_stride int16 per transport block, found by tb[i].harq_off used as an
                                       * opaque 64-bit id chosen by the caller (e.g. ulsch_id << 8 | harq_pid -- the way the T2
                                       * card is addressed, nrLDPC_decoder_offload.c:546-547).  Allocated on first use, kept until
                                       * nrLDPC_hip_harq_release(); with several GPUs the buffers live on the GPU that decodes
                                       * the block (and follow it if a later round is given to another one). */

typedef struct nrLDPC_hip_dec_batch {
  t_nrLDPC_dec_params params; /* shared by every block of the batch (homogeneous batch = one launch) */
  uint32_t n_blocks;
  const int8_t *llr;          /* block b at llr + b*llr_stride, ncols*Z int8 each */
  uint32_t llr_stride;        /* bytes, >= ncols*Z; multiples of 16 give the widest loads */
  int8_t *out;                /* block b at out + b*out_stride; BIT: 4*ceil(ncols*Z/32) bytes, else ncols*Z bytes */
  uint32_t out_stride;        /* bytes, multiple of 4 */
  int32_t *n_iter;            /* [n_blocks] return value of each block (same meaning as LDPCdecoder's) */
  int32_t mem;                /* NRLDPC_HIP_MEM_* for llr/out/n_iter alike */
  void *stream;               /* hipStream_t for DEVICE mem; NULL = HIP's default (null) stream */
  int32_t kernel;             /* 0 = best available for (BG,Z,R); 1 = generic kernel (any code); 2 = fast kernel or error;
                               * 3 / 4 = fast kernel with the throughput / latency workgroup shape forced (0 and 2 pick the
                               * shape from n_blocks: latency shape up to one workgroup round of the GPU; for Zc <= 64 a launch
                               * that fills the GPU packs several blocks into a workgroup); 5 = that multi-block variant forced */
} nrLDPC_hip_dec_batch_t;
/* 0 on success, negative on bad parameters / HIP error.  DEVICE mem: asynchronous w.r.t. the host. */
int32_t LDPCdecoder_batch(const nrLDPC_hip_dec_batch_t *b);

/* A MIXED batch of code blocks in one call: every block with its own code, iteration cap and buffers -- what a slot's
 * segments look like when several UEs with different allocations are decoded together (BASELINE configs[2]: short BG2 blocks
 * of Zc = 64 and Zc = 208 in one batch).  Device memory only; outMode and the stop mode (check_crc NULL / non-NULL) must be
 * the same for all blocks; block i reports into n_iter[i].  The blocks are sorted by workgroup shape into as few launches as
 * the shapes allow (a launch whose last workgroup round is partly empty takes smaller blocks along); the job list derived
 * from an array that repeats byte for byte is reused.  0, negative on bad parameters / HIP error; enqueue only. */
typedef struct nrLDPC_hip_dec_job {
  t_nrLDPC_dec_params params;
  const int8_t *llr; /* ncols(BG, R) * Z int8, 4-byte aligned for the fast kernel */
  int8_t *out;       /* BIT: 4 * ceil(ncols*Z / 32) bytes (4-byte aligned), else ncols*Z bytes */
} nrLDPC_hip_dec_job_t;
int32_t LDPCdecoder_jobs(const nrLDPC_hip_dec_job_t *jobs, uint32_t n_jobs, int32_t *n_iter, int32_t mem, void *stream);

typedef struct nrLDPC_hip_enc_batch {
  uint8_t BG;
  uint16_t Zc;
  uint8_t Kb;            /* information columns entering the parity (see encoder_implemparams_t.Kb) */
  uint32_t n_blocks;
  const uint8_t *in;     /* block b at in + b*in_stride: K/8 bytes, MSB first (K = 22*Zc / 10*Zc) */
  uint32_t in_stride;
  uint8_t *out;          /* block b at out + b*out_stride: (66|50)*Zc bytes, one bit per byte */
  uint32_t out_stride;
  int32_t mem;
  void *stream;
} nrLDPC_hip_enc_batch_t;
int32_t LDPCencoder_batch(const nrLDPC_hip_enc_batch_t *b);

/* ---------------------------------------------------------------------------------------------------
 * Transport-block chain on the GPU (what the reference does on the CPU around the codec):
 *   nrLDPC_hip_dlsch_encode: TB CRC attach -> nr_segmentation (+ CB CRC24B, fillers) -> LDPC encode ->
 *     nr_rate_matching_ldpc -> nr_interleaving_ldpc, the body of nr_dlsch_encoding()/ldpc8blocks()
 *     (openair1/PHY/NR_TRANSPORT/nr_dlsch_coding.c:145-404), for a batch of transport blocks;
 *   nrLDPC_hip_ulsch_decode: nr_deinterleaving_ldpc -> nr_rate_matching_ldpc_rx (HARQ combining) -> int8 pack
 *     -> LDPC decode with CRC early stop -> reassembly + TB CRC, the body of nr_ulsch_decoding()/
 *     nr_processULSegment()/nr_postDecode() (nr_ulsch_decoding.c:122-470, SCHED_NR/phy_procedures_nr_gNB.c:271-300).
 * ------------------------------------------------------------------------------------------------- */
typedef struct nrLDPC_hip_tb {
  uint32_t A;        /* transport block size in bits (multiple of 8) */
  uint32_t G;        /* coded bits of the TB (nr_get_G) */
  uint32_t tbslbrm;  /* Tbslbrm as passed to nr_rate_matching_ldpc (0 = full circular buffer) */
  uint8_t BG;        /* base graph (rel15->maintenance_parms_v3.ldpcBaseGraph) */
  uint8_t Qm;        /* modulation order 2/4/6/8 */
  uint8_t Nl;        /* layers */
  uint8_t rv;        /* redundancy version */
  /* decode only */
  uint8_t numMaxIter;
  uint8_t round;     /* HARQ round; 0 clears the soft buffer first (d_to_be_cleared) */
  int32_t llrLen;    /* in/out: state of nr_get_R_ldpc_decoder across rounds (ulsch_harq->llrLen) */
  /* buffer placement (bytes for payload/coded, int16 elements for llr/harq) */
  uint64_t payload_off; /* A/8 bytes */
  uint64_t coded_off;   /* encode: G bytes, one bit per byte (the reference's `output`); decode: G int16 LLRs */
  uint64_t harq_off;    /* decode: C soft buffers of harq_stride int16 each, kept by the caller across rounds */
} nrLDPC_hip_tb_t;

typedef struct nrLDPC_hip_tb_batch {
  uint32_t n_tb;
  nrLDPC_hip_tb_t *tb;     /* host array [n_tb] (llrLen is updated by the decode call) */
  uint8_t *payload;        /* encode: in, decode: out */
  void *coded;             /* encode: uint8_t* out; decode: const int16_t* in */
  int16_t *harq;           /* decode: soft buffers (device memory when mem = DEVICE or mem & HARQ_DEVICE; unused with HARQ_LIBRARY) */
  uint32_t harq_stride;    /* int16 per code block, >= 66*384 */
  uint8_t *ack;            /* decode out [n_tb]: 1 = every segment decoded and the TB CRC holds */
  int32_t *iter_max;       /* decode out [n_tb]: largest per-segment pass count */
  int32_t mem;             /* NRLDPC_HIP_MEM_HOST or _DEVICE: payload / coded / harq / ack / iter_max alike; decode: optionally
                            * | NRLDPC_HIP_MEM_HARQ_DEVICE or | NRLDPC_HIP_MEM_HARQ_LIBRARY for the soft buffers.  HOST: `coded`
                            * in page-locked memory (nrLDPC_hip_host_alloc / nrLDPC_hip_host_register / hipHostMalloc) is read by
                            * the GPU in place -- the segments' workgroups pull their LLRs over the link while others decode --,
                            * pageable memory goes through a staged copy first */
  void *stream;            /* DEVICE mem: enqueue only (except the small per-call job upload) */
} nrLDPC_hip_tb_batch_t;
int32_t nrLDPC_hip_dlsch_encode(const nrLDPC_hip_tb_batch_t *b);
int32_t nrLDPC_hip_ulsch_decode(const nrLDPC_hip_tb_batch_t *b);
/* The same chain calls with data scrambling (38.211 7.3.1.1 / 6.3.1.1) inside; `scr` = host array of n_tb entries, one
 * codeword per transport block, whose sequence starts at the block's codeword bit 0.
 *   encode_scrambled: for each block ceil(G/32) uint32_t words at coded + coded_off (a byte offset, multiple of 4); bit k of
 *     word w = f(32w + k) ^ c(32w + k) -- nrLDPC_hip_dlsch_encode followed by nrLDPC_hip_codeword_scrambling; the bits
 *     behind G are 0 and nothing behind the last word is written.
 *   decode_scrambled: every output (payload, ack, iter_max, llrLen, soft buffers) as nrLDPC_hip_codeword_unscrambling on the
 *     block's G LLRs followed by nrLDPC_hip_ulsch_decode; the LLR array itself is only read.
 * Every mem mode of the unscrambled calls.  Negative -- before anything is enqueued or written -- for a NULL scr,
 * n_RNTI > 0xFFFF, Nid > 1023, q > 1, G > 2^21, (encode) coded_off % 4 != 0; nrLDPC_hip_last_error() names the reason. */
typedef struct nrLDPC_hip_tb_scr {
  uint32_t n_RNTI; /* <= 0xFFFF */
  uint16_t Nid;    /* <= 1023 */
  uint8_t q;       /* codeword index, 0 or 1; PUSCH: 0 */
  uint8_t pad;
} nrLDPC_hip_tb_scr_t; /* one per transport block; c_init = n_RNTI * 2^15 + q * 2^14 + Nid */
int32_t nrLDPC_hip_dlsch_encode_scrambled(const nrLDPC_hip_tb_batch_t *b, const nrLDPC_hip_tb_scr_t *scr);
int32_t nrLDPC_hip_ulsch_decode_scrambled(const nrLDPC_hip_tb_batch_t *b, const nrLDPC_hip_tb_scr_t *scr);
/* Soft buffers kept by the library (NRLDPC_HIP_MEM_HARQ_LIBRARY).  release: forget one transport block's buffers (its HARQ
 * process ended) / all of them; read: copy int16 values [first, first + n) of a block's C x harq_stride soft values to host
 * memory (diagnostics and tests; a device-memory decode call that wrote them must have completed on its stream).  0, or -1
 * (unknown id, range outside the buffers). */
int32_t nrLDPC_hip_harq_release(uint64_t id);
int32_t nrLDPC_hip_harq_release_all(void);
int32_t nrLDPC_hip_harq_read(uint64_t id, int16_t *dst, uint64_t first, uint64_t n);
/* Page-locked host memory for callers that do not link the HIP runtime themselves (a C gNB): LLR arrays placed here are
 * read by the GPU in place.  alloc returns NULL on failure; register / unregister pin an existing allocation (0 / -1). */
void *nrLDPC_hip_host_alloc(uint64_t bytes);
void nrLDPC_hip_host_free(void *p);
int32_t nrLDPC_hip_host_register(void *p, uint64_t bytes);
int32_t nrLDPC_hip_host_unregister(void *p);
/* ---------------------------------------------------------------------------------------------------
 * Codeword scrambling (38.211 5.2.1 Gold sequence, 6.3.1.1 PUSCH / 7.3.1.1 PDSCH): the reference's nr_codeword_scrambling()
 * and nr_codeword_unscrambling() (openair1/PHY/NR_TRANSPORT/nr_scrambling.c:27-78) on the GPU, with
 * c_init = n_RNTI * 2^15 + q * 2^14 + Nid (PUSCH: q = 0).  Word w of the sequence holds c(32w + k) in bit k.
 *   scrambling:   `in` = `size` bytes holding one bit each (bit 0 of a byte, as the reference reads them: the output of
 *                 nrLDPC_hip_dlsch_encode); out[w] bit k = in[32w + k] ^ c(32w + k), ceil(size/32) words.  The bits behind
 *                 `size` in the last word are 0 (the reference leaves its input's padding XOR c there).
 *   unscrambling: `size` int16 LLRs negated in place where c = 1, as the reference's multiplication by -1 does (-32768 stays
 *                 -32768).  Only [0, size) is touched; the reference also negates up to 31 values behind `size`.
 * mem = NRLDPC_HIP_MEM_HOST (synchronous) or NRLDPC_HIP_MEM_DEVICE (enqueued on `stream`, NULL = the default stream; `in`
 * and `out` / `llr` in device memory -- hipMalloc or managed -- of one GPU, which runs the kernel).
 * 0, or negative -- before anything is enqueued or written -- for n_RNTI > 0xFFFF, Nid > 1023, q > 1, size > 2^21, another
 * mem value, a NULL buffer or (DEVICE) a buffer that is not device memory of the GPU `in` is on; nrLDPC_hip_last_error()
 * names the reason.
 * These are the separate passes over a codeword; nrLDPC_hip_dlsch_encode_scrambled / nrLDPC_hip_ulsch_decode_scrambled
 * scramble inside the transport-block chain calls.
 * gold_words: words first_word .. first_word + n_words - 1 of the sequence of c_init (c_init < 2^31, first_word < 2^17 - 50)
 * on the host -- no GPU involved; the jump-ahead the kernels use, for checking them.  0 / -1. */
int32_t nrLDPC_hip_codeword_scrambling(const uint8_t *in, uint32_t size, uint8_t q, uint32_t Nid, uint32_t n_RNTI,
                                       uint32_t *out, int32_t mem, void *stream);
int32_t nrLDPC_hip_codeword_unscrambling(int16_t *llr, uint32_t size, uint8_t q, uint32_t Nid, uint32_t n_RNTI,
                                         int32_t mem, void *stream);
int32_t nrLDPC_hip_gold_words(uint32_t c_init, uint32_t first_word, uint32_t n_words, uint32_t *out);
/* Modulation mapping and soft demapping, the reference's nr_modulation() (openair1/PHY/MODULATION/nr_modulation.c:115-244)
 * and nr_ulsch_compute_llr() for one stream (openair1/PHY/NR_TRANSPORT/nr_ulsch_llr_computation.c:316-363) on the GPU.
 * Qm = 2, 4, 6, 8; the constellations of nr_generate_modulation_table(): bit b of a symbol's index = codeword bit iQm + b,
 * even bits give re, odd bits im.
 *   modulation: `in` = packed words (bit k of word w = bit 32w + k: the output of nrLDPC_hip_codeword_scrambling and
 *     nrLDPC_hip_dlsch_encode_scrambled), `length` bits; out = length/Qm (re, im) int16 pairs, nothing behind them written.
 *     Symbol i is always bits iQm .. iQm+Qm-1.  Deliberate differences: the reference's 64QAM loop bound length - 192 is
 *     computed in uint32 (it wraps below 192 bits and the loop reads past the input), and its 12-bit tail writes two
 *     symbols where one may be valid.
 *   ulsch_llr: nb_re REs; every array c16, one entry per RE (rxdataF_comp = the equalised y, ul_ch_mag / b / c = the channel
 *     magnitudes; an array the Qm does not use may be NULL).  Per RE: A = y (QPSK: A >> 3), B = subs(mag, |A|),
 *     C = subs(magb, |B|), D = subs(magc, |C|) (|-32768| = -32768, subs saturating); llr = A.r A.i B.r B.i C.r C.i D.r D.i
 *     cut to Qm values -- exactly nb_re*Qm written (for Qm >= 4 the reference rounds nb_re up to a multiple of 8 and reads
 *     and writes up to 7 REs behind it; not reproduced).
 * mem = NRLDPC_HIP_MEM_HOST (synchronous) or NRLDPC_HIP_MEM_DEVICE (enqueued on `stream`; every buffer in device memory of
 * one GPU, the ulsch_llr arrays 4-byte aligned).  0, or negative -- before anything is enqueued or written -- for a bad Qm,
 * length % Qm != 0, length (nb_re*Qm) > 2^21, another mem value, a NULL buffer or (DEVICE) a buffer that is not device
 * memory of that GPU; nrLDPC_hip_last_error() names the reason.
 * mod_table: the 2^Qm points as (re, im) pairs in index order, on the host (for checking); 0, or -1 for a bad Qm. */
int32_t nrLDPC_hip_mod_table(uint8_t Qm, int16_t *out);
int32_t nrLDPC_hip_modulation(const uint32_t *in, uint32_t length, uint8_t Qm, int16_t *out, int32_t mem, void *stream);
int32_t nrLDPC_hip_ulsch_llr(const int32_t *rxdataF_comp, const int32_t *ul_ch_mag, const int32_t *ul_ch_magb,
                             const int32_t *ul_ch_magc, uint32_t nb_re, uint8_t Qm, int16_t *llr, int32_t mem, void *stream);
/* The UL-SCH chain call from symbols: every output (payload, ack, iter_max, llrLen, soft buffers) as nrLDPC_hip_ulsch_llr on
 * each block's symbols followed by nrLDPC_hip_ulsch_decode_scrambled on the result; the LLRs never exist in memory.
 * Block i's symbol record is read as int16 at coded + coded_off (coded 4-byte aligned, coded_off even): with S = G/Qm, Qm/2
 * planes of S c16 values one after another -- y, mag_a (Qm >= 4), mag_b (Qm >= 6), mag_c (Qm = 8) -- exactly G int16, the
 * range the block's LLRs would take.  The planes are in codeword symbol order: with Nl layers, symbol k is layer k mod Nl's
 * RE k div Nl (layer demapping moves whole symbols, so it commutes with demapping).  Every mem mode of the LLR call.
 * Negative -- before anything is enqueued or written -- for anything decode_scrambled refuses, G % Qm != 0, a bad Qm, a
 * record that is not 4-byte aligned. */
int32_t nrLDPC_hip_ulsch_decode_symbols(const nrLDPC_hip_tb_batch_t *b, const nrLDPC_hip_tb_scr_t *scr);
/* The DL-SCH chain call that ends in layer-mapped symbols: the reference's PDSCH path from the transport block to the hand-off
 * to resource mapping (openair1/PHY/NR_TRANSPORT/nr_dlsch.c:150-205: nr_dlsch_encoding, nr_codeword_scrambling, nr_modulation,
 * nr_layer_mapping into tx_layers[Nl][...]) for one codeword per block.  With S = G/Qm, block i's output is written at
 * coded + coded_off (coded_off a byte offset, a multiple of 4; coded 4-byte aligned): Nl layer planes one after another, each
 * S/Nl c16 points (int16 re, im) -- exactly 4 G/Qm bytes per block, nothing outside them.  Entry k of plane l is the point of
 * codeword symbol k Nl + l; the point of symbol s is the nr_qam.h / nrLDPC_hip_mod_table entry of bits sQm .. sQm+Qm-1 of the
 * scrambled codeword (bit b = index bit b, as nrLDPC_hip_modulation).  Bit for bit: nrLDPC_hip_dlsch_encode_scrambled, then
 * nrLDPC_hip_modulation(G), then nrLDPC_hip_layer_mapping(Nl, layer_stride = S/Nl).  With Nl = 1 the output is the modulation
 * output; the layout is that of the UL symbol record.  Every mem mode and the multi-GPU cut of the encode calls.  Negative --
 * before anything is enqueued or written -- for anything encode_scrambled refuses, Nl > 4 (layers 5-8 carry two codewords in
 * the reference, and a block here is one), coded_off % 4 != 0, or a `coded` that is not 4-byte aligned.
 * layer_mapping: nr_layer_mapping for one codeword (openair1/PHY/MODULATION/nr_modulation.c:246-270), Nl = 1..4:
 * out[l layer_stride + i] = in[Nl i + l] for i < n_symbs/Nl, in c16 units; layer_stride (>= n_symbs/Nl) plays the role of
 * the reference's layerSz, and nothing between the planes is written.  `in` and `out` must not overlap.  mem as
 * nrLDPC_hip_modulation (HOST synchronous, DEVICE enqueued on `stream`, both arrays device memory of one GPU).  0, or negative
 * -- before anything is enqueued or written -- for n_symbs % Nl != 0, a bad Nl, a short stride, n_symbs > 2^21, overlapping
 * arrays, another mem value, a NULL array or (DEVICE) an array that is not device memory of that GPU. */
int32_t nrLDPC_hip_dlsch_encode_symbols(const nrLDPC_hip_tb_batch_t *b, const nrLDPC_hip_tb_scr_t *scr);
int32_t nrLDPC_hip_layer_mapping(const int16_t *in, uint32_t n_symbs, uint8_t Nl, int16_t *out, uint32_t layer_stride, int32_t mem,
                                 void *stream);
/* The UL receive front for one layer: the reference's channel level with its shift log2_maxh (nr_rx_pusch_tp, openair1/PHY/
 * NR_TRANSPORT/nr_ulsch_demodulation.c:1612-1647 with nr_ulsch_scale_channel :382-415 and nr_ulsch_channel_level :434-466) and
 * nr_ulsch_channel_compensation (:468-577: matched filter and maximum ratio combining over the receive antennas) on the GPU, from
 * the extracted REs and channel estimates (rxFext[aarx], chFext[aarx] of inner_rx, :1281-1324) to the symbol records
 * nrLDPC_hip_ulsch_decode_symbols reads.  nrOfLayers == 1 and rho == NULL only; transform precoding and PTRS are
 * not here; the _grid calls below read the OFDM grid itself, and two layers of 64QAM / 256QAM take the MMSE calls behind them.  rxFext / chFext are c16 arrays (int16 re, im), antenna a's values ant_stride c16
 * behind antenna 0's; n_rx = 1..8.  A descriptor (host memory) names one OFDM symbol's data REs of one transport block:
 *   channel_compensation: for each of the n_seg segments and each RE r < nb_re, over the antennas in order (csrc/nr_rx_front.h
 *     has the arithmetic, with int16 sums that wrap and packs that saturate exactly where the reference's do), with
 *     s = shift[tb] taken as 0..31 (a value outside is clamped: it may come from device memory): plane k (k < Qm/2: y, mag_a,
 *     mag_b, mag_c) of the block's record receives its value at c16 index sym_off + r, the record being int16 at
 *     records + rec_off and a plane `plane` c16 values long (S = G/Qm for a record decode_symbols reads; sym_off = the
 *     reference's llr_offset[symbol]/Qm).  Exactly nb_re c16 entries of each of the Qm/2 planes are written per segment and
 *     nothing else -- not the gaps between segments, not the planes a Qm does not use -- and they are overwritten, not
 *     accumulated into: no memset as in :1307-1311 is needed.  shift has an entry for every tb the descriptors name.
 *   channel_level: descriptor i (n_tb of them, every tb < n_tb once) names block tb's measurement symbol (ch_off, nb_re > 0;
 *     the other fields are not looked at): log2_maxh[tb] = max(0, (log2_approx(avgs) >> 1) + 1 + log2_approx(n_rx >> 2)),
 *     avgs = max(0, the antennas' averages over the symbol rounded up to 16 REs, the padding counting as zeros).
 * mem = NRLDPC_HIP_MEM_HOST (synchronous; every array host memory) or NRLDPC_HIP_MEM_DEVICE (enqueued on `stream`: rxFext,
 * chFext, shift / log2_maxh and records in device memory of one GPU, 4-byte aligned; the descriptors stay host memory and are
 * uploaded through the calling thread's page-locked area, like the chain's jobs).  So level -> compensation -> decode_symbols
 * on one stream take a slot from extracted REs to payloads with the records as the only array in between.  A stream that is
 * being captured is refused: graph capture of these two calls is not supported yet.
 * 0, or negative -- before anything is enqueued or written -- for a NULL array, n_rx outside 1..8, a bad Qm, rec_off odd,
 * sym_off + nb_re > plane, two segments of a call whose output ranges overlap, nb_re*Qm > 2^21, (level) nb_re = 0 or a tb that
 * is out of range or named twice, another mem value, (DEVICE) a buffer that is not device memory of that GPU or not 4-byte
 * aligned, a capturing stream; nrLDPC_hip_last_error() names the reason.
 * compensate_host / level_host: the same arithmetic on the CPU, no GPU involved, for checking the kernels: one segment (out =
 * Qm/2 planes of nb_re c16 one after another; shift clamped as above) / one block (avg, when not NULL, receives the n_rx
 * averages).  0 / -1. */
typedef struct nrLDPC_hip_rx_seg {
  uint32_t tb;      /* index into shift / log2_maxh */
  uint8_t Qm;       /* 2, 4, 6, 8 */
  uint8_t pad[3];
  uint32_t nb_re;   /* data REs of this OFDM symbol */
  uint32_t plane;   /* c16 values per plane of the block's record */
  uint32_t sym_off; /* first codeword symbol of this OFDM symbol */
  uint32_t pad2;
  uint64_t rx_off;  /* c16 offset of antenna 0's first RE in rxFext */
  uint64_t ch_off;  /* the same in chFext */
  uint64_t rec_off; /* int16 offset of the block's record in records, even */
} nrLDPC_hip_rx_seg_t;
int32_t nrLDPC_hip_ulsch_channel_level(const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, const nrLDPC_hip_rx_seg_t *first_sym,
                                       uint32_t n_tb, int32_t *log2_maxh, int32_t mem, void *stream);
int32_t nrLDPC_hip_ulsch_channel_compensation(const int16_t *rxFext, const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride,
                                              const nrLDPC_hip_rx_seg_t *seg, uint32_t n_seg, const int32_t *shift, int16_t *records,
                                              int32_t mem, void *stream);
int32_t nrLDPC_hip_ulsch_compensate_host(const int16_t *rxFext, const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, uint32_t nb_re,
                                         uint8_t Qm, int32_t shift, int16_t *out);
int32_t nrLDPC_hip_ulsch_level_host(const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, uint32_t nb_re, int32_t *avg,
                                    int32_t *log2_maxh);
/* The same front read straight from what a gNB has in memory -- the FFT output grid rxdataF[aarx] and the full-width channel
 * estimates ul_ch_estimates[aarx] of a DMRS symbol -- with nr_ulsch_extract_rbs (nr_ulsch_demodulation.c:279-380) fused into
 * the kernels' loads: no rxFext / chFext arrays exist.  csrc/nr_rx_grid.h defines the extraction once for host and device.  A
 * symbol has a pattern: NRLDPC_HIP_RXG_FULL (no DMRS: all 12 subcarriers of an RB, p(j) = j), _DMRS1 (type 1: the odd ones,
 * p(j) = 2j + 1) or _DMRS2 (type 2: those with p % 6 >= 2, p(j) = 6 (j/4) + 2 + j%4).  Data RE j < nb_re of a segment is read
 * from the grid at c16 index rx_off + a rx_ant_stride + (start_re + p(j)) mod fft_size and its estimate at ch_off +
 * a ch_ant_stride + p(j) (the grid wraps at fft_size, the estimates do not), for antenna a; the two arrays have an antenna
 * stride each.  Everything else -- arithmetic, records, write set, mem modes, the refusals -- is that of
 * nrLDPC_hip_ulsch_channel_compensation / _channel_level run on arrays extracted that way, bit for bit.  HOST mode stages the
 * c16 ranges the descriptors reach and nothing else.  Further refusals: a pattern that is none of the three, fft_size = 0,
 * start_re >= fft_size, nb_re above the pattern's count within fft_size subcarriers, which is p(nb_re - 1) >= fft_size.  The
 * calls do not know the arrays' extents; the Python wrappers, which do, refuse a descriptor that reaches outside.
 * One deviation: the reference's one-piece type-2 branch reads rxF[idx] (:352) where every other branch reads
 * rxF[start_re + idx]; start_re is added here.
 * extract_host: the extraction of one OFDM symbol of one antenna on the CPU, no GPU involved, for checking: rxdataF points at
 * the symbol's subcarrier 0, ul_ch at the estimate of PUSCH subcarrier 0, rxFext / chFext receive nb_re c16 each.  0 / -1.
 * pusch_grid_segments (host only, no GPU): the descriptors of n_alloc PUSCH allocations as nr_rx_pusch_tp derives them
 * (:1584-1665): one segment per OFDM symbol with nb_re = get_nb_re_pusch > 0, allocation after allocation in symbol order,
 * sym_off the running sum (llr_offset / Qm), start_re = (first_carrier_offset + (rb_start + bwp_start) 12) % fft_size, rx_off =
 * rx_slot_off + symbol fft_size, ch_off = the allocation's ch_off + d fft_size with d the DMRS symbol whose estimates the OFDM
 * symbol reads; first_sym_out[i] = allocation i's measurement symbol, its first with REs.  alloc.dmrs_symbol chooses d, two modes:
 *   NRLDPC_HIP_DMRS_SYMBOL_FOLLOW (255, the reference's INVALID_VALUE, its value at :1460): as the reference with chest_time = 0
 *     wherever the DMRS symbols carry data (one deviation, below).
 *     pusch_vars->dmrs_symbol becomes the allocation's first DMRS symbol during estimation (:1477-1478) and the level reads that one
 *     (:1606): first_sym_out names it.  The symbol loop sets dmrs_symbol = symbol when it reaches a DMRS symbol, before that
 *     symbol's inner_rx (:1403-1408, :1414), and inner_rx extracts at dmrs_symbol ofdm_symbol_size (:1294): every segment names the
 *     latest DMRS symbol of the allocation at or before its OFDM symbol, those in front of the first DMRS symbol the first.  The
 *     reference's symbol jobs share pusch_vars->dmrs_symbol and run on a thread pool; this is its result with the symbols run
 *     in order, one job in flight.  One deliberate deviation: the reference creates a symbol job only for a symbol with REs
 *     (:1654-1666, num_pusch_symbols_per_thread = 1), so with type 1 and two CDM groups without data, where a DMRS symbol has no
 *     REs, :1408 never runs and the reference keeps the first DMRS symbol's estimates for the whole slot.  Here the symbols behind
 *     such a DMRS symbol read its estimates all the same; to reproduce the reference there, pass the first DMRS symbol explicitly.
 *   0..13: that symbol for every segment and for first_sym_out.  This is chest_time = 1, where dmrs_symbol is the first DMRS
 *     symbol for the whole slot (:1535-1537, after pusch_chest_time_avg), and any slot with a single DMRS symbol.  An explicit
 *     symbol on a slot with several DMRS symbols is NOT what the reference does with chest_time = 0: the symbols behind the second
 *     DMRS symbol would be demodulated with the first one's estimates.
 * At most `cap` segments are written, *n_seg_out receives their number.  Refused: a dmrs_symbol of 14..254, 255 with no DMRS
 * symbol inside the allocation's symbols (the reference would read estimates at 255 fft_size),
 * start_symbol + nr_of_symbols > 14, nr_of_symbols = 0, a DMRS symbol of the allocation followed by another (the reference
 * asserts, :421), rb_size = 0, 12 rb_size > fft_size, first_carrier_offset >= fft_size, a dmrs_config_type other than 0 (type 1)
 * or 1 (type 2), num_dmrs_cdm_grps_no_data other than 1 or 2, the sum of nb_re above plane, no symbol with REs, more than cap
 * segments, and type 2 with two CDM groups without data: the reference's extraction then writes 8 REs per RB where nb_re
 * counts 4, and its level, which runs over the symbol rounded up to 16 REs, sums extracted entries beyond nb_re that are not
 * zeros -- a value this interface, which reads nb_re entries, cannot reproduce. */
#define NRLDPC_HIP_RXG_FULL 0
#define NRLDPC_HIP_RXG_DMRS1 1
#define NRLDPC_HIP_RXG_DMRS2 2
#define NRLDPC_HIP_DMRS_SYMBOL_FOLLOW 255 /* alloc.dmrs_symbol: every symbol reads the latest DMRS symbol at or before it */
typedef struct nrLDPC_hip_rx_grid_seg {
  uint32_t tb;       /* index into shift / log2_maxh */
  uint8_t Qm;        /* 2, 4, 6, 8 */
  uint8_t pattern;   /* NRLDPC_HIP_RXG_* */
  uint8_t pad[2];
  uint32_t nb_re;    /* data REs of this OFDM symbol */
  uint32_t plane;    /* c16 values per plane of the block's record */
  uint32_t sym_off;  /* first codeword symbol of this OFDM symbol */
  uint32_t fft_size; /* N, the OFDM symbol size */
  uint32_t start_re; /* grid subcarrier of PUSCH subcarrier 0, < N */
  uint32_t pad2;
  uint64_t rx_off;   /* c16 offset of antenna 0's subcarrier 0 of this OFDM symbol in rxdataF */
  uint64_t ch_off;   /* c16 offset of antenna 0's estimate of PUSCH subcarrier 0, of the symbol whose estimates are used */
  uint64_t rec_off;  /* int16 offset of the block's record in records, even */
} nrLDPC_hip_rx_grid_seg_t;
typedef struct nrLDPC_hip_pusch_alloc {
  uint32_t tb;                        /* index into shift / log2_maxh */
  uint8_t Qm;
  uint8_t dmrs_config_type;           /* 0: type 1, 1: type 2 */
  uint8_t num_dmrs_cdm_grps_no_data;  /* 1 or 2 */
  uint8_t dmrs_symbol;                /* NRLDPC_HIP_DMRS_SYMBOL_FOLLOW (chest_time = 0), or 0..13: one symbol's estimates for all */
  uint32_t fft_size;                  /* N */
  uint32_t first_carrier_offset;
  uint32_t bwp_start, rb_start, rb_size;
  uint32_t start_symbol, nr_of_symbols;
  uint32_t ul_dmrs_symb_pos;          /* bit s: symbol s carries DMRS */
  uint32_t plane;                     /* c16 values per plane of the block's record (G / Qm) */
  uint32_t pad;
  uint64_t rx_slot_off;               /* c16 offset of antenna 0's symbol 0, subcarrier 0 of the slot in rxdataF */
  uint64_t ch_off;                    /* c16 offset of antenna 0's estimates of symbol 0 in ul_ch */
  uint64_t rec_off;                   /* int16 offset of the block's record in records, even */
} nrLDPC_hip_pusch_alloc_t;
int32_t nrLDPC_hip_ulsch_channel_level_grid(const int16_t *ul_ch, uint32_t n_rx, uint64_t ch_ant_stride, const nrLDPC_hip_rx_grid_seg_t *first_sym,
                                            uint32_t n_tb, int32_t *log2_maxh, int32_t mem, void *stream);
int32_t nrLDPC_hip_ulsch_channel_compensation_grid(const int16_t *rxdataF, const int16_t *ul_ch, uint32_t n_rx, uint64_t rx_ant_stride,
                                                   uint64_t ch_ant_stride, const nrLDPC_hip_rx_grid_seg_t *seg, uint32_t n_seg, const int32_t *shift,
                                                   int16_t *records, int32_t mem, void *stream);
int32_t nrLDPC_hip_ulsch_extract_host(const int16_t *rxdataF, const int16_t *ul_ch, uint32_t pattern, uint32_t fft_size, uint32_t start_re,
                                      uint32_t nb_re, int16_t *rxFext, int16_t *chFext);
int32_t nrLDPC_hip_pusch_grid_segments(const nrLDPC_hip_pusch_alloc_t *alloc, uint32_t n_alloc, nrLDPC_hip_rx_grid_seg_t *seg_out, uint32_t cap,
                                       nrLDPC_hip_rx_grid_seg_t *first_sym_out, uint32_t *n_seg_out);
/* Two layers, 64QAM and 256QAM: the reference's MMSE receiver (inner_rx, nr_ulsch_demodulation.c:1348-1389: Qm >= 6 goes through
 * nr_ulsch_mmse_2layers :869-1260 and then the per-layer nr_ulsch_compute_llr) from the OFDM grid and the per-layer channel
 * estimates to the symbol records nrLDPC_hip_ulsch_decode_symbols reads with Nl = 2, bit for bit; csrc/nr_rx_mmse.h has the
 * arithmetic.  The descriptors are those of the _grid calls above (pusch_grid_segments derives them, with plane = G/Qm = twice the
 * allocation's REs and sym_off = llr_offset[symbol]/Qm counted per layer); n_rx = 2 or 4, the antenna counts the reference
 * accepts (:915-941).  The estimates of layer l, antenna a ("pair" l n_rx + a, :917-935) lie at ch_off + (l n_rx + a)
 * ch_ant_stride + p(j): 2 n_rx arrays.
 *   mmse_2layers_grid: per RE the two layers' matched filters over the antennas (:505-548), H^H H with saturating sums (:646-687,
 *     :756-867), nvar[tb] added to its diagonal when it is not 0 (:1103-1113, a 32-bit add on the packed word, as written), the
 *     determinant (:580-640); then per quad of four consecutive REs counted from the segment's RE 0 -- one 128-bit vector --
 *     the shared shift b = log2_approx(sum of det >> 2) - 8, the magnitudes (the same for both layers) and y0 d - y1 b,
 *     y1 a - y0 c (:1174-1256, :689-750), with s = shift[tb] clamped to 0..31.  A last quad that is only partly inside nb_re
 *     computes with the reference's zero padding in its outer lanes (they enter the sum, with what nvar makes of them).  Layer
 *     de-mapping (:1431-1438) is in the store: RE r of layer l is c16 index 2 (sym_off + r) + l of each plane k < Qm/2.  The
 *     write set per segment is exactly entries 2 sym_off .. 2 (sym_off + nb_re) - 1 of each of the Qm/2 planes, overwritten.
 *   channel_level_grid_mmse: log2_maxh[tb] = max(0, (log2_approx(avgs) >> 1) - 3) (:1639-1647), avgs = max(0, the 2 n_rx pairs'
 *     averages) of the measurement symbol scaled by nr_ulsch_scale_channel with shift_ch_ext = log2_approx(max_ch[tb] >> 11)
 *     (:1614, the general branch :392-402).
 * max_ch and nvar come out of the reference's channel estimator (nr_ul_channel_estimation.c:187, :468-469): inputs here, one
 * value per tb like shift, read from device memory in DEVICE mode, where pusch_channel_estimation_meas writes them.
 * mem modes, staging and refusals are those of the _grid calls; further refusals: Qm other than 6 or 8 (two layers of QPSK /
 * 16QAM take the ML receiver, which writes LLRs: the _ml calls below), n_rx other than 2 or 4, 2 (sym_off + nb_re) > plane, a NULL
 * nvar / max_ch or (DEVICE) one that is not device memory of that GPU, two segments whose doubled output ranges overlap.
 * One deviation: where the reference aborts (AssertFatal :1181, a determinant lane <= 0) the arithmetic goes on with what the
 * instructions give (a quad of zero determinants: b = -8); such a block fails its CRC.
 * mmse_2layers_host / level_mmse_host: the same arithmetic on the CPU, no GPU involved, for checking: one segment from extracted
 * arrays (chFext: the 2 n_rx pairs ant_stride apart, rxFext: the n_rx antennas ant_stride apart; out = layer 0's Qm/2 planes of
 * nb_re c16, then layer 1's) / one block (avg, when not NULL, receives the 2 n_rx averages).  0 / -1. */
int32_t nrLDPC_hip_ulsch_channel_level_grid_mmse(const int16_t *ul_ch, uint32_t n_rx, uint64_t ch_ant_stride,
                                                 const nrLDPC_hip_rx_grid_seg_t *first_sym, uint32_t n_tb, const int32_t *max_ch,
                                                 int32_t *log2_maxh, int32_t mem, void *stream);
int32_t nrLDPC_hip_ulsch_mmse_2layers_grid(const int16_t *rxdataF, const int16_t *ul_ch, uint32_t n_rx, uint64_t rx_ant_stride,
                                           uint64_t ch_ant_stride, const nrLDPC_hip_rx_grid_seg_t *seg, uint32_t n_seg, const int32_t *shift,
                                           const uint32_t *nvar, int16_t *records, int32_t mem, void *stream);
int32_t nrLDPC_hip_ulsch_mmse_2layers_host(const int16_t *rxFext, const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, uint32_t nb_re,
                                           uint8_t Qm, int32_t shift, uint32_t nvar, int16_t *out);
int32_t nrLDPC_hip_ulsch_level_mmse_host(const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, uint32_t nb_re, int32_t max_ch,
                                         int32_t *avg, int32_t *log2_maxh);
/* Two layers, QPSK and 16QAM: the reference's max-log ML receiver (inner_rx, nr_ulsch_demodulation.c:1348-1389: Qm < 6 goes
 * through nr_ulsch_compute_ML_llr, nr_ulsch_llr_computation.c:2100-2129) from the OFDM grid and the per-layer channel estimates
 * to LLRs in codeword order, the array nrLDPC_hip_ulsch_decode_scrambled reads; csrc/nr_rx_ml.h has the arithmetic, in the
 * 256-bit variants an x86 build of the reference takes.  The descriptors, the pairs and their layout are those of the _mmse
 * calls above (pusch_grid_segments derives them: plane = G/Qm = twice the allocation's REs, sym_off counted per layer, rec_off =
 * the block's coded_off in int16, even); n_rx = 1..8 (2 and 4 have kernels of their own, the rest take a loop).  nvar is not an
 * input: the ML path does not use it.
 *   ml_2layers_grid: per RE the two layers' matched filters and ul_ch_maga over the antennas (:505-548), rho[0][1] and rho[1][0],
 *     each the saturating sum over the antennas in order of pack(conj(h_l) h_l' >> s) (:550-570; formed separately, as written:
 *     the arithmetic shift makes them differ from each other's conjugate by rounding), s = shift[tb] clamped to 0..31; then per
 *     layer nr_ulsch_qpsk_qpsk (:528-682) with nr_ulsch_shift_llr's >> 4 (:2076-2098), or nr_ulsch_qam16_qam16 (:1124-1350) --
 *     layer 1 is the same function with the streams, magnitudes and rho swapped (:2115-2121).  QPSK forms num - den, 16QAM
 *     den - num, as written.  Layer de-mapping (nr_ulsch_demodulation.c:1431-1438) is in the store: bit m of layer l of the
 *     segment's RE r is int16 rec_off + Qm (2 (sym_off + r) + l) + m.  The write set per segment is exactly int16 rec_off + 2 Qm
 *     sym_off .. rec_off + 2 Qm (sym_off + nb_re) - 1, overwritten.  Qm is per segment; one call may mix 2 and 4.
 *   channel_level_grid_ml: log2_maxh[tb] = max(0, log2_approx(avgs) >> 1) (:1639-1647: neither the MMSE's - 3 nor the single
 *     layer's term), avgs and the scaling by max_ch[tb] as in channel_level_grid_mmse.
 * Three deviations, all in which REs are computed, none in an RE's value.  The reference's loops run `for (i = 0; i <
 * length >> 3; i += 2)` over 16 REs each, so (1) when nb_re >> 3 is even and nb_re % 8 != 0 (18, 20, 36 REs; 3 or 11 PRBs) its
 * last nb_re % 8 REs are never computed and their LLRs are whatever the buffer held, and (2) when nb_re >> 3 is odd it computes
 * and stores up to 8 REs behind nb_re; (3) nr_ulsch_shift_llr shifts 4 (nb_re >> 2) REs from an address-dependent start, so some
 * QPSK REs are shifted never or twice.  Here exactly nb_re REs per segment are computed, each by the per-RE definition, QPSK
 * LLRs are shifted exactly once, and nothing behind nb_re is written.
 * mem modes and staging are those of the _grid calls (HOST stages only the ranges the descriptors reach and copies back only
 * the segments' entries).  Refused before anything is enqueued or written: everything channel_compensation_grid refuses; Qm
 * other than 2 or 4 (64QAM / 256QAM take mmse_2layers_grid); n_rx outside 1..8; 2 (sym_off + nb_re) > plane; two segments whose
 * output ranges overlap; a NULL max_ch or (DEVICE) one that is not device memory of that GPU; a capturing stream.
 * ml_2layers_host / level_ml_host: the same arithmetic on the CPU, no GPU involved, for checking: one segment from extracted
 * arrays (chFext: the 2 n_rx pairs ant_stride apart, rxFext: the n_rx antennas ant_stride apart; out = 2 nb_re Qm int16, bit m
 * of layer l of RE r at Qm (2 r + l) + m) / one block (avg, when not NULL, receives the 2 n_rx averages).  0 / -1. */
int32_t nrLDPC_hip_ulsch_channel_level_grid_ml(const int16_t *ul_ch, uint32_t n_rx, uint64_t ch_ant_stride,
                                               const nrLDPC_hip_rx_grid_seg_t *first_sym, uint32_t n_tb, const int32_t *max_ch,
                                               int32_t *log2_maxh, int32_t mem, void *stream);
int32_t nrLDPC_hip_ulsch_ml_2layers_grid(const int16_t *rxdataF, const int16_t *ul_ch, uint32_t n_rx, uint64_t rx_ant_stride,
                                         uint64_t ch_ant_stride, const nrLDPC_hip_rx_grid_seg_t *seg, uint32_t n_seg, const int32_t *shift,
                                         int16_t *llr, int32_t mem, void *stream);
int32_t nrLDPC_hip_ulsch_ml_2layers_host(const int16_t *rxFext, const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, uint32_t nb_re,
                                         uint8_t Qm, int32_t shift, int16_t *out);
int32_t nrLDPC_hip_ulsch_level_ml_host(const int16_t *chFext, uint32_t n_rx, uint64_t ant_stride, uint32_t nb_re, int32_t max_ch,
                                       int32_t *avg, int32_t *log2_maxh);
/* ---------------------------------------------------------------------------------------------------
 * PUSCH DMRS channel estimation from the OFDM grid: nr_pusch_channel_estimation (openair1/PHY/NR_ESTIMATION/
 * nr_ul_channel_estimation.c:67-473) for one list of descriptors, one per (allocation, DMRS symbol), times n_rx antennas.  It
 * writes the full-width estimates that the _grid calls above read, so that channel_estimation -> channel_level_grid ->
 * channel_compensation_grid -> ulsch_decode_symbols on one stream takes a slot from rxdataF to payload bytes.  csrc/nr_chest.h
 * defines the arithmetic once for host and device, bit for bit the reference's: the pilots of nr_pusch_dmrs_rx, and the four
 * estimators NRLDPC_HIP_CHEST_TYPE1_INTERP / _TYPE2_INTERP (chest_freq = 0) and _TYPE1_AVG / _TYPE2_AVG (chest_freq = 1).
 * For antenna a the symbol is read at c16 index rx_off + a rx_ant_stride + subcarrier (the grid wraps at fft_size; start_re is
 * bwp_start_subcarrier) and exactly 12 rb_size c16 are written at ch_off + a ch_ant_stride, overwritten: the reference's memset
 * of the whole symbol and its TYPE1_INTERP spill of four entries behind the allocation are not reproduced.  est_delay holds
 * one int32 per (descriptor, antenna) at delay_off + a, the value nr_est_delay would have found (pusch_est_delay below
 * searches it on the GPU, in fp32; the reference's fixed-point IDFT is not built); NULL means 0 everywhere.  max_ch and nvar: pusch_channel_estimation_meas below.  Deviations from the
 * reference: TYPE2_AVG reads every RE relative to the descriptor's symbol and PRB b uses pilots 4b .. 4b + 3.
 * mem = HOST stages one contiguous span of the grid, from the lowest to the highest c16 any (descriptor, antenna) pair reads,
 * works on a bounce of the span of estimates from the lowest to the highest c16 written, and copies only the write set back to
 * ul_ch: the spans grow with the distance between descriptors and with the antenna strides.  mem = DEVICE enqueues on `stream`;
 * the first call per (GPU, fft_size) also allocates that size's delay table (41 fft_size c16, kept until the process ends) and
 * uploads it with a synchronous copy, so it blocks: run one call per fft_size at start-up where the first slot must not wait.
 * Refused before anything is enqueued: NULL arrays, n_rx outside 1..8, an unknown mode, a port outside 0..7 (type 1) / 0..11
 * (type 2), rb_size = 0, 12 rb_size > fft_size, start_re >= fft_size, an fft_size other than 128, 256, 512, 1024, 1536, 2048,
 * 4096, 6144, 8192, c_init >= 2^31, dmrs_offset > 2^20, a descriptor whose nushift would move a read to index fft_size, output
 * ranges of two (descriptor, antenna) pairs that overlap, a misaligned or foreign device pointer, a capturing stream.
 * pusch_chest_host: one descriptor, antenna 0, on the CPU from the same header, no GPU (rx_off and ch_off apply).
 * pusch_dmrs_host: n conjugated pilots from sequence symbol dmrs_offset on (type 0: type 1, 1: type 2).
 * delay_table_host: row get_delay_idx(delay) of the delay table of fft_size (fft_size c16).
 * pusch_chest_segments (host only): one descriptor per DMRS symbol of each allocation, in symbol order; ch_off = the
 * allocation's ch_off + symbol fft_size, where nrLDPC_hip_pusch_grid_segments makes the grid calls read when dmrs_symbol names
 * that symbol; delay_off = descriptor index times n_rx; c_init as nr_gold_pusch (nr_gold.c:107-108). */
#define NRLDPC_HIP_CHEST_TYPE1_INTERP 0
#define NRLDPC_HIP_CHEST_TYPE2_INTERP 1
#define NRLDPC_HIP_CHEST_TYPE1_AVG 2
#define NRLDPC_HIP_CHEST_TYPE2_AVG 3
typedef struct nrLDPC_hip_chest_seg {
  uint8_t mode;         /* NRLDPC_HIP_CHEST_* */
  uint8_t port;         /* antenna port p - 1000 */
  uint8_t pad[2];
  uint32_t fft_size;    /* N, the OFDM symbol size */
  uint32_t start_re;    /* grid subcarrier of PUSCH subcarrier 0, < N */
  uint32_t rb_size;
  uint32_t dmrs_offset; /* first sequence symbol: 12 (bwp_start + rb_start) / 2 (type 1) or / 3 (type 2) */
  uint32_t c_init;      /* of the symbol's Gold sequence */
  uint32_t delay_off;   /* index of antenna 0's entry in est_delay */
  uint32_t pad2;
  uint64_t rx_off;      /* c16 offset of antenna 0's subcarrier 0 of the DMRS symbol in rxdataF */
  uint64_t ch_off;      /* c16 offset of antenna 0's estimate of PUSCH subcarrier 0 in ul_ch */
} nrLDPC_hip_chest_seg_t;
typedef struct nrLDPC_hip_pusch_chest_cfg {
  uint32_t slot, scid, dmrs_scrambling_id, port;
  uint32_t chest_freq;  /* 0: interpolation in frequency, 1: average per PRB */
} nrLDPC_hip_pusch_chest_cfg_t;
int32_t nrLDPC_hip_pusch_channel_estimation(const int16_t *rxdataF, uint64_t rx_ant_stride, int16_t *ul_ch, uint64_t ch_ant_stride, uint32_t n_rx,
                                            const nrLDPC_hip_chest_seg_t *seg, uint32_t n_seg, const int32_t *est_delay, int32_t mem, void *stream);
int32_t nrLDPC_hip_pusch_chest_host(const int16_t *rxdataF, const nrLDPC_hip_chest_seg_t *seg, int32_t est_delay, int16_t *ul_ch);
int32_t nrLDPC_hip_pusch_dmrs_host(uint32_t c_init, uint32_t dmrs_offset, uint32_t n, uint32_t port, uint32_t type, int16_t *out);
int32_t nrLDPC_hip_delay_table_host(uint32_t fft_size, int32_t delay, int16_t *out);
int32_t nrLDPC_hip_pusch_chest_segments(const nrLDPC_hip_pusch_alloc_t *alloc, const nrLDPC_hip_pusch_chest_cfg_t *cfg, uint32_t n_alloc, uint32_t n_rx,
                                        nrLDPC_hip_chest_seg_t *seg_out, uint32_t cap, uint32_t *n_seg_out);
/* The estimator's measurements and the time average of its estimates: what nr_rx_pusch_tp has when the estimation loop ends
 * (nr_ulsch_demodulation.c:1470-1535), so that a rank-2 slot needs no host value between rxdataF and the payload.
 * pusch_channel_estimation_meas: ul_ch is written exactly as pusch_channel_estimation writes it, same write set, same bits, and
 * in the same call max_ch[tb] and nvar[tb] (tb < n_tb) receive what the reference passes on to its two-layer receivers, in the
 * int32 / uint32 arrays channel_level_grid_mmse / _ml and mmse_2layers_grid read.  Descriptor i belongs to block seg_tb[i] (host
 * memory, like the descriptors); a block's descriptors -- all its DMRS symbols, both layers' ports -- need not be adjacent.
 *   One descriptor is one call of nr_pusch_channel_estimation (one DMRS symbol, one port, all n_rx antennas) with noise_amp2, a
 *   uint64, and nest_count starting at 0 (nr_ul_channel_estimation.c:148-149):
 *     TYPE1_INTERP  max over the 3 rb_size LS pairs of |r|, |i| of the int32 value BEFORE the int16 cast (:186-187: a full-scale
 *       grid gives more than 32767 where the estimate wraps); every RE k < 12 rb_size adds c16amp2(c16sub(ul_ls_est[k], ul_ch[k]))
 *       (:246-247), ul_ls_est[k] the cast LS value of pair k >> 2, ul_ch[k] the estimate the call stores, the difference wrapping
 *       to int16, its square sum a uint32; nest_count = 12 rb_size n_rx.
 *     TYPE2_INTERP  per pair n < 2 rb_size: max over ch = (ch0 + ch1) >> 1 (:268-269), noise_amp2 += c16amp2(c16sub(ch0, ch))
 *       (:273); nest_count = 2 rb_size n_rx.
 *     TYPE1_AVG / TYPE2_AVG  max over the averages of PRBs 1 .. rb_size - 2: the first and the last PRB are not looked at, as
 *       written (:295, :330 against :309-311), so rb_size <= 2 contributes nothing; nest_count = 0.  TYPE2_AVG takes the values
 *       this estimator forms (its two deviations above).
 *     nvar_tmp = (uint32_t)(noise_amp2 / nest_count), 0 when nest_count = 0 (:468-469, nr_ulsch_demodulation.c:1481).
 *   max_ch[tb] = the maximum over the block's descriptors and antennas, from 0 (:1470, :1489); nvar[tb] = (sum of the block's
 *   nvar_tmp, a uint32 sum) / nvar_div[tb] (:1491, :1524), where the caller passes nvar_div[tb] = nr_of_symbols nrOfLayers n_rx
 *   (host memory) -- all symbols of the allocation, not its DMRS symbols, as written.  A block without a descriptor gets 0 and 0.
 *   Integer maximum and sum do not depend on the order, so the values are bit for bit the reference's.
 * mem, staging and refusals are pusch_channel_estimation's; refused besides, before anything is enqueued or written: a NULL
 * seg_tb / nvar_div / max_ch / nvar, seg_tb[i] >= n_tb, nvar_div[tb] = 0, (DEVICE) max_ch / nvar that are not 4-byte aligned device
 * memory of that GPU.  A capturing stream is refused.
 * pusch_chest_meas_host: one descriptor over n_rx antennas on the CPU from csrc/nr_chest.h, no GPU (rx_off and delay_off apply,
 * est_delay may be NULL; nothing is stored but the three results): *max_ch from 0, *noise_amp2, *nest_count.
 * pusch_chest_time_avg: nr_chest_time_domain_avg (openair1/PHY/NR_REFSIG/dmrs_nr.c:343-417).  For plane q < n_plane of descriptor
 * i the 12 rb_size c16 at ch_off[0] + q ch_ant_stride are overwritten with the average of those at ch_off[0 .. n_sym - 1] + q
 * ch_ant_stride: the later symbols are added to the first with adds_epi16 -- saturating per int16 component, one symbol after
 * the other in the order given -- then >> 1 (two symbols), >> 2 (four), C's / 3 (three: towards zero, not a shift).  n_sym = 1
 * reads and writes nothing; the other symbols' estimates stay as they are.  The reference loops over nb_antennas_rx planes of
 * ch_estimates, which with two layers are layer 0's alone: n_plane = n_rx reproduces that, n_plane = 2 n_rx averages both layers.
 * Afterwards the grid calls read the first DMRS symbol: the caller puts first_dmrs_out into the allocation's dmrs_symbol
 * (:1535-1536 of nr_ulsch_demodulation.c).  mem as above (HOST stages the span from the lowest to the highest c16 the descriptors
 * reach and copies only the write set back).  Refused: NULL arrays, n_plane outside 1..16, n_sym outside 1..4 (the reference
 * asserts beyond four), rb_size = 0, write ranges of two (descriptor, plane) pairs that overlap, a later symbol's range that
 * overlaps a written range, another mem value, a misaligned or foreign device pointer, a capturing stream.
 * pusch_chest_time_avg_host: one descriptor, one plane, on the CPU from the same header, no GPU.
 * pusch_chest_avg_segments (host only): one descriptor per allocation with ch_off[k] = the allocation's ch_off + (its k-th DMRS
 * symbol) fft_size and first_dmrs_out[i] = its first DMRS symbol.  It counts the DMRS symbols inside the allocation where the
 * reference counts the bitmap's bits from symbol 0 (get_dmrs_symbols_in_slot); a valid PDU has no DMRS bit outside its symbols, so
 * the two are equal.  Refused: what pusch_chest_segments refuses of the allocation's symbols and width, no DMRS symbol, more than
 * four, more descriptors than cap. */
typedef struct nrLDPC_hip_chest_avg_seg {
  uint64_t ch_off[4]; /* c16 offset of plane 0's estimate of PUSCH subcarrier 0 in the k-th DMRS symbol; [0] is overwritten */
  uint32_t n_sym;     /* DMRS symbols, 1..4 */
  uint32_t rb_size;
} nrLDPC_hip_chest_avg_seg_t;
int32_t nrLDPC_hip_pusch_channel_estimation_meas(const int16_t *rxdataF, uint64_t rx_ant_stride, int16_t *ul_ch, uint64_t ch_ant_stride, uint32_t n_rx,
                                                 const nrLDPC_hip_chest_seg_t *seg, uint32_t n_seg, const int32_t *est_delay, const uint32_t *seg_tb,
                                                 const uint32_t *nvar_div, uint32_t n_tb, int32_t *max_ch, uint32_t *nvar, int32_t mem, void *stream);
int32_t nrLDPC_hip_pusch_chest_meas_host(const int16_t *rxdataF, uint64_t rx_ant_stride, uint32_t n_rx, const nrLDPC_hip_chest_seg_t *seg,
                                         const int32_t *est_delay, int32_t *max_ch, uint64_t *noise_amp2, uint32_t *nest_count);
int32_t nrLDPC_hip_pusch_chest_time_avg(int16_t *ul_ch, uint64_t ch_ant_stride, uint32_t n_plane, const nrLDPC_hip_chest_avg_seg_t *seg, uint32_t n_seg,
                                        int32_t mem, void *stream);
int32_t nrLDPC_hip_pusch_chest_time_avg_host(int16_t *ul_ch, const nrLDPC_hip_chest_avg_seg_t *seg);
int32_t nrLDPC_hip_pusch_chest_avg_segments(const nrLDPC_hip_pusch_alloc_t *alloc, uint32_t n_alloc, nrLDPC_hip_chest_avg_seg_t *out, uint32_t cap,
                                            uint32_t *n_out, uint8_t *first_dmrs_out);
/* The delay search: what nr_est_delay (common/utils/nr/nr_common.c:968-990) looks for in the LS estimates of the same DMRS symbol,
 * so that pusch_est_delay -> pusch_channel_estimation(_meas) -> level -> compensation -> decode on one stream needs no host value.
 * csrc/nr_delay.h defines it once for host and device.  For one descriptor (the estimation's, unchanged) and antenna a, N =
 * fft_size:
 *   x[k], k < N, indexed from the allocation's first RE as the reference's ul_ls_est is, zero for k >= 12 rb_size.  TYPE1_INTERP:
 *     x[4n + j], j = 0..3, is the int16-cast LS value of pilot pair n (nr_ul_channel_estimation.c:176-192); TYPE2_INTERP: REs 0..3
 *     of 6-RE block m hold ch & ~3 per component, REs 4, 5 hold ch (:264-272).  Bit for bit csrc/nr_chest.h's values.  Every antenna
 *     starts from zeros (the reference's type-2 line :270 adds into an array it clears once per call: not reproduced).
 *   y[n] = sum_k x[k] exp(+2 pi i k n / N), unnormalised, in fp32; P[n] = |y[n]|^2.
 *   The scan n = 0 .. N - 1 with P > best (strict) from best = 0, position 0; a position > N/2 has N subtracted.
 *   flags = NRLDPC_HIP_DELAY_RUNNING_MAX: best and its position are cleared per descriptor and carried from antenna 0 to antenna a,
 *     as the reference's delay_t is: antenna a receives the position of the largest sample over antennas 0 .. a.
 *   flags = NRLDPC_HIP_DELAY_PER_ANTENNA: cleared per antenna -- for a receiver whose antennas see different delays.
 *   TYPE1_AVG / TYPE2_AVG descriptors take no delay: 0.  Nothing is clamped: the estimator clamps where it reads the value.
 * The call writes exactly n_rx int32 at est_delay[delay_off + a], the array the estimation calls read, and, where peak is given,
 * the best that belongs to each delay at the same indices.  An all-zero symbol gives delay 0 and peak 0.
 * This is the quantity the reference's fixed-point IDFT (oai_dfts.c) approximates, not a port of it: where two samples are closer
 * than the transforms' errors the two may pick different samples.  Host form, kernel and the kernel run on the
 * CPU perform the same IEEE operations in the same order and agree bit for bit, peaks included.
 * mem = HOST stages the span of the grid the pilots lie in, as pusch_channel_estimation does.  mem = DEVICE enqueues two kinds of
 * launches on `stream` (one search per fft_size, one combination) and returns; the first call per (GPU, fft_size) also allocates
 * that size's twiddle table (fft_size + 4 float pairs, kept until the process ends) and uploads it with a synchronous copy, so
 * it blocks: run one call per fft_size at start-up where the first slot must not wait.
 * Refused before anything is enqueued or written: what pusch_channel_estimation refuses of n_rx, mem and the descriptors, a NULL
 * rxdataF / seg / est_delay, an unknown flag, delay ranges [delay_off, delay_off + n_rx) of two descriptors that overlap, a
 * misaligned or foreign device pointer, a capturing stream.
 * pusch_est_delay_host: one descriptor over n_rx antennas on the CPU from the same header, no GPU (rx_off and delay_off apply). */
#define NRLDPC_HIP_DELAY_RUNNING_MAX 0
#define NRLDPC_HIP_DELAY_PER_ANTENNA 1
int32_t nrLDPC_hip_pusch_est_delay(const int16_t *rxdataF, uint64_t rx_ant_stride, uint32_t n_rx, const nrLDPC_hip_chest_seg_t *seg, uint32_t n_seg,
                                   uint32_t flags, int32_t *est_delay, float *peak, int32_t mem, void *stream);
int32_t nrLDPC_hip_pusch_est_delay_host(const int16_t *rxdataF, uint64_t rx_ant_stride, uint32_t n_rx, const nrLDPC_hip_chest_seg_t *seg, uint32_t flags,
                                        int32_t *est_delay, float *peak);
/* ---------------------------------------------------------------------------------------------------
 * PDSCH resource mapping with DMRS onto the transmit grid: the resource mapping loop of nr_generate_pdsch (openair1/PHY/
 * NR_TRANSPORT/nr_dlsch.c:205-474) and its unit-precoding copy (:483-535) for one list of descriptors, one per (allocation, OFDM
 * symbol), times n_tx antennas -- the mirror image of pusch_channel_estimation + channel_compensation_grid, so that
 * dlsch_encode_symbols -> pdsch_resource_mapping on one stream takes a slot from payload bytes to txdataF.  csrc/nr_pdsch_map.h
 * defines the mapping once for host and device.
 * Read: for layer l < Nl the nb_re c16 at int16 offset lay_off + 2 (l plane + sym_off) of `layers` (the layer planes
 * dlsch_encode_symbols wrote at lay_off), and the descriptors.  Written: for every descriptor and antenna a < n_tx exactly the
 * 12 rb_size c16 at txdataF index tx_off + a tx_ant_stride + (start_re + i) mod fft_size, i = 0 .. 12 rb_size - 1, overwritten;
 * nothing else.  Antenna a < Nl receives layer a, the antennas Nl <= a < n_tx zeros (unit precoding, pmi = 0).
 * The value at allocation subcarrier i, by the symbol's pattern:
 *   NRLDPC_HIP_PDM_FULL (no DMRS)  data everywhere: mulhrs(amp, x) per component, x the next entry of the layer plane.
 *   _DMRS1 / _DMRS2 (DMRS type 1 / 2), the pilot test first as in the reference:
 *     pilot of the layer's port  i = 4n + 2k' + delta (type 1), 6n + k' + delta (type 2); the j-th pilot of the allocation (k' =
 *       j & 1) is the unconjugated QPSK point (nrLDPC_hip_mod_table(2)) of bits 2 (dmrs_offset + j) and the next of the Gold
 *       sequence of c_init, times Wt[l_prime] Wf[k'] amp at shift 15, flooring; delta, Wf, Wt: nr_sch_dmrs.c:37-57
 *     data                       i % 2 >= ncdm (type 1), i % 6 >= 2 ncdm (type 2): x amp >> 15, truncating (not mulhrs)
 *     everything else            0
 * Deviations from the reference: every data RE of a FULL symbol is mulhrs (the reference's scalar tail, the
 * last len % 4 REs of each piece of a symbol, omits the final shift, :428-435, :460-467), and the pattern is decided by i, never
 * by the grid subcarrier (allowed_xlsch_re_in_dmrs_symbol takes diff = fft_size at the first subcarrier, dmrs_nr.c:45-48).
 * PTRS, interleaved VRB mapping and CSI-RS / SSB collisions are not built; precoding matrices other than unit: the precoded call
 * below.
 * mem = HOST: synchronous; stages the span of the layer planes the descriptors reach, works on a bounce of the span of the grid
 * from the lowest to the highest c16 written, and copies only the write set back.  mem = DEVICE enqueues on `stream` (one launch
 * per pattern present); the descriptors go through the calling thread's page-locked job area.
 * Refused before anything is enqueued or written: NULL arrays, n_tx outside 1..8 or below a descriptor's Nl, a pattern that is
 * none of the three, Nl outside 1..4, (DMRS symbols) ncdm outside 1..2 (type 1) / 1..3 (type 2), l_prime > 1, a port outside
 * 0..7 (type 1) / 0..11 (type 2), c_init >= 2^31, dmrs_offset > 2^20; amp <= 0, rb_size = 0, 12 rb_size > fft_size, start_re >=
 * fft_size, an fft_size other than 128, 256, 512, 1024, 1536, 2048, 4096, 6144, 8192, nb_re that is not the pattern's number of
 * data REs (rb_size times those of a PRB, the same for every layer's port), sym_off + nb_re > plane, lay_off odd, output
 * ranges of two (descriptor, antenna) pairs that overlap, another mem value, (DEVICE) an array that is not device memory of
 * one GPU or not 4-byte aligned, a capturing stream; nrLDPC_hip_last_error() names the reason.  The calls do not know the
 * arrays' extents; the Python wrappers, which do, refuse a descriptor that reaches outside.
 * pdsch_map_host: one descriptor and one antenna on the CPU from the same header, no GPU: layer 0 .. Nl - 1 maps that layer,
 * a negative layer writes the zeros of an antenna behind the layers; tx_off and lay_off apply.  0 / -1.
 * pdsch_dmrs_host: n unconjugated pilots (before Wt Wf amp) from sequence symbol dmrs_offset on.
 * pdsch_map_segments (host only, no GPU): one descriptor per OFDM symbol of each allocation, in symbol order: start_re =
 * (first_carrier_offset + (rb_start + bwp_start) 12) % fft_size (:208-210), dmrs_offset = (rb_start + bwp_start) 6 (type 1) or 4
 * (type 2), without bwp_start when si_rnti (:260-263), l_prime by the reference's rule (:229-230, :264-269) starting from the
 * lowest set bit of dl_dmrs_symb_pos, layer l's port the l-th set bit of dmrs_ports (get_dmrs_port, nr_common.c:494; an empty
 * bitmap is port 0), c_init as nr_init_pdsch_dmrs (nr_gold.c:87-88), sym_off the running sum of nb_re, tx_off = tx_slot_off +
 * symbol fft_size.  Refused: start_symbol + nr_of_symbols > 14, nr_of_symbols = 0, no port for a layer, the running sum
 * different from plane at the end, scid > 1, dl_dmrs_scrambling_id > 65535, slot >= 160, amp outside 1..32767, more than cap
 * descriptors, and anything the mapping call would refuse. */
#define NRLDPC_HIP_PDM_FULL 0
#define NRLDPC_HIP_PDM_DMRS1 1
#define NRLDPC_HIP_PDM_DMRS2 2
typedef struct nrLDPC_hip_pdsch_map_seg {
  uint8_t pattern;      /* NRLDPC_HIP_PDM_* */
  uint8_t Nl;           /* layers, 1..4 */
  uint8_t ncdm;         /* numDmrsCdmGrpsNoData (DMRS symbols) */
  uint8_t l_prime;      /* 0, or 1 for the second symbol of a double-symbol DMRS */
  uint8_t port[4];      /* layer l's antenna port p - 1000 (DMRS symbols) */
  int16_t amp;          /* > 0 */
  uint16_t pad;
  uint32_t fft_size;    /* N, the OFDM symbol size */
  uint32_t start_re;    /* grid subcarrier of PDSCH subcarrier 0, < N */
  uint32_t rb_size;
  uint32_t nb_re;       /* data REs per layer in this OFDM symbol */
  uint32_t sym_off;     /* first entry of each layer plane this symbol takes */
  uint32_t plane;       /* c16 values per layer plane (G / (Qm Nl)) */
  uint32_t dmrs_offset; /* first sequence symbol (DMRS symbols) */
  uint32_t c_init;      /* of the symbol's Gold sequence (DMRS symbols) */
  uint32_t pad2;
  uint64_t tx_off;      /* c16 offset of antenna 0's subcarrier 0 of this OFDM symbol in txdataF */
  uint64_t lay_off;     /* int16 offset of the block's dlsch_encode_symbols output in layers, even */
} nrLDPC_hip_pdsch_map_seg_t;
typedef struct nrLDPC_hip_pdsch_alloc {
  uint32_t Nl;
  uint32_t plane;                     /* c16 values per layer plane (G / (Qm Nl)) */
  uint32_t dmrs_config_type;          /* 0: type 1, 1: type 2 */
  uint32_t num_dmrs_cdm_grps_no_data;
  uint32_t dmrs_ports;                /* bit p: port p carries a layer, lowest first */
  uint32_t scid, dl_dmrs_scrambling_id, slot;
  uint32_t si_rnti;                   /* != 0: the DMRS reference point leaves bwp_start out */
  int32_t amp;
  uint32_t fft_size;                  /* N */
  uint32_t first_carrier_offset;
  uint32_t bwp_start, rb_start, rb_size;
  uint32_t start_symbol, nr_of_symbols;
  uint32_t dl_dmrs_symb_pos;          /* bit s: symbol s carries DMRS */
  uint64_t tx_slot_off;               /* c16 offset of antenna 0's symbol 0, subcarrier 0 of the slot in txdataF */
  uint64_t lay_off;                   /* int16 offset of the block's dlsch_encode_symbols output in layers, even */
} nrLDPC_hip_pdsch_alloc_t;
int32_t nrLDPC_hip_pdsch_resource_mapping(const int16_t *layers, int16_t *txdataF, uint64_t tx_ant_stride, uint32_t n_tx,
                                          const nrLDPC_hip_pdsch_map_seg_t *seg, uint32_t n_seg, int32_t mem, void *stream);
int32_t nrLDPC_hip_pdsch_map_host(const int16_t *layers, const nrLDPC_hip_pdsch_map_seg_t *seg, int32_t layer, int16_t *txdataF);
int32_t nrLDPC_hip_pdsch_dmrs_host(uint32_t c_init, uint32_t dmrs_offset, uint32_t n, int16_t *out);
int32_t nrLDPC_hip_pdsch_map_segments(const nrLDPC_hip_pdsch_alloc_t *alloc, uint32_t n_alloc, nrLDPC_hip_pdsch_map_seg_t *seg_out, uint32_t cap,
                                      uint32_t *n_seg_out);
/* ---------------------------------------------------------------------------------------------------
 * PDSCH resource mapping with precoding: the same mapping, then layers to antenna ports through per-PRG matrices -- both branches
 * of the precoding loop of nr_generate_pdsch (nr_dlsch.c:486-589) with nr_layer_precoder_simd (openair1/PHY/MODULATION/
 * nr_modulation.c:720-821).  pdsch_resource_mapping stays as it is; this call takes the same descriptors plus, parallel to them,
 * one nrLDPC_hip_pdsch_prg_t each: prg_size (rel15->precodingAndBeamforming.prg_size; 0 = unit precoding of the whole descriptor)
 * and the range pmi_off, pmi_count of the descriptor's PMIs in the flat list pmi_list[n_pmi] (prgs_list[].pm_idx, one per PRG), and
 * the precoding-matrix table pm[n_pm] (gNB_config.pmi_list.pmi_pdu; nfapi_nr_pm_pdu_t with room for 8 ports), found by pm_idx, in
 * any order.  Let m_l[i] be what pdsch_resource_mapping yields for layer l at allocation subcarrier i.  RE i lies in RB i / 12, its
 * pmi = prg_size > 0 ? pmi_list[pmi_off + (i / 12) / prg_size] : 0.  Antenna a < n_tx receives
 *   pmi == 0   m_a[i] for a < Nl, otherwise 0: a copy, bit for bit the unit call's result.  Unit and other PRGs may be mixed.
 *   pmi != 0   the sum over l = 0 .. Nl - 1, in this order, from 0, accumulated with adds_epi16 (saturating per component), of
 *              x w >> 15 with x = m_l[i], w = weights[l][a] of the matrix whose pm_idx is pmi:
 *                re = low16((x.r w.r + x.i nwi) as wrapping int32 >> 15), nwi = -w.i cast to int16 (-(-32768) stays -32768)
 *                im = low16((x.r w.i + x.i w.r) as wrapping int32 >> 15); the shifted value is cut to 16 bits, not saturated.
 * Deviation from the reference: it sends the one RB step of a symbol that reaches or crosses fft_size through
 * nr_layer_precoder_cm (c16maddShift, tools_defs.h:226-231), which accumulates with wrap-around and negates w.i in int32; here
 * every RE is the SIMD definition above.  The two agree whenever no accumulation leaves int16 and no w.i is -32768.
 * Read and written as pdsch_resource_mapping: exactly the 12 rb_size c16 per (descriptor, antenna < n_tx), overwritten, wrapping
 * at fft_size.  The matrices and PMI lists are host memory in both mem modes: the PMIs are resolved against the table on the host
 * and travel, with the matrices in use, in the descriptors' one upload through the calling thread's page-locked job area.
 * Refused before anything is enqueued or written: everything pdsch_resource_mapping refuses; a NULL prg; with a PMI that is not
 * 0: n_tx < 2, a NULL table, a PMI that no table entry carries, numLayers != Nl, num_ant_ports < n_tx or > 8; pm_idx == 0 in the
 * table or a pm_idx twice in it; a PMI range shorter than ceil(rb_size / prg_size) or reaching outside pmi_list (a NULL pmi_list
 * has no entries).  With prg_size = 0 the range is not looked at.
 * pdsch_precode_host: one descriptor and antenna `ant` < n_tx on the CPU from the same header, no GPU; tx_off and lay_off apply
 * (the caller adds ant tx_ant_stride to tx_off).  0 / -1.
 * pdsch_precode_segments (host only, no GPU): pdsch_map_segments' descriptors for each allocation plus, per descriptor, the
 * allocation's alloc_prg[i]: every symbol of an allocation shares the range.  Refused: what pdsch_map_segments refuses (under its
 * name), a range shorter than ceil(rb_size / prg_size) or reaching beyond n_pmi, more than cap descriptors. */
typedef struct nrLDPC_hip_pm_pdu {
  uint16_t pm_idx;           /* 1..65535; 0 is the unit matrix and has no entry */
  uint16_t numLayers;
  uint16_t num_ant_ports;    /* >= n_tx, <= 8 */
  uint16_t pad;
  int16_t weights[4][8][2];  /* [layer][antenna port] (Re, Im), Q15 */
} nrLDPC_hip_pm_pdu_t;
typedef struct nrLDPC_hip_pdsch_prg {
  uint32_t prg_size;         /* RBs per PRG; 0: unit precoding */
  uint32_t pmi_off;          /* the descriptor's first PMI in pmi_list */
  uint32_t pmi_count;        /* >= ceil(rb_size / prg_size) */
} nrLDPC_hip_pdsch_prg_t;
int32_t nrLDPC_hip_pdsch_resource_mapping_precoded(const int16_t *layers, int16_t *txdataF, uint64_t tx_ant_stride, uint32_t n_tx,
                                                   const nrLDPC_hip_pdsch_map_seg_t *seg, const nrLDPC_hip_pdsch_prg_t *prg, uint32_t n_seg,
                                                   const uint16_t *pmi_list, uint32_t n_pmi, const nrLDPC_hip_pm_pdu_t *pm, uint32_t n_pm, int32_t mem,
                                                   void *stream);
int32_t nrLDPC_hip_pdsch_precode_host(const int16_t *layers, const nrLDPC_hip_pdsch_map_seg_t *seg, const nrLDPC_hip_pdsch_prg_t *prg,
                                      const uint16_t *pmi_list, uint32_t n_pmi, const nrLDPC_hip_pm_pdu_t *pm, uint32_t n_pm, uint32_t n_tx, uint32_t ant,
                                      int16_t *txdataF);
int32_t nrLDPC_hip_pdsch_precode_segments(const nrLDPC_hip_pdsch_alloc_t *alloc, const nrLDPC_hip_pdsch_prg_t *alloc_prg, uint32_t n_alloc, uint32_t n_pmi,
                                          nrLDPC_hip_pdsch_map_seg_t *seg_out, nrLDPC_hip_pdsch_prg_t *prg_out, uint32_t cap, uint32_t *n_seg_out);
/* ---------------------------------------------------------------------------------------------------
 * The reference's OFFLOAD plugin slot (`ldpc_interface_offload`, loaded with the suffix "_t2": nr_init.c:138-139).  Same
 * signatures as LDPCdecoder / LDPCencoder, the semantics of nrLDPC_decoder/nrLDPC_decoder_offload.c:1036-1140: one
 * segment per call, rate (de)matching + (de)interleaving + HARQ combining inside, soft buffers kept on the device per
 * (ulsch_id, segment).  libldpc_hip_t2.so (csrc/ldpc_t2_shim.c) exports them under the plugin names.
 *   decoder: p_llr = E int8 LLRs in transmission order; p_decParams: BG, Z, R, numMaxIter + E, Qm, rv, F, setCombIn
 *     (0: the soft buffer starts afresh, 1: combine); C = segment number r; p_out = ceil(K/8) decoded bytes.  Parity-check
 *     stop.  Returns the passes run (> numMaxIter: not decoded), < 0 on a hard error (nr_ulsch_decoding.c:269).
 *   encoder: input[0] = the segment's K - F bits (CB CRC attached by the caller), output[0] = E rate-matched,
 *     interleaved bits, one per byte; impp: BG, Zc, K, F, Kb, E, Qm, rv.  Returns 0 / -1.
 * ------------------------------------------------------------------------------------------------- */
int32_t nrLDPC_hip_offload_init(void);
int32_t nrLDPC_hip_offload_decoder(t_nrLDPC_dec_params *p_decParams, uint8_t harq_pid, uint8_t ulsch_id, uint8_t C, int8_t *p_llr,
                                   int8_t *p_out, t_nrLDPC_time_stats *p_profiler, decode_abort_t *ab);
int32_t nrLDPC_hip_offload_encoder(uint8_t **input, uint8_t **output, encoder_implemparams_t *impp);
/* helpers with the reference's semantics (nr_segmentation parameter part, nr_get_E, nr_get_R_ldpc_decoder) */
int32_t nrLDPC_hip_segmentation(uint32_t B, uint8_t BG, uint32_t *C, uint32_t *K, uint32_t *Zc, uint32_t *F); /* returns Kb, -1 */
uint32_t nrLDPC_hip_get_E(uint32_t G, uint32_t C, uint32_t Qm, uint32_t Nl, uint32_t r);
int32_t nrLDPC_hip_get_R_ldpc_decoder(int32_t rvidx, int32_t E, int32_t BG, int32_t Z, int32_t *llrLen, int32_t round);
/* Columns of the code graph nrLDPC_hip_ulsch_decode() decodes a segment on; R = what nr_get_R_ldpc_decoder chose (its mode has
 * 68 / 35 / 27 resp. 52 / 32 / 17 columns, nrLDPCdecoder_defs.h:53-57, 80-84).  A first transmission (round 0: the soft buffer is
 * cleared, nr_ulsch_decoding.c:418-422) leaves every position behind the last one it reaches at zero; a check node that closes on
 * an all-zero degree-1 column sends zeros to its other neighbours in every pass (nrLDPC_cnProc.h:105-114: the minimum over the
 * OTHER inputs), and the chain stops on the CRC -- so the rows behind the last column that received anything are not run: same
 * payload, verdict and pass count as on the whole mode.  NRLDPC_HIP_TB_TRUNC=0 turns it off.  -1: invalid parameters. */
int32_t nrLDPC_hip_ulsch_decoder_columns(int32_t BG, uint32_t Zc, uint32_t C, uint32_t F, uint32_t K, uint32_t Tbslbrm, int32_t rv,
                                         uint32_t E, int32_t round, int32_t R);

/* Introspection for tests and benchmarks */
int32_t nrLDPC_hip_num_llr(int BG, int Z, int R);      /* ncols*Z, -1 if invalid */
int32_t nrLDPC_hip_out_bytes(int BG, int Z, int R, int outMode);
int32_t nrLDPC_hip_lds_bytes(int BG, int Z, int R);    /* LDS a decoder workgroup uses for this code */
/* info = {rows, columns, edges of the (BG, R) base graph; 1 if the fast decoder kernel serves the code; its workgroup
 * size; its LDS bytes; check-node and bit-node tasks per pass (fast kernel)}.  0, or -1 for an invalid code. */
int32_t nrLDPC_hip_code_info(int BG, int Z, int R, int32_t info[8]);
/* resident submission path behind LDPCdecoder (csrc/ldpc_server.h): out = {status (-1 not started yet, 0 in use, 1 switched
 * off or unavailable), caller slots, server kernel launches so far, calls served through it, and summed over those calls
 * in ns: GPU doorbell-seen -> payload staged, staged -> decoded, host doorbell -> completion seen, whole host call} */
int32_t nrLDPC_hip_server_stats(int64_t out[8]);
/* HIP events around the stages of the calling thread's nrLDPC_hip_ulsch_decode calls, recorded on the stream the kernels
 * run on (primary device): enable != 0 switches the recording on for the calls that follow; out_us, when not NULL, receives
 * the last recorded call's {de-matching kernel, decoder launches (the fused segment kernel), reassembly + verdict kernels,
 * their sum} in microseconds (waits for that call).  What bench.py's chain_roofline is computed from.  0 / -1. */
int32_t nrLDPC_hip_chain_timing(int32_t enable, float out_us[4]);
/* check_crc() of openair1/PHY/CODING/crc_byte.c:314-380 (same arguments, same result): the predicate to put into
 * t_nrLDPC_dec_params::check_crc by callers that do not carry OAI's own -- it selects the CRC evaluated on the GPU -- and a
 * correct host implementation for whoever calls it. */
int nrLDPC_hip_check_crc(uint8_t *decoded_bytes, uint32_t n, uint8_t crc_type);
const char *nrLDPC_hip_last_error(void);
const char *nrLDPC_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif
