/*
 * tb_chain.h -- device jobs of the transport-block chain around the LDPC codec (SURVEY section 8 rows a16-a20,
 * f2, f3): TB CRC attach, code-block segmentation + CB CRC, rate matching + bit interleaving (TX);
 * de-interleaving + rate de-matching with HARQ soft combining + int16->int8 pack, TB reassembly + TB CRC (RX).
 */
#ifndef TB_CHAIN_H
#define TB_CHAIN_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tb_jobs.h"

/* TB CRC attach in two steps: per-chunk partial CRCs XOR-ed into acc[tb], then the CRC bytes.  acc[] must be zero on
 * entry and is zero again on exit (uploaded as zeros with the plan; no memset per call) */
/* with_final = 0: only the partial CRCs (the fused TX kernel places the CRC bytes itself and clears acc) */
hipError_t tb_launch_tx_crc(const tb_tx_tb_job *jobs, uint32_t n_tb, const tb_crc_chunk_job *chunks, uint32_t n_chunks,
                            const uint8_t *payload, uint8_t *scratch, uint32_t *acc, const uint32_t *pow24a,
                            const uint32_t *pow16, int with_final, hipStream_t s);
hipError_t tb_launch_tx_segment(const tb_tx_seg_job *jobs, uint32_t n, uint8_t *scratch, const uint32_t *pow24b, hipStream_t s);
hipError_t tb_launch_tx_ratematch(const tb_tx_seg_job *jobs, uint32_t n, const uint8_t *scratch, uint8_t *coded, hipStream_t s);
/* segmentation + CB CRC + encoding + rate matching + interleaving in one kernel (bit-packed encoder, tb_tx_core.h).  Its LDS
 * behind the encoder's (ldpc_enc_launch_shape): the CB CRC's meeting place, the segment's bytes, the selection chunk's Qm <= 8
 * sub-streams (the CRC byte table lies there until the selection starts), then what the store form adds (tb_jobs.h):
 * the chunk's sequence words and the carry words (TB_TX_FUSED_SCR_LDS) or the constellation (TB_TX_FUSED_SYM_LDS). */
#define TB_TX_SEL_SYMS 2048 /* modulation symbols per selection chunk: Qm sub-streams of that many bits are staged in LDS */
#define TB_TX_SEL_STRIDE (TB_TX_SEL_SYMS / 32 + 1) /* words from one sub-stream to the next */
#define TB_TX_SEG_LDS (1056 + 16) /* K / 8 <= 1056 segment bytes; the image is written in dwords and cleared to K / 8 + 8 */
#define TB_TX_FUSED_EXTRA_LDS (8 + TB_TX_SEG_LDS + 8 * TB_TX_SEL_STRIDE * 4)
struct tb_tx_fused_lds {
  uint32_t *red;    /* [2] */
  uint8_t *c;       /* [TB_TX_SEG_LDS] */
  uint32_t *tab;    /* [256], = sel */
  uint32_t *sel;    /* [8][TB_TX_SEL_STRIDE] */
  uint32_t *seq;    /* [TB_TX_SCR_WORDS], packed and symbol store only */
  uint32_t *behind; /* the packed store's carry words / the symbol store's constellation */
};
TB_HD tb_tx_fused_lds tb_tx_fused_carve(uint32_t *behind_encoder)
{
  tb_tx_fused_lds l;
  l.red = behind_encoder;
  l.c = reinterpret_cast<uint8_t *>(l.red + 2);
  l.tab = l.sel = reinterpret_cast<uint32_t *>(l.c + TB_TX_SEG_LDS);
  l.seq = l.sel + 8 * TB_TX_SEL_STRIDE;
  l.behind = l.seq + TB_TX_SCR_WORDS;
  return l;
}
/* what a segment's workgroup stores: E bytes holding a bit each at coded + out_off; the packed, scrambled words (jobs' c_init /
 * bit_off / h_* / t_*, tb_tx_scr.h): ceil(G/32) per TB at coded + out_off, tickets[] zero on entry and on exit, parts[] one slot
 * per (shared word, segment); the symbols (nrLDPC_hip_dlsch_encode_symbols; jobs' c_init / bit_off / Nl / plane, tb_tx_sym.h):
 * 4 G / Qm bytes of layer planes per TB at coded + out_off */
enum tb_tx_out { TB_TX_OUT_BYTES, TB_TX_OUT_PACKED, TB_TX_OUT_SYMBOLS };
struct ldpc_enc_job;
/* enc_lds = the encoder's LDS; tickets, parts: TB_TX_OUT_PACKED only (nullptr otherwise) */
hipError_t tb_launch_tx_fused(tb_tx_out mode, const tb_tx_seg_job *jobs, const struct ldpc_enc_job *ejobs, uint32_t n, int n_threads,
                              int enc_lds, const uint8_t *scratch, uint8_t *coded, const uint32_t *pow24b, uint32_t *acc,
                              uint32_t *tickets, uint32_t *parts, hipStream_t s);
hipError_t tb_launch_rx_dematch(const tb_rx_seg_job *jobs, uint32_t n, uint32_t lds_elems, const int16_t *llr, int16_t *harq,
                                int8_t *scratch, hipStream_t s, int wide = 0);
/* scrambled codewords: each segment's LLRs are unscrambled on the way in (jobs' c_init / bit_off; tb_rx_core.h) */
hipError_t tb_launch_rx_dematch_scr(const tb_rx_seg_job *jobs, uint32_t n, uint32_t lds_elems, const int16_t *llr, int16_t *harq,
                                    int8_t *scratch, hipStream_t s, int wide = 0);
/* scrambled codewords received as symbol records (nrLDPC_hip_ulsch_decode_symbols): `llr` holds each block's planar record
 * (jobs' plane), demapped and unscrambled on the way in (tb_rx_core.h) */
hipError_t tb_launch_rx_dematch_sym(const tb_rx_seg_job *jobs, uint32_t n, uint32_t lds_elems, const int16_t *llr, int16_t *harq,
                                    int8_t *scratch, hipStream_t s, int wide = 0);
/* Fused segment kernel (tb_rx_fused.hip): one workgroup takes a code segment from the received LLRs to its payload bytes --
 * de-matching (tb_rx_core.h) as the prologue of the decoder's block body, and instead of an output row the segment's bytes
 * of the payload, its share of the TB CRC and, from the last segment of a transport block to finish, the block's verdict.
 * Jobs = ldpc_dec_job with seg_idx >= 0 (a job with seg_idx < 0 is decoded as by ldpc_launch_dec_fast_jobs).  done[] and
 * the abort flags are zero on entry and on exit. */
struct tb_rx_fused_args {
  const tb_rx_seg_job *segs;
  const tb_rx_tb_job *tbs;
  const int16_t *llr;  /* device memory, or the device address of page-locked host memory (pulled over the link) */
  int16_t *harq;
  uint8_t *payload;
  uint8_t *ack;
  int32_t *iter_max;
  unsigned long long *slots; /* per segment: {CRC share, pass count | generation << 16}: written by the segment, read by
                                the last segment of its transport block to finish */
  uint32_t *gen;       /* per TB: generation, + 1 per call (never reset: the slots of earlier calls stay distinguishable) */
  int *done;           /* per TB: segments finished (zero on entry and on exit) */
  const uint32_t *pow24a;
  /* First-round stagger.  The workgroups that share a CU start together and would stay in step -- all of them in their
   * memory-bound prologue (the CU's VALUs idle, HBM contended by every CU at once), then all of them decoding.  Workgroup
   * b < stagger_cus * stagger_slots waits (b / stagger_cus) * stagger_ticks (10 ns each) before it starts, so that one
   * workgroup's prologue runs under its neighbour's decoding; a workgroup that finishes is replaced at once, so the later
   * rounds inherit the offset.  0 ticks: off. */
  uint32_t stagger_ticks, stagger_cus, stagger_slots;
  /* != 0: the int8 decoder input of a segment never leaves the CU -- it lives this many bytes into the workgroup's LDS (behind
   * the decoder's own arrays: the launch's LDS size includes it) instead of in the segment's scratch row; every job of the
   * launch is a fused one then.  The plan does this when the row fits without costing the CU a workgroup. */
  uint32_t lrow_off;
  /* != 0: some job of the launch carries LDPC_JOB_MUTE_CHECK (retransmissions): the instantiation that looks for mute items */
  uint32_t mute;
  /* != 0: every job of the launch has this lifting size, one block per workgroup (ldpc_dec_fast_block.h ZC) */
  uint32_t zc;
  /* bit 0: the prologue runs at raised issue priority, bit 1: the epilogue too (NRLDPC_HIP_TB_PRIO, default 1: level with 3) */
  uint32_t prio_pro;
  /* diagnostics (NRLDPC_HIP_TB_TRACE=<file>): per workgroup {HW_ID, XCC_ID, wall clock at start, after the prologue, after
   * the last pass, at the end, pass count, after: the LDS image is cleared, the LLRs are scattered, the soft buffer is streamed,
   * the decoder input is visible to the workgroup, 0...} as 16 x uint64; NULL normally */
  unsigned long long *trace;
  /* != 0: the segments' LLRs are a scrambled codeword (nrLDPC_hip_ulsch_decode_scrambled): the instantiation that unscrambles
   * them in its prologue (jobs' c_init / bit_off), with TB_RX_SCR_LDS bytes of sequence behind each segment's LDS image */
  uint32_t scr;
  /* != 0 (with scr): the segments' input is the symbol record of nrLDPC_hip_ulsch_decode_symbols (jobs' plane): the
   * instantiation that demaps it in its prologue */
  uint32_t sym;
};
struct ldpc_dec_args;
hipError_t tb_launch_rx_fused(const struct ldpc_dec_args &a, const tb_rx_fused_args &x, int n_threads, int lds_bytes, uint32_t n_jobs,
                              hipStream_t s);
hipError_t tb_rx_fused_init(void);
/* codeword scrambling (tb_scrambling.hip, 38.211 5.2.1 / 6.3.1.1 / 7.3.1.1) with the sequence of c_init: out[ceil(size/32)] words
 * from `size` bytes holding a bit each (bit 0 of a byte) / `size` int16 LLRs negated in place where the sequence has a one */
hipError_t nr_launch_scramble_bits(const uint8_t *in, uint32_t size, uint32_t c_init, uint32_t *out, hipStream_t s);
hipError_t nr_launch_unscramble_llr(int16_t *llr, uint32_t size, uint32_t c_init, hipStream_t s);
/* modulation mapping / soft demapping (tb_qam.hip, nr_qam.h): length / Qm points from the packed bits in[] (ceil(length/32)
 * words); nb_re RE's Qm LLRs from planes[k] = y, mag_a, mag_b, mag_c (k < Qm/2, one c16 word per RE, 4-byte aligned) */
hipError_t nr_launch_modulation(const uint32_t *in, uint32_t length, uint32_t Qm, int16_t *out, hipStream_t s);
hipError_t nr_launch_ulsch_llr(const uint32_t *const planes[4], uint32_t nb_re, uint32_t Qm, int16_t *llr, hipStream_t s);
/* the first for every transport block of an encode call in one launch: jobs[i] packs G bits from in + in_off into the words at
 * out + out_off (4-byte aligned); max_g = the largest G */
hipError_t nr_launch_scramble_bits_tb(const tb_scr_tb_job *jobs, uint32_t n_tb, uint32_t max_g, const uint8_t *in, uint8_t *out, hipStream_t s);
/* the symbol encode's three-kernel path: jobs[i] scrambles, maps and layer-maps G bits (one per byte) from in + in_off into Nl
 * planes of G / (Qm Nl) points at out + out_off (4-byte aligned), every transport block in one launch; max_s = the largest G / Qm */
hipError_t nr_launch_scramble_map_tb(const tb_sym_tb_job *jobs, uint32_t n_tb, uint32_t max_s, const uint8_t *in, uint8_t *out, hipStream_t s);
/* nr_layer_mapping for one codeword: out[l stride + i] = in[Nl i + l], c16 words, i < n_symbs / Nl, Nl = 1..4 (tb_qam.hip) */
hipError_t nr_launch_layer_mapping(const int16_t *in, uint32_t n_symbs, uint32_t Nl, int16_t *out, uint32_t stride, hipStream_t s);
/* reassembly per segment (payload copy + partial TB CRC into acc[tb], zero on entry and on exit), then per-TB verdict */
hipError_t tb_launch_rx_assemble(const tb_rx_tb_job *jobs, uint32_t n_tb, const tb_rx_seg_job *segs, uint32_t n_seg,
                                 const int32_t *n_iter, uint8_t *scratch, uint8_t *payload, uint8_t *ack, int32_t *iter_max,
                                 uint32_t *acc, int *tb_abort, const uint32_t *pow24a, const uint32_t *pow16, hipStream_t s);
#endif
