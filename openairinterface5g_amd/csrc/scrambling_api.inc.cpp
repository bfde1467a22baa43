/*
 * scrambling_api.inc.cpp -- codeword (un)scrambling entry points (included into ldpc_api.cpp; shares its library state, and the
 * call scopes of slot_call.inc.cpp).  The sequence itself: nr_gold.h, on the GPU tb_scrambling.hip, on the host nr_hip_gold_words
 * (nr_coding_host.c).
 */

namespace {

/* 38.211 7.3.1.1 / 6.3.1.1: n_RNTI < 2^16, n_ID < 1024, q = codeword 0 / 1 */
int scr_validate(uint32_t n_rnti, uint32_t q, uint32_t n_id)
{
  if (n_rnti > 0xffffu)
    return set_error("scrambling: n_RNTI above 0xFFFF");
  if (n_id > 1023u)
    return set_error("scrambling: n_ID above 1023");
  if (q > 1u)
    return set_error("scrambling: q must be 0 or 1");
  return 0;
}

int scr_check_call(const void *p, uint32_t size, int32_t mem, uint32_t n_rnti, uint32_t q, uint32_t n_id)
{
  if (scr_validate(n_rnti, q, n_id) != 0)
    return -1;
  if (size > NR_SCR_MAX_BITS)
    return set_error("scrambling: size above 2^21 bits");
  if (check_mem("scrambling", mem) != 0)
    return -1;
  if (size && !p)
    return set_error("null argument");
  return 0;
}

/* the scrambled transport-block chain calls: every argument of the batch is checked before anything is enqueued */
int scr_check_batch(const nrLDPC_hip_tb_batch_t *b, const nrLDPC_hip_tb_scr_t *scr, bool encode)
{
  if (!scr && b->n_tb)
    return set_error("scrambled: scr is NULL");
  for (uint32_t i = 0; i < b->n_tb; i++) {
    if (scr_validate(scr[i].n_RNTI, scr[i].q, scr[i].Nid) != 0)
      return -1;
    if (b->tb[i].G > NR_SCR_MAX_BITS)
      return set_error("scrambled: G above 2^21 bits");
    if (encode && (b->tb[i].coded_off & 3u))
      return set_error("encode_scrambled: coded_off must be a multiple of 4");
  }
  return 0;
}

} // namespace

extern "C" {

int32_t nrLDPC_hip_dlsch_encode_scrambled(const nrLDPC_hip_tb_batch_t *b, const nrLDPC_hip_tb_scr_t *scr)
{
  return (tb_check_encode_batch(b) != 0 || scr_check_batch(b, scr, true) != 0) ? -1 : tb_encode_sharded(b, scr, false);
}

int32_t nrLDPC_hip_ulsch_decode_scrambled(const nrLDPC_hip_tb_batch_t *b, const nrLDPC_hip_tb_scr_t *scr)
{
  return (tb_check_decode_batch(b) != 0 || scr_check_batch(b, scr, false) != 0) ? -1 : tb_decode_sharded(b, scr, false);
}

int32_t nrLDPC_hip_gold_words(uint32_t c_init, uint32_t first_word, uint32_t n_words, uint32_t *out)
{
  /* the arguments are checked once, by nr_hip_gold_words (nr_coding_host.c); here its code becomes the error text */
  switch (nr_hip_gold_words(c_init, first_word, n_words, out)) {
    case 0: return 0;
    case NR_HIP_GOLD_BAD_C_INIT: return set_error("gold_words: c_init must be below 2^31");
    case NR_HIP_GOLD_BAD_FIRST_WORD: return set_error("gold_words: first_word must be below 2^17 - 50");
    case NR_HIP_GOLD_NULL_OUT: return set_error("null argument");
    default: return set_error("gold_words: invalid arguments");
  }
}

int32_t nrLDPC_hip_codeword_scrambling(const uint8_t *in, uint32_t size, uint8_t q, uint32_t Nid, uint32_t n_RNTI, uint32_t *out,
                                       int32_t mem, void *stream)
{
  if (scr_check_call(in, size, mem, n_RNTI, q, Nid) != 0)
    return -1;
  if (size && !out)
    return set_error("null argument");
  if (size == 0)
    return 0;
  const uint32_t c_init = nr_gold_c_init(n_RNTI, q, Nid), out_bytes = 4u * ((size + 31u) >> 5);
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    DeviceCall dc;
    if (dc.open("scrambling", {{in, 1}, {out, 1}}, DEV_NEEDS_IN_OUT, stream) != 0)
      return -1;
    HIP_TRY(nr_launch_scramble_bits(in, size, c_init, out, dc.s));
    return 0;
  }
  StagedCall st;
  if (st.open() != 0)
    return -1;
  const size_t in_o = st.take(size);
  if (st.ensure(out_bytes) != 0)
    return -1;
  memcpy(st.h(in_o), in, size);
  const auto launch = [&] {
    HIP_TRY(nr_launch_scramble_bits(st.d(in_o), size, c_init, reinterpret_cast<uint32_t *>(st.d_out()), st.stream()));
    return 0;
  };
  if (st.run(size, launch, out_bytes) != 0)
    return -1;
  memcpy(out, st.h_out(), out_bytes);
  return 0;
}

int32_t nrLDPC_hip_codeword_unscrambling(int16_t *llr, uint32_t size, uint8_t q, uint32_t Nid, uint32_t n_RNTI, int32_t mem, void *stream)
{
  if (scr_check_call(llr, size, mem, n_RNTI, q, Nid) != 0)
    return -1;
  if (size == 0)
    return 0;
  const uint32_t c_init = nr_gold_c_init(n_RNTI, q, Nid);
  const size_t bytes = (size_t)size * sizeof(int16_t);
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    DeviceCall dc;
    if (dc.open("unscrambling", {{llr, 1}}, "`llr` in device memory", stream) != 0)
      return -1;
    HIP_TRY(nr_launch_unscramble_llr(llr, size, c_init, dc.s));
    return 0;
  }
  StagedCall st;
  if (st.open() != 0)
    return -1;
  const size_t llr_o = st.take(bytes);
  if (st.ensure(0) != 0)
    return -1;
  memcpy(st.h(llr_o), llr, bytes);
  const auto launch = [&] {
    HIP_TRY(nr_launch_unscramble_llr(reinterpret_cast<int16_t *>(st.d(llr_o)), size, c_init, st.stream()));
    return 0;
  };
  /* in place: the values come back from the input area */
  if (st.run(bytes, launch, bytes, true) != 0)
    return -1;
  memcpy(llr, st.h(llr_o), bytes);
  return 0;
}

} /* extern "C" */
