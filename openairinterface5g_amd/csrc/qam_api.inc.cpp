/*
 * qam_api.inc.cpp -- modulation mapping, soft demapping and the UL-SCH chain call that takes symbols (included into ldpc_api.cpp;
 * uses the batch checks of scrambling_api.inc.cpp and the call scopes of slot_call.inc.cpp).  The constellations and the
 * demapper: nr_qam.h; the standalone kernels: tb_qam.hip; the demapper inside the chain: tb_rx_core.h (the symbol source of phase A).  And the DL-SCH
 * chain call that ends in layer-mapped symbols (the fused segment kernel's symbol store: tb_tx_sym.h) with the standalone
 * layer mapping.
 */

namespace {

/* decode_symbols: what decode_scrambled checks, and a record that starts on a symbol and on a 4-byte boundary */
int sym_check_batch(const nrLDPC_hip_tb_batch_t *b, const nrLDPC_hip_tb_scr_t *scr)
{
  if (scr_check_batch(b, scr, false) != 0)
    return -1;
  if (b->n_tb && (reinterpret_cast<uintptr_t>(b->coded) & 3u))
    return set_error("decode_symbols: the symbol records must be 4-byte aligned (coded)");
  for (uint32_t i = 0; i < b->n_tb; i++) {
    if (qam_check_qm(b->tb[i].Qm) != 0)
      return -1;
    if (b->tb[i].G % b->tb[i].Qm)
      return set_error("decode_symbols: G must be a multiple of Qm");
    if (b->tb[i].coded_off & 1u)
      return set_error("decode_symbols: coded_off must be even");
  }
  return 0;
}

/* encode_symbols: what encode_scrambled checks, one codeword per block (Nl <= 4), every block valid, a 4-byte aligned array */
int sym_check_encode(const nrLDPC_hip_tb_batch_t *b, const nrLDPC_hip_tb_scr_t *scr)
{
  if (scr_check_batch(b, scr, true) != 0)
    return -1;
  if (b->n_tb && (reinterpret_cast<uintptr_t>(b->coded) & 3u))
    return set_error("encode_symbols: coded must be 4-byte aligned");
  for (uint32_t i = 0; i < b->n_tb; i++) {
    if (b->tb[i].Nl > 4)
      return set_error("encode_symbols: Nl above 4 (layers 5-8 carry two codewords)");
    if (tb_validate(b->tb[i]) != 0)
      return -1;
  }
  return 0;
}

} // namespace

extern "C" {

int32_t nrLDPC_hip_mod_table(uint8_t Qm, int16_t *out)
{
  switch (nr_hip_mod_table(Qm, out)) {
    case 0: return 0;
    case NR_HIP_QAM_BAD_QM: return set_error("mod_table: Qm must be 2, 4, 6 or 8");
    default: return set_error("null argument");
  }
}

int32_t nrLDPC_hip_modulation(const uint32_t *in, uint32_t length, uint8_t Qm, int16_t *out, int32_t mem, void *stream)
{
  if (qam_check_qm(Qm) != 0)
    return -1;
  if (length % Qm)
    return set_error("modulation: length must be a multiple of Qm");
  if (length > NR_SCR_MAX_BITS)
    return set_error("modulation: length above 2^21 bits");
  if (check_mem("modulation", mem) != 0)
    return -1;
  if (length && (!in || !out))
    return set_error("null argument");
  if (length == 0)
    return 0;
  const size_t in_bytes = 4u * (size_t)((length + 31u) >> 5), out_bytes = (size_t)(length / Qm) * 4u;
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    DeviceCall dc;
    if (dc.open("modulation", {{in, 1}, {out, 1}}, DEV_NEEDS_IN_OUT, stream) != 0)
      return -1;
    HIP_TRY(nr_launch_modulation(in, length, Qm, out, dc.s));
    return 0;
  }
  StagedCall st;
  if (st.open() != 0)
    return -1;
  const size_t in_o = st.take(in_bytes);
  if (st.ensure(out_bytes) != 0)
    return -1;
  memcpy(st.h(in_o), in, in_bytes);
  const auto launch = [&] {
    HIP_TRY(nr_launch_modulation(reinterpret_cast<const uint32_t *>(st.d(in_o)), length, Qm, reinterpret_cast<int16_t *>(st.d_out()), st.stream()));
    return 0;
  };
  if (st.run(in_bytes, launch, out_bytes) != 0)
    return -1;
  memcpy(out, st.h_out(), out_bytes);
  return 0;
}

int32_t nrLDPC_hip_ulsch_llr(const int32_t *rxdataF_comp, const int32_t *ul_ch_mag, const int32_t *ul_ch_magb, const int32_t *ul_ch_magc,
                             uint32_t nb_re, uint8_t Qm, int16_t *llr, int32_t mem, void *stream)
{
  if (qam_check_qm(Qm) != 0)
    return -1;
  if ((uint64_t)nb_re * Qm > NR_SCR_MAX_BITS)
    return set_error("ulsch_llr: nb_re * Qm above 2^21");
  if (check_mem("ulsch_llr", mem) != 0)
    return -1;
  const int32_t *in[4] = {rxdataF_comp, ul_ch_mag, ul_ch_magb, ul_ch_magc};
  const uint32_t np = Qm / 2u;
  if (nb_re) {
    if (!llr)
      return set_error("null argument");
    for (uint32_t k = 0; k < np; k++)
      if (!in[k])
        return set_error("null argument");
  }
  if (nb_re == 0)
    return 0;
  const size_t plane_bytes = (size_t)nb_re * 4u, out_bytes = (size_t)nb_re * Qm * 2u;
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    /* the planes beyond Qm / 2 are not read: NULL, as an array that was not given */
    DeviceCall dc;
    if (dc.open("ulsch_llr", {{llr, 1}, {in[0], 4}, {np > 1 ? in[1] : nullptr, 4}, {np > 2 ? in[2] : nullptr, 4}, {np > 3 ? in[3] : nullptr, 4}},
                DEV_NEEDS_ALIGNED, stream) != 0)
      return -1;
    const uint32_t *pl[4] = {nullptr, nullptr, nullptr, nullptr};
    for (uint32_t k = 0; k < np; k++)
      pl[k] = reinterpret_cast<const uint32_t *>(in[k]);
    HIP_TRY(nr_launch_ulsch_llr(pl, nb_re, Qm, llr, dc.s));
    return 0;
  }
  StagedCall st;
  if (st.open() != 0)
    return -1;
  size_t plane_o[4] = {0, 0, 0, 0};
  for (uint32_t k = 0; k < np; k++)
    plane_o[k] = st.take(plane_bytes);
  if (st.ensure(out_bytes) != 0)
    return -1;
  const uint32_t *pl[4] = {nullptr, nullptr, nullptr, nullptr};
  for (uint32_t k = 0; k < np; k++) {
    memcpy(st.h(plane_o[k]), in[k], plane_bytes);
    pl[k] = reinterpret_cast<const uint32_t *>(st.d(plane_o[k]));
  }
  const auto launch = [&] {
    HIP_TRY(nr_launch_ulsch_llr(pl, nb_re, Qm, reinterpret_cast<int16_t *>(st.d_out()), st.stream()));
    return 0;
  };
  if (st.run(st.top, launch, out_bytes) != 0)
    return -1;
  memcpy(llr, st.h_out(), out_bytes);
  return 0;
}

int32_t nrLDPC_hip_ulsch_decode_symbols(const nrLDPC_hip_tb_batch_t *b, const nrLDPC_hip_tb_scr_t *scr)
{
  return (tb_check_decode_batch(b) != 0 || sym_check_batch(b, scr) != 0) ? -1 : tb_decode_sharded(b, scr, true);
}

int32_t nrLDPC_hip_dlsch_encode_symbols(const nrLDPC_hip_tb_batch_t *b, const nrLDPC_hip_tb_scr_t *scr)
{
  return (tb_check_encode_batch(b) != 0 || sym_check_encode(b, scr) != 0) ? -1 : tb_encode_sharded(b, scr, true);
}

int32_t nrLDPC_hip_layer_mapping(const int16_t *in, uint32_t n_symbs, uint8_t Nl, int16_t *out, uint32_t layer_stride, int32_t mem, void *stream)
{
  if (Nl < 1 || Nl > 4)
    return set_error("layer_mapping: Nl must be 1..4 (one codeword)");
  if (n_symbs % Nl)
    return set_error("layer_mapping: n_symbs must be a multiple of Nl");
  if (n_symbs > NR_SCR_MAX_BITS)
    return set_error("layer_mapping: n_symbs above 2^21");
  const uint32_t per_layer = n_symbs / Nl;
  if (layer_stride < per_layer)
    return set_error("layer_mapping: layer_stride below n_symbs / Nl");
  if (check_mem("layer_mapping", mem) != 0)
    return -1;
  if (n_symbs && (!in || !out))
    return set_error("null argument");
  if (n_symbs == 0)
    return 0;
  const size_t in_bytes = (size_t)n_symbs * 4u, plane_bytes = (size_t)per_layer * 4u;
  const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), o0 = reinterpret_cast<uintptr_t>(out);
  if (i0 < o0 + ((size_t)(Nl - 1) * layer_stride * 4u + plane_bytes) && o0 < i0 + in_bytes)
    return set_error("layer_mapping: in and out overlap");
  if (mem == NRLDPC_HIP_MEM_DEVICE) {
    DeviceCall dc;
    if (dc.open("layer_mapping", {{in, 1}, {out, 1}}, DEV_NEEDS_IN_OUT, stream) != 0)
      return -1;
    HIP_TRY(nr_launch_layer_mapping(in, n_symbs, Nl, out, layer_stride, dc.s));
    return 0;
  }
  StagedCall st;
  if (st.open() != 0)
    return -1;
  const size_t in_o = st.take(in_bytes);
  if (st.ensure(in_bytes) != 0)
    return -1;
  memcpy(st.h(in_o), in, in_bytes);
  /* the planes side by side on the device; on the host each goes to its place (nothing between them is written) */
  const auto launch = [&] {
    HIP_TRY(nr_launch_layer_mapping(reinterpret_cast<const int16_t *>(st.d(in_o)), n_symbs, Nl, reinterpret_cast<int16_t *>(st.d_out()), per_layer,
                                    st.stream()));
    return 0;
  };
  if (st.run(in_bytes, launch, in_bytes) != 0)
    return -1;
  for (uint32_t l = 0; l < Nl; l++)
    memcpy(reinterpret_cast<uint8_t *>(out) + (size_t)l * layer_stride * 4u, st.h_out() + l * plane_bytes, plane_bytes);
  return 0;
}

} /* extern "C" */
