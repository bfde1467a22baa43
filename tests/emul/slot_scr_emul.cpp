/*
 * slot_scr_emul.cpp -- the standalone scrambling kernels and the transport-block packer on the CPU (test infrastructure):
 * tb_scrambling.hip and tb_scr_pack.hip are #included as they are and read against the host shim (hip_host/); see
 * slot_rx_emul.cpp for the idea.  Every kernel here fills the workgroup's Gold words behind a wave-wide jump (a ballot per set bit
 * of the word index, nr_gold_dev.h) and one barrier, so the workgroups run on real threads.  No plan: the launchers take the
 * caller's arrays and c_init.
 */
#include "slot_emul_common.h"
#include "tb_scrambling.hip"
#include "tb_scr_pack.hip"

extern "C" {

/* in: size bytes (one bit each); out: ceil(size / 32) words */
int32_t slot_emul_scramble_bits(const uint8_t *in, uint32_t size, uint32_t c_init, uint32_t *out)
{
  WithThreads t;
  return launched(nr_launch_scramble_bits(in, size, c_init, out, nullptr));
}

/* llr: size int16, in place */
int32_t slot_emul_unscramble_llr(int16_t *llr, uint32_t size, uint32_t c_init)
{
  WithThreads t;
  return launched(nr_launch_unscramble_llr(llr, size, c_init, nullptr));
}

/* the packed, scrambled store of an encode call over n_tb job records (tb_chain.h); max_g = the largest G */
int32_t slot_emul_scramble_bits_tb(const tb_scr_tb_job *jobs, uint32_t n_tb, uint32_t max_g, const uint8_t *in, uint8_t *out)
{
  WithThreads t;
  return launched(nr_launch_scramble_bits_tb(jobs, n_tb, max_g, in, out, nullptr));
}

} /* extern "C" */
