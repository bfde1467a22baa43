/*
 * slot_delay_emul.cpp -- the PUSCH delay search on the CPU (test infrastructure): tb_rx_delay.hip is #included as it is and read
 * against the host shim (hip_host/), so the LDS transform with its barriers, the wave shuffles, the reduction through the buffer's
 * first entries and the combining launch run as the GPU compiles them, one real thread per work-item (run_grid_threads).  The plan,
 * the twiddle table and the launch loop are the library's own (rx_delay_plan.h), the launchers the .hip file's.  The entry point is
 * the DEVICE mem branch of nrLDPC_hip_pusch_est_delay: checks, plan, tables, launches, on the caller's arrays exactly as given.
 *
 * Two builds (tests/test_rx_delay_host.py): a shared library that Python loads, without sanitizers; and, with
 * -DDELAY_EMUL_MAIN -fsanitize=address,undefined, a stand-alone program that runs the entry point on heap arrays of exactly the
 * extents include/nrLDPC_hip.h documents and checks delays and peaks bit for bit against nr_delay.h run serially.
 */
#include "slot_emul_common.h"
#include <map>
#define NR_DLY_DYNAMIC_LDS(type, name) HIP_HOST_DYNAMIC_LDS(type, name)
#include "rx_plan.h"
#include "rx_delay_plan.h"
#include "tb_rx_delay.hip"

extern "C" {

const char *slot_delay_emul_last_error() { return slot_emul_error.c_str(); }

/* nr_dly_fold alone: no symbol has its largest sample at N/2 or N/2 + 1 (the LS values repeat over four or six REs), so the fold
 * is also looked at directly */
int32_t slot_emul_delay_fold(uint32_t N, uint32_t pos) { return nr_dly_fold(N, pos); }

/* peak may be null, as in the library */
int32_t slot_emul_pusch_est_delay(const int16_t *rxdataF, uint64_t rx_ant_stride, uint32_t n_rx, const nrLDPC_hip_chest_seg_t *seg, uint32_t n_seg,
                                  uint32_t flags, int32_t *est_delay, float *peak)
{
  if (rxf_check_common("est_delay", n_rx, NRLDPC_HIP_MEM_DEVICE) != 0)
    return -1;
  if (n_seg && (!rxdataF || !seg || !est_delay))
    return set_error("null argument");
  if (!aligned4({rxdataF, est_delay, peak}))
    return set_error("est_delay: every array 4-byte aligned");
  DelayPlan p;
  if (dly_check_flags(flags) != 0 || dly_plan(seg, n_seg, n_rx, rx_ant_stride, p) != 0)
    return -1;
  if (n_seg == 0)
    return 0;
  /* the twiddle tables, each in an allocation of exactly 2 fft_size + NR_DLY_ONE_WORDS words as the library's device copies are */
  std::map<uint32_t, std::unique_ptr<uint32_t[]>> tabs;
  for (uint32_t i = 0; i < n_seg; i++) {
    if (nr_che_is_avg(seg[i].mode))
      continue;
    std::unique_ptr<uint32_t[]> &d = tabs[seg[i].fft_size];
    if (!d) {
      std::vector<uint32_t> t;
      dly_fill_twiddles(seg[i].fft_size, t);
      d.reset(new uint32_t[t.size()]);
      memcpy(d.get(), t.data(), t.size() * 4u);
    }
    p.jobs[i].tw = reinterpret_cast<const nr_dly_c *>(d.get());
  }
  const DelayLayout dl(p);
  const auto base = tables_copy(dl.lay, dl.lay.upload_bytes());
  WithThreads t;
  return dly_launch(p, dl, base.get(), c16(rxdataF), rx_ant_stride, n_rx, flags, est_delay, peak, nullptr);
}

} /* extern "C" */

#ifdef DELAY_EMUL_MAIN
#include <stdio.h>
#include <random>

namespace {

uint32_t calls = 0, bad = 0;

/* descriptors of one call, each on a symbol of its own, results at delay_off = 3 + i (n_rx + 1): exactly the documented extents */
void run(std::mt19937 &rng, const std::vector<uint32_t> &sizes, uint32_t n_rx, uint32_t flags, bool with_peak, bool zero_symbol)
{
  const uint32_t n_seg = (uint32_t)sizes.size();
  std::vector<nrLDPC_hip_chest_seg_t> seg(n_seg);
  uint64_t sym_off = 0;
  for (uint32_t i = 0; i < n_seg; i++) {
    nrLDPC_hip_chest_seg_t &g = seg[i];
    memset(&g, 0, sizeof g);
    const uint32_t N = sizes[i];
    g.mode = (uint8_t)(i % 5u == 4u ? NR_CHE_TYPE1_AVG : (i & 1u));
    g.port = (uint8_t)((i & 2u) ? 2u : (i & 1u));
    g.fft_size = N;
    g.rb_size = i % 3u == 0u ? N / 12u : (i % 3u == 1u ? 1u + i : N / 30u + 1u);
    g.start_re = (N - 12u * g.rb_size / 2u) % N & ~1u; /* across the wrap, even: nushift never reaches N */
    if (nr_che_reaches_n(g.mode, g.port, N, g.start_re, g.rb_size))
      g.port = 0;
    g.dmrs_offset = 6u * (3u + i);
    g.c_init = (0x2345678u + 991u * i) & 0x7fffffffu;
    g.delay_off = 3u + i * (n_rx + 1u);
    g.rx_off = sym_off;
    sym_off += N;
  }
  const uint64_t rx_stride = sym_off + 3u;
  const size_t rx_n = (size_t)(n_rx - 1) * rx_stride + sym_off, d_n = 3u + (size_t)(n_seg - 1) * (n_rx + 1u) + n_rx;
  std::unique_ptr<int16_t[]> rx(new int16_t[2 * rx_n]);
  std::unique_ptr<int32_t[]> dl(new int32_t[d_n]), want(new int32_t[d_n]);
  std::unique_ptr<float[]> pk(new float[d_n]), wpk(new float[d_n]);
  for (size_t i = 0; i < 2 * rx_n; i++)
    rx[i] = (int16_t)((int)(rng() % 6001u) - 3000);
  if (zero_symbol)
    for (uint32_t a = 0; a < n_rx; a++)
      memset(rx.get() + 2 * (seg[0].rx_off + a * rx_stride), 0, (size_t)seg[0].fft_size * 4u);
  for (size_t i = 0; i < d_n; i++) {
    dl[i] = want[i] = 0x5a5a5a5a;
    pk[i] = wpk[i] = -7.0f;
  }
  const int32_t rc = slot_emul_pusch_est_delay(rx.get(), rx_stride, n_rx, seg.data(), n_seg, flags, dl.get(), with_peak ? pk.get() : nullptr);
  bool ok = rc == 0;
  for (uint32_t i = 0; ok && i < n_seg; i++) {
    std::vector<uint32_t> tw;
    dly_fill_twiddles(seg[i].fft_size, tw);
    ok = dly_host_seg(seg[i], c16(rx.get()), rx_stride, n_rx, flags, tw.data(), want.get(), with_peak ? wpk.get() : nullptr) == 0;
  }
  ok = ok && memcmp(dl.get(), want.get(), d_n * 4u) == 0 && memcmp(pk.get(), wpk.get(), d_n * 4u) == 0; /* and nothing but the write set */
  if (zero_symbol)
    for (uint32_t a = 0; a < n_rx; a++)
      ok = ok && dl[seg[0].delay_off + a] == 0 && (!with_peak || pk[seg[0].delay_off + a] == 0.0f);
  calls++;
  if (!ok) {
    bad++;
    printf("MISMATCH est_delay (%u descriptors, n_rx %u, flags %u): %s\n", n_seg, n_rx, flags, slot_emul_error.c_str());
  }
}

} // namespace

int main()
{
  std::mt19937 rng(20252);
  for (uint32_t flags = 0; flags < 2u; flags++) {
    run(rng, {128, 256, 512, 1024, 1536}, 3, flags, true, false);
    run(rng, {128, 128, 256}, 1, flags, false, true);
    run(rng, {1536, 128}, 8, flags, true, true);
  }
  run(rng, {2048, 4096, 6144, 8192}, 1, 0, true, false);
  run(rng, {8192, 1536}, 2, 1, true, false);
  printf("%u %u\n", calls, bad);
  return bad != 0;
}
#endif
