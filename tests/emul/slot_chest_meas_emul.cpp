/*
 * slot_chest_meas_emul.cpp -- the measuring PUSCH channel estimation and the time average of its estimates on the CPU (test
 * infrastructure): tb_rx_chest_meas.hip is #included as it is and read against the host shim (hip_host/), so the wave shuffles, the
 * LDS reduction, the atomics, the finishing launch and every work-item's 16-byte-or-words decision run as the GPU compiles them.
 * The plans and the table layout are the library's own (rx_chest_plan.h, rx_chest_meas_plan.h), the launchers the .hip file's.  An
 * entry point is the DEVICE mem branch of the library call of the same name: checks, plan, tables, launches, in place on the
 * caller's arrays, which are used exactly as given.
 *
 * Two builds (tests/test_rx_chest_meas_host.py): a shared library that Python loads, without sanitizers; and, with
 * -DCHEST_MEAS_EMUL_MAIN -fsanitize=address,undefined, a stand-alone program that runs the entry points on heap arrays of exactly
 * the extents include/nrLDPC_hip.h documents and checks them against nr_chest.h run serially.
 */
#include "slot_emul_common.h"
#include <map>
#include "rx_plan.h"
#include "rx_chest_plan.h"
#include "rx_chest_meas_plan.h"
#include "tb_rx_chest_meas.hip"

extern "C" {

const char *slot_chest_meas_emul_last_error() { return slot_emul_error.c_str(); }

/* est_delay may be null, as in the library */
int32_t slot_emul_pusch_channel_estimation_meas(const int16_t *rxdataF, uint64_t rx_ant_stride, int16_t *ul_ch, uint64_t ch_ant_stride, uint32_t n_rx,
                                                const nrLDPC_hip_chest_seg_t *seg, uint32_t n_seg, const int32_t *est_delay, const uint32_t *seg_tb,
                                                const uint32_t *nvar_div, uint32_t n_tb, int32_t *max_ch, uint32_t *nvar)
{
  if (rxf_check_common("channel_estimation_meas", n_rx, NRLDPC_HIP_MEM_DEVICE) != 0)
    return -1;
  if ((n_seg && (!rxdataF || !ul_ch || !seg || !seg_tb)) || (n_tb && (!nvar_div || !max_ch || !nvar)))
    return set_error("null argument");
  if (!aligned4({rxdataF, ul_ch, est_delay, max_ch, nvar}))
    return set_error("channel_estimation_meas: every array 4-byte aligned");
  ChestPlan p;
  ChestMeasPlan m;
  if (che_plan(seg, n_seg, n_rx, rx_ant_stride, ch_ant_stride, p) != 0 || che_meas_plan(seg, n_seg, n_rx, seg_tb, nvar_div, n_tb, m) != 0)
    return -1;
  if (n_seg == 0 && n_tb == 0)
    return 0;
  /* the delay tables, each in an allocation of exactly NR_CHE_DELAY_ROWS fft_size words as the library's device copies are */
  std::map<uint32_t, std::unique_ptr<uint32_t[]>> tabs;
  for (uint32_t i = 0; i < n_seg; i++) {
    std::unique_ptr<uint32_t[]> &d = tabs[seg[i].fft_size];
    if (!d) {
      std::vector<uint32_t> t;
      che_fill_table(seg[i].fft_size, t);
      d.reset(new uint32_t[t.size()]);
      memcpy(d.get(), t.data(), t.size() * 4u);
    }
    p.jobs[i].tab = d.get();
  }
  const CheLayout cl(p, &m);
  const auto base = tables_copy(cl.lay, cl.lay.upload_bytes());
  const CheMeasDev md = cl.meas(base.get(), max_ch, nvar);
  /* the library's loop (che_launch of rx_chest_api.inc.cpp): one launch a mode over its part of the workgroup table, then the finish */
  WithThreads t;
  const rx_chest_wg *wgs = cl.at<rx_chest_wg>(base.get(), cl.wg);
  for (uint32_t mode = 0; mode < NR_CHE_MODES; wgs += p.n_wg[mode++])
    if (launched(nr_launch_rx_chest_meas(mode, wgs, p.n_wg[mode], cl.at<rx_chest_job>(base.get(), cl.job), md.mjobs, c16(rxdataF), rx_ant_stride, c16(ul_ch),
                                         ch_ant_stride, est_delay, md.mx, md.noise, nullptr)) != 0)
      return -1;
  return launched(nr_launch_rx_chest_finish(md.tbs, n_tb, md.list, md.mjobs, md.mx, md.noise, md.max_ch, md.nvar, nullptr));
}

int32_t slot_emul_pusch_chest_time_avg(int16_t *ul_ch, uint64_t ch_ant_stride, uint32_t n_plane, const nrLDPC_hip_chest_avg_seg_t *seg, uint32_t n_seg)
{
  if (n_seg && (!ul_ch || !seg))
    return set_error("null argument");
  if (!aligned4({ul_ch}))
    return set_error("chest_time_avg: every array 4-byte aligned");
  ChestAvgPlan p;
  if (che_avg_plan(seg, n_seg, n_plane, ch_ant_stride, p) != 0)
    return -1;
  if (p.wgs.empty())
    return 0;
  const auto tab = table2(p.wgs, p.jobs);
  const auto base = tables_copy(tab);
  return launched(nr_launch_rx_chest_time_avg(tab.first(base.get()), (uint32_t)p.wgs.size(), tab.second(base.get()), c16(ul_ch), ch_ant_stride, nullptr));
}

} /* extern "C" */

#ifdef CHEST_MEAS_EMUL_MAIN
#include <stdio.h>
#include <random>

namespace {

uint32_t calls = 0, bad = 0;

/* one descriptor's antenna from nr_chest.h, unit after unit, with a Gold sequence made word by word: out = 12 rb_size c16 */
void serial_one(const nrLDPC_hip_chest_seg_t &g, const uint32_t *rx, int32_t d, uint32_t *out, int32_t &mx, uint64_t &noise)
{
  std::vector<uint32_t> gold, tab;
  uint32_t w0;
  dmrs_gold_words(g.c_init, g.dmrs_offset, nr_che_pilots_per_rb(g.mode) * g.rb_size, gold, w0);
  che_fill_table(g.fft_size, tab);
  const uint32_t *fwd = tab.data() + (size_t)nr_che_delay_idx(d) * g.fft_size, *inv = tab.data() + (size_t)nr_che_inv_delay_idx(d) * g.fft_size;
  for (uint32_t u = 0; u < nr_che_units(g.mode, g.rb_size); u++) {
    const uint64_t bits = dmrs_bits(gold, w0, g.dmrs_offset + nr_che_unit_first_pilot(g.mode, u));
    if (g.mode == NR_CHE_TYPE1_INTERP) {
      nr_che_t1_interp(rx, g.fft_size, g.start_re, g.rb_size, g.port, g.dmrs_offset, bits, fwd, inv, u, out + 4u * u);
      noise += nr_che_t1_meas(rx, g.fft_size, g.start_re, g.port, g.dmrs_offset, bits, u, out + 4u * u, &mx);
    } else if (g.mode == NR_CHE_TYPE2_INTERP) {
      nr_che_t2_interp(rx, g.fft_size, g.start_re, g.port, g.dmrs_offset, bits, inv, u, out + 4u * u);
      noise += nr_che_t2_meas(rx, g.fft_size, g.start_re, g.port, g.dmrs_offset, bits, u, &mx);
    } else {
      const uint32_t v = nr_che_avg(g.mode, rx, g.fft_size, g.start_re, g.port, g.dmrs_offset, bits, u);
      mx = nr_che_avg_meas(g.rb_size, u, v, mx);
      for (uint32_t k = 0; k < 12u; k++)
        out[12u * u + k] = v;
    }
  }
}

void expect(bool ok, const char *what, uint32_t a, uint32_t b)
{
  calls++;
  if (!ok) {
    bad++;
    printf("MISMATCH %s (case %u, %u): %s\n", what, a, b, slot_emul_error.c_str());
  }
}

/* n_sym DMRS symbols x n_layer ports of one block a descriptor set; three blocks, the middle one without a descriptor */
void run_meas(std::mt19937 &rng, uint32_t mode, uint32_t rb, uint32_t n_rx, uint32_t N, uint32_t k0, bool hot, bool delays, uint32_t shift)
{
  const uint32_t n_tb = 3, n_sym = 2, n_layer = 2, n_seg = 2u * n_sym * n_layer;
  const uint64_t rx_stride = (uint64_t)n_sym * N + 5u, ch_stride = (uint64_t)n_seg * 12u * rb + 3u;
  std::vector<nrLDPC_hip_chest_seg_t> seg(n_seg);
  std::vector<uint32_t> seg_tb(n_seg);
  for (uint32_t i = 0; i < n_seg; i++) {
    nrLDPC_hip_chest_seg_t &g = seg[i];
    memset(&g, 0, sizeof g);
    g.mode = (uint8_t)mode;
    g.port = (uint8_t)((i & 1u) ? 2u : 0u); /* the second layer's port has nushift / delta 1 */
    g.fft_size = N;
    g.start_re = k0;
    g.rb_size = rb;
    g.dmrs_offset = 18;
    g.c_init = (0x1234567u + 77u * i) & 0x7fffffffu;
    g.delay_off = i * n_rx;
    g.rx_off = (uint64_t)((i >> 1) % n_sym) * N;
    g.ch_off = shift + (uint64_t)i * 12u * rb;
    seg_tb[i] = (i & 2u) ? 2u : 0u; /* interleaved */
  }
  if (nr_che_reaches_n(mode, 2, N, k0, rb))
    return;
  /* exactly the documented extents */
  const size_t rx_n = (size_t)(n_rx - 1) * rx_stride + (size_t)n_sym * N, ch_n = shift + (size_t)(n_rx - 1) * ch_stride + (size_t)n_seg * 12u * rb;
  std::unique_ptr<int16_t[]> rx(new int16_t[2 * rx_n]), ch(new int16_t[2 * ch_n]), ref(new int16_t[2 * ch_n]);
  std::unique_ptr<int32_t[]> dl(new int32_t[(size_t)n_seg * n_rx]), mx(new int32_t[n_tb]);
  std::unique_ptr<uint32_t[]> nv(new uint32_t[n_tb]);
  for (size_t i = 0; i < 2 * rx_n; i++)
    rx[i] = hot ? ((rng() & 1u) ? 32767 : -32767) : (int16_t)((int)(rng() % 4001u) - 2000);
  for (size_t i = 0; i < 2 * ch_n; i++)
    ch[i] = ref[i] = (int16_t)0x5a5a;
  for (size_t i = 0; i < (size_t)n_seg * n_rx; i++)
    dl[i] = delays ? (int32_t)(rng() % 9u) - 4 : 0;
  const uint32_t div[3] = {14u * n_layer * n_rx, 7u, 3u * n_layer * n_rx};
  for (int rep = 0; rep < 2; rep++) { /* twice on one set of arrays: the accumulators are the call's own */
    mx[0] = mx[1] = mx[2] = -1;
    nv[0] = nv[1] = nv[2] = 0xffffffffu;
    const int32_t rc = slot_emul_pusch_channel_estimation_meas(rx.get(), rx_stride, ch.get(), ch_stride, n_rx, seg.data(), n_seg, delays ? dl.get() : nullptr,
                                                               seg_tb.data(), div, n_tb, mx.get(), nv.get());
    int32_t emx[3] = {0, 0, 0};
    uint32_t env[3] = {0, 0, 0};
    for (uint32_t i = 0; i < n_seg; i++) {
      int32_t m = 0;
      uint64_t noise = 0;
      for (uint32_t a = 0; a < n_rx; a++)
        serial_one(seg[i], c16(rx.get()) + seg[i].rx_off + a * rx_stride, delays ? dl[seg[i].delay_off + a] : 0,
                   c16(ref.get()) + seg[i].ch_off + a * ch_stride, m, noise);
      emx[seg_tb[i]] = std::max(emx[seg_tb[i]], m);
      env[seg_tb[i]] += nr_che_nvar_tmp(noise, nr_che_nest_per_antenna(mode, rb) * n_rx);
    }
    bool ok = rc == 0 && memcmp(ch.get(), ref.get(), 4 * ch_n) == 0;
    for (uint32_t t = 0; t < n_tb; t++)
      ok = ok && mx[t] == emx[t] && nv[t] == env[t] / div[t];
    expect(ok, "channel_estimation_meas", mode, rb);
  }
}

void run_avg(std::mt19937 &rng, uint32_t n_sym, uint32_t rb, uint32_t shift, uint32_t n_plane)
{
  const uint32_t N = 12u * rb + 7u; /* symbols 12 rb + 7 apart: every symbol has another alignment */
  const uint64_t stride = (uint64_t)4u * N + 1u;
  nrLDPC_hip_chest_avg_seg_t g;
  memset(&g, 0, sizeof g);
  g.n_sym = n_sym;
  g.rb_size = rb;
  for (uint32_t s = 0; s < n_sym; s++)
    g.ch_off[s] = shift + (uint64_t)s * N;
  const size_t n = shift + (size_t)(n_plane - 1) * stride + (size_t)(n_sym - 1) * N + 12u * rb;
  std::unique_ptr<int16_t[]> ch(new int16_t[2 * n]), ref(new int16_t[2 * n]);
  for (size_t i = 0; i < 2 * n; i++) {
    const uint32_t r = rng() % 8u;
    ch[i] = ref[i] = r == 0 ? 32767 : (r == 1 ? -32768 : (r == 2 ? 20000 : (r == 3 ? -20000 : (int16_t)(rng() & 0xffffu))));
  }
  for (uint32_t q = 0; n_sym > 1 && q < n_plane; q++)
    for (uint32_t k = 0; k < 12u * rb; k++) {
      uint32_t w[NR_CHE_AVG_MAX_SYM];
      for (uint32_t s = 0; s < n_sym; s++)
        w[s] = c16(ref.get())[g.ch_off[s] + q * stride + k];
      c16(ref.get())[g.ch_off[0] + q * stride + k] = nr_che_tavg(w, n_sym);
    }
  const int32_t rc = slot_emul_pusch_chest_time_avg(ch.get(), stride, n_plane, &g, 1);
  expect(rc == 0 && memcmp(ch.get(), ref.get(), 4 * n) == 0, "chest_time_avg", n_sym, rb);
}

} // namespace

int main()
{
  std::mt19937 rng(20251);
  for (uint32_t mode = 0; mode < NR_CHE_MODES; mode++) {
    for (uint32_t rb : {1u, 2u, 3u, 22u})
      for (uint32_t n_rx : {1u, 3u})
        run_meas(rng, mode, rb, n_rx, 512, (rb * 5u + mode) % 512u, rb == 3, n_rx == 3, rb & 3u);
    run_meas(rng, mode, 20, 2, 256, 100, true, true, 1); /* across the grid's wrap, full scale */
  }
  run_meas(rng, NR_CHE_TYPE1_INTERP, 86, 2, 1536, 1000, true, false, 2); /* two workgroups feed one descriptor's sum */
  run_meas(rng, NR_CHE_TYPE2_AVG, 257, 1, 4096, 3000, false, false, 3); /* the second piece of an averaging mode */
  for (uint32_t n_sym = 1; n_sym <= 4; n_sym++)
    for (uint32_t rb : {1u, 5u, 22u})
      for (uint32_t shift = 0; shift < 4; shift++)
        run_avg(rng, n_sym, rb, shift, 2u + 2u * (shift & 1u));
  printf("%u %u\n", calls, bad);
  return bad != 0;
}
#endif
