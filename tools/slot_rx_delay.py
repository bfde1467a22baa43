#!/usr/bin/env python3
"""What the PUSCH delay search costs on the GPU: nrLDPC_hip_pusch_est_delay alone, and the pair est_delay + estimation, next to
nrLDPC_hip_pusch_channel_estimation's own time from the same run.  One block with one TYPE1_INTERP DMRS symbol, port 0, at 106 PRBs
(N = 2048) and 273 PRBs (N = 4096), with 1 and 4 antennas; the grid carries a two-tap channel so that the search has a peak.

  python tools/slot_rx_delay.py [reps]      -> one JSON line; times in microseconds (median, min, max, p10, p90 over reps)

The calls refuse a capturing stream, so nothing is replayed from a graph: every timed leg is enqueued behind a filler (a matrix
product) that keeps the GPU busy while the host enqueues, and the events around it see GPU time -- the descriptor upload and the
kernels -- not the host's enqueueing.  The legs alternate inside one loop so that they see the same machine:

  est_delay                  the search alone (PER_ANTENNA): one search launch and the combining launch
  estimation                 nrLDPC_hip_pusch_channel_estimation reading the delays the search left on the device
  est_delay_estimation       the two calls back to back

Before timing, the delays and peaks are compared with the host form's, bit for bit.  These are first timings of a new call: there
is no earlier build to compare with, and no threshold is attached to them.
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import openairinterface5g_amd as pkg  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
m = pkg.ldpc
pkg.LDPCinit()
LC, LD = m._chest_lib(), m._delay_lib()
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    fill_a = torch.randn(6144, 6144, dtype=torch.float16, device="cuda")
    fill_c = torch.empty_like(fill_a)
torch.cuda.synchronize()
s_ptr = side.cuda_stream
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
res = {"reps": reps, "configs": {}}
for rb, N in ((106, 2048), (273, 4096)):
    for n_rx in (1, 4):
        rng = np.random.default_rng(rb + n_rx)
        stride = 14 * N
        alloc = dict(tb=0, Qm=6, dmrs_config_type=0, num_dmrs_cdm_grps_no_data=1, dmrs_symbol=2, fft_size=N, first_carrier_offset=N - 6 * rb, bwp_start=0,
                     rb_start=0, rb_size=rb, start_symbol=0, nr_of_symbols=14, ul_dmrs_symb_pos=1 << 2, plane=14 * 12 * rb, rx_slot_off=0, ch_off=0, rec_off=0)
        cseg = m.pusch_chest_segments([alloc], [dict(slot=3, scid=0, dmrs_scrambling_id=77, port=0, chest_freq=0)], n_rx)
        c = cseg[0]
        # the DMRS symbol on the air: tap tau[a] and a weak second tap, noise; everything else on the grid is noise
        tau = [5, -3, 7, -6][:n_rx]
        rx_h = rng.integers(-60, 61, (n_rx, stride, 2)).astype(np.int16)
        p = m.pusch_dmrs_host(c["c_init"], c["dmrs_offset"], 6 * rb, 0, 0).astype(np.float64)
        re = 2 * np.arange(6 * rb)
        for a in range(n_rx):
            h = 2000.0 * (1.2 ** a) * (np.exp(-2j * np.pi * re * tau[a] / N) + 0.05 * np.exp(-2j * np.pi * re * 11 / N))
            v = h * (p[:, 0] - 1j * p[:, 1]) / (23170.0 * np.sqrt(2.0))
            rx_h[a, c["rx_off"] + (c["start_re"] + re) % N] += np.rint(np.stack([v.real, v.imag], -1)).astype(np.int16)
        with torch.cuda.stream(side):
            rx = torch.from_numpy(rx_h.reshape(-1).copy()).cuda()
            ch = torch.zeros(n_rx * stride * 2, dtype=torch.int16, device="cuda")
            dl = torch.zeros(n_rx, dtype=torch.int32, device="cuda")
            pk = torch.zeros(n_rx, dtype=torch.float32, device="cuda")
        seg_arr = m._chest_seg_array(cseg)

        def est_delay():
            assert LD.nrLDPC_hip_pusch_est_delay(rx.data_ptr(), stride, n_rx, seg_arr, 1, m.DELAY_PER_ANTENNA, dl.data_ptr(), pk.data_ptr(), m.MEM_DEVICE,
                                                 s_ptr) == 0, m.last_error()

        def estimation():
            assert LC.nrLDPC_hip_pusch_channel_estimation(rx.data_ptr(), stride, ch.data_ptr(), stride, n_rx, seg_arr, 1, dl.data_ptr(), m.MEM_DEVICE,
                                                          s_ptr) == 0, m.last_error()

        def both():
            est_delay()
            estimation()
        legs = {"est_delay": est_delay, "estimation": estimation, "est_delay_estimation": both}
        for fn in legs.values():
            with torch.cuda.stream(side):
                for _ in range(3):
                    fn()
        torch.cuda.synchronize()
        want_d, want_p = m.pusch_est_delay_host(rx_h.reshape(-1, 2), stride, n_rx, c, m.DELAY_PER_ANTENNA)
        out = {"delays": dl.cpu().numpy().tolist(), "tau": tau,
               "equals_host_form": bool(np.array_equal(dl.cpu().numpy(), want_d) and np.array_equal(pk.cpu().numpy().view(np.uint32), want_p.view(np.uint32)))}
        ts = {k: [] for k in legs}
        for _ in range(reps):
            for k, fn in legs.items():
                with torch.cuda.stream(side):
                    torch.mm(fill_a, fill_a, out=fill_c)
                    e0.record()
                    fn()
                    e1.record()
                torch.cuda.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3)
        for k, v in ts.items():
            out[k + "_us"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "p10": float(np.percentile(v, 10)),
                              "p90": float(np.percentile(v, 90))}
        res["configs"][f"rb{rb}_N{N}_nrx{n_rx}"] = out
print(json.dumps(res))
