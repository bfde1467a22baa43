#!/usr/bin/env python3
"""One slot's 64 transport blocks (the slot of tools/slot_rx_front.py's grid leg: 273 PRB x 13 symbols, 64QAM, n_rx = 4, N = 4096,
one type-1 DMRS symbol per block) from the OFDM grid in device memory: nrLDPC_hip_pusch_channel_estimation, then
channel_level_grid, channel_compensation_grid and ulsch_decode_symbols, in one process, timed with HIP events.

  python tools/slot_rx_chest.py [reps]      -> one JSON line; times in milliseconds (mean, median, min, max over reps)

The calls refuse a capturing stream, so nothing is replayed from a graph: every timed call is enqueued behind a filler (four
decode calls) that keeps the GPU busy while the host enqueues, and the events around it see GPU time -- the descriptor upload
and the kernel -- not the host's enqueueing.  The legs alternate inside one loop so that they see the same machine:

  estimation                 the estimation launch alone (TYPE1_INTERP, or TYPE1_AVG with "avg" as the second argument)
  device_copy                a plain device copy that reads and writes as many bytes as the launch: per (block, antenna) the
                             12 rb_size c16 of the DMRS symbol that hold the pilots (the other half of each sector comes along) and
                             the 12 rb_size c16 of estimates, so 4 bytes in and 4 bytes out per RE and antenna
  front                      channel_level_grid + channel_compensation_grid
  estimation_front           the three calls
  decode_symbols             the slot's decode, the figure everything else is small or large against

Before timing, the chain runs once and the payloads and ACKs are checked, and the device's estimates of one block are compared
with the host form's.

  python tools/slot_rx_chest.py [reps] meas -> one JSON line: what max_ch / nvar and the time average cost

One rank-2 block over the carrier (273 PRB, N = 4096, n_rx = 4, ports 0 and 1), one and two DMRS symbols, each estimator mode:
per configuration the legs, alternating inside one loop, each one call behind a filler (a matrix product) and between two events,

  estimation                 nrLDPC_hip_pusch_channel_estimation on the 2 x DMRS-symbols descriptors
  estimation_meas            nrLDPC_hip_pusch_channel_estimation_meas on the same descriptors (its estimates and results are
                             checked against the first call's and the host form's before timing)
  level                      nrLDPC_hip_ulsch_channel_level_grid_mmse on the block: what one more small launch with a table
                             upload costs, the yardstick for the difference of the first two
  time_avg                   nrLDPC_hip_pusch_chest_time_avg over the 2 n_rx planes (two DMRS symbols only)

A library without the two new calls (NRLDPC_HIP_LIB naming an older build) is timed on the legs it has.
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import openairinterface5g_amd as pkg  # noqa: E402

HBM_PEAK = 8.0e12                            # bytes/s, the figure bench.py uses
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
chest_freq = 1 if len(sys.argv) > 2 and sys.argv[2] == "avg" else 0
m = pkg.ldpc
pkg.LDPCinit()
LG, LC = m._rxg_lib(), m._chest_lib()


def measure_meas():
    """the `meas` mode (module docstring)"""
    n_rx, rb, N = 4, 273, 4096
    L = pkg.load_library()
    has_meas = hasattr(L, "nrLDPC_hip_pusch_channel_estimation_meas")
    LM, LX = (m._chest_meas_lib() if has_meas else None), m._rxm_lib()
    rng = np.random.default_rng(3)
    stride = 14 * N
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rx = torch.from_numpy(rng.integers(-2000, 2001, (n_rx * stride * 2,)).astype(np.int16)).cuda()
        ch = torch.zeros(2 * n_rx * stride * 2, dtype=torch.int16, device="cuda")
        ch2 = torch.zeros_like(ch)
        mx, nv, lv = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(3))
        fill_a = torch.randn(6144, 6144, dtype=torch.float16, device="cuda")
        fill_c = torch.empty_like(fill_a)
    torch.cuda.synchronize()
    s_ptr = side.cuda_stream
    res = {"reps": reps, "n_rx": n_rx, "rb": rb, "fft_size": N, "layers": 2, "library_has_meas": has_meas, "configs": {}}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for mode in range(4):
        for n_dmrs in (1, 2):
            pos = (1 << 2) | ((1 << 11) if n_dmrs == 2 else 0)
            alloc = dict(tb=0, Qm=6, dmrs_config_type=mode & 1, num_dmrs_cdm_grps_no_data=1, dmrs_symbol=2, fft_size=N, first_carrier_offset=N - 6 * rb,
                         bwp_start=0, rb_start=0, rb_size=rb, start_symbol=0, nr_of_symbols=14, ul_dmrs_symb_pos=pos, plane=2 * 14 * 12 * rb, rx_slot_off=0,
                         ch_off=0, rec_off=0)
            cfg = dict(slot=3, scid=0, dmrs_scrambling_id=77, port=0, chest_freq=mode >> 1)
            csegs = []
            for layer, port in enumerate((0, 1)):
                mine = m.pusch_chest_segments([alloc], [dict(cfg, port=port)], n_rx)
                csegs += [dict(c, ch_off=c["ch_off"] + layer * n_rx * stride, delay_off=0) for c in mine]
            first = m.pusch_grid_segments([alloc])[1]
            seg_arr, first_arr = m._chest_seg_array(csegs), m._rx_grid_seg_array(first)
            tb_arr, div_arr = m._u32_array([0] * len(csegs)), m._u32_array([14 * 2 * n_rx])

            def estimation(out=ch):
                assert LC.nrLDPC_hip_pusch_channel_estimation(rx.data_ptr(), stride, out.data_ptr(), stride, n_rx, seg_arr, len(csegs), None, m.MEM_DEVICE,
                                                              s_ptr) == 0, m.last_error()

            def estimation_meas():
                assert LM.nrLDPC_hip_pusch_channel_estimation_meas(rx.data_ptr(), stride, ch2.data_ptr(), stride, n_rx, seg_arr, len(csegs), None, tb_arr,
                                                                   div_arr, 1, mx.data_ptr(), nv.data_ptr(), m.MEM_DEVICE, s_ptr) == 0, m.last_error()

            def level():
                assert LX.nrLDPC_hip_ulsch_channel_level_grid_mmse(ch.data_ptr(), n_rx, stride, first_arr, 1, mx.data_ptr(), lv.data_ptr(), m.MEM_DEVICE,
                                                                   s_ptr) == 0, m.last_error()
            legs = {"estimation": estimation, "level": level}
            out = {"descriptors": len(csegs)}
            if has_meas:
                legs["estimation_meas"] = estimation_meas
                with torch.cuda.stream(side):
                    estimation()
                    estimation_meas()
                torch.cuda.synchronize()
                want_mx, want_nv = 0, 0
                rx_h = rx.cpu().numpy().reshape(-1, 2)
                for c in csegs:
                    a, noise, nest = m.pusch_chest_meas_host(rx_h, stride, n_rx, c)
                    want_mx, want_nv = max(want_mx, a), want_nv + (noise // nest if nest else 0)
                out["meas_equals_plain_and_host_form"] = bool(torch.equal(ch, ch2)) and int(mx[0]) == want_mx and int(nv[0]) == want_nv // (14 * 2 * n_rx)
                out["max_ch"], out["nvar"] = int(mx[0]), int(nv[0])
                if n_dmrs == 2:
                    asegs = m.pusch_chest_avg_segments([alloc])[0]
                    avg_arr = m._chest_avg_seg_array(asegs)

                    def time_avg():
                        assert LM.nrLDPC_hip_pusch_chest_time_avg(ch2.data_ptr(), stride, 2 * n_rx, avg_arr, 1, m.MEM_DEVICE, s_ptr) == 0, m.last_error()
                    legs["time_avg"] = time_avg
            for fn in legs.values():
                with torch.cuda.stream(side):
                    for _ in range(3):
                        fn()
            torch.cuda.synchronize()
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
            if has_meas:
                out["meas_minus_plain_us"] = {"median": float(np.median(ts["estimation_meas"]) - np.median(ts["estimation"])),
                                              "min": float(np.min(ts["estimation_meas"]) - np.min(ts["estimation"]))}
            res["configs"][f"{('TYPE1_INTERP', 'TYPE2_INTERP', 'TYPE1_AVG', 'TYPE2_AVG')[mode]}_dmrs{n_dmrs}"] = out
    print(json.dumps(res))


if len(sys.argv) > 2 and sys.argv[2] == "meas":
    measure_meas()
    sys.exit(0)
A = 213176
while m.nr_segmentation(A + 24, 1) is None:
    A += 8
Qm, n_rx, n, rb, N = 6, 4, 64, 273, 4096
symbols = [12 * rb] * 2 + [6 * rb] + [12 * rb] * 10      # 13 data-bearing symbols, symbol 2 a type-1 DMRS symbol with half the REs
S = sum(symbols)
G = S * Qm
tbs = [dict(A=A, G=G, BG=1, Qm=Qm, Nl=1, rv=0, tbslbrm=0, round=0) for _ in range(n)]
rng = np.random.default_rng(1)
scr = [(int(rng.integers(0, 0x10000)), 0, int(rng.integers(0, 1024))) for _ in range(n)]
po, co, ho, _ = m.tb_layout(tbs)
cw, total = m.tb_layout_packed(tbs)
allocs = [dict(tb=i, Qm=Qm, dmrs_config_type=0, num_dmrs_cdm_grps_no_data=1, dmrs_symbol=2, fft_size=N, first_carrier_offset=N - 6 * rb, bwp_start=0,
               rb_start=0, rb_size=rb, start_symbol=0, nr_of_symbols=13, ul_dmrs_symb_pos=1 << 2, plane=S, rx_slot_off=i * 14 * N, ch_off=i * 14 * N,
               rec_off=int(co[i])) for i in range(n)]
cfgs = [dict(slot=i % 20, scid=i & 1, dmrs_scrambling_id=int(rng.integers(0, 65536)), port=0, chest_freq=chest_freq) for i in range(n)]
gsegs, gfirst = m.pusch_grid_segments(allocs)
csegs = m.pusch_chest_segments(allocs, cfgs, n_rx)
assert len(csegs) == n and [c["ch_off"] for c in csegs] == [f["ch_off"] for f in gfirst]
gseg_arr, gfirst_arr, cseg_arr = m._rx_grid_seg_array(gsegs), m._rx_grid_seg_array(gfirst), m._chest_seg_array(csegs)
gstride = n * 14 * N
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    payload = torch.randint(0, 256, (int(po[-1]) + 16,), dtype=torch.uint8, device="cuda")
    words = torch.zeros(total // 4 + 4, dtype=torch.int32, device="cuda")
    m.PreparedTbBatch(tbs, payload, words, scrambling=scr).encode()
    pts = torch.zeros(2 * S, dtype=torch.int16, device="cuda")
    rx_g = torch.zeros(n_rx, gstride, 2, dtype=torch.int16, device="cuda")
    ch_g = torch.zeros(n_rx, gstride, 2, dtype=torch.int16, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(2)
    j12, j6 = torch.arange(12 * rb, device="cuda"), torch.arange(6 * rb, device="cuda")

    def put(at, y):                          # per block and antenna a flat complex gain (in y), additive noise
        y = torch.view_as_real(y) + 150 * torch.randn(n_rx, y.shape[1], 2, device="cuda", generator=gen)
        rx_g[:, at] = y.round().clamp(-32768, 32767).to(torch.int16)
    for i in range(n):
        m.modulation(words[cw[i] // 4:], G, Qm, out=pts)
        x = torch.view_as_complex(pts.view(S, 2).float() / 23170.0)
        h = torch.polar(1200 + 1400 * torch.rand(n_rx, device="cuda", generator=gen), 6.2832 * torch.rand(n_rx, device="cuda", generator=gen))
        h = torch.view_as_complex(torch.view_as_real(h).round().contiguous())
        for g in (g for g in gsegs if g["tb"] == i):
            p_idx = 2 * j6 + 1 if g["pattern"] == m.RXG_DMRS1 else j12
            put(g["rx_off"] + (g["start_re"] + p_idx) % N, h[:, None] * x[None, g["sym_off"]:g["sym_off"] + g["nb_re"]])
        c = csegs[i]                         # the transmitted DMRS: the conjugate of the receiver's pilots, unit magnitude (see tests/test_gpu_rx_chest.py)
        p = torch.from_numpy(m.pusch_dmrs_host(c["c_init"], c["dmrs_offset"], 6 * rb, c["port"], 0).astype(np.float32)).cuda()
        put(c["rx_off"] + (c["start_re"] + 2 * j6) % N, h[:, None] * torch.complex(p[:, 0], -p[:, 1])[None, :] / (23170.0 * 2 ** 0.5))
    rec = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
    shift = torch.zeros(n, dtype=torch.int32, device="cuda")
    harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
    pay_out = torch.zeros_like(payload)
    ack = torch.zeros(n, dtype=torch.uint8, device="cuda")
    itm = torch.zeros(n, dtype=torch.int32, device="cuda")
    dec = m.PreparedTbBatch(tbs, pay_out, rec, harq, ack, itm, scrambling=scr, symbols=True)
    chest_bytes = n * n_rx * 12 * rb * 4     # read, and as many written
    copy_src = torch.zeros(chest_bytes, dtype=torch.uint8, device="cuda")
    copy_dst = torch.zeros_like(copy_src)
torch.cuda.synchronize()
s_ptr = side.cuda_stream


def estimation():
    assert LC.nrLDPC_hip_pusch_channel_estimation(rx_g.data_ptr(), gstride, ch_g.data_ptr(), gstride, n_rx, cseg_arr, n, None, m.MEM_DEVICE, s_ptr) == 0, m.last_error()


def front():
    assert LG.nrLDPC_hip_ulsch_channel_level_grid(ch_g.data_ptr(), n_rx, gstride, gfirst_arr, n, shift.data_ptr(), m.MEM_DEVICE, s_ptr) == 0, m.last_error()
    assert LG.nrLDPC_hip_ulsch_channel_compensation_grid(rx_g.data_ptr(), ch_g.data_ptr(), n_rx, gstride, gstride, gseg_arr, len(gsegs), shift.data_ptr(),
                                                         rec.data_ptr(), m.MEM_DEVICE, s_ptr) == 0, m.last_error()


def estimation_front():
    estimation()
    front()


def device_copy():
    copy_dst.copy_(copy_src)


def filler():
    for _ in range(4):
        dec.decode()


with torch.cuda.stream(side):
    estimation_front()
    dec.decode()
torch.cuda.synchronize()
c0 = csegs[n // 2]
got = ch_g.cpu().numpy()
want = np.zeros((gstride, 2), np.int16)
m.pusch_chest_host(rx_g[n_rx - 1].cpu().numpy(), c0, 0, want)
res = {"reps": reps, "n_tb": n, "n_rx": n_rx, "Qm": Qm, "fft_size": N, "rb": rb, "mode": "TYPE1_AVG" if chest_freq else "TYPE1_INTERP",
       "descriptors": len(csegs), "log2_maxh": sorted(set(shift.cpu().tolist())), "all_ack": bool(ack.cpu().numpy().all()),
       "payload_ok": all(bool(torch.equal(pay_out[int(po[i]):int(po[i]) + A // 8], payload[int(po[i]):int(po[i]) + A // 8])) for i in range(n)),
       "device_equals_host_form": bool(np.array_equal(got[n_rx - 1, c0["ch_off"]:c0["ch_off"] + 12 * rb], want[c0["ch_off"]:c0["ch_off"] + 12 * rb])),
       "bytes_read": chest_bytes, "bytes_written": chest_bytes}
legs = {"estimation": estimation, "device_copy": device_copy, "front": front, "estimation_front": estimation_front, "decode_symbols": dec.decode}
for fn in legs.values():
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
torch.cuda.synchronize()
ts = {k: [] for k in legs}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for _ in range(reps):
    for k, fn in legs.items():
        with torch.cuda.stream(side):
            filler()
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        ts[k].append(e0.elapsed_time(e1))
for k, v in ts.items():
    res[k + "_ms"] = {"mean": float(np.mean(v)), "median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    res[k + "_spread"] = (float(np.max(v)) - float(np.min(v))) / float(np.mean(v))
for k in ("estimation", "device_copy"):
    res[k + "_share_of_hbm_peak"] = {"median": 2 * chest_bytes / (float(np.median(ts[k])) * 1e-3) / HBM_PEAK, "best": 2 * chest_bytes / (float(np.min(ts[k])) * 1e-3) / HBM_PEAK}
med = lambda k: float(np.median(ts[k]))
res["estimation_over_copy"] = {"median": med("estimation") / med("device_copy"), "min": float(np.min(ts["estimation"]) / np.min(ts["device_copy"]))}
res["estimation_front_over_front"] = {"median": med("estimation_front") / med("front"), "min": float(np.min(ts["estimation_front"]) / np.min(ts["front"]))}
res["estimation_over_decode"] = {"median": med("estimation") / med("decode_symbols")}
print(json.dumps(res))
