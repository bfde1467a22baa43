#!/usr/bin/env python3
"""One slot's 64 transport blocks (the slot of tools/slot_chain_demod.py: 273 PRB x 13 data symbols, 64QAM) from extracted REs
and channel estimates of n_rx = 4 antennas in device memory: channel level, channel compensation and ulsch_decode_symbols, in
one process, timed with HIP events.

  python tools/slot_rx_front.py [reps]      -> one JSON line; times in milliseconds (mean, min, max over reps)

The two front calls refuse a capturing stream, so nothing here is replayed from a graph: every timed call is enqueued behind a
filler (four decode calls) that keeps the GPU busy while the host enqueues, and the events around it see GPU time -- the
descriptor upload and the kernel -- not the host's enqueueing.  The yardstick for the compensation kernel is nrLDPC_hip_ulsch_llr
on the same number of REs (64 launches, one per block), timed the same way in the same run; both as a share of the HBM peak with
bytes counted from the shapes (compensation: 8 n_rx in + 2 Qm out per RE; ulsch_llr: 2 Qm in + 2 Qm out).

The grid leg: the same REs laid into OFDM grids (N = 4096, first_carrier_offset = N - 6 * 273, one type-1 DMRS symbol per block) and
read by nrLDPC_hip_ulsch_channel_compensation_grid, against the launch above on the pre-extracted arrays and a plain device copy
that moves the same number of bytes (half of them read, half written), the three alternating inside one loop so that they see the
same machine; the records of the two launches are compared.
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
m = pkg.ldpc
pkg.LDPCinit()
L = m._rxf_lib()
A = 213176
while m.nr_segmentation(A + 24, 1) is None:
    A += 8
Qm, n_rx, n = 6, 4, 64
rb = 273
symbols = [12 * rb] * 2 + [6 * rb] + [12 * rb] * 10      # 13 data-bearing symbols, one of them a DMRS symbol with half the REs
S = sum(symbols)
G = S * Qm
assert G == (12 * 13 - 6) * 273 * 6
tbs = [dict(A=A, G=G, BG=1, Qm=Qm, Nl=1, rv=0, tbslbrm=0, round=0) for _ in range(n)]
rng = np.random.default_rng(1)
scr = [(int(rng.integers(0, 0x10000)), 0, int(rng.integers(0, 1024))) for _ in range(n)]
po, co, ho, _ = m.tb_layout(tbs)
cw, total = m.tb_layout_packed(tbs)
segs, first, rec_off, n_in = m.rx_front_segments(tbs, [symbols] * n)
seg_arr, first_arr = m._rx_seg_array(segs), m._rx_seg_array(first)
stride = n_in
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    payload = torch.randint(0, 256, (int(po[-1]) + 16,), dtype=torch.uint8, device="cuda")
    words = torch.zeros(total // 4 + 4, dtype=torch.int32, device="cuda")
    m.PreparedTbBatch(tbs, payload, words, scrambling=scr).encode()
    pts = torch.zeros(2 * S, dtype=torch.int16, device="cuda")
    rx = torch.zeros(n_rx, stride, 2, dtype=torch.int16, device="cuda")
    ch = torch.zeros(n_rx, stride, 2, dtype=torch.int16, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(2)
    for i in range(n):                       # per block and antenna a flat complex gain, additive noise
        m.modulation(words[cw[i] // 4:], G, Qm, out=pts)
        x = torch.view_as_complex(pts.view(S, 2).float() / 23170.0)
        h = torch.polar(1200 + 1400 * torch.rand(n_rx, device="cuda", generator=gen), 6.2832 * torch.rand(n_rx, device="cuda", generator=gen))
        hq = torch.view_as_real(h).round()
        y = torch.view_as_complex(hq.contiguous())[:, None] * x[None, :]
        y = torch.view_as_real(y) + 150 * torch.randn(n_rx, S, 2, device="cuda", generator=gen)
        rx[:, i * S:(i + 1) * S] = y.round().clamp(-32768, 32767).to(torch.int16)
        ch[:, i * S:(i + 1) * S] = hq.to(torch.int16)[:, None, :]
    rec = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
    llr = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
    shift = torch.zeros(n, dtype=torch.int32, device="cuda")
    harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
    pay_out = torch.zeros_like(payload)
    ack = torch.zeros(n, dtype=torch.uint8, device="cuda")
    itm = torch.zeros(n, dtype=torch.int32, device="cuda")
    dec = m.PreparedTbBatch(tbs, pay_out, rec, harq, ack, itm, scrambling=scr, symbols=True)
torch.cuda.synchronize()
s_ptr = side.cuda_stream


def level():
    assert L.nrLDPC_hip_ulsch_channel_level(ch.data_ptr(), n_rx, stride, first_arr, n, shift.data_ptr(), m.MEM_DEVICE, s_ptr) == 0, m.last_error()


def compensation():
    assert L.nrLDPC_hip_ulsch_channel_compensation(rx.data_ptr(), ch.data_ptr(), n_rx, stride, seg_arr, len(segs), shift.data_ptr(), rec.data_ptr(),
                                                   m.MEM_DEVICE, s_ptr) == 0, m.last_error()


def llr_64():
    for i in range(n):
        m.ulsch_llr(rec[co[i]:co[i] + 2 * S], [rec[co[i] + 2 * S:co[i] + 4 * S], rec[co[i] + 4 * S:co[i] + 6 * S]], Qm, out=llr[co[i]:])


def all_three():
    level()
    compensation()
    dec.decode()


def filler():
    for _ in range(4):
        dec.decode()


def timed(fn):
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        with torch.cuda.stream(side):
            filler()
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"mean": float(np.mean(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


with torch.cuda.stream(side):
    level()
    compensation()
    dec.decode()
torch.cuda.synchronize()
res = {"reps": reps, "n_tb": n, "n_rx": n_rx, "Qm": Qm, "segments": len(segs), "res_total": n * S, "log2_maxh": sorted(set(shift.cpu().tolist())),
       "all_ack": bool(ack.cpu().numpy().all()), "payload_ok": bool(torch.equal(pay_out[:int(po[-1])], payload[:int(po[-1])]))}
res["level_ms"] = timed(level)
res["compensation_ms"] = timed(compensation)
res["decode_symbols_ms"] = timed(dec.decode)
res["level_compensation_decode_ms"] = timed(all_three)
res["ulsch_llr_64_launches_ms"] = timed(llr_64)
comp_bytes, llr_bytes = n * S * (8 * n_rx + 2 * Qm), n * S * 4 * Qm
for key, t, b in (("compensation", res["compensation_ms"], comp_bytes), ("ulsch_llr", res["ulsch_llr_64_launches_ms"], llr_bytes)):
    res[key + "_bytes"] = b
    res[key + "_share_of_hbm_peak"] = {k: b / (t[k2] * 1e-3) / HBM_PEAK for k, k2 in (("mean", "mean"), ("best", "min"), ("worst", "max"))}
    res[key + "_spread"] = (t["max"] - t["min"]) / t["mean"]
res["front_over_slot"] = (res["level_ms"]["mean"] + res["compensation_ms"]["mean"]) / res["level_compensation_decode_ms"]["mean"]

# ---- the grid leg ----
N = 4096
allocs = [dict(tb=i, Qm=Qm, dmrs_config_type=0, num_dmrs_cdm_grps_no_data=1, dmrs_symbol=2, fft_size=N, first_carrier_offset=N - 6 * rb, bwp_start=0,
               rb_start=0, rb_size=rb, start_symbol=0, nr_of_symbols=13, ul_dmrs_symb_pos=1 << 2, plane=S, rx_slot_off=i * 14 * N, ch_off=i * 14 * N,
               rec_off=int(rec_off[i])) for i in range(n)]
gsegs, gfirst = m.pusch_grid_segments(allocs)
assert [g["nb_re"] for g in gsegs] == [s_["nb_re"] for s_ in segs] and [g["sym_off"] for g in gsegs] == [s_["sym_off"] for s_ in segs]
gstride = n * 14 * N
LG = m._rxg_lib()
gseg_arr, gfirst_arr = m._rx_grid_seg_array(gsegs), m._rx_grid_seg_array(gfirst)
with torch.cuda.stream(side):
    rx_g = torch.zeros(n_rx, gstride, 2, dtype=torch.int16, device="cuda")
    ch_g = torch.zeros(n_rx, gstride, 2, dtype=torch.int16, device="cuda")
    j12, j6 = torch.arange(12 * rb, device="cuda"), 2 * torch.arange(6 * rb, device="cuda") + 1
    for g, e in zip(gsegs, segs):
        p_idx = j6 if g["pattern"] == m.RXG_DMRS1 else j12
        rx_g[:, g["rx_off"] + (g["start_re"] + p_idx) % N] = rx[:, e["rx_off"]:e["rx_off"] + e["nb_re"]]
        ch_g[:, g["ch_off"] + p_idx] = ch[:, e["ch_off"]:e["ch_off"] + e["nb_re"]]      # flat per block: every symbol writes the same estimates
    rec_g = torch.zeros_like(rec)
    shift_g = torch.zeros_like(shift)
    copy_src = torch.zeros(comp_bytes // 2, dtype=torch.uint8, device="cuda")
    copy_dst = torch.zeros_like(copy_src)
torch.cuda.synchronize()


def level_grid():
    assert LG.nrLDPC_hip_ulsch_channel_level_grid(ch_g.data_ptr(), n_rx, gstride, gfirst_arr, n, shift_g.data_ptr(), m.MEM_DEVICE, s_ptr) == 0, m.last_error()


def compensation_grid():
    assert LG.nrLDPC_hip_ulsch_channel_compensation_grid(rx_g.data_ptr(), ch_g.data_ptr(), n_rx, gstride, gstride, gseg_arr, len(gsegs), shift.data_ptr(),
                                                         rec_g.data_ptr(), m.MEM_DEVICE, s_ptr) == 0, m.last_error()


def device_copy():
    copy_dst.copy_(copy_src)


with torch.cuda.stream(side):
    level()
    compensation()
    level_grid()
    compensation_grid()
torch.cuda.synchronize()
res["grid_equals_extracted"] = bool(torch.equal(rec_g, rec)) and bool(torch.equal(shift_g, shift))
legs = {"compensation_grid": compensation_grid, "compensation_extracted": compensation, "device_copy": device_copy}
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
res["grid_leg"] = {"fft_size": N, "rb": rb, "dmrs": "type 1, one symbol", "bytes_each": comp_bytes}
for k, v in ts.items():
    res["grid_leg"][k + "_ms"] = {"mean": float(np.mean(v)), "min": float(np.min(v)), "max": float(np.max(v)), "median": float(np.median(v))}
    res["grid_leg"][k + "_share_of_hbm_peak"] = {"mean": comp_bytes / (float(np.mean(v)) * 1e-3) / HBM_PEAK, "best": comp_bytes / (float(np.min(v)) * 1e-3) / HBM_PEAK}
    res["grid_leg"][k + "_spread"] = (float(np.max(v)) - float(np.min(v))) / float(np.mean(v))
res["grid_leg"]["grid_over_extracted"] = {"mean": float(np.mean(ts["compensation_grid"]) / np.mean(ts["compensation_extracted"])),
                                          "median": float(np.median(ts["compensation_grid"]) / np.median(ts["compensation_extracted"])),
                                          "min": float(np.min(ts["compensation_grid"]) / np.min(ts["compensation_extracted"]))}
res["level_grid_ms"] = timed(level_grid)
print(json.dumps(res))
