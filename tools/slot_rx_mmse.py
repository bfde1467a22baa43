#!/usr/bin/env python3
"""One slot's 64 two-layer transport blocks (273 PRB x 13 data symbols, 64QAM, Nl = 2) from the OFDM grids of n_rx = 4 antennas
and the per-layer channel estimates in device memory: the MMSE channel level, the two-layer MMSE receiver and
ulsch_decode_symbols, in one process, timed with HIP events.

  python tools/slot_rx_mmse.py [reps]      -> one JSON line; times in microseconds (mean, min, max, median over reps)

Modelled on tools/slot_rx_front.py: the calls refuse a capturing stream, so every timed call is enqueued behind a filler (four
decode calls) that keeps the GPU busy while the host enqueues, and the events around it see GPU time -- the descriptor upload and
the kernel.  The yardstick is nrLDPC_hip_ulsch_channel_compensation_grid at n_rx = 4 on the same REs (layer 0's estimates, records
of its own), alternating with the MMSE launch inside one loop so that both see the same machine.  Bytes are counted from the
shapes: MMSE 4 * 3 n_rx in (the grid and two layers' estimates) + 2 Qm out per RE, compensation 8 n_rx in + 2 Qm out; shares are
of the HBM peak bench.py uses.  Bytes and a share of the peak are given for these two launches only; the level launch,
decode_symbols and the three back to back are reported as times.  The tool stops before timing when a block does not decode.

The channel is that of the end-to-end tests (tests/test_rx_mmse_host.py): per block a flat 4 x 2 matrix with gains of 400..480
and nearly orthogonal columns, max_ch below 2048, noise sigma 3 per component, nvar 18.
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
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
m = pkg.ldpc
pkg.LDPCinit()
LM, LG = m._rxm_lib(), m._rxg_lib()
Qm, n_rx, n, rb, N = 6, 4, 64, 273, 4096
S = (12 * 12 + 6) * rb                       # REs per layer: 12 full symbols and a type-1 DMRS symbol with half the REs
G = 2 * S * Qm
A = G // 2 // 8 * 8                          # rate 1/2
while m.nr_segmentation(A + 24, 1) is None:
    A += 8
tbs = [dict(A=A, G=G, BG=1, Qm=Qm, Nl=2, rv=0, tbslbrm=0, round=0) for _ in range(n)]
rng = np.random.default_rng(1)
scr = [(int(rng.integers(0, 0x10000)), 0, int(rng.integers(0, 1024))) for _ in range(n)]
po, co, ho, _ = m.tb_layout(tbs)
cw, total = m.tb_layout_packed(tbs)
gstride = n * 14 * N
allocs = [dict(tb=i, Qm=Qm, dmrs_config_type=0, num_dmrs_cdm_grps_no_data=1, dmrs_symbol=2, fft_size=N, first_carrier_offset=N - 6 * rb, bwp_start=0,
               rb_start=0, rb_size=rb, start_symbol=0, nr_of_symbols=13, ul_dmrs_symb_pos=1 << 2, plane=2 * S, rx_slot_off=i * 14 * N, ch_off=i * 14 * N,
               rec_off=int(co[i])) for i in range(n)]
segs, first = m.pusch_grid_segments(allocs)
assert sum(g["nb_re"] for g in segs) == n * S
# the yardstick's descriptors: the same REs as one layer, records of its own
ysegs, yfirst = m.pusch_grid_segments([dict(a, plane=S, rec_off=i * Qm * S) for i, a in enumerate(allocs)])
seg_arr, first_arr, yseg_arr, yfirst_arr = (m._rx_grid_seg_array(v) for v in (segs, first, ysegs, yfirst))
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    payload = torch.randint(0, 256, (int(po[-1]) + 16,), dtype=torch.uint8, device="cuda")
    words = torch.zeros(total // 4 + 4, dtype=torch.int32, device="cuda")
    m.PreparedTbBatch(tbs, payload, words, scrambling=scr).encode()
    pts = torch.zeros(2 * 2 * S, dtype=torch.int16, device="cuda")
    rx_g = torch.zeros(n_rx, gstride, 2, dtype=torch.int16, device="cuda")
    ch_g = torch.zeros(2 * n_rx, gstride, 2, dtype=torch.int16, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(2)
    max_ch = torch.zeros(n, dtype=torch.int32, device="cuda")
    sign = torch.tensor([1.0, -1.0, 1.0, -1.0], device="cuda")
    j12, j6 = torch.arange(12 * rb, device="cuda"), 2 * torch.arange(6 * rb, device="cuda") + 1
    for i in range(n):
        m.modulation(words[cw[i] // 4:], G, Qm, out=pts)
        x = torch.view_as_complex(pts.view(S, 2, 2).float() / 23170.0).t()                    # [layer, RE]: symbol 2 r + l is layer l
        col = torch.polar(400 + 80 * torch.rand(n_rx, device="cuda", generator=gen), 6.2832 * torch.rand(n_rx, device="cuda", generator=gen))
        turn = torch.polar(torch.ones(1, device="cuda"), 6.2832 * torch.rand(1, device="cuda", generator=gen))
        hq = torch.view_as_real(torch.stack([col, col * turn * sign])).round()               # [layer, antenna, 2]
        h = torch.view_as_complex(hq.contiguous())
        y = torch.view_as_real(torch.einsum("la,lr->ar", h, x)) + 3.0 * torch.randn(n_rx, S, 2, device="cuda", generator=gen)
        y = y.round().clamp(-32768, 32767).to(torch.int16)
        max_ch[i] = int(hq.abs().max())
        for g in segs[13 * i:13 * i + 13]:
            p_idx = j6 if g["pattern"] == m.RXG_DMRS1 else j12
            rx_g[:, g["rx_off"] + (g["start_re"] + p_idx) % N] = y[:, g["sym_off"]:g["sym_off"] + g["nb_re"]]
        ch_g[:, first[i]["ch_off"]:first[i]["ch_off"] + 12 * rb] = hq.to(torch.int16).view(2 * n_rx, 1, 2)
    rec = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
    rec_y = torch.zeros(n * Qm * S + 16, dtype=torch.int16, device="cuda")
    shift, shift_y = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    nvar = torch.full((n,), 18, dtype=torch.int32, device="cuda")
    harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
    pay_out = torch.zeros_like(payload)
    ack = torch.zeros(n, dtype=torch.uint8, device="cuda")
    itm = torch.zeros(n, dtype=torch.int32, device="cuda")
    dec = m.PreparedTbBatch(tbs, pay_out, rec, harq, ack, itm, scrambling=scr, symbols=True)
torch.cuda.synchronize()
s_ptr = side.cuda_stream


def level():
    assert LM.nrLDPC_hip_ulsch_channel_level_grid_mmse(ch_g.data_ptr(), n_rx, gstride, first_arr, n, max_ch.data_ptr(), shift.data_ptr(), m.MEM_DEVICE,
                                                       s_ptr) == 0, m.last_error()


def mmse():
    assert LM.nrLDPC_hip_ulsch_mmse_2layers_grid(rx_g.data_ptr(), ch_g.data_ptr(), n_rx, gstride, gstride, seg_arr, len(segs), shift.data_ptr(),
                                                 nvar.data_ptr(), rec.data_ptr(), m.MEM_DEVICE, s_ptr) == 0, m.last_error()


def compensation_grid():
    assert LG.nrLDPC_hip_ulsch_channel_compensation_grid(rx_g.data_ptr(), ch_g.data_ptr(), n_rx, gstride, gstride, yseg_arr, len(ysegs),
                                                         shift_y.data_ptr(), rec_y.data_ptr(), m.MEM_DEVICE, s_ptr) == 0, m.last_error()


def all_three():
    level()
    mmse()
    dec.decode()


def filler():
    for _ in range(4):
        dec.decode()


def stats(v, nbytes=None):
    us = 1e3 * np.asarray(v)
    out = {"mean": float(us.mean()), "min": float(us.min()), "max": float(us.max()), "median": float(np.median(us)),
           "spread": float((us.max() - us.min()) / us.mean())}
    if nbytes is not None:
        out["bytes"] = nbytes
        out["share_of_hbm_peak"] = {"mean": nbytes / (out["mean"] * 1e-6) / HBM_PEAK, "best": nbytes / (out["min"] * 1e-6) / HBM_PEAK}
    return out


def timed(legs):
    """the legs alternating inside one loop; milliseconds per leg and repetition"""
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
    return ts


with torch.cuda.stream(side):
    LG.nrLDPC_hip_ulsch_channel_level_grid(ch_g.data_ptr(), n_rx, gstride, yfirst_arr, n, shift_y.data_ptr(), m.MEM_DEVICE, s_ptr)
    all_three()
torch.cuda.synchronize()
res = {"reps": reps, "n_tb": n, "n_rx": n_rx, "Qm": Qm, "Nl": 2, "segments": len(segs), "res_per_layer": n * S, "A": A,
       "log2_maxh": sorted(set(shift.cpu().tolist())), "all_ack": bool(ack.cpu().numpy().all()),
       "payload_ok": all(bool(torch.equal(pay_out[int(po[i]):int(po[i]) + A // 8], payload[int(po[i]):int(po[i]) + A // 8])) for i in range(n))}
assert res["all_ack"] and res["payload_ok"], res          # no timing of a slot that does not decode
mmse_bytes, comp_bytes = n * S * (4 * 3 * n_rx + 2 * Qm), n * S * (8 * n_rx + 2 * Qm)
ts = timed({"mmse": mmse, "compensation_grid": compensation_grid})
res["mmse_us"], res["compensation_grid_us"] = stats(ts["mmse"], mmse_bytes), stats(ts["compensation_grid"], comp_bytes)
res["mmse_share_over_yardstick_share"] = res["mmse_us"]["share_of_hbm_peak"]["mean"] / res["compensation_grid_us"]["share_of_hbm_peak"]["mean"]
ts = timed({"level": level, "decode_symbols": dec.decode, "all_three": all_three})
res["level_mmse_us"], res["decode_symbols_us"], res["level_mmse_decode_us"] = stats(ts["level"]), stats(ts["decode_symbols"]), stats(ts["all_three"])
res["front_over_slot"] = (res["level_mmse_us"]["mean"] + res["mmse_us"]["mean"]) / res["level_mmse_decode_us"]["mean"]
print(json.dumps(res))
