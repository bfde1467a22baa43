#!/usr/bin/env python3
"""One slot's 64 two-layer transport blocks (273 PRB x 13 symbols, Nl = 2) at QPSK and at 16QAM from the OFDM grids of n_rx = 4
antennas and the per-layer channel estimates in device memory: the ML channel level, the two-layer max-log ML receiver and
ulsch_decode_scrambled, in one process, timed with HIP events.

  python tools/slot_rx_ml.py [reps]      -> one JSON line; times in microseconds (mean, min, max, median over reps)

Modelled on tools/slot_rx_mmse.py: the calls refuse a capturing stream, so every timed call is enqueued behind a filler (four
decode calls) that keeps the GPU busy while the host enqueues, and the events around it see GPU time -- the descriptor upload and
the kernel.  Two yardsticks, alternating with the ML launches inside one loop so that all see the same machine:
nrLDPC_hip_ulsch_channel_compensation_grid at n_rx = 4 on the same REs at the same Qm (layer 0's estimates, records of its own),
and nrLDPC_hip_ulsch_mmse_2layers_grid on a 64QAM slot of the same REs.  Bytes are counted from the shapes: ML 4 * 3 n_rx in (the
grid and two layers' estimates) + 4 Qm out per RE, MMSE 12 n_rx in + 2 Qm out, compensation 8 n_rx in + 2 Qm out; shares are of
the HBM peak bench.py uses.  The tool stops before timing when a block of an ML slot does not decode.

The channel is that of the end-to-end tests (tests/test_rx_ml_host.py): per block a flat 4 x 2 matrix with gains of 400..480 and
nearly orthogonal columns, max_ch below 2048, noise sigma 3 per component.
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
LL, LM, LG = m._rxl_lib(), m._rxm_lib(), m._rxg_lib()
n_rx, n, rb, N = 4, 64, 273, 4096
S = (12 * 12 + 6) * rb                       # REs per layer: 12 full symbols and a type-1 DMRS symbol with half the REs
gstride = n * 14 * N
side = torch.cuda.Stream()
s_ptr = side.cuda_stream


class Slot:
    """the descriptors, grids, estimates and outputs of one slot at one Qm; ML for Qm 2 / 4, MMSE for Qm 6"""

    def __init__(self, Qm, rx_g, ch_g, fill):
        self.Qm, self.ml = Qm, Qm < 6
        G = 2 * S * Qm
        A = G // 2 // 8 * 8                  # rate 1/2
        while m.nr_segmentation(A + 24, 1) is None:
            A += 8
        self.A = A
        self.tbs = [dict(A=A, G=G, BG=1, Qm=Qm, Nl=2, rv=0, tbslbrm=0, round=0) for _ in range(n)]
        rng = np.random.default_rng(Qm)
        self.scr = [(int(rng.integers(0, 0x10000)), 0, int(rng.integers(0, 1024))) for _ in range(n)]
        self.po, co, ho, _ = m.tb_layout(self.tbs)
        cw, total = m.tb_layout_packed(self.tbs)
        allocs = [dict(tb=i, Qm=Qm, dmrs_config_type=0, num_dmrs_cdm_grps_no_data=1, dmrs_symbol=2, fft_size=N, first_carrier_offset=N - 6 * rb,
                       bwp_start=0, rb_start=0, rb_size=rb, start_symbol=0, nr_of_symbols=13, ul_dmrs_symb_pos=1 << 2, plane=2 * S,
                       rx_slot_off=i * 14 * N, ch_off=i * 14 * N, rec_off=int(co[i])) for i in range(n)]
        segs, first = m.pusch_grid_segments(allocs)
        assert sum(g["nb_re"] for g in segs) == n * S
        ysegs, yfirst = m.pusch_grid_segments([dict(a, plane=S, rec_off=i * Qm * S) for i, a in enumerate(allocs)])
        self.n_seg = len(segs)
        self.seg_arr, self.first_arr, self.yseg_arr, self.yfirst_arr = (m._rx_grid_seg_array(v) for v in (segs, first, ysegs, yfirst))
        self.rx_g, self.ch_g = rx_g, ch_g
        with torch.cuda.stream(side):
            self.payload = torch.randint(0, 256, (int(self.po[-1]) + 16,), dtype=torch.uint8, device="cuda")
            self.max_ch = torch.full((n,), 480, dtype=torch.int32, device="cuda")
            if fill:
                words = torch.zeros(total // 4 + 4, dtype=torch.int32, device="cuda")
                m.PreparedTbBatch(self.tbs, self.payload, words, scrambling=self.scr).encode()
                pts = torch.zeros(2 * 2 * S, dtype=torch.int16, device="cuda")
                gen = torch.Generator(device="cuda").manual_seed(2)
                sign = torch.tensor([1.0, -1.0, 1.0, -1.0], device="cuda")
                j12, j6 = torch.arange(12 * rb, device="cuda"), 2 * torch.arange(6 * rb, device="cuda") + 1
                for i in range(n):
                    m.modulation(words[cw[i] // 4:], G, Qm, out=pts)
                    x = torch.view_as_complex(pts.view(S, 2, 2).float() / 23170.0).t()            # [layer, RE]: symbol 2 r + l is layer l
                    col = torch.polar(400 + 80 * torch.rand(n_rx, device="cuda", generator=gen),
                                      6.2832 * torch.rand(n_rx, device="cuda", generator=gen))
                    turn = torch.polar(torch.ones(1, device="cuda"), 6.2832 * torch.rand(1, device="cuda", generator=gen))
                    hq = torch.view_as_real(torch.stack([col, col * turn * sign])).round()       # [layer, antenna, 2]
                    h = torch.view_as_complex(hq.contiguous())
                    y = torch.view_as_real(torch.einsum("la,lr->ar", h, x)) + 3.0 * torch.randn(n_rx, S, 2, device="cuda", generator=gen)
                    y = y.round().clamp(-32768, 32767).to(torch.int16)
                    self.max_ch[i] = int(hq.abs().max())
                    for g in segs[13 * i:13 * i + 13]:
                        p_idx = j6 if g["pattern"] == m.RXG_DMRS1 else j12
                        rx_g[:, g["rx_off"] + (g["start_re"] + p_idx) % N] = y[:, g["sym_off"]:g["sym_off"] + g["nb_re"]]
                    ch_g[:, first[i]["ch_off"]:first[i]["ch_off"] + 12 * rb] = hq.to(torch.int16).view(2 * n_rx, 1, 2)
            self.out = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")          # LLRs (ML) or symbol records (MMSE)
            self.rec_y = torch.zeros(n * Qm * S + 16, dtype=torch.int16, device="cuda")
            self.shift, self.shift_y = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
            self.nvar = torch.full((n,), 18, dtype=torch.int32, device="cuda")
            self.harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
            self.pay_out = torch.zeros_like(self.payload)
            self.ack = torch.zeros(n, dtype=torch.uint8, device="cuda")
            self.itm = torch.zeros(n, dtype=torch.int32, device="cuda")
            self.dec = m.PreparedTbBatch(self.tbs, self.pay_out, self.out, self.harq, self.ack, self.itm, scrambling=self.scr, symbols=not self.ml)
        torch.cuda.synchronize()

    def level(self):
        fn = LL.nrLDPC_hip_ulsch_channel_level_grid_ml if self.ml else LM.nrLDPC_hip_ulsch_channel_level_grid_mmse
        assert fn(self.ch_g.data_ptr(), n_rx, gstride, self.first_arr, n, self.max_ch.data_ptr(), self.shift.data_ptr(), m.MEM_DEVICE, s_ptr) == 0, \
            m.last_error()

    def receiver(self):
        if self.ml:
            rc = LL.nrLDPC_hip_ulsch_ml_2layers_grid(self.rx_g.data_ptr(), self.ch_g.data_ptr(), n_rx, gstride, gstride, self.seg_arr, self.n_seg,
                                                     self.shift.data_ptr(), self.out.data_ptr(), m.MEM_DEVICE, s_ptr)
        else:
            rc = LM.nrLDPC_hip_ulsch_mmse_2layers_grid(self.rx_g.data_ptr(), self.ch_g.data_ptr(), n_rx, gstride, gstride, self.seg_arr, self.n_seg,
                                                       self.shift.data_ptr(), self.nvar.data_ptr(), self.out.data_ptr(), m.MEM_DEVICE, s_ptr)
        assert rc == 0, m.last_error()

    def compensation_grid(self):
        assert LG.nrLDPC_hip_ulsch_channel_compensation_grid(self.rx_g.data_ptr(), self.ch_g.data_ptr(), n_rx, gstride, gstride, self.yseg_arr,
                                                             self.n_seg, self.shift_y.data_ptr(), self.rec_y.data_ptr(), m.MEM_DEVICE, s_ptr) == 0, \
            m.last_error()

    def all_three(self):
        self.level()
        self.receiver()
        self.dec.decode()

    def check(self):
        with torch.cuda.stream(side):
            self.all_three()
        torch.cuda.synchronize()
        ok = all(bool(torch.equal(self.pay_out[int(self.po[i]):int(self.po[i]) + self.A // 8],
                                  self.payload[int(self.po[i]):int(self.po[i]) + self.A // 8])) for i in range(n))
        return {"A": self.A, "log2_maxh": sorted(set(self.shift.cpu().tolist())), "all_ack": bool(self.ack.cpu().numpy().all()), "payload_ok": ok}


def stats(v, nbytes=None):
    us = 1e3 * np.asarray(v)
    out = {"mean": float(us.mean()), "min": float(us.min()), "max": float(us.max()), "median": float(np.median(us)),
           "spread": float((us.max() - us.min()) / us.mean())}
    if nbytes is not None:
        out["bytes"] = nbytes
        out["share_of_hbm_peak"] = {"mean": nbytes / (out["mean"] * 1e-6) / HBM_PEAK, "best": nbytes / (out["min"] * 1e-6) / HBM_PEAK}
    return out


def timed(legs, filler):
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
                for _ in range(4):
                    filler()
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return ts


# the three slots read one grid and one set of estimates: those of the 16QAM slot.  The QPSK slot gets a grid of its own for its
# decode check and then times on the shared one; the 64QAM MMSE slot is a yardstick for time alone (its blocks are not decoded).
rx_g = torch.zeros(n_rx, gstride, 2, dtype=torch.int16, device="cuda")
ch_g = torch.zeros(2 * n_rx, gstride, 2, dtype=torch.int16, device="cuda")
res = {"reps": reps, "n_tb": n, "n_rx": n_rx, "Nl": 2, "res_per_layer": n * S}
q2 = Slot(2, rx_g, ch_g, True)
res["qpsk"] = q2.check()
q4 = Slot(4, rx_g, ch_g, True)                       # overwrites the grid with the 16QAM slot's
res["qam16"] = q4.check()
assert all(res[k]["all_ack"] and res[k]["payload_ok"] for k in ("qpsk", "qam16")), res      # no timing of a slot that does not decode
q6 = Slot(6, rx_g, ch_g, False)
res["segments"] = q4.n_seg
with torch.cuda.stream(side):
    for q in (q2, q4, q6):
        q.level()
        LG.nrLDPC_hip_ulsch_channel_level_grid(ch_g.data_ptr(), n_rx, gstride, q.yfirst_arr, n, q.shift_y.data_ptr(), m.MEM_DEVICE, s_ptr)
torch.cuda.synchronize()
nb = lambda inp, outp: n * S * (inp + outp)
legs = {"ml_qpsk": q2.receiver, "compensation_grid_qpsk": q2.compensation_grid, "ml_qam16": q4.receiver, "compensation_grid_qam16": q4.compensation_grid,
        "mmse_qam64": q6.receiver}
sizes = {"ml_qpsk": nb(12 * n_rx, 8), "compensation_grid_qpsk": nb(8 * n_rx, 4), "ml_qam16": nb(12 * n_rx, 16), "compensation_grid_qam16": nb(8 * n_rx, 8),
         "mmse_qam64": nb(12 * n_rx, 12)}
ts = timed(legs, q4.dec.decode)
for k in legs:
    res[k + "_us"] = stats(ts[k], sizes[k])
for k, y in (("ml_qpsk", "compensation_grid_qpsk"), ("ml_qam16", "compensation_grid_qam16"), ("ml_qpsk", "mmse_qam64"), ("ml_qam16", "mmse_qam64")):
    res[k + "_over_" + y] = res[k + "_us"]["mean"] / res[y + "_us"]["mean"]
with torch.cuda.stream(side):
    q4.all_three()                                    # the 16QAM slot's LLRs again, behind the shared grid's last writer
torch.cuda.synchronize()
ts = timed({"level": q4.level, "decode_scrambled": q4.dec.decode, "all_three": q4.all_three}, q4.dec.decode)
res["level_ml_us"], res["decode_scrambled_qam16_us"], res["level_ml_decode_qam16_us"] = stats(ts["level"]), stats(ts["decode_scrambled"]), stats(ts["all_three"])
res["front_over_slot_qam16"] = (res["level_ml_us"]["mean"] + res["ml_qam16_us"]["mean"]) / res["level_ml_decode_qam16_us"]["mean"]
print(json.dumps(res))
