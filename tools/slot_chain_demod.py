#!/usr/bin/env python3
"""One slot's 64 transport blocks (273 PRB x 13 symbols, 64QAM: 1664 code segments; BASELINE configs[3]/[4]) on device
buffers, the demapper inside the decode call against the separate pass, timed with HIP events in one process:

  UL: (a) ulsch_decode_scrambled on ready LLRs | (b) 64 x ulsch_llr + ulsch_decode_scrambled | (c) ulsch_decode_symbols
  DL: dlsch_encode_scrambled                   | dlsch_encode_scrambled + 64 x modulation

  python tools/slot_chain_demod.py [reps]      -> one JSON line, milliseconds per call (mean over reps)

First transmissions (rv 0) at a noise level every block decodes at; the soft buffers are cleared by every call.  Every
variant is captured in a HIP graph and replayed: GPU time, not the host's enqueueing.
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import openairinterface5g_amd as pkg  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
m = pkg.ldpc
pkg.LDPCinit()
A = 213176
while m.nr_segmentation(A + 24, 1) is None:
    A += 8
Qm = 6
G = (12 * 13 - 6) * 273 * 6
S = G // Qm
n = 64
u = 3575                                     # 64QAM inner level; ideal magnitudes 4u, 2u
tbs = [dict(A=A, G=G, BG=1, Qm=Qm, Nl=1, rv=0, tbslbrm=0, round=0) for _ in range(n)]
rng = np.random.default_rng(1)
scr = [(int(rng.integers(0, 0x10000)), 0, int(rng.integers(0, 1024))) for _ in range(n)]
po, co, ho, segs = m.tb_layout(tbs)
cw, total = m.tb_layout_packed(tbs)
side = torch.cuda.Stream()   # every call is made and captured on this stream
with torch.cuda.stream(side):
    payload = torch.randint(0, 256, (int(po[-1]) + 16,), dtype=torch.uint8, device="cuda")
    words = torch.zeros(total // 4 + 4, dtype=torch.int32, device="cuda")
    enc_s = m.PreparedTbBatch(tbs, payload, words, scrambling=scr)
    enc_s.encode()
    rec = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")    # y in plane 0, then mag_a, mag_b
    pts = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")    # the DL arm's output
    for i in range(n):
        m.modulation(words[cw[i] // 4:], G, Qm, out=rec[co[i]:])
    for i in range(n):
        y = rec[co[i]:co[i] + 2 * S].float()
        rec[co[i]:co[i] + 2 * S] = (y + 0.15 * u * torch.randn_like(y)).round().clamp(-32768, 32767).to(torch.int16)
        rec[co[i] + 2 * S:co[i] + 4 * S] = 4 * u
        rec[co[i] + 4 * S:co[i] + 6 * S] = 2 * u
    llr = torch.zeros_like(rec)
    for i in range(n):
        m.ulsch_llr(rec[co[i]:co[i] + 2 * S], [rec[co[i] + 2 * S:co[i] + 4 * S], rec[co[i] + 4 * S:co[i] + 6 * S]], Qm, out=llr[co[i]:])
    llr_work = torch.zeros_like(llr)
    harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
    pay_out = torch.zeros_like(payload)
    ack = torch.zeros(n, dtype=torch.uint8, device="cuda")
    itm = torch.zeros(n, dtype=torch.int32, device="cuda")
    dec_a = m.PreparedTbBatch(tbs, pay_out, llr, harq, ack, itm, scrambling=scr)
    dec_b = m.PreparedTbBatch(tbs, pay_out, llr_work, harq, ack, itm, scrambling=scr)
    dec_c = m.PreparedTbBatch(tbs, pay_out, rec, harq, ack, itm, scrambling=scr, symbols=True)


def llr_then_decode():
    for i in range(n):
        m.ulsch_llr(rec[co[i]:co[i] + 2 * S], [rec[co[i] + 2 * S:co[i] + 4 * S], rec[co[i] + 4 * S:co[i] + 6 * S]], Qm,
                    out=llr_work[co[i]:])
    dec_b.decode()


def encode_then_modulation():
    enc_s.encode()
    for i in range(n):
        m.modulation(words[cw[i] // 4:], G, Qm, out=pts[co[i]:])


def timed(fn):
    """GPU time per call: the call captured once in a HIP graph, the graph replayed `reps` times between two events"""
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        g.replay()
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


res = {"reps": reps, "n_tb": n, "G": G, "Qm": Qm}
res["a_decode_scrambled_ms"] = timed(dec_a.decode)
torch.cuda.synchronize()
res["a_all_ack"] = bool(ack.cpu().numpy().all())
res["b_ulsch_llr_plus_decode_scrambled_ms"] = timed(llr_then_decode)
torch.cuda.synchronize()
res["b_llr_equal"] = bool(torch.equal(llr, llr_work))
res["c_decode_symbols_ms"] = timed(dec_c.decode)
torch.cuda.synchronize()
res["c_all_ack"] = bool(ack.cpu().numpy().all())
res["dl_encode_scrambled_ms"] = timed(enc_s.encode)
res["dl_encode_scrambled_plus_modulation_ms"] = timed(encode_then_modulation)
print(json.dumps(res))
