#!/usr/bin/env python3
"""One slot's 64 transport blocks (273 PRB x 13 symbols, 64QAM: 1664 code segments; BASELINE configs[3]) on device buffers,
the DL-SCH chain to layer-mapped symbols in one call against the separate passes, timed with HIP events in one process:

  (a) dlsch_encode_scrambled | (b) (a) + 64 x modulation (+ 64 x layer_mapping when Nl > 1) | (c) dlsch_encode_symbols

for Nl = 1 and Nl = 2 (G = 245700 is a multiple of Qm Nl = 12).

  python tools/slot_chain_mod.py [reps]      -> one JSON line, milliseconds per call (mean over reps)

Every variant is captured in a HIP graph and replayed: GPU time, not the host's enqueueing.  (b) and (c) must give the same
bytes (`*_equal`).
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
rng = np.random.default_rng(1)
scr = [(int(rng.integers(0, 0x10000)), 0, int(rng.integers(0, 1024))) for _ in range(n)]
side = torch.cuda.Stream()   # every call is made and captured on this stream


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
for Nl in (1, 2):
    tbs = [dict(A=A, G=G, BG=1, Qm=Qm, Nl=Nl, rv=0, tbslbrm=0, round=0) for _ in range(n)]
    po, _, _, _ = m.tb_layout(tbs)
    cw, total = m.tb_layout_packed(tbs)
    cs, total_s = m.tb_layout_symbols(tbs)
    with torch.cuda.stream(side):
        payload = torch.randint(0, 256, (int(po[-1]) + 16,), dtype=torch.uint8, device="cuda")
        words = torch.zeros(total // 4 + 4, dtype=torch.int32, device="cuda")
        pts = torch.zeros(total_s // 2 + 16, dtype=torch.int16, device="cuda")      # (b): the points in codeword order
        sep = torch.zeros(total_s // 2 + 16, dtype=torch.int16, device="cuda")      # (b): ... layer mapped
        fused = torch.zeros(total_s // 2 + 16, dtype=torch.int16, device="cuda")   # (c); the 16-byte gaps stay 0 in both
        enc_s = m.PreparedTbBatch(tbs, payload, words, scrambling=scr)
        enc_y = m.PreparedTbBatch(tbs, payload, fused, scrambling=scr, symbols=True)

    def separate():
        enc_s.encode()
        for i in range(n):
            m.modulation(words[cw[i] // 4:], G, Qm, out=(pts if Nl > 1 else sep)[cs[i] // 2:])
        if Nl > 1:
            for i in range(n):
                m.layer_mapping(pts[cs[i] // 2:cs[i] // 2 + 2 * S], Nl, out=sep[cs[i] // 2:])

    k = f"nl{Nl}_"
    res[k + "a_encode_scrambled_ms"] = timed(enc_s.encode)
    res[k + "b_encode_scrambled_plus_mod_layers_ms"] = timed(separate)
    res[k + "c_encode_symbols_ms"] = timed(enc_y.encode)
    torch.cuda.synchronize()
    res[k + "equal"] = bool(torch.equal(fused, sep))
print(json.dumps(res))
