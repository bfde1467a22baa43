#!/usr/bin/env python3
"""One slot's 64 transport blocks (273 PRB x 13 symbols, 64QAM: 1664 code segments; BASELINE configs[3]/[4]) on device
buffers, scrambling inside the chain calls against the separate passes, timed with HIP events in one process:

  DL: dlsch_encode                    | dlsch_encode + 64 x codeword_scrambling  | dlsch_encode_scrambled
  UL: ulsch_decode                    | 64 x codeword_unscrambling + ulsch_decode | ulsch_decode_scrambled

  python tools/slot_chain_scrambled.py [reps]      -> one JSON line, milliseconds per call (mean over reps)

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
G = (12 * 13 - 6) * 273 * 6
n = 64
tbs = [dict(A=A, G=G, BG=1, Qm=6, Nl=1, rv=0, tbslbrm=0, round=0) for _ in range(n)]
rng = np.random.default_rng(1)
scr = [(int(rng.integers(0, 0x10000)), 0, int(rng.integers(0, 1024))) for _ in range(n)]
po, co, ho, segs = m.tb_layout(tbs)
cw, total = m.tb_layout_packed(tbs)
side = torch.cuda.Stream()   # every call is made and captured on this stream
with torch.cuda.stream(side):
    payload = torch.randint(0, 256, (int(po[-1]) + 16,), dtype=torch.uint8, device="cuda")
    coded = torch.zeros(int(co[-1]) + 16, dtype=torch.uint8, device="cuda")
    words = torch.zeros(total // 4 + 4, dtype=torch.int32, device="cuda")
    words2 = torch.zeros_like(words)
    enc = m.PreparedTbBatch(tbs, payload, coded)
    enc_s = m.PreparedTbBatch(tbs, payload, words, scrambling=scr)
    enc.encode()
    llr = ((1.0 - 2.0 * coded.float()) * 10 + 2.0 * torch.randn(coded.numel(), device="cuda")).round().clamp(-127, 127).to(torch.int16)
    llr_plain = llr.clone()                 # what the unscrambled calls decode
    for i, (r, q, nid) in enumerate(scr):   # the received signs of the scrambled codeword
        m.codeword_unscrambling(llr[co[i]:co[i] + G], q, nid, r, size=G)
    llr_work = llr.clone()
    harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
    pay_out = torch.zeros_like(payload)
    ack = torch.zeros(n, dtype=torch.uint8, device="cuda")
    itm = torch.zeros(n, dtype=torch.int32, device="cuda")
    dec = m.PreparedTbBatch(tbs, pay_out, llr_plain, harq, ack, itm)     # baseline: unscrambled LLRs, unscrambled call
    dec_w = m.PreparedTbBatch(tbs, pay_out, llr_work, harq, ack, itm)    # after the separate unscrambling pass
    dec_s = m.PreparedTbBatch(tbs, pay_out, llr, harq, ack, itm, scrambling=scr)


def two_pass_encode():
    enc.encode()
    for i, (r, q, nid) in enumerate(scr):
        m.codeword_scrambling(coded[co[i]:co[i] + G], q, nid, r, out=words2[cw[i] // 4:], size=G)


def two_pass_decode():
    llr_work.copy_(llr)       # (the pass modifies its input: restore it; timed separately below and subtracted)
    for i, (r, q, nid) in enumerate(scr):
        m.codeword_unscrambling(llr_work[co[i]:co[i] + G], q, nid, r, size=G)
    dec_w.decode()


def restore_only():
    llr_work.copy_(llr)


def timed(fn):
    """GPU time per call: the call captured once in a HIP graph, the graph replayed `reps` times between two events (so the
    separate passes' 64 enqueues from Python are not what is measured)"""
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


res = {"reps": reps, "n_tb": n, "G": G}
res["dlsch_encode_ms"] = timed(enc.encode)
res["dlsch_encode_plus_scrambling_ms"] = timed(two_pass_encode)
res["dlsch_encode_scrambled_ms"] = timed(enc_s.encode)
res["ulsch_decode_ms"] = timed(dec.decode)
torch.cuda.synchronize()
res["decode_all_ack"] = bool(ack.cpu().numpy().all())
res["llr_restore_ms"] = timed(restore_only)
res["unscrambling_plus_ulsch_decode_ms"] = timed(two_pass_decode) - res["llr_restore_ms"]
res["ulsch_decode_scrambled_ms"] = timed(dec_s.decode)
torch.cuda.synchronize()
res["decode_scrambled_all_ack"] = bool(ack.cpu().numpy().all())
res["encode_words_equal"] = bool(torch.equal(words, words2))
print(json.dumps(res))
