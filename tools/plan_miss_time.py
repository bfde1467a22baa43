#!/usr/bin/env python3
"""Time of a DL / UL chain call whose plan is NOT in the cache: 32 descriptor arrays (one rv / numMaxIter differs) cycled through the
24-slot LRU cache, so every call builds and uploads its plan.  64-TB slot of bench_extra config4/5, device buffers."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
import openairinterface5g_amd as pkg  # noqa: E402

m = pkg.ldpc
pkg.LDPCinit()
A = 213176
while m.nr_segmentation(A + 24, 1) is None:
    A += 8
G = (12 * 13 - 6) * 273 * 6
tbs = [dict(A=A, G=G, BG=1, Qm=6, Nl=1, rv=0, tbslbrm=0, round=0) for _ in range(64)]
po, co, ho, segs = m.tb_layout(tbs)
payload = torch.randint(0, 256, (int(po[-1]) + 16,), dtype=torch.uint8, device="cuda")
coded = torch.zeros(int(co[-1]) + 16, dtype=torch.uint8, device="cuda")
enc = []
for j in range(32):
    t = [dict(x) for x in tbs]
    t[j]["rv"] = 2
    enc.append(m.PreparedTbBatch(t, payload, coded))
base = m.PreparedTbBatch(tbs, payload, coded)
base.encode()
torch.cuda.synchronize()
llr = ((1.0 - 2.0 * coded.float()) * 10).round().to(torch.int16)
harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
pay_out = torch.zeros_like(payload)
ack = torch.zeros(64, dtype=torch.uint8, device="cuda")
itm = torch.zeros(64, dtype=torch.int32, device="cuda")
dec = []
for j in range(32):
    t = [dict(x) for x in tbs]
    t[j]["numMaxIter"] = 9
    dec.append(m.PreparedTbBatch(t, pay_out, llr, harq, ack, itm))


def cycle(batches, fn, rounds):
    for b in batches:          # warm: code tables, buffers; fills the cache with the LAST 24, so the next call misses
        fn(b)
    torch.cuda.synchronize()
    host = []
    t0 = time.perf_counter()
    for _ in range(rounds):
        for b in batches:
            h0 = time.perf_counter()
            fn(b)
            host.append(time.perf_counter() - h0)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (rounds * len(batches)) * 1e3, sorted(host)[len(host) // 2] * 1e3


e_ms, e_host = cycle(enc, lambda b: b.encode(), 6)
d_ms, d_host = cycle(dec, lambda b: b.decode(), 6)
print(json.dumps({"lib": str(m.load_library()._name), "dl_miss_ms_per_call": e_ms, "dl_miss_host_ms_median": e_host,
                  "ul_miss_ms_per_call": d_ms, "ul_miss_host_ms_median": d_host}))
