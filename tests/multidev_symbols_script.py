"""Helper of test_gpu_qam.py::test_decode_symbols_sharded_over_logical_devices (run in a subprocess, so that NRLDPC_HIP_DEVICES
is read by a fresh library): nrLDPC_hip_ulsch_decode_symbols on host buffers over two HARQ rounds; dumps every output to
argv[1] (.npz), with `ok` = whether each round equals ulsch_llr + the scrambled LLR call of the same process."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import openairinterface5g_amd as hip  # noqa: E402
from test_gpu_tb_chain import make_tbs  # noqa: E402
from test_gpu_qam import rx_symbols  # noqa: E402

hip.LDPCinit()
m = hip.ldpc
rng = np.random.default_rng(4343)
res = {}
tbs = make_tbs() + make_tbs()[:5]
scr = [(int(rng.integers(0, 0x10000)), int(rng.integers(0, 2)), int(rng.integers(0, 1024))) for _ in tbs]
pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
tx = m.dlsch_encode_scrambled_host(tbs, pays, scr)
segs = [m.nr_segmentation(t["A"] + (24 if t["A"] > 3824 else 16), t["BG"])["C"] for t in tbs]
harq_a = np.zeros((sum(segs), m.HARQ_STRIDE), np.int16)
harq_b = harq_a.copy()
rx_a = [dict(t) for t in tbs]
rx_b = [dict(t) for t in tbs]
ok = []
for rnd in range(2):
    syms = [rx_symbols(rng, w, t["G"], t["Qm"], 0.45 if rnd == 0 else 0.25) for w, t in zip(tx, tbs)]
    recs = m.pack_symbol_records([[y] + mg for y, mg in syms])
    llrs = [m.ulsch_llr(y, mg, t["Qm"]) for (y, mg), t in zip(syms, tbs)]
    for t in rx_a + rx_b:
        t["round"] = rnd
    pa, aa, ia = m.ulsch_decode_symbols_host(rx_a, recs, harq_a, scr)
    pb, ab, ib = m.ulsch_decode_scrambled_host(rx_b, llrs, harq_b, scr)
    ok.append(all(np.array_equal(x, y) for x, y in zip(pa, pb)) and np.array_equal(aa, ab) and np.array_equal(ia, ib) and
              np.array_equal(harq_a, harq_b) and [t["llrLen"] for t in rx_a] == [t["llrLen"] for t in rx_b])
    res[f"rx{rnd}_pay"] = np.concatenate(pa)
    res[f"rx{rnd}_ack"], res[f"rx{rnd}_itm"] = np.asarray(aa), np.asarray(ia)
    res[f"rx{rnd}_harq"] = harq_a.copy()
res["llr_len"] = np.array([t["llrLen"] for t in rx_a])
res["ok"] = np.array(ok)
np.savez(sys.argv[1], **res)
