"""Helper of test_gpu_tb_scrambled.py::test_decode_scrambled_sharded_over_logical_devices (run in a subprocess, so that
NRLDPC_HIP_DEVICES is read by a fresh library): the scrambled chain calls on host buffers over two HARQ rounds; dumps every
output to argv[1] (.npz), with `ok` = whether each round equals unscrambling + the unscrambled call of the same process."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import openairinterface5g_amd as hip  # noqa: E402
from test_gpu_tb_chain import make_tbs  # noqa: E402

hip.LDPCinit()
m = hip.ldpc
rng = np.random.default_rng(4242)
res = {}
tbs = make_tbs() + make_tbs()[:5]
scr = [(int(rng.integers(0, 0x10000)), int(rng.integers(0, 2)), int(rng.integers(0, 1024))) for _ in tbs]
pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
res["tx"] = np.concatenate(m.dlsch_encode_scrambled_host(tbs, pays, scr))
f = m.dlsch_encode_host(tbs, pays)
segs = [m.nr_segmentation(t["A"] + (24 if t["A"] > 3824 else 16), t["BG"])["C"] for t in tbs]
harq_a = np.zeros((sum(segs), m.HARQ_STRIDE), np.int16)
harq_b = harq_a.copy()
rx_a = [dict(t) for t in tbs]
rx_b = [dict(t) for t in tbs]
ok = []
for rnd in range(2):
    llrs = []
    for t, c, (n_rnti, q, n_id) in zip(rx_a, f, scr):
        y = (1.0 - 2.0 * c.astype(np.float64) + (1.1 if rnd == 0 else 0.6) * rng.standard_normal(c.size)) * 8.0
        x = np.clip(np.rint(y), -127, 127).astype(np.int16)
        m.codeword_unscrambling(x, q, n_id, n_rnti)         # (an involution: this scrambles the signs)
        llrs.append(x)
    for t in rx_a + rx_b:
        t["round"] = rnd
    ref = [x.copy() for x in llrs]
    for x, (n_rnti, q, n_id) in zip(ref, scr):
        m.codeword_unscrambling(x, q, n_id, n_rnti)
    pa, aa, ia = m.ulsch_decode_scrambled_host(rx_a, llrs, harq_a, scr)
    pb, ab, ib = m.ulsch_decode_host(rx_b, ref, harq_b)
    ok.append(all(np.array_equal(x, y) for x, y in zip(pa, pb)) and np.array_equal(aa, ab) and np.array_equal(ia, ib) and
              np.array_equal(harq_a, harq_b) and [t["llrLen"] for t in rx_a] == [t["llrLen"] for t in rx_b])
    res[f"rx{rnd}_pay"] = np.concatenate(pa)
    res[f"rx{rnd}_ack"], res[f"rx{rnd}_itm"] = np.asarray(aa), np.asarray(ia)
    res[f"rx{rnd}_harq"] = harq_a.copy()
res["llr_len"] = np.array([t["llrLen"] for t in rx_a])
res["ok"] = np.array(ok)
np.savez(sys.argv[1], **res)
