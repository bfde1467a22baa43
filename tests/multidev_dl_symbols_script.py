"""Helper of test_gpu_dl_symbols.py::test_encode_symbols_sharded_over_logical_devices (run in a subprocess, so that
NRLDPC_HIP_DEVICES is read by a fresh library): nrLDPC_hip_dlsch_encode_symbols on host and on device buffers; dumps every
output to argv[1] (.npz), with `ok` = whether each equals the numpy definition (scrambling, modulation, layer mapping)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import torch  # noqa: E402
import openairinterface5g_amd as hip  # noqa: E402
from layer_np import symbols_np  # noqa: E402
from test_gpu_tb_chain import make_tbs  # noqa: E402

hip.LDPCinit()
m = hip.ldpc
rng = np.random.default_rng(4545)
tbs = make_tbs() + make_tbs()[:5]
scr = [(int(rng.integers(0, 0x10000)), int(rng.integers(0, 2)), int(rng.integers(0, 1024))) for _ in tbs]
pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
want = [symbols_np(f, s, t["Qm"], t["Nl"]) for f, s, t in zip(m.dlsch_encode_host(tbs, pays), scr, tbs)]
res, ok = {}, []
host = m.dlsch_encode_symbols_host(tbs, pays, scr)
ok.append(all(np.array_equal(a, b) for a, b in zip(host, want)))
res["host"] = np.concatenate([h.reshape(-1) for h in host])
po, _, _, _ = m.tb_layout(tbs)
cs, total = m.tb_layout_symbols(tbs)
pay_h = np.zeros(int(po[-1]) + 16, np.uint8)
for i, t in enumerate(tbs):
    pay_h[po[i]:po[i] + t["A"] // 8] = pays[i]
coded = torch.full((total // 4 + 4,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
m.dlsch_encode_symbols_device(tbs, torch.from_numpy(pay_h).cuda(), coded, scr)
torch.cuda.synchronize()
dev = coded.cpu().numpy().view(np.uint32)
ok.append(all(np.array_equal(dev[cs[i] // 4:cs[i] // 4 + t["G"] // t["Qm"]].view(np.int16).reshape(want[i].shape), want[i])
              for i, t in enumerate(tbs)))
res["device"] = dev
res["ok"] = np.array(ok)
np.savez(sys.argv[1], **res)
