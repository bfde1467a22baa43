#!/usr/bin/env python3
"""One slot's 64 transport blocks (273 PRB x 13 symbols, 64QAM, one layer, N = 4096, one type-1 DMRS symbol per block, n_tx = 4:
three antennas behind the layer receive zeros) from layer planes in device memory onto the transmit grid:
nrLDPC_hip_pdsch_resource_mapping, in one process, timed with HIP events.

  python tools/slot_tx_map.py [reps]      -> one JSON line; times in milliseconds (mean, median, min, max over reps)

The call refuses a capturing stream, so nothing is replayed from a graph: every timed call is enqueued behind a filler (four
encode calls) that keeps the GPU busy while the host enqueues, and the events around it see GPU time -- the descriptor upload
and the kernels -- not the host's enqueueing.  (That holds while the filler outlasts the host: on the first hardware run it did
not, the calls' plans for 832 descriptors take the host longer than four encode launches take the GPU, and the events measured
the enqueue; profiles/r13/README.md has the kernel times from a trace beside them.)  The legs alternate inside one loop so that they see the same machine:

  mapping                    the mapping call alone (three launches: the patterns FULL and DMRS1 are present)
  device_copy                a plain device copy that reads the bytes the call reads (4 per data RE of the layer) and writes
                             the bytes it writes (4 per RE and antenna)
  encode_symbols             the slot's dlsch_encode_symbols, the figure the mapping is small or large against

The precoding arm, in the same loop: the same slot with two layers per block (Nl = 2, ports 0 and 1, layer planes of random
values), n_tx = 4, prg_size = 2 and PMIs 1, 2, 1, ... (none 0) through two 2 x 4 matrices:

  precoded                   nrLDPC_hip_pdsch_resource_mapping_precoded
  unit_same_descriptors      nrLDPC_hip_pdsch_resource_mapping with n_tx = 4 on the same descriptors: the same bytes written
  copy_of_bytes_written      a plain device copy of as many bytes as either call writes

Before timing, each chain runs once and the grid of one block is compared with the host form's.
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
LM = m._pdm_lib()
A = 213176
while m.nr_segmentation(A + 24, 1) is None:
    A += 8
Qm, n_tx, n, rb, N = 6, 4, 64, 273, 4096
S = (12 * 12 + 6) * rb                        # 13 symbols, symbol 2 a type-1 DMRS symbol with half the REs
G = S * Qm
tbs = [dict(A=A, G=G, BG=1, Qm=Qm, Nl=1, rv=0, tbslbrm=0) for _ in range(n)]
rng = np.random.default_rng(1)
scr = [(int(rng.integers(0, 0x10000)), 0, int(rng.integers(0, 1024))) for _ in range(n)]
po = m.tb_layout(tbs)[0]
co, total = m.tb_layout_symbols(tbs)
allocs = [dict(Nl=1, plane=S, dmrs_config_type=0, num_dmrs_cdm_grps_no_data=1, dmrs_ports=1, scid=i & 1, dl_dmrs_scrambling_id=int(rng.integers(0, 65536)),
               slot=i % 20, si_rnti=0, amp=512, fft_size=N, first_carrier_offset=N - 6 * rb, bwp_start=0, rb_start=0, rb_size=rb, start_symbol=0,
               nr_of_symbols=13, dl_dmrs_symb_pos=1 << 2, tx_slot_off=i * 14 * N, lay_off=int(co[i]) // 2) for i in range(n)]
segs = m.pdsch_map_segments(allocs)
assert len(segs) == 13 * n
seg_arr = m._pdm_seg_array(segs)
stride = n * 14 * N
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    payload = torch.randint(0, 256, (int(po[-1]) + 16,), dtype=torch.uint8, device="cuda")
    layers = torch.zeros(total // 2 + 8, dtype=torch.int16, device="cuda")
    tx = torch.zeros(n_tx, stride, 2, dtype=torch.int16, device="cuda")
    bytes_read, bytes_written = n * S * 4, n * n_tx * 13 * 12 * rb * 4
    copy_src = torch.zeros(max(bytes_read, bytes_written), dtype=torch.uint8, device="cuda")
    copy_dst = torch.zeros(bytes_written, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
s_ptr = side.cuda_stream


def encode_symbols():
    m.dlsch_encode_symbols_device(tbs, payload, layers, scr, stream=s_ptr)


def mapping():
    assert LM.nrLDPC_hip_pdsch_resource_mapping(layers.data_ptr(), tx.data_ptr(), stride, n_tx, seg_arr, len(segs), m.MEM_DEVICE, s_ptr) == 0, m.last_error()


def device_copy():
    copy_dst[:bytes_read].copy_(copy_src[:bytes_read])       # as many bytes read as the layer planes hold
    copy_dst[bytes_read:].fill_(0)                           # the rest is written without a read: pilots and zero planes


# ---- the precoding arm ----
LP = m._pre_lib()
Nl2 = 2
allocs2 = [dict(a, Nl=Nl2, dmrs_ports=0b11, lay_off=2 * i * Nl2 * S) for i, a in enumerate(allocs)]
n_prg = (rb + 1) // 2
pmis = [1 + (q & 1) for q in range(n_prg)] * n
segs2, prgs2 = m.pdsch_precode_segments(allocs2, [dict(prg_size=2, pmi_off=i * n_prg, pmi_count=n_prg) for i in range(n)], len(pmis))
assert len(segs2) == 13 * n
seg2_arr = m._pdm_seg_array(segs2)
prg2_arr = m._struct_array(m.nrLDPC_hip_pdsch_prg_t, prgs2, m._PDM_PRG_KEYS)
pmi_arr = np.ascontiguousarray(pmis, np.uint16)
table = [dict(pm_idx=t + 1, numLayers=Nl2, num_ant_ports=n_tx, weights=rng.integers(-16384, 16385, (Nl2, n_tx, 2)).astype(np.int16)) for t in range(2)]
pm_arr, n_pm = m.pdsch_pm_table(table)
with torch.cuda.stream(side):
    layers2 = torch.randint(-32768, 32768, (n * Nl2 * S, 2), dtype=torch.int16, device="cuda")
    tx2 = torch.zeros(n_tx, stride, 2, dtype=torch.int16, device="cuda")
    written_src = torch.zeros(bytes_written, dtype=torch.uint8, device="cuda")
    written_dst = torch.zeros(bytes_written, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()


def precoded():
    assert LP.nrLDPC_hip_pdsch_resource_mapping_precoded(layers2.data_ptr(), tx2.data_ptr(), stride, n_tx, seg2_arr, prg2_arr, len(segs2), pmi_arr.ctypes.data,
                                                         len(pmis), pm_arr, n_pm, m.MEM_DEVICE, s_ptr) == 0, m.last_error()


def unit_same_descriptors():
    assert LM.nrLDPC_hip_pdsch_resource_mapping(layers2.data_ptr(), tx2.data_ptr(), stride, n_tx, seg2_arr, len(segs2), m.MEM_DEVICE, s_ptr) == 0, m.last_error()


def copy_of_bytes_written():
    written_dst.copy_(written_src)


def filler():
    for _ in range(4):
        encode_symbols()


with torch.cuda.stream(side):
    encode_symbols()
    mapping()
torch.cuda.synchronize()
i0 = n // 2
lay_h, got = layers.cpu().numpy().reshape(-1, 2), tx.cpu().numpy()
want = np.zeros((n_tx, stride, 2), np.int16)
for s in segs[13 * i0:13 * i0 + 13]:
    for a in range(n_tx):
        m.pdsch_map_host(lay_h, s, 0 if a == 0 else -1, want[a])
lo, hi = i0 * 14 * N, (i0 + 1) * 14 * N
res = {"reps": reps, "n_tb": n, "n_tx": n_tx, "Nl": 1, "Qm": Qm, "fft_size": N, "rb": rb, "descriptors": len(segs),
       "device_equals_host_form": bool(np.array_equal(got[:, lo:hi], want[:, lo:hi])), "bytes_read": bytes_read, "bytes_written": bytes_written}
with torch.cuda.stream(side):
    precoded()
torch.cuda.synchronize()
lay2_h, got2 = layers2.cpu().numpy(), tx2.cpu().numpy()
want2 = np.zeros((n_tx, stride, 2), np.int16)
for s, g in zip(segs2[13 * i0:13 * i0 + 13], prgs2[13 * i0:13 * i0 + 13]):
    for a in range(n_tx):
        m.pdsch_precode_host(lay2_h, s, g, pmis, table, n_tx, a, want2[a])
res.update({"precoded_Nl": Nl2, "precoded_prg_size": 2, "precoded_equals_host_form": bool(np.array_equal(got2[:, lo:hi], want2[:, lo:hi])),
            "precoded_block_is_not_zero": bool(want2[:, lo:hi].any())})
legs = {"mapping": mapping, "device_copy": device_copy, "encode_symbols": encode_symbols, "precoded": precoded,
        "unit_same_descriptors": unit_same_descriptors, "copy_of_bytes_written": copy_of_bytes_written}
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
for k, v in ts.items():
    res[k + "_ms"] = {"mean": float(np.mean(v)), "median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    res[k + "_spread"] = (float(np.max(v)) - float(np.min(v))) / float(np.mean(v))
for k in ("mapping", "device_copy"):
    res[k + "_share_of_hbm_peak"] = {"median": (bytes_read + bytes_written) / (float(np.median(ts[k])) * 1e-3) / HBM_PEAK}
med = lambda k: float(np.median(ts[k]))
res["mapping_over_copy"] = {"median": med("mapping") / med("device_copy"), "min": float(np.min(ts["mapping"]) / np.min(ts["device_copy"]))}
res["mapping_over_encode"] = {"median": med("mapping") / med("encode_symbols")}
for k in ("precoded", "unit_same_descriptors", "copy_of_bytes_written"):
    res[k + "_bytes_written_share_of_hbm_peak"] = {"median": bytes_written / (med(k) * 1e-3) / HBM_PEAK}
res["precoded_over_unit"] = {"median": med("precoded") / med("unit_same_descriptors"), "min": float(np.min(ts["precoded"]) / np.min(ts["unit_same_descriptors"]))}
res["precoded_over_copy"] = {"median": med("precoded") / med("copy_of_bytes_written"), "min": float(np.min(ts["precoded"]) / np.min(ts["copy_of_bytes_written"]))}
print(json.dumps(res))
