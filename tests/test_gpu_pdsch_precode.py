"""PDSCH resource mapping with precoding on the GPU (csrc/tb_tx_map.hip through nrLDPC_hip_pdsch_resource_mapping_precoded): DEVICE
and HOST mode against the CPU form of the same header (nrLDPC_hip_pdsch_precode_host, which test_pdsch_precode_host.py holds to the
literal restatement of the reference), bit for bit, with a canary fill that shows the exact write set; all-zero PMIs against the
unit call; the refusals that need a device; payload bytes to txdataF on one stream against the restatement."""
import numpy as np
import pytest

import pdsch_map_np as ref
import pdsch_precode_np as pre
from test_gpu_pdsch_map import CANARY, dl_alloc, mixed_case
from test_gpu_tb_chain import valid_tbs
from test_gpu_tb_scrambled import rand_scr

pytestmark = pytest.mark.gpu

EXTREME = (32767, -32768, -32767)
HOT = 6           # the descriptor with the saturating inputs: no DMRS, 25 RBs, amp 32767


def table_for(rng, Nl):
    """three matrices, found by pm_idx; the last one of extreme weights, half of them real"""
    hot = rng.choice(EXTREME, (Nl, 8, 2))
    hot[..., 1] *= rng.integers(0, 2, (Nl, 8))                         # two full-scale products wrap in the madd more often than they clamp
    w = [rng.integers(-32768, 32768, (Nl, 8, 2)), rng.integers(-20000, 20000, (Nl, 8, 2)), hot]
    return [dict(pm_idx=idx, numLayers=Nl, num_ant_ports=8, weights=w[k].astype(np.int16)) for k, idx in enumerate((11, 3, 500))]


def mixed_precoded(rng, n_tx, Nl, stride4):
    """mixed_case's descriptors (all three patterns and every (pattern, ncdm) of its PORTS with l' = 1 among them, rb_size 1, 2, 3, 5,
    25, 106, fft_size 128, 256, 1536, both wrap positions, every residue of tx_off + start_re and of sym_off mod 4) with prg_size 0, 1,
    2, 3 and wideband in turn, PMI lists with unit PRGs between precoded ones, saturating inputs in descriptor HOT, and an antenna
    stride that is odd or (stride4) a multiple of 4"""
    segs, lay, stride = mixed_case(rng, n_tx, Nl)
    assert stride % 2 == 1
    if stride4:
        stride += 4 - stride % 4
    assert {s["rb_size"] for s in segs} == {1, 2, 3, 5, 25, 106} and {s["fft_size"] for s in segs} == {128, 256, 1536}
    assert {s["pattern"] for s in segs if s["rb_size"] == 106} == {0, 1, 2} and {s["l_prime"] for s in segs} == {0, 1}
    prgs, pmis = [], [500]
    for i, s in enumerate(segs):
        size = (0, 1, 2, 3, s["rb_size"])[i % 5]
        if i == HOT:
            size = 3
        n = -(-s["rb_size"] // size) if size else 0
        prgs.append(dict(prg_size=size, pmi_off=len(pmis), pmi_count=n))
        pmis += [500] * n if i == HOT else [(11, 0, 3, 3, 0, 0, 11)[(q + i) % 7] for q in range(n)]
    assert {g["prg_size"] for g in prgs} >= {0, 1, 2, 3, 25, 106}
    h = segs[HOT]
    assert h["pattern"] == 0 and h["amp"] == 32767
    for l in range(Nl):
        at = h["lay_off"] // 2 + l * h["plane"] + h["sym_off"]
        lay[at:at + h["nb_re"]] = rng.choice(EXTREME, (h["nb_re"], 2))
    return segs, prgs, pmis, lay, stride


def prg_edges_inside_groups(segs, prgs, pmis, stride, n_tx):
    """PRG boundaries between two different PMIs that fall inside a thread's 16-byte group of the grid (the array itself is aligned)"""
    n = 0
    for s, g in zip(segs, prgs):
        if not g["prg_size"]:
            continue
        for q in range(1, g["pmi_count"]):
            i = 12 * g["prg_size"] * q
            if pmis[g["pmi_off"] + q] != pmis[g["pmi_off"] + q - 1] and i < 12 * s["rb_size"]:
                n += sum(1 for a in range(n_tx) if (s["tx_off"] + a * stride + s["start_re"] + i) % 4 and (s["start_re"] + i) % s["fft_size"])
    return n


def host_form(m, segs, prgs, pmis, table, lay, stride, n_tx):
    tx = np.full((n_tx * stride, 2), CANARY, np.int16)
    for s, g in zip(segs, prgs):
        for a in range(n_tx):
            m.pdsch_precode_host(lay, dict(s, tx_off=s["tx_off"] + a * stride), g, pmis, table, n_tx, a, tx)
    return tx


@pytest.mark.parametrize("n_tx,Nl,stride4", [(2, 1, False), (2, 2, True), (4, 2, False), (4, 4, True), (8, 3, False), (3, 2, True)])
def test_precoded_mapping_equals_the_host_form(hip, n_tx, Nl, stride4):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(1300 + 10 * n_tx + Nl)
    segs, prgs, pmis, lay, stride = mixed_precoded(rng, n_tx, Nl, stride4)
    assert (stride % 4 == 0) == stride4
    table = table_for(rng, Nl)
    want = host_form(m, segs, prgs, pmis, table, lay, stride, n_tx)
    written = (want != CANARY).any(-1)
    assert written.sum() >= n_tx * sum(12 * s["rb_size"] for s in segs) - 8 and not written.all()   # a value may equal the canary by chance
    if Nl > 1:                                                         # the hot descriptor clamps in both directions
        h = segs[HOT]
        hot = want.reshape(n_tx, stride, 2)[:, h["tx_off"]:h["tx_off"] + h["fft_size"]]
        assert (hot == 32767).any() and (hot == -32768).any()
    # DEVICE
    tx_d = torch.full((n_tx * stride, 2), CANARY, dtype=torch.int16, device="cuda")
    assert tx_d.data_ptr() % 16 == 0 and prg_edges_inside_groups(segs, prgs, pmis, stride, n_tx) > 0
    m.pdsch_resource_mapping_precoded(torch.from_numpy(lay).cuda(), tx_d, stride, n_tx, segs, prgs, pmis, table)
    torch.cuda.synchronize()
    got = tx_d.cpu().numpy()
    assert np.array_equal(got, want), ("device", n_tx, Nl, np.argwhere(got != want)[:4])
    # HOST
    tx_h = np.full((n_tx * stride, 2), CANARY, np.int16)
    m.pdsch_resource_mapping_precoded(lay, tx_h, stride, n_tx, segs, prgs, pmis, table)
    assert np.array_equal(tx_h, want), ("host", n_tx, Nl, np.argwhere(tx_h != want)[:4])


@pytest.mark.parametrize("n_tx,Nl", [(1, 1), (4, 2), (8, 4)])
def test_all_zero_pmis_equal_the_unit_call(hip, n_tx, Nl):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(77 + n_tx)
    segs, prgs, pmis, lay, stride = mixed_precoded(rng, n_tx, Nl, False)
    zeros = [0] * len(pmis)
    lay_d = torch.from_numpy(lay).cuda()
    unit = torch.full((n_tx * stride, 2), CANARY, dtype=torch.int16, device="cuda")
    got = torch.full((n_tx * stride, 2), CANARY, dtype=torch.int16, device="cuda")
    m.pdsch_resource_mapping(lay_d, unit, stride, n_tx, segs)
    m.pdsch_resource_mapping_precoded(lay_d, got, stride, n_tx, segs, prgs, zeros, None)
    torch.cuda.synchronize()
    assert torch.equal(got, unit) and not bool((unit == CANARY).all())
    got_h = np.full((n_tx * stride, 2), CANARY, np.int16)
    m.pdsch_resource_mapping_precoded(lay, got_h, stride, n_tx, segs, prgs, zeros, None)
    assert np.array_equal(got_h, unit.cpu().numpy())


def test_precoded_mapping_refusals_on_the_device(hip):
    import ctypes as C
    import torch
    m = hip.ldpc
    L = m._pre_lib()
    N = 128
    good = dict(pattern=1, Nl=1, ncdm=1, l_prime=0, port=[0], amp=512, fft_size=N, start_re=100, rb_size=2, nb_re=12, sym_off=0, plane=12,
                dmrs_offset=0, c_init=5, tx_off=0, lay_off=0)
    arr = m._pdm_seg_array([good])
    garr = m._struct_array(m.nrLDPC_hip_pdsch_prg_t, [dict(prg_size=1, pmi_off=0, pmi_count=2)], m._PDM_PRG_KEYS)
    pmis = (C.c_uint16 * 2)(0, 9)
    # antenna 0 = layer 0 times 1/2, antenna 1 = layer 0 times -1/2 in RB 1; RB 0 is unit
    tab, n_pm = m.pdsch_pm_table([dict(pm_idx=9, numLayers=1, num_ant_ports=2, weights=[[(16384, 0), (-16384, 0)]])])
    lay_h, tx_h = np.zeros(64, np.int16), np.full(4 * N, CANARY, np.int16)
    lay_d = torch.zeros(64, dtype=torch.int16, device="cuda")
    tx_d = torch.full((4 * N,), CANARY, dtype=torch.int16, device="cuda")

    def call(lay, tx, stream=None, segs=arr, n=1, n_tx=2, stride=N):
        return L.nrLDPC_hip_pdsch_resource_mapping_precoded(lay, tx, stride, n_tx, segs, garr, n, pmis, 2, tab, n_pm, m.MEM_DEVICE, stream)
    for lay, tx in ((lay_h.ctypes.data, tx_d.data_ptr()), (lay_d.data_ptr(), tx_h.ctypes.data)):
        assert call(lay, tx) < 0 and "device memory" in m.last_error()
    assert call(lay_d.data_ptr(), tx_d.data_ptr() + 2) < 0 and "4-byte" in m.last_error()
    assert call(lay_d.data_ptr() + 2, tx_d.data_ptr()) < 0 and "4-byte" in m.last_error()
    assert call(lay_d.data_ptr(), tx_d.data_ptr(), segs=m._pdm_seg_array([dict(good, pattern=5)])) < 0 and "pattern must be" in m.last_error()
    assert call(lay_d.data_ptr(), tx_d.data_ptr(), stride=20) < 0 and "overlap" in m.last_error()      # across antennas through a short stride
    assert call(lay_d.data_ptr(), tx_d.data_ptr(), n_tx=1) < 0 and "at least 2" in m.last_error()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    note = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        note.add_(1)
        rc = call(lay_d.data_ptr(), tx_d.data_ptr(), stream=side.cuda_stream)
        err = m.last_error()
    assert rc < 0 and "captured" in err
    torch.cuda.synchronize()
    assert bool((tx_d == CANARY).all()), "a refused call writes nothing"
    # and the good call runs: the layer is zeros, so its data REs are 0 and its pilots +-256; RB 0 is unit (antenna 1 zeros), RB 1 is
    # halved with the sign flipped on antenna 1
    assert call(lay_d.data_ptr(), tx_d.data_ptr()) == 0
    torch.cuda.synchronize()
    out = tx_d.cpu().numpy().reshape(2, N, 2)
    assert np.all(out[:, :100] == CANARY) and np.all(out[:, 124:] == CANARY)
    assert np.all(np.abs(out[0, 100:112:2]) == 256) and np.all(out[0, 101:124:2] == 0) and np.all(out[1, 100:112] == 0)
    assert np.all(np.abs(out[0, 112:124:2]) == 128) and np.all(out[1, 112:124:2] == -out[0, 112:124:2]) and np.all(out[1, 113:124:2] == 0)


def test_payload_to_precoded_txdataf_on_one_stream(hip):
    """dlsch_encode_symbols -> pdsch_resource_mapping_precoded on one non-default stream for two transport blocks of two layers on four
    antennas, 14 symbols, one DMRS type each, against the restatement (mapping without the defects, every precoded RE by the SIMD
    definition) fed with the separately checked encode_symbols output"""
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(4243)
    N, n_tx = 512, 4
    shapes = [dict(Nl=2, Qm=2, BG=2, rb=3, k0=N - 20, typ=0, ncdm=1, ports=0b11, pos=1 << 2, data=13 * 12 + 6, prg=2, pmis=[1, 0]),
              dict(Nl=2, Qm=6, BG=1, rb=5, k0=40, typ=1, ncdm=2, ports=0b1100, pos=0b11 << 3, data=12 * 12 + 2 * 4, prg=1, pmis=[2, 2, 0, 1, 2])]
    tbs = []
    for h in shapes:
        S = h["data"] * h["rb"]
        G = h["Qm"] * h["Nl"] * S
        tbs.append(dict(A=valid_tbs(G // 2, h["BG"]), G=G, BG=h["BG"], Qm=h["Qm"], Nl=h["Nl"], rv=0, tbslbrm=0))
    n = len(tbs)
    scr = rand_scr(rng, n)
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    po = m.tb_layout(tbs)[0]
    co, total = m.tb_layout_symbols(tbs)
    allocs = [dl_alloc(N, h["rb"], h["k0"], h["Nl"], h["typ"], h["ncdm"], h["ports"], h["pos"], h["data"] * h["rb"], 3 + i, 77 + i, i, 700 + 300 * i,
                       i * 14 * N + 1 + i, int(co[i]) // 2) for i, h in enumerate(shapes)]
    pmis = shapes[0]["pmis"] + shapes[1]["pmis"]
    alloc_prgs = [dict(prg_size=shapes[0]["prg"], pmi_off=0, pmi_count=2), dict(prg_size=shapes[1]["prg"], pmi_off=2, pmi_count=5)]
    table = [dict(pm_idx=t + 1, numLayers=2, num_ant_ports=4, weights=[[tuple(int(v) for v in rng.integers(-23170, 23171, 2)) for _ in range(4)] for _ in range(2)])
             for t in range(2)]
    segs, prgs = m.pdsch_precode_segments(allocs, alloc_prgs, len(pmis))
    assert len(segs) == 28 and prgs == [alloc_prgs[0]] * 14 + [alloc_prgs[1]] * 14
    stride = n * 14 * N + 7
    planes = m.dlsch_encode_symbols_host(tbs, pays, scr)
    want = np.full((n_tx, stride, 2), CANARY, np.int16)
    for i, a in enumerate(allocs):
        mapped, used = ref.pdsch_resource_mapping(a, [[(int(r), int(q)) for r, q in planes[i][l]] for l in range(a["Nl"])], a["Nl"], literal_tail=False,
                                                  literal_allowed=False, fill=None)
        assert used == [a["plane"]] * a["Nl"]
        g = alloc_prgs[i]
        tx, _ = pre.precode_all_simd(a, mapped, n_tx, g["prg_size"], pmis[g["pmi_off"]:g["pmi_off"] + g["pmi_count"]], table, fill=None)
        for ant in range(n_tx):
            for sym in range(14):
                for k, v in enumerate(tx[ant][sym]):
                    if v is not None:
                        want[ant, a["tx_slot_off"] + sym * N + k] = v
    pay_h = np.zeros(int(po[-1]) + 16, np.uint8)
    for i, t in enumerate(tbs):
        pay_h[po[i]:po[i] + t["A"] // 8] = pays[i]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pay_d = torch.from_numpy(pay_h).cuda()
        lay_d = torch.zeros(total // 2 + 8, dtype=torch.int16, device="cuda")
        tx_d = torch.full((n_tx * stride, 2), CANARY, dtype=torch.int16, device="cuda")
        m.dlsch_encode_symbols_device(tbs, pay_d, lay_d, scr, stream=side.cuda_stream)
        m.pdsch_resource_mapping_precoded(lay_d, tx_d, stride, n_tx, segs, prgs, pmis, table, stream=side.cuda_stream)
    torch.cuda.synchronize()
    got = tx_d.cpu().numpy().reshape(n_tx, stride, 2)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
