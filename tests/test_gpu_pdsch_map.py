"""PDSCH resource mapping with DMRS on the GPU (csrc/tb_tx_map.hip through nrLDPC_hip_pdsch_resource_mapping): DEVICE and HOST mode
against the CPU form of the same header (nrLDPC_hip_pdsch_map_host, which test_pdsch_map_host.py holds to the literal restatement of
the reference), bit for bit, with a canary fill that shows the exact write set; the refusals that need a device; payload bytes to
txdataF on one stream against the restatement; and a loop-back of the mapped grid through the UL receive front to payload bytes."""
import numpy as np
import pytest

import pdsch_map_np as ref
from test_gpu_tb_chain import valid_tbs
from test_gpu_tb_scrambled import rand_scr

pytestmark = pytest.mark.gpu

CANARY = 0x5a5a
FULL, DMRS1, DMRS2 = 0, 1, 2
# ports with the same number of data REs for 1..4 layers: (pattern, ncdm) -> ports, data REs per PRB
PORTS = {(DMRS1, 1): ([0, 1, 4, 5], 6), (DMRS1, 2): ([2, 0, 7, 1], 0), (DMRS2, 1): ([1, 0, 6, 7], 8), (DMRS2, 2): ([2, 3, 8, 9], 4),
         (DMRS2, 3): ([4, 0, 11, 3], 0), (FULL, 0): ([0, 0, 0, 0], 12)}


def mixed_case(rng, n_tx, Nl):
    """descriptors of all three patterns, rb_size 1, 2, 3, 5, 25 and 106 (106 RBs = 1272 REs: two pieces per antenna), both wrap
    positions (inside a 4-RE group / PRB and between PRBs), every residue of tx_off + start_re and of sym_off mod 4, fft_size 1536
    and the fft_size = 256, type 2, two groups, delta = 2 case of the reference's first-subcarrier defect, l' = 1, an odd antenna
    stride (the phase differs per antenna)"""
    shapes = [(FULL, 0, 1, 1536, 0), (DMRS1, 1, 2, 1536, 1535), (DMRS2, 1, 3, 1536, 1536 - 7), (FULL, 0, 5, 1536, 1536 - 6), (DMRS1, 2, 25, 1536, 1536 - 146),
              (DMRS2, 2, 25, 1536, 1536 - 36), (FULL, 0, 25, 1536, 501), (DMRS2, 3, 25, 1536, 1536 - 150), (FULL, 0, 106, 1536, 1536 - 636),
              (DMRS1, 1, 106, 1536, 1536 - 634), (DMRS2, 2, 106, 1536, 130), (FULL, 0, 106, 1536, 1536 - 7), (DMRS1, 1, 2, 1536, 1536 - 24),
              (DMRS2, 2, 3, 256, 256 - 7), (DMRS2, 2, 5, 256, 0), (FULL, 0, 3, 128, 126), (DMRS1, 1, 5, 1536, 7), (FULL, 0, 2, 256, 253)]
    slot = 1536 + 4
    segs, lay_at = [], 2
    for i, (pattern, ncdm, rb, N, k0) in enumerate(shapes):
        ports, per_rb = PORTS[(pattern, ncdm)]
        nb_re, sym_off = per_rb * rb, (i * 7) % 4 + (i % 3)
        plane = sym_off + nb_re + (i % 2)
        segs.append(dict(pattern=pattern, Nl=Nl, ncdm=ncdm, l_prime=(i >> 1) & 1 if pattern else 0, port=ports[:Nl] if pattern else [], amp=(1, 512, 32767, 9000)[i % 4],
                         fft_size=N, start_re=k0, rb_size=rb, nb_re=nb_re, sym_off=sym_off, plane=plane, dmrs_offset=int(rng.integers(0, 900)) if pattern else 0,
                         c_init=int(rng.integers(0, 1 << 31)) if pattern else 0, tx_off=i * slot + (i % 4), lay_off=2 * lay_at))
        lay_at += Nl * plane + (i % 3)
    assert {(s["tx_off"] + s["start_re"]) % 4 for s in segs} == {0, 1, 2, 3} and {s["sym_off"] % 4 for s in segs} == {0, 1, 2, 3}
    stride = len(shapes) * slot + 5
    lay = rng.integers(-32768, 32768, (lay_at + 4, 2)).astype(np.int16)
    lay[::7] = rng.choice([32767, -32768], (len(lay[::7]), 2))
    return segs, lay, stride


def host_form(m, segs, lay, stride, n_tx):
    tx = np.full((n_tx * stride, 2), CANARY, np.int16)
    for s in segs:
        for a in range(n_tx):
            m.pdsch_map_host(lay, dict(s, tx_off=s["tx_off"] + a * stride), a if a < s["Nl"] else -1, tx)
    return tx


@pytest.mark.parametrize("n_tx,Nl", [(1, 1), (2, 2), (4, 4), (3, 2), (2, 1)])
def test_mapping_equals_the_host_form(hip, n_tx, Nl):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(900 + 10 * n_tx + Nl)
    segs, lay, stride = mixed_case(rng, n_tx, Nl)
    want = host_form(m, segs, lay, stride, n_tx)
    written = (want != CANARY).any(-1)
    assert written.sum() >= n_tx * sum(12 * s["rb_size"] for s in segs) - 8 and not written.all()   # a value may equal the canary by chance
    # DEVICE
    tx_d = torch.full((n_tx * stride, 2), CANARY, dtype=torch.int16, device="cuda")
    m.pdsch_resource_mapping(torch.from_numpy(lay).cuda(), tx_d, stride, n_tx, segs)
    torch.cuda.synchronize()
    got = tx_d.cpu().numpy()
    assert np.array_equal(got, want), ("device", n_tx, Nl, np.argwhere(got != want)[:4])
    # HOST
    tx_h = np.full((n_tx * stride, 2), CANARY, np.int16)
    m.pdsch_resource_mapping(lay, tx_h, stride, n_tx, segs)
    assert np.array_equal(tx_h, want), ("host", n_tx, Nl, np.argwhere(tx_h != want)[:4])


def test_mapping_refusals_on_the_device(hip):
    import torch
    m = hip.ldpc
    L = m._pdm_lib()
    N = 128
    good = dict(pattern=DMRS1, Nl=1, ncdm=1, l_prime=0, port=[0], amp=512, fft_size=N, start_re=100, rb_size=2, nb_re=12, sym_off=0, plane=12,
                dmrs_offset=0, c_init=5, tx_off=0, lay_off=0)
    arr = m._pdm_seg_array([good])
    lay_h, tx_h = np.zeros(64, np.int16), np.full(4 * N, CANARY, np.int16)
    lay_d = torch.zeros(64, dtype=torch.int16, device="cuda")
    tx_d = torch.full((4 * N,), CANARY, dtype=torch.int16, device="cuda")

    def call(lay, tx, stream=None, segs=arr, n=1, n_tx=2, stride=N):
        return L.nrLDPC_hip_pdsch_resource_mapping(lay, tx, stride, n_tx, segs, n, m.MEM_DEVICE, stream)
    for lay, tx in ((lay_h.ctypes.data, tx_d.data_ptr()), (lay_d.data_ptr(), tx_h.ctypes.data)):
        assert call(lay, tx) < 0 and "device memory" in m.last_error()
    assert call(lay_d.data_ptr(), tx_d.data_ptr() + 2) < 0 and "4-byte" in m.last_error()
    assert call(lay_d.data_ptr() + 2, tx_d.data_ptr()) < 0 and "4-byte" in m.last_error()
    assert call(lay_d.data_ptr(), tx_d.data_ptr(), segs=m._pdm_seg_array([dict(good, pattern=5)])) < 0 and "pattern must be" in m.last_error()
    assert call(lay_d.data_ptr(), tx_d.data_ptr(), stride=20) < 0 and "overlap" in m.last_error()      # across antennas through a short stride
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
    # and the good call runs: antenna 0 maps the layer (zeros: the data REs are 0, the pilots +-256), antenna 1 receives zeros
    assert call(lay_d.data_ptr(), tx_d.data_ptr()) == 0
    torch.cuda.synchronize()
    out = tx_d.cpu().numpy().reshape(2, N, 2)
    assert np.all(out[:, :100] == CANARY) and np.all(out[:, 124:] == CANARY)
    assert np.all(np.abs(out[0, 100:124:2]) == 256) and np.all(out[0, 101:124:2] == 0) and np.all(out[1, 100:124] == 0)


def dl_alloc(N, rb, k0, Nl, typ, ncdm, ports, symb_pos, plane, slot, nid, scid, amp, tx_slot_off, lay_off, rb_start=2, bwp_start=1):
    return dict(Nl=Nl, plane=plane, dmrs_config_type=typ, num_dmrs_cdm_grps_no_data=ncdm, dmrs_ports=ports, scid=scid, dl_dmrs_scrambling_id=nid, slot=slot,
                si_rnti=0, rnti=0x1234, amp=amp, fft_size=N, first_carrier_offset=(k0 - 12 * (rb_start + bwp_start)) % N, bwp_start=bwp_start,
                rb_start=rb_start, rb_size=rb, start_symbol=0, nr_of_symbols=14, dl_dmrs_symb_pos=symb_pos, tx_slot_off=tx_slot_off, lay_off=lay_off)


def test_payload_to_txdataf_on_one_stream(hip):
    """dlsch_encode_symbols -> pdsch_resource_mapping on one non-default stream, nothing but descriptors crossing the link and no
    synchronisation in between, against the numpy restatement (defects off) fed with the separately checked encode_symbols output"""
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(4242)
    N = 512
    shapes = [dict(Nl=1, Qm=2, BG=2, rb=3, k0=N - 20, typ=0, ncdm=1, ports=0b1, pos=1 << 2, data=13 * 12 + 6),
              dict(Nl=2, Qm=6, BG=1, rb=5, k0=40, typ=1, ncdm=2, ports=0b1100, pos=0b11 << 3, data=12 * 12 + 2 * 4)]
    tbs = []
    for h in shapes:
        S = h["data"] * h["rb"]
        G = h["Qm"] * h["Nl"] * S
        tbs.append(dict(A=valid_tbs(G // 2, h["BG"]), G=G, BG=h["BG"], Qm=h["Qm"], Nl=h["Nl"], rv=0, tbslbrm=0))
    n, n_tx = len(tbs), 3
    scr = rand_scr(rng, n)
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    po = m.tb_layout(tbs)[0]
    co, total = m.tb_layout_symbols(tbs)
    allocs = [dl_alloc(N, h["rb"], h["k0"], h["Nl"], h["typ"], h["ncdm"], h["ports"], h["pos"], h["data"] * h["rb"], 3 + i, 77 + i, i, 700 + 300 * i,
                       i * 14 * N + 1 + i, int(co[i]) // 2) for i, h in enumerate(shapes)]
    segs = m.pdsch_map_segments(allocs)
    assert len(segs) == 28
    stride = n * 14 * N + 7
    # the restatement, block by block, on the symbols of the host call
    planes = m.dlsch_encode_symbols_host(tbs, pays, scr)
    want = np.full((n_tx, stride, 2), CANARY, np.int16)
    for i, a in enumerate(allocs):
        tx, used = ref.pdsch_resource_mapping(a, [[(int(r), int(q)) for r, q in planes[i][l]] for l in range(a["Nl"])], n_tx, literal_tail=False,
                                              literal_allowed=False, fill=None)
        assert used == [a["plane"]] * a["Nl"]
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
        m.pdsch_resource_mapping(lay_d, tx_d, stride, n_tx, segs, stream=side.cuda_stream)
    torch.cuda.synchronize()
    got = tx_d.cpu().numpy().reshape(n_tx, stride, 2)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


def test_loop_back_through_the_ul_receive_front(hip):
    """One layer, noiseless, type 1, two CDM groups without data, 16QAM, amp 512: the mapped grid read as rxdataF by
    pusch_channel_estimation (delay NULL) -> channel_level_grid -> channel_compensation_grid -> ulsch_decode_symbols with the same
    scrambling identity returns the payload bytes with ACK.  Exact equality of the payloads."""
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(31)
    N, rb, Qm = 512, 25, 4
    S = 13 * 12 * rb
    tbs = [dict(A=valid_tbs(S * Qm // 2, 1), G=Qm * S, BG=1, Qm=Qm, Nl=1, rv=0, tbslbrm=0)]
    scr = rand_scr(rng, 1)
    pays = [rng.integers(0, 256, tbs[0]["A"] // 8, dtype=np.uint8)]
    po, co, ho, _ = m.tb_layout(tbs)
    k0, rb_start, bwp_start = N - 100, 2, 1
    fco = (k0 - 12 * (rb_start + bwp_start)) % N
    dl = dl_alloc(N, rb, k0, 1, 0, 2, 0b1, 1 << 2, S, 5, 123, 1, 512, 3, 0, rb_start, bwp_start)
    ul = dict(tb=0, Qm=Qm, dmrs_config_type=0, num_dmrs_cdm_grps_no_data=2, dmrs_symbol=2, fft_size=N, first_carrier_offset=fco, bwp_start=bwp_start,
              rb_start=rb_start, rb_size=rb, start_symbol=0, nr_of_symbols=14, ul_dmrs_symb_pos=1 << 2, plane=S, rx_slot_off=3, ch_off=9, rec_off=int(co[0]))
    cfg = dict(slot=5, scid=1, dmrs_scrambling_id=123, port=0, chest_freq=0)
    msegs = m.pdsch_map_segments([dl])
    gsegs, first = m.pusch_grid_segments([ul])
    csegs = m.pusch_chest_segments([ul], [cfg], 1)
    assert [(c["c_init"], c["dmrs_offset"], c["start_re"]) for c in csegs] == [(s["c_init"], s["dmrs_offset"], s["start_re"]) for s in msegs if s["pattern"]]
    planes = m.dlsch_encode_symbols_host(tbs, pays, scr)
    stride = 14 * N + 16
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lay_d = torch.from_numpy(np.ascontiguousarray(planes[0]).reshape(-1)).cuda()
        grid = torch.zeros(2 * stride, dtype=torch.int16, device="cuda")
        m.pdsch_resource_mapping(lay_d, grid, stride, 1, msegs)
        ch_d = torch.zeros(2 * stride, dtype=torch.int16, device="cuda")
        harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
        out = torch.zeros(int(po[-1]) + 16, dtype=torch.uint8, device="cuda")
        ack = torch.zeros(1, dtype=torch.uint8, device="cuda")
        itm = torch.zeros(1, dtype=torch.int32, device="cuda")
        rec = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
        lv_d = torch.zeros(1, dtype=torch.int32, device="cuda")
        m.pusch_channel_estimation(grid, stride, ch_d, stride, 1, csegs, None)
        m.ulsch_channel_level_grid(ch_d, 1, stride, first, out=lv_d)
        m.ulsch_channel_compensation_grid(grid, ch_d, 1, stride, stride, gsegs, lv_d, rec)
        m.ulsch_decode_symbols_device([dict(t, round=0, llrLen=0) for t in tbs], rec, harq, out, ack, itm, scr)
    torch.cuda.synchronize()
    assert ack.cpu().numpy().all()
    assert np.array_equal(out.cpu().numpy()[:tbs[0]["A"] // 8], pays[0])
