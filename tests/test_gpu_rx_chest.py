"""PUSCH DMRS channel estimation on the GPU (csrc/tb_rx_chest.hip through nrLDPC_hip_pusch_channel_estimation): DEVICE and HOST mode
against the CPU form of the same header (nrLDPC_hip_pusch_chest_host, which test_rx_chest_host.py holds to the literal restatement of
the reference), bit for bit, with canaries around every output range; the refusals that need a device; and end to end from a
synthetic slot on the grid through estimation, channel_level_grid, channel_compensation_grid and decode_symbols on one stream."""
import numpy as np
import pytest

from test_gpu_tb_chain import valid_tbs
from test_gpu_tb_scrambled import rand_scr

pytestmark = pytest.mark.gpu

CANARY = 0x5a5a
T1I, T2I, T1A, T2A = 0, 1, 2, 3


def mixed_case(rng, n_rx, N=1536):
    """descriptors of all four modes, rb_size 1, 2, 3, 5, 25 and 106, both wrap cases (inside a pilot pair / PRB and between PRBs), every
    residue of ch_off mod 4, several pieces per descriptor (106 RBs = 318 groups > 256)"""
    n_sym = 4
    rs, cs = n_sym * N + 5, 0
    shapes = [(T1I, 0, 1, 0), (T2I, 1, 2, N - 1), (T1A, 1, 3, N - 7), (T2A, 4, 5, N - 6), (T1I, 3, 25, N - 12 * 12 - 2), (T2I, 2, 25, N - 36),
              (T1A, 6, 25, 500), (T2A, 11, 25, N - 150), (T1I, 5, 106, N - 636), (T2I, 9, 106, N - 636), (T1A, 2, 106, 130), (T2A, 0, 106, N - 7),
              (T1I, 7, 2, N - 24), (T2I, 6, 3, 0), (T1I, 1, 5, 7), (T1I, 4, 3, N - 2)]
    segs, at = [], 3
    for i, (mode, port, rb, k0) in enumerate(shapes):
        at += (i & 3) + 1                                              # ch_off takes every residue mod 4
        segs.append(dict(mode=mode, port=port, fft_size=N, start_re=k0, rb_size=rb, dmrs_offset=int(rng.integers(0, 900)),
                         c_init=int(rng.integers(0, 1 << 31)), delay_off=i * n_rx, rx_off=(i % n_sym) * N + 2, ch_off=at))
        at += 12 * rb + 3
    cs = at + 6 + (n_rx & 1)                                           # an odd antenna stride for odd n_rx: the phase differs per antenna
    rx = rng.integers(-32768, 32768, (n_rx * rs, 2)).astype(np.int16)
    rx[::7] = rng.choice([32767, -32768], (len(rx[::7]), 2))
    delay = rng.integers(-24, 25, len(segs) * n_rx).astype(np.int32)
    return segs, rx, rs, cs, delay


def host_form(m, segs, rx, rs, cs, n_rx, delay):
    ch = np.full((n_rx * cs, 2), CANARY, np.int16)
    for s in segs:
        for a in range(n_rx):
            d = 0 if delay is None else int(delay[s["delay_off"] + a])
            m.pusch_chest_host(rx, dict(s, rx_off=s["rx_off"] + a * rs, ch_off=s["ch_off"] + a * cs), d, ch)
    return ch


@pytest.mark.parametrize("n_rx", [1, 2, 4, 3])
def test_estimation_equals_the_host_form(hip, n_rx):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(50 + n_rx)
    segs, rx, rs, cs, delay = mixed_case(rng, n_rx)
    for dl in (delay, None):
        want = host_form(m, segs, rx, rs, cs, n_rx, dl)
        written = want != CANARY
        assert written.any() and not written.all()
        # DEVICE
        rx_d = torch.from_numpy(rx).cuda()
        ch_d = torch.full((n_rx * cs, 2), CANARY, dtype=torch.int16, device="cuda")
        dl_d = None if dl is None else torch.from_numpy(dl).cuda()
        m.pusch_channel_estimation(rx_d, rs, ch_d, cs, n_rx, segs, dl_d)
        torch.cuda.synchronize()
        got = ch_d.cpu().numpy()
        assert np.array_equal(got, want), ("device", n_rx, np.argwhere(got != want)[:4])
        # HOST
        ch_h = np.full((n_rx * cs, 2), CANARY, np.int16)
        m.pusch_channel_estimation(rx, rs, ch_h, cs, n_rx, segs, dl)
        assert np.array_equal(ch_h, want), ("host", n_rx, np.argwhere(ch_h != want)[:4])


def test_estimation_refusals_on_the_device(hip):
    import torch
    m = hip.ldpc
    L = m._chest_lib()
    N = 128
    good = dict(mode=T1I, port=0, fft_size=N, start_re=100, rb_size=2, dmrs_offset=0, c_init=5, delay_off=0, rx_off=0, ch_off=4)
    arr = m._chest_seg_array([good])
    rx_h, ch_h = np.zeros(4 * N, np.int16), np.full(4 * N, CANARY, np.int16)
    rx_d = torch.zeros(4 * N, dtype=torch.int16, device="cuda")
    ch_d = torch.full((4 * N,), CANARY, dtype=torch.int16, device="cuda")
    dl_d, dl_h = torch.zeros(2, dtype=torch.int32, device="cuda"), np.zeros(2, np.int32)

    def call(rx, ch, dl=None, stream=None, segs=arr, n=1):
        return L.nrLDPC_hip_pusch_channel_estimation(rx, N, ch, N, 2, segs, n, dl, m.MEM_DEVICE, stream)
    for rx, ch, dl in ((rx_h.ctypes.data, ch_d.data_ptr(), None), (rx_d.data_ptr(), ch_h.ctypes.data, None), (rx_d.data_ptr(), ch_d.data_ptr(), dl_h.ctypes.data)):
        assert call(rx, ch, dl) < 0 and "device memory" in m.last_error()
    assert call(rx_d.data_ptr(), ch_d.data_ptr() + 2) < 0 and "4-byte" in m.last_error()
    assert call(rx_d.data_ptr() + 2, ch_d.data_ptr()) < 0 and "4-byte" in m.last_error()
    assert call(rx_d.data_ptr(), ch_d.data_ptr(), segs=m._chest_seg_array([dict(good, mode=5)])) < 0 and "mode must be" in m.last_error()
    assert call(rx_d.data_ptr(), ch_d.data_ptr(), segs=m._chest_seg_array([good, dict(good, ch_off=20)]), n=2) < 0 and "overlap" in m.last_error()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    note = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        note.add_(1)
        rc = call(rx_d.data_ptr(), ch_d.data_ptr(), dl_d.data_ptr(), stream=side.cuda_stream)
        err = m.last_error()
    assert rc < 0 and "captured" in err
    torch.cuda.synchronize()
    assert bool((ch_d == CANARY).all()), "a refused call writes nothing"
    # and the good call runs
    assert call(rx_d.data_ptr(), ch_d.data_ptr(), dl_d.data_ptr()) == 0
    torch.cuda.synchronize()
    out = ch_d.cpu().numpy().reshape(-1, 2)
    assert np.all(out[:4] == CANARY) and np.all(out[4:28] == 0) and np.all(out[28:N // 2 + 4] == CANARY)


# ---- end to end ----------------------------------------------------------------------------------------------------------
E2E_N_RX = 2
E2E_FILL = -4321                                                       # what ul_ch holds where nothing was estimated


def e2e_allocs(m):
    """Two transport blocks in grids of their own size: a type-1 allocation that straddles the wrap of a 1536-point grid, estimated
    by interpolation (64QAM, DMRS in symbol 2), and a type-2 allocation in a 512-point grid, averaged per PRB (16QAM, DMRS in
    symbol 3, port 1: w_f alternates).  Returns the blocks, the allocations and the estimation settings."""
    shapes = [dict(N=1536, n_rb=106, rb=25, typ=0, Qm=6, BG=1, dmrs=2, cfg=dict(slot=7, scid=1, dmrs_scrambling_id=333, port=0, chest_freq=0)),
              dict(N=512, n_rb=24, rb=5, typ=1, Qm=4, BG=2, dmrs=3, cfg=dict(slot=3, scid=0, dmrs_scrambling_id=41, port=1, chest_freq=1))]
    tbs, allocs = [], []
    for i, h in enumerate(shapes):
        S = (13 * 12 + (6 if h["typ"] == 0 else 8)) * h["rb"]
        tbs.append(dict(A=valid_tbs(S * h["Qm"] // 2, h["BG"]), G=h["Qm"] * S, BG=h["BG"], Qm=h["Qm"], Nl=1, rv=0, tbslbrm=0))
    co = m.tb_layout(tbs)[1]
    for i, h in enumerate(shapes):
        N = h["N"]
        rb_start = h["n_rb"] // 2 - (h["rb"] + 1) // 2 if i == 0 else 3
        allocs.append(dict(tb=i, Qm=h["Qm"], dmrs_config_type=h["typ"], num_dmrs_cdm_grps_no_data=1, dmrs_symbol=h["dmrs"], fft_size=N,
                           first_carrier_offset=N - 6 * h["n_rb"], bwp_start=0, rb_start=rb_start, rb_size=h["rb"], start_symbol=0, nr_of_symbols=14,
                           ul_dmrs_symb_pos=1 << h["dmrs"], plane=tbs[i]["G"] // h["Qm"], rx_slot_off=i * 14 * 1536 + 3, ch_off=i * 14 * 1536 + 9,
                           rec_off=int(co[i])))
    return tbs, allocs, [h["cfg"] for h in shapes]


def e2e_slot(m, rng, allocs, csegs, gsegs, tx, sigma=0.05):
    """The slot on the grid, [n_rx, rx_stride, 2]: per block and antenna a flat complex gain g and additive noise; a data RE is
    y = g x / 23170, as in the tests of the front, and a DMRS RE is y = g conj(p) / (23170 sqrt 2) for the conjugated pilot p of
    pusch_dmrs_host: p y is then 23170 sqrt 2 g, which every estimator brings to g (two shift-16 products added, or shift-15
    products averaged).  Returns the grid, its stride and g as c16 [n_alloc, n_rx, 2]."""
    n_rx = E2E_N_RX
    rx_stride = len(allocs) * 14 * 1536 + 7
    rx = np.full((n_rx, rx_stride, 2), 1234, np.int16)
    gains = []

    def put(at, v):
        v = v + sigma * 1500 * (rng.standard_normal(v.shape) + 1j * rng.standard_normal(v.shape))
        rx[:, at] = np.clip(np.rint(np.stack([v.real, v.imag], 2)), -32768, 32767).astype(np.int16)
    for i, al in enumerate(allocs):
        N = al["fft_size"]
        g = np.rint(rng.uniform(1200, 2600, n_rx) * np.exp(1j * rng.uniform(0, 2 * np.pi, n_rx)))
        gains.append(np.stack([g.real, g.imag], 1).astype(np.int16))
        x = (tx[i][0][:, 0].astype(np.float64) + 1j * tx[i][0][:, 1]) / 23170.0
        for s in (s for s in gsegs if s["tb"] == i):
            j = np.arange(s["nb_re"])
            p_j = {m.RXG_FULL: j, m.RXG_DMRS1: 2 * j + 1, m.RXG_DMRS2: 6 * (j // 4) + 2 + j % 4}[s["pattern"]]
            put(s["rx_off"] + (s["start_re"] + p_j) % N, g[:, None] * x[None, s["sym_off"]:s["sym_off"] + s["nb_re"]])
        c = csegs[i]                                                   # one DMRS symbol per allocation
        typ = al["dmrs_config_type"]
        n_pil = (4 if typ else 6) * al["rb_size"]
        p = m.pusch_dmrs_host(c["c_init"], c["dmrs_offset"], n_pil, c["port"], typ).astype(np.float64)
        k = np.arange(n_pil)
        re = 6 * (k // 2) + k % 2 if typ else 2 * k                      # ports 0 and 1 of either type: delta = 0, nushift = 0
        put(c["rx_off"] + (c["start_re"] + re) % N, g[:, None] * (p[:, 0] - 1j * p[:, 1])[None, :] / (23170.0 * np.sqrt(2.0)))
    return rx, rx_stride, np.stack(gains)


def test_estimation_front_and_decode_on_one_stream(hip):
    """rxdataF to payload bytes with nothing but descriptors crossing the link; and the same records, shifts and decoder output
    as with the host form's estimates uploaded in place of the estimation call."""
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(77)
    n_rx = E2E_N_RX
    tbs, allocs, cfgs = e2e_allocs(m)
    n = len(tbs)
    scr = rand_scr(rng, n)
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    po, co, ho, nseg = m.tb_layout(tbs)
    gsegs, first = m.pusch_grid_segments(allocs)
    csegs = m.pusch_chest_segments(allocs, cfgs, n_rx)
    assert [c["mode"] for c in csegs] == [T1I, T2A] and csegs[0]["start_re"] + 12 * allocs[0]["rb_size"] > allocs[0]["fft_size"]
    assert [c["ch_off"] for c in csegs] == [f["ch_off"] for f in first]
    tx = m.dlsch_encode_symbols_host(tbs, pays, scr)
    rx, rx_stride, gains = e2e_slot(m, rng, allocs, csegs, gsegs, tx)
    ch_stride = n * 14 * 1536 + 64
    delay = np.array([3, -2, 0, 1], np.int32)                          # per (descriptor, antenna); a flat channel shows none of it
    # the host form's estimates: near the gains, and the array the second run uploads
    ch_np = np.full((n_rx * ch_stride, 2), E2E_FILL, np.int16)
    rx_flat = rx.reshape(-1, 2)
    for c in csegs:
        for a in range(n_rx):
            m.pusch_chest_host(rx_flat, dict(c, rx_off=c["rx_off"] + a * rx_stride, ch_off=c["ch_off"] + a * ch_stride), int(delay[c["delay_off"] + a]), ch_np)
    for i, c in enumerate(csegs):
        for a in range(n_rx):
            est = ch_np[c["ch_off"] + a * ch_stride:c["ch_off"] + a * ch_stride + 12 * c["rb_size"]].astype(np.int32)
            # noise of 75 per component: an estimate carries at most 75 / 2 (four shift-15 products of 75 each averaged; the
            # interpolation's pair weights give less), six sigma of that over these few hundred entries; the two rotations by a
            # table of 1 / 256 steps and the truncations add less than 40.  A wrong scale would miss by 700 or more.
            assert np.abs(est - gains[i, a]).max() < 6 * 75 / 2 + 40, (i, a, np.abs(est - gains[i, a]).max())
    outs = []
    side = torch.cuda.Stream()
    for which in ("estimated", "uploaded"):
        rxt = [dict(t, round=0, llrLen=0) for t in tbs]
        harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
        out = torch.zeros(int(po[-1]) + 16, dtype=torch.uint8, device="cuda")
        ack = torch.zeros(n, dtype=torch.uint8, device="cuda")
        itm = torch.zeros(n, dtype=torch.int32, device="cuda")
        rec = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
        lv_d = torch.zeros(n, dtype=torch.int32, device="cuda")
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            rx_d = torch.from_numpy(rx.reshape(-1)).cuda()
            if which == "estimated":
                ch_d = torch.full((n_rx * ch_stride * 2,), E2E_FILL, dtype=torch.int16, device="cuda")
                m.pusch_channel_estimation(rx_d, rx_stride, ch_d, ch_stride, n_rx, csegs, torch.from_numpy(delay).cuda())
            else:
                ch_d = torch.from_numpy(ch_np.reshape(-1)).cuda()
            m.ulsch_channel_level_grid(ch_d, n_rx, ch_stride, first, out=lv_d)
            m.ulsch_channel_compensation_grid(rx_d, ch_d, n_rx, rx_stride, ch_stride, gsegs, lv_d, rec)
            m.ulsch_decode_symbols_device(rxt, rec, harq, out, ack, itm, scr)
        torch.cuda.synchronize()
        outs.append((ch_d.cpu().numpy(), lv_d.cpu().numpy(), rec.cpu().numpy(), out.cpu().numpy(), ack.cpu().numpy(), itm.cpu().numpy(),
                     harq.cpu().numpy()))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    assert outs[0][4].all(), outs[0][4]
    for i, t in enumerate(tbs):
        assert np.array_equal(outs[0][3][po[i]:po[i] + t["A"] // 8], pays[i]), i
