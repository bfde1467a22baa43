"""The UL receive front read from the OFDM grid (nrLDPC_hip_ulsch_channel_level_grid / _channel_compensation_grid), bit for bit
against (a) the extraction in numpy followed by the numpy restatement of the reference (rx_front_np.py) and (b) the existing GPU
calls on the numpy-extracted arrays; its refusals; and end to end from a synthetic grid through pusch_grid_segments, level_grid,
compensation_grid and decode_symbols against the existing path fed with numpy-compensated records.

Where the wrap falls in a thread group: thread group g of a segment takes REs 4g - phase .. 4g - phase + 3, phase = (c16 address
of the segment's first output) & 3 = (rec_off / 2 + sym_off) & 3 for a 16-byte aligned record array.  A segment whose RE w is the
first one behind the wrap (start_re = N - p(w)) has the wrap between two groups when (w + phase) % 4 == 0 and inside a group
otherwise; grid_case() places every pattern and size both ways by choosing sym_off, and checks that it did."""
import numpy as np
import pytest

from rx_front_np import compensate_np, level_np
from test_gpu_rx_front import through_channel
from test_gpu_tb_chain import valid_tbs
from test_gpu_tb_scrambled import rand_scr

pytestmark = pytest.mark.gpu
CANARY = 0x5a5a
FULL, DMRS1, DMRS2 = 0, 1, 2
PER_RB = {FULL: 12, DMRS1: 6, DMRS2: 8}
SHIFTS = (0, 1, 7, 12, 15, 16, 31)


def p_of(pattern, j):
    return [lambda j: j, lambda j: 2 * j + 1, lambda j: 6 * (j // 4) + 2 + j % 4][pattern](j)


def extract_np(rx, ch, s):
    """[n_rx, nb_re, 2] each: the closed form of the issue, checked against the reference's literal loops in test_rx_grid_host.py"""
    idx = np.array([p_of(s["pattern"], j) for j in range(s["nb_re"])])
    return rx[:, s["rx_off"] + (s["start_re"] + idx) % s["fft_size"]], ch[:, s["ch_off"] + idx]


def grid_case(rng, Qm, n_rx):
    """Two blocks (N = 128 and N = 1536), every pattern with 1, 3 and (N = 1536) 25 RBs, each placed with the wrap between two
    thread groups, inside one, not at all and with start_re = 0; every segment in an OFDM symbol and a channel range of its own;
    different antenna strides for the grid and the estimates."""
    segs, kinds = [], set()
    rx_at, ch_at, rec_at = 3, 5, 2
    planes = []
    for tb, (N, sizes) in enumerate(((128, (1, 3)), (1536, (1, 3, 25)))):
        off, mine = int(rng.integers(0, 4)), []
        for rb in sizes:
            for pattern in (FULL, DMRS1, DMRS2):
                nb = PER_RB[pattern] * rb
                for place in ("between", "inside", "none", "zero"):
                    w = nb // 2 + (1 if rb > 1 else 0)                        # the first RE behind the wrap
                    start_re = {"between": N - p_of(pattern, w), "inside": N - p_of(pattern, w), "none": 7, "zero": 0}[place]
                    if place in ("between", "inside"):                       # sym_off so that (w + phase) % 4 is 0 / is not
                        want = 0 if place == "between" else 1 + len(mine) % 3
                        while (w + rec_at // 2 + off) % 4 != want:
                            off += 1
                        kinds.add((pattern, rb, (w + ((rec_at // 2 + off) & 3)) % 4 == 0))
                    mine.append(dict(tb=tb, Qm=Qm, pattern=pattern, nb_re=nb, sym_off=off, fft_size=N, start_re=start_re, rx_off=rx_at, ch_off=ch_at,
                                     rec_off=rec_at))
                    off += nb + len(mine) % 3
                    rx_at += N + len(mine) % 2
                    ch_at += p_of(pattern, nb - 1) + 1 + len(mine) % 4
        plane = off + int(rng.integers(0, 5))
        for s in mine:
            s["plane"] = plane
        segs += mine
        planes.append(plane)
        rec_at += 2 * 4 * plane + 2 * int(rng.integers(0, 4))
    assert kinds == {(p, rb, b) for p in (FULL, DMRS1, DMRS2) for rb in (1, 3, 25) for b in (True, False)}
    rx_stride, ch_stride = rx_at + 11, ch_at + 6
    rx = rng.integers(-32768, 32768, (n_rx, rx_stride, 2)).astype(np.int16)
    ch = rng.integers(-32768, 32768, (n_rx, ch_stride, 2)).astype(np.int16)
    ch[:, [c for s in segs if s["tb"] == 1 for c in range(s["ch_off"], s["ch_off"] + p_of(s["pattern"], s["nb_re"] - 1) + 1)]] >>= 5
    shift = np.array([SHIFTS[(tb + Qm + n_rx) % len(SHIFTS)] for tb in range(2)], np.int32)
    # the extracted form of the same call, and what the records must hold
    want = np.full(rec_at + 64, CANARY, np.int16)
    n_ext = sum(s["nb_re"] for s in segs)
    rx_e, ch_e = np.zeros((n_rx, n_ext, 2), np.int16), np.zeros((n_rx, n_ext, 2), np.int16)
    ext_segs, at = [], 0
    for s in segs:
        nb = s["nb_re"]
        rx_e[:, at:at + nb], ch_e[:, at:at + nb] = extract_np(rx, ch, s)
        ext_segs.append(dict(tb=s["tb"], Qm=Qm, nb_re=nb, plane=s["plane"], sym_off=s["sym_off"], rx_off=at, ch_off=at, rec_off=s["rec_off"]))
        pl = compensate_np(rx_e[:, at:at + nb], ch_e[:, at:at + nb], Qm, int(shift[s["tb"]]))
        for k in range(Qm // 2):
            o = s["rec_off"] + 2 * (k * s["plane"] + s["sym_off"])
            want[o:o + 2 * nb] = pl[k].reshape(-1)
        at += nb
    return segs, ext_segs, rx, ch, rx_stride, ch_stride, rx_e, ch_e, shift, want


def measurement_symbols(segs, n_rx):
    """indices into grid_case's segments: a DMRS1 / DMRS2 / FULL segment of 3 RBs per block, rotating; any order"""
    pick = lambda tb, pat: next(i for i, s in enumerate(segs) if s["tb"] == tb and s["pattern"] == pat and s["nb_re"] == PER_RB[pat] * 3)
    return [pick(1, (n_rx + 1) % 3), pick(0, n_rx % 3)]


GRID_PARAMS = [(1, 6), (2, 6), (3, 6), (4, 6), (8, 6), (2, 2), (2, 4), (2, 8)]


@pytest.mark.parametrize("n_rx,Qm", GRID_PARAMS)
def test_grid_compensation_and_level(hip, n_rx, Qm):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(2000 * Qm + n_rx)
    segs, ext_segs, rx, ch, rx_stride, ch_stride, rx_e, ch_e, shift, want = grid_case(rng, Qm, n_rx)
    n_ext = rx_e.shape[1]
    fi = measurement_symbols(segs, n_rx)
    first, ext_first = [segs[i] for i in fi], [ext_segs[i] for i in fi]
    lv_want = np.array([level_np(extract_np(rx, ch, segs[i])[1])[0] for i in fi[::-1]], np.int32)
    rx0, ch0 = rx.copy(), ch.copy()
    # host mode
    rec = np.full(want.size, CANARY, np.int16)
    m.ulsch_channel_compensation_grid(rx.reshape(-1), ch.reshape(-1), n_rx, rx_stride, ch_stride, segs, shift, rec)
    assert np.array_equal(rec, want), (Qm, n_rx, "host", np.flatnonzero(rec != want)[:8])
    assert np.array_equal(m.ulsch_channel_level_grid(ch.reshape(-1), n_rx, ch_stride, first), lv_want)
    assert np.array_equal(rx, rx0) and np.array_equal(ch, ch0)
    # device mode, the record array 16-, 4- and 8-byte aligned; the existing calls on the extracted arrays beside it
    rx_d, ch_d = torch.from_numpy(rx.reshape(-1)).cuda(), torch.from_numpy(ch.reshape(-1)).cuda()
    rxe_d, che_d = torch.from_numpy(rx_e.reshape(-1)).cuda(), torch.from_numpy(ch_e.reshape(-1)).cuda()
    sh_d = torch.from_numpy(shift).cuda()
    for pad in (0, 2, 4):
        rec_d = torch.full((want.size + 8,), CANARY, dtype=torch.int16, device="cuda")
        old_d = torch.full((want.size + 8,), CANARY, dtype=torch.int16, device="cuda")
        lv_d = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        lo_d = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        m.ulsch_channel_level_grid(ch_d, n_rx, ch_stride, first, out=lv_d)
        m.ulsch_channel_compensation_grid(rx_d, ch_d, n_rx, rx_stride, ch_stride, segs, sh_d, rec_d[pad:])
        m.ulsch_channel_level(che_d, n_rx, n_ext, ext_first, out=lo_d)
        m.ulsch_channel_compensation(rxe_d, che_d, n_rx, n_ext, ext_segs, sh_d, old_d[pad:])
        torch.cuda.synchronize()
        got = rec_d.cpu().numpy()
        assert (got[:pad] == CANARY).all() and (got[pad + want.size:] == CANARY).all()
        assert np.array_equal(got[pad:pad + want.size], want), (Qm, n_rx, pad, np.flatnonzero(got[pad:pad + want.size] != want)[:8])
        assert torch.equal(rec_d, old_d) and torch.equal(lv_d, lo_d)
        assert lv_d.cpu().numpy().tolist() == lv_want.tolist() + [-7, -7]
    assert np.array_equal(rx_d.cpu().numpy(), rx0.reshape(-1)) and np.array_equal(ch_d.cpu().numpy(), ch0.reshape(-1))
    # the shift the level call wrote, used from device memory by the compensation call on the same stream
    rec_d = torch.full((want.size,), CANARY, dtype=torch.int16, device="cuda")
    lv_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.ulsch_channel_level_grid(ch_d, n_rx, ch_stride, first, out=lv_d)
        m.ulsch_channel_compensation_grid(rx_d, ch_d, n_rx, rx_stride, ch_stride, segs, lv_d, rec_d)
    torch.cuda.synchronize()
    rec = np.full(want.size, CANARY, np.int16)
    m.ulsch_channel_compensation(rx_e.reshape(-1), ch_e.reshape(-1), n_rx, n_ext, ext_segs, lv_want, rec)
    assert np.array_equal(rec_d.cpu().numpy(), rec)


# ---- end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rb", [2, 25])
def test_grid_front_then_decode_symbols_equals_numpy_records(hip, rb):
    """one transport block, 14 symbols, a type-1 DMRS symbol, an allocation that straddles the wrap of a 1536-point grid"""
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(90 + rb)
    Qm, n_rx, N, n_rb, sigma = 6, 4, 1536, 106, 0.2
    S = (13 * 12 + 6) * rb
    tb = dict(A=valid_tbs(S * Qm // 2, 1 if rb > 2 else 2), G=Qm * S, BG=1 if rb > 2 else 2, Qm=Qm, Nl=1, rv=0, tbslbrm=0)
    scr = rand_scr(rng, 1)
    pay = rng.integers(0, 256, tb["A"] // 8, dtype=np.uint8)
    po, co, ho, nseg = m.tb_layout([tb])
    al = dict(tb=0, Qm=Qm, dmrs_config_type=0, num_dmrs_cdm_grps_no_data=1, dmrs_symbol=2, fft_size=N, first_carrier_offset=N - 6 * n_rb, bwp_start=0,
              rb_start=n_rb // 2 - (rb + 1) // 2, rb_size=rb, start_symbol=0, nr_of_symbols=14, ul_dmrs_symb_pos=1 << 2, plane=S, rx_slot_off=14 * N,
              ch_off=9, rec_off=int(co[0]))
    segs, first = m.pusch_grid_segments([al])
    assert len(segs) == 14 and sum(s["nb_re"] for s in segs) == S and segs[0]["start_re"] + 12 * rb > N
    tx = m.dlsch_encode_symbols_host([tb], [pay], scr)
    rx_e, ch_e = through_channel(rng, tx[0][0], n_rx, sigma)
    rx_stride, ch_stride = 28 * N + 5, 14 * N + 64
    rx = np.full((n_rx, rx_stride, 2), 1234, np.int16)
    ch = np.full((n_rx, ch_stride, 2), -4321, np.int16)
    ch[:, segs[0]["ch_off"]:segs[0]["ch_off"] + 12 * rb] = ch_e[:, :1]                       # a flat channel: the estimates of the DMRS symbol
    for s in segs:
        idx = np.array([p_of(s["pattern"], j) for j in range(s["nb_re"])])
        rx[:, s["rx_off"] + (s["start_re"] + idx) % N] = rx_e[:, s["sym_off"]:s["sym_off"] + s["nb_re"]]
    # the existing path: numpy level and compensation, pack_symbol_records, decode_symbols
    lv = level_np(ch_e[:, :first[0]["nb_re"]])[0]
    parts = [compensate_np(rx_e[:, s["sym_off"]:s["sym_off"] + s["nb_re"]], ch_e[:, s["sym_off"]:s["sym_off"] + s["nb_re"]], Qm, lv) for s in segs]
    rec_np = np.zeros(int(co[-1]) + 16, np.int16)
    rec_np[co[0]:co[0] + tb["G"]] = m.pack_symbol_records([[np.concatenate([p[k] for p in parts]) for k in range(Qm // 2)]])[0]
    outs = []
    side = torch.cuda.Stream()
    for which in (0, 1):
        rxt = [dict(tb, round=0, llrLen=0)]
        harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
        out = torch.zeros(int(po[-1]) + 16, dtype=torch.uint8, device="cuda")
        ack = torch.zeros(1, dtype=torch.uint8, device="cuda")
        itm = torch.zeros(1, dtype=torch.int32, device="cuda")
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            if which == 0:
                rx_d, ch_d = torch.from_numpy(rx.reshape(-1)).cuda(), torch.from_numpy(ch.reshape(-1)).cuda()
                rec = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
                lv_d = torch.zeros(1, dtype=torch.int32, device="cuda")
                m.ulsch_channel_level_grid(ch_d, n_rx, ch_stride, first, out=lv_d)
                m.ulsch_channel_compensation_grid(rx_d, ch_d, n_rx, rx_stride, ch_stride, segs, lv_d, rec)
            else:
                rec = torch.from_numpy(rec_np).cuda()
            m.ulsch_decode_symbols_device(rxt, rec, harq, out, ack, itm, scr)
        torch.cuda.synchronize()
        if which == 0:
            assert lv_d.cpu().numpy().tolist() == [lv] and np.array_equal(rec.cpu().numpy(), rec_np)
        outs.append((out.cpu().numpy()[po[0]:po[0] + tb["A"] // 8], ack.cpu().numpy(), itm.cpu().numpy(), harq.cpu().numpy()))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_rx_grid_invalid_input(hip):
    import torch
    m = hip.ldpc
    L = m._rxg_lib()
    n_rx, N = 2, 128
    rs, cs = 2 * N, N + 8
    good = dict(tb=0, Qm=4, pattern=DMRS1, nb_re=16, plane=32, sym_off=4, fft_size=N, start_re=100, rx_off=N, ch_off=3, rec_off=0)
    rx_h, ch_h = np.zeros(2 * n_rx * rs, np.int16), np.zeros(2 * n_rx * cs, np.int16)
    rec_h, sh_h, lv_h = np.full(512, CANARY, np.int16), np.zeros(2, np.int32), np.full(2, -7, np.int32)
    rx_d, ch_d = torch.zeros(2 * n_rx * rs, dtype=torch.int16, device="cuda"), torch.zeros(2 * n_rx * cs, dtype=torch.int16, device="cuda")
    rec_d = torch.full((512,), CANARY, dtype=torch.int16, device="cuda")
    sh_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    lv_d = torch.full((2,), -7, dtype=torch.int32, device="cuda")

    def comp(mode, segs, rx=True, ch=True, shift=True, rec=True, n=n_rx, mem=None, stream=None, desc=True, rec_ptr=None):
        h = mode == "host"
        x, c, r, s = (rx_h.ctypes.data, ch_h.ctypes.data, rec_h.ctypes.data, sh_h.ctypes.data) if h else (rx_d.data_ptr(), ch_d.data_ptr(),
                                                                                                         rec_d.data_ptr(), sh_d.data_ptr())
        mem = (m.MEM_HOST if h else m.MEM_DEVICE) if mem is None else mem
        return L.nrLDPC_hip_ulsch_channel_compensation_grid(x if rx else None, c if ch else None, n, rs, cs, m._rx_grid_seg_array(segs) if desc else None,
                                                            len(segs), s if shift else None, (rec_ptr or r) if rec else None, mem, stream)

    def level(mode, fs, ch=True, out=True, n=n_rx, mem=None, stream=None, desc=True):
        c, o = (ch_h.ctypes.data, lv_h.ctypes.data) if mode == "host" else (ch_d.data_ptr(), lv_d.data_ptr())
        mem = (m.MEM_HOST if mode == "host" else m.MEM_DEVICE) if mem is None else mem
        return L.nrLDPC_hip_ulsch_channel_level_grid(c if ch else None, n, cs, m._rx_grid_seg_array(fs) if desc else None, len(fs), o if out else None,
                                                     mem, stream)

    for mode in ("host", "device"):
        bad_calls = [
            (lambda: comp(mode, [good], rx=False), "null"), (lambda: comp(mode, [good], ch=False), "null"),
            (lambda: comp(mode, [good], shift=False), "null"), (lambda: comp(mode, [good], rec=False), "null"),
            (lambda: comp(mode, [good], desc=False), "null"),
            (lambda: comp(mode, [good], n=0), "n_rx"), (lambda: comp(mode, [good], n=9), "n_rx"),
            (lambda: comp(mode, [dict(good, Qm=5)]), "Qm"), (lambda: comp(mode, [dict(good, Qm=0)]), "Qm"),
            (lambda: comp(mode, [dict(good, rec_off=3)]), "even"),
            (lambda: comp(mode, [dict(good, sym_off=17)]), "plane"),
            (lambda: comp(mode, [good, dict(good, sym_off=10, nb_re=8)]), "overlap"),
            (lambda: comp(mode, [good, dict(good, Qm=2, rec_off=2 * 32, sym_off=19, nb_re=2)]), "overlap"),
            (lambda: comp(mode, [dict(good, pattern=FULL, fft_size=1 << 21, Qm=8, nb_re=(1 << 18) + 1, plane=1 << 19)]), "2^21"),
            (lambda: comp(mode, [good], mem=7), "mem"),
            (lambda: comp(mode, [dict(good, pattern=3)]), "pattern"),
            (lambda: comp(mode, [dict(good, start_re=N)]), "start_re"), (lambda: comp(mode, [dict(good, fft_size=0)]), "start_re"),
            (lambda: comp(mode, [dict(good, plane=300, nb_re=65)]), "count"),                              # DMRS1: 64 within 128
            (lambda: comp(mode, [dict(good, plane=300, pattern=DMRS2, nb_re=85)]), "p(nb_re - 1)"),        # DMRS2: 84
            (lambda: comp(mode, [dict(good, plane=300, pattern=FULL, nb_re=129)]), "count"),
            (lambda: level(mode, [good], ch=False), "null"), (lambda: level(mode, [good], out=False), "null"),
            (lambda: level(mode, [good], desc=False), "null"),
            (lambda: level(mode, [good], n=0), "n_rx"), (lambda: level(mode, [good], n=9), "n_rx"),
            (lambda: level(mode, [dict(good, nb_re=0)]), "no REs"),
            (lambda: level(mode, [dict(good, tb=1)]), "tb"), (lambda: level(mode, [good, good]), "tb"),
            (lambda: level(mode, [good], mem=3), "mem"),
            (lambda: level(mode, [dict(good, pattern=7)]), "pattern"), (lambda: level(mode, [dict(good, start_re=N + 1)]), "start_re"),
            (lambda: level(mode, [dict(good, nb_re=65)]), "count"),
        ]
        for call, why in bad_calls:
            assert call() < 0, (mode, why)
            assert why in m.last_error(), (mode, why, m.last_error())
    # DEVICE mem with a host array, and a record that is not 4-byte aligned
    arr = m._rx_grid_seg_array([good])
    for x, c, s in ((rx_h.ctypes.data, ch_d.data_ptr(), sh_d.data_ptr()), (rx_d.data_ptr(), ch_h.ctypes.data, sh_d.data_ptr()),
                    (rx_d.data_ptr(), ch_d.data_ptr(), sh_h.ctypes.data)):
        assert L.nrLDPC_hip_ulsch_channel_compensation_grid(x, c, n_rx, rs, cs, arr, 1, s, rec_d.data_ptr(), m.MEM_DEVICE, None) < 0
        assert "device memory" in m.last_error()
    assert comp("device", [good], rec_ptr=rec_h.ctypes.data) < 0 and "device memory" in m.last_error()
    assert comp("device", [good], rec_ptr=rec_d.data_ptr() + 2) < 0 and "4-byte" in m.last_error()
    assert L.nrLDPC_hip_ulsch_channel_level_grid(ch_d.data_ptr(), n_rx, cs, arr, 1, lv_h.ctypes.data, m.MEM_DEVICE, None) < 0
    assert "device memory" in m.last_error()
    assert L.nrLDPC_hip_ulsch_channel_level_grid(ch_h.ctypes.data, n_rx, cs, arr, 1, lv_d.data_ptr(), m.MEM_DEVICE, None) < 0
    assert "device memory" in m.last_error()
    # the wrappers know the extents: a descriptor that reaches outside is refused before the call
    with pytest.raises(ValueError):
        m.ulsch_channel_compensation_grid(rx_d, ch_d, n_rx, rs, cs, [dict(good, rx_off=3 * N + 1)], sh_d, rec_d)
    with pytest.raises(ValueError):
        m.ulsch_channel_level_grid(ch_d, n_rx, cs, [dict(good, ch_off=cs + 8 - 31)], out=lv_d)
    # a stream that is being captured
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    note = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        note.add_(1)
        rc_c = comp("device", [good], stream=side.cuda_stream)
        err_c = m.last_error()
        rc_l = level("device", [good], stream=side.cuda_stream)
        err_l = m.last_error()
    assert rc_c < 0 and "captured" in err_c and rc_l < 0 and "captured" in err_l
    torch.cuda.synchronize()
    assert (rec_d.cpu().numpy() == CANARY).all() and (rec_h == CANARY).all()
    assert (lv_d.cpu().numpy() == -7).all() and (lv_h == -7).all()
    # and the same arguments without the fault are accepted
    assert comp("device", [good]) == 0 and comp("host", [good]) == 0 and level("device", [good]) == 0 and level("host", [good]) == 0
    torch.cuda.synchronize()
    assert (rec_h[8:8 + 32] == 0).all() and (rec_h[:8] == CANARY).all() and lv_h[0] == 1 and int(lv_d[0]) == 1
