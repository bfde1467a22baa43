"""The two-layer MMSE receiver on the GPU (nrLDPC_hip_ulsch_mmse_2layers_grid / _channel_level_grid_mmse), bit for bit against the
numpy restatement of the reference (rx_mmse_np.py) on arrays extracted in numpy; its write set; HOST against DEVICE mode; its
refusals; and end to end from dlsch_encode_symbols with Nl = 2 through the channel that test_rx_mmse_host.py fixes, level, MMSE
and decode_symbols on one stream.

A thread takes the quad of REs 4q .. 4q + 3 of its segment, a workgroup PIECE_QUADS of them.  A segment whose RE w is the first one
behind the grid's wrap (start_re = N - p(w)) has the wrap between two quads when w % 4 == 0 and inside a quad otherwise; grid_case()
places every pattern both ways and checks that it did."""
import numpy as np
import pytest

from rx_mmse_np import level_mmse_np, mmse_np, records_np
from test_gpu_rx_grid import extract_np, p_of
from test_rx_mmse_host import E2E_NVAR, mmse_e2e_case, mmse_e2e_channel, mmse_e2e_record

pytestmark = pytest.mark.gpu
CANARY = 0x5a5a
FULL, DMRS1, DMRS2 = 0, 1, 2
PER_RB = {FULL: 12, DMRS1: 6, DMRS2: 8}
PIECE_QUADS = 256                      # NR_RXF_THREADS: the quads of one workgroup


def pairs_np(rx, ch, s, n_rx):
    """rx int16 [n_rx, nb_re, 2], ch int16 [2, n_rx, nb_re, 2] of a segment; ch holds the 2 n_rx pairs one stride apart"""
    a, b = extract_np(rx, ch, s)
    return a, b.reshape(2, n_rx, s["nb_re"], 2)


def grid_case(rng, Qm, n_rx):
    """Two blocks with a shift and an nvar each (0 and not 0).  Block 0 (N = 128): every pattern with 1 and 3 RBs -- DMRS1 gives 6
    and 18 REs, a partial last quad -- each with the wrap between two quads, inside one, and not at all.  Block 1 (N = 2048): 90 RBs
    FULL, more than one workgroup's piece, with the wrap in its second piece, and a 3-RB segment of each pattern.  Every segment
    in an OFDM symbol and a channel range of its own; different antenna strides for the grid and the estimates."""
    segs, kinds = [], set()
    rx_at, ch_at, rec_at = 3, 5, 2
    for tb, (N, cases) in enumerate(((128, [(p, rb) for rb in (1, 3) for p in (FULL, DMRS1, DMRS2)]),
                                     (2048, [(FULL, 90), (DMRS1, 3), (DMRS2, 3), (FULL, 3)]))):
        off, mine = 1, []
        for pattern, rb in cases:
            nb = PER_RB[pattern] * rb
            for place in ("between", "inside", "none"):
                w = 4 * max(1, nb // 8) if rb < 90 else 4 * (PIECE_QUADS + 1)           # the first RE behind the wrap
                w += place == "inside"
                assert 0 < w < nb
                start_re = N - p_of(pattern, w) if place != "none" else 7
                if place != "none":
                    kinds.add((pattern, rb, w % 4 == 0))
                mine.append(dict(tb=tb, Qm=Qm, pattern=pattern, nb_re=nb, sym_off=off, fft_size=N, start_re=start_re, rx_off=rx_at, ch_off=ch_at,
                                 rec_off=rec_at))
                off += nb + len(mine) % 3
                rx_at += N + len(mine) % 2
                ch_at += p_of(pattern, nb - 1) + 1 + len(mine) % 4
        plane = 2 * off + int(rng.integers(0, 5))
        for s in mine:
            s["plane"] = plane
        segs += mine
        rec_at += 2 * (Qm // 2) * plane + 2 * int(rng.integers(0, 4))
    assert kinds == {(p, rb, b) for p in (FULL, DMRS1, DMRS2) for rb in (1, 3) for b in (True, False)} | {(FULL, 90, True), (FULL, 90, False)}
    big = [s for s in segs if s["nb_re"] == 1080]
    assert big and all((s["nb_re"] + 3) // 4 > PIECE_QUADS for s in big)                 # it really spans two workgroups
    assert any(s["sym_off"] & 1 for s in segs) and any(s["nb_re"] % 4 for s in segs)
    rx_stride, ch_stride = rx_at + 11, ch_at + 6
    rx = rng.integers(-32768, 32768, (n_rx, rx_stride, 2)).astype(np.int16)
    ch = rng.integers(-32768, 32768, (2 * n_rx, ch_stride, 2)).astype(np.int16)
    for s in segs:                                                                         # block 1: a channel of moderate size
        if s["tb"] == 1:
            ch[:, s["ch_off"]:s["ch_off"] + p_of(s["pattern"], s["nb_re"] - 1) + 1] >>= 5
    shift = np.array([(3, 9), (0, 6)][Qm == 8], np.int32)
    nvar = np.array([0, 70000] if n_rx == 2 else [37, 0], np.int32)
    want = np.full(rec_at + 64, CANARY, np.int16)
    for s in segs:
        a, b = pairs_np(rx, ch, s, n_rx)
        records_np(want, mmse_np(a, b, Qm, int(shift[s["tb"]]), int(nvar[s["tb"]])), Qm, s["plane"], s["sym_off"], s["rec_off"])
    return segs, rx, ch, rx_stride, ch_stride, shift, nvar, want


@pytest.mark.parametrize("n_rx,Qm", [(2, 6), (4, 6), (2, 8), (4, 8)])
def test_mmse_grid_equals_numpy(hip, n_rx, Qm):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(3000 * Qm + n_rx)
    segs, rx, ch, rx_stride, ch_stride, shift, nvar, want = grid_case(rng, Qm, n_rx)
    rx0, ch0 = rx.copy(), ch.copy()
    # the write set: only the segments' doubled ranges of Qm/2 planes differ from the canary
    touched = np.zeros(want.size, bool)
    for s in segs:
        for k in range(Qm // 2):
            o = s["rec_off"] + 2 * (k * s["plane"] + 2 * s["sym_off"])
            touched[o:o + 4 * s["nb_re"]] = True
    assert (want[~touched] == CANARY).all()
    # host mode
    rec = np.full(want.size, CANARY, np.int16)
    m.ulsch_mmse_2layers_grid(rx.reshape(-1), ch.reshape(-1), n_rx, rx_stride, ch_stride, segs, shift, nvar, rec)
    assert np.array_equal(rec, want), (Qm, n_rx, "host", np.flatnonzero(rec != want)[:8])
    assert np.array_equal(rx, rx0) and np.array_equal(ch, ch0)
    # device mode, the record array 16-, 4- and 8-byte aligned
    rx_d, ch_d = torch.from_numpy(rx.reshape(-1)).cuda(), torch.from_numpy(ch.reshape(-1)).cuda()
    sh_d, nv_d = torch.from_numpy(shift).cuda(), torch.from_numpy(nvar).cuda()
    for pad in (0, 2, 4):
        rec_d = torch.full((want.size + 8,), CANARY, dtype=torch.int16, device="cuda")
        m.ulsch_mmse_2layers_grid(rx_d, ch_d, n_rx, rx_stride, ch_stride, segs, sh_d, nv_d, rec_d[pad:])
        torch.cuda.synchronize()
        got = rec_d.cpu().numpy()
        assert (got[:pad] == CANARY).all() and (got[pad + want.size:] == CANARY).all()
        assert np.array_equal(got[pad:pad + want.size], want), (Qm, n_rx, pad, np.flatnonzero(got[pad:pad + want.size] != want)[:8])
        assert np.array_equal(got[pad:pad + want.size], rec)                       # HOST and DEVICE modes agree
    assert np.array_equal(rx_d.cpu().numpy(), rx0.reshape(-1)) and np.array_equal(ch_d.cpu().numpy(), ch0.reshape(-1))


def level_case(n_rx):
    """three blocks' measurement symbols, one of each pattern, named in any order; estimates of three sizes"""
    rng = np.random.default_rng(70 + n_rx)
    N, cs = 512, 3 * 512 + 40
    ch = (rng.integers(-32768, 32768, (2 * n_rx, cs, 2)) >> np.array([0, 4, 6])[rng.integers(0, 3, (2 * n_rx, 1, 1))]).astype(np.int16)
    first = [dict(tb=2, Qm=6, pattern=DMRS1, nb_re=18, plane=400, sym_off=0, fft_size=N, start_re=500, rx_off=0, ch_off=7, rec_off=0),
             dict(tb=0, Qm=8, pattern=FULL, nb_re=300, plane=800, sym_off=0, fft_size=N, start_re=3, rx_off=0, ch_off=N + 1, rec_off=0),
             dict(tb=1, Qm=6, pattern=DMRS2, nb_re=8 * 13, plane=400, sym_off=0, fft_size=N, start_re=0, rx_off=0, ch_off=2 * N + 9, rec_off=0)]
    max_ch = np.array([1500, 2048, 32767], np.int32)                              # shift_ch_ext 0, 1, 4: both branches of the scale
    return ch, cs, first, max_ch


@pytest.mark.parametrize("n_rx", [2, 4])
def test_level_grid_mmse_equals_numpy(hip, n_rx):
    import torch
    m = hip.ldpc
    ch, cs, first, max_ch = level_case(n_rx)
    want = np.zeros(3, np.int32)
    for f in first:
        pairs = extract_np(ch[:1], ch, f)[1].reshape(2, n_rx, f["nb_re"], 2)
        want[f["tb"]] = level_mmse_np(pairs, int(max_ch[f["tb"]]))[0]
    assert len(set(want.tolist())) > 1
    got = m.ulsch_channel_level_grid_mmse(ch.reshape(-1), n_rx, cs, first, max_ch)
    assert got.tolist() == want.tolist()
    lv_d = torch.full((5,), -7, dtype=torch.int32, device="cuda")
    m.ulsch_channel_level_grid_mmse(torch.from_numpy(ch.reshape(-1)).cuda(), n_rx, cs, first, torch.from_numpy(max_ch).cuda(), out=lv_d)
    torch.cuda.synchronize()
    assert lv_d.cpu().numpy().tolist() == want.tolist() + [-7, -7]


# ---- end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Qm,n_rx", [(6, 2), (6, 4), (8, 2), (8, 4)])
def test_two_layer_front_then_decode_symbols(hip, Qm, n_rx):
    """dlsch_encode_symbols with Nl = 2 as the transmitter, the channel test_rx_mmse_host.py decodes with the reference arithmetic
    alone, estimates supplied by the test; level -> MMSE -> decode_symbols on one stream"""
    import torch
    m = hip.ldpc
    tb, scr, pay, syms, H, max_ch, seed = mmse_e2e_case(Qm, n_rx)
    N, rb, S = 256, syms[0] // 12, tb["G"] // Qm
    po, co, ho, nseg = m.tb_layout([tb])
    al = dict(tb=0, Qm=Qm, dmrs_config_type=0, num_dmrs_cdm_grps_no_data=1, dmrs_symbol=2, fft_size=N, first_carrier_offset=N - 6 * 8, bwp_start=0,
              rb_start=2, rb_size=rb, start_symbol=0, nr_of_symbols=14, ul_dmrs_symb_pos=1 << 2, plane=S, rx_slot_off=N, ch_off=9, rec_off=int(co[0]))
    segs, first = m.pusch_grid_segments([al])
    assert [s["nb_re"] for s in segs] == syms and all(s["plane"] == 2 * sum(syms) for s in segs)
    tx = m.dlsch_encode_symbols_host([tb], [pay], [scr])[0]
    assert tx.shape == (2, sum(syms), 2)
    rx_e, ch_e = mmse_e2e_channel(tx, H, seed)
    rx_stride, ch_stride = 15 * N + 5, 14 * N + 64
    rx = np.full((n_rx, rx_stride, 2), 1234, np.int16)
    ch = np.full((2 * n_rx, ch_stride, 2), -4321, np.int16)
    ch[:, segs[0]["ch_off"]:segs[0]["ch_off"] + 12 * rb] = H.reshape(2 * n_rx, 1, 2)       # a flat channel: the DMRS symbol's estimates
    for s in segs:
        idx = np.array([p_of(s["pattern"], j) for j in range(s["nb_re"])])
        rx[:, s["rx_off"] + (s["start_re"] + idx) % N] = rx_e[:, s["sym_off"]:s["sym_off"] + s["nb_re"]]
    lv = level_mmse_np(ch_e[:, :, :syms[0]], max_ch)[0]
    rec_np = np.zeros(int(co[-1]) + 16, np.int16)
    rec_np[co[0]:co[0] + tb["G"]] = mmse_e2e_record(tb, syms, rx_e, ch_e, lv)
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
                mc_d = torch.tensor([max_ch], dtype=torch.int32, device="cuda")
                nv_d = torch.tensor([E2E_NVAR], dtype=torch.int32, device="cuda")
                m.ulsch_channel_level_grid_mmse(ch_d, n_rx, ch_stride, first, mc_d, out=lv_d)
                m.ulsch_mmse_2layers_grid(rx_d, ch_d, n_rx, rx_stride, ch_stride, segs, lv_d, nv_d, rec)
            else:
                rec = torch.from_numpy(rec_np).cuda()
            m.ulsch_decode_symbols_device(rxt, rec, harq, out, ack, itm, [scr])
        torch.cuda.synchronize()
        if which == 0:
            assert lv_d.cpu().numpy().tolist() == [lv] and np.array_equal(rec.cpu().numpy(), rec_np)
        outs.append((out.cpu().numpy()[po[0]:po[0] + tb["A"] // 8], ack.cpu().numpy(), itm.cpu().numpy(), harq.cpu().numpy()))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    assert outs[0][1].all() and np.array_equal(outs[0][0], pay)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_rx_mmse_invalid_input(hip):
    import torch
    m = hip.ldpc
    L = m._rxm_lib()
    n_rx, N = 2, 128
    rs, cs = 2 * N, N + 8
    good = dict(tb=0, Qm=6, pattern=DMRS1, nb_re=16, plane=64, sym_off=4, fft_size=N, start_re=100, rx_off=N, ch_off=3, rec_off=0)
    rx_h, ch_h = np.zeros(2 * n_rx * rs, np.int16), np.zeros(2 * 2 * n_rx * cs, np.int16)
    rec_h, sh_h, nv_h, mc_h, lv_h = (np.full(1024, CANARY, np.int16), np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32),
                                     np.full(2, -7, np.int32))
    dev = lambda a: torch.from_numpy(a.copy()).cuda()
    rx_d, ch_d, rec_d, sh_d, nv_d, mc_d, lv_d = dev(rx_h), dev(ch_h), dev(rec_h), dev(sh_h), dev(nv_h), dev(mc_h), dev(lv_h)
    addr = lambda a: a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()

    def mmse(mode, segs, n=n_rx, mem=None, stream=None, desc=True, **swap):
        """swap: an array's name -> None, or another address"""
        arrs = dict(rx=rx_h, ch=ch_h, shift=sh_h, nvar=nv_h, rec=rec_h) if mode == "host" else dict(rx=rx_d, ch=ch_d, shift=sh_d, nvar=nv_d, rec=rec_d)
        p = {k: swap.get(k, addr(v)) for k, v in arrs.items()}
        mem = (m.MEM_HOST if mode == "host" else m.MEM_DEVICE) if mem is None else mem
        return L.nrLDPC_hip_ulsch_mmse_2layers_grid(p["rx"], p["ch"], n, rs, cs, m._rx_grid_seg_array(segs) if desc else None, len(segs), p["shift"],
                                                    p["nvar"], p["rec"], mem, stream)

    def level(mode, fs, n=n_rx, mem=None, stream=None, desc=True, **swap):
        arrs = dict(ch=ch_h, max_ch=mc_h, out=lv_h) if mode == "host" else dict(ch=ch_d, max_ch=mc_d, out=lv_d)
        p = {k: swap.get(k, addr(v)) for k, v in arrs.items()}
        mem = (m.MEM_HOST if mode == "host" else m.MEM_DEVICE) if mem is None else mem
        return L.nrLDPC_hip_ulsch_channel_level_grid_mmse(p["ch"], n, cs, m._rx_grid_seg_array(fs) if desc else None, len(fs), p["max_ch"], p["out"],
                                                          mem, stream)

    for mode in ("host", "device"):
        bad_calls = [
            (lambda: mmse(mode, [good], rx=None), "null"), (lambda: mmse(mode, [good], ch=None), "null"),
            (lambda: mmse(mode, [good], shift=None), "null"), (lambda: mmse(mode, [good], nvar=None), "null"),
            (lambda: mmse(mode, [good], rec=None), "null"), (lambda: mmse(mode, [good], desc=False), "null"),
            (lambda: mmse(mode, [good], n=1), "n_rx"), (lambda: mmse(mode, [good], n=3), "n_rx"), (lambda: mmse(mode, [good], n=8), "n_rx"),
            (lambda: mmse(mode, [dict(good, Qm=4)]), "Qm"), (lambda: mmse(mode, [dict(good, Qm=2)]), "Qm"), (lambda: mmse(mode, [dict(good, Qm=7)]), "Qm"),
            (lambda: mmse(mode, [dict(good, rec_off=3)]), "even"),
            (lambda: mmse(mode, [dict(good, sym_off=17)]), "plane"),                               # 2 (17 + 16) = 66 > 64
            (lambda: mmse(mode, [dict(good, sym_off=0, nb_re=16), dict(good, sym_off=15, nb_re=8)]), "overlap"),   # entries 30, 31 twice
            (lambda: mmse(mode, [dict(good, pattern=FULL, fft_size=1 << 21, Qm=8, nb_re=(1 << 17) + 1, plane=1 << 19)]), "2^21"),
            (lambda: mmse(mode, [good], mem=7), "mem"),
            (lambda: mmse(mode, [dict(good, pattern=3)]), "pattern"),
            (lambda: mmse(mode, [dict(good, start_re=N)]), "start_re"), (lambda: mmse(mode, [dict(good, fft_size=0)]), "start_re"),
            (lambda: mmse(mode, [dict(good, plane=300, nb_re=65)]), "count"),
            (lambda: level(mode, [good], ch=None), "null"), (lambda: level(mode, [good], out=None), "null"),
            (lambda: level(mode, [good], max_ch=None), "null"), (lambda: level(mode, [good], desc=False), "null"),
            (lambda: level(mode, [good], n=1), "n_rx"), (lambda: level(mode, [good], n=5), "n_rx"),
            (lambda: level(mode, [dict(good, nb_re=0)]), "no REs"),
            (lambda: level(mode, [dict(good, tb=1)]), "tb"), (lambda: level(mode, [good, good]), "tb"),
            (lambda: level(mode, [good], mem=3), "mem"),
            (lambda: level(mode, [dict(good, pattern=7)]), "pattern"), (lambda: level(mode, [dict(good, nb_re=65)]), "count"),
        ]
        for call, why in bad_calls:
            assert call() < 0, (mode, why)
            assert why in m.last_error(), (mode, why, m.last_error())
    # DEVICE mem with a host array, and a record that is not 4-byte aligned
    for name, host in (("rx", rx_h), ("ch", ch_h), ("shift", sh_h), ("nvar", nv_h), ("rec", rec_h)):
        assert mmse("device", [good], **{name: addr(host)}) < 0 and "device memory" in m.last_error(), name
    assert mmse("device", [good], rec=rec_d.data_ptr() + 2) < 0 and "4-byte" in m.last_error()
    for name, host in (("ch", ch_h), ("max_ch", mc_h), ("out", lv_h)):
        assert level("device", [good], **{name: addr(host)}) < 0 and "device memory" in m.last_error(), name
    # the wrappers know the extents: a descriptor that reaches outside is refused before the call
    with pytest.raises(ValueError):
        m.ulsch_mmse_2layers_grid(rx_d, ch_d, n_rx, rs, cs, [dict(good, rx_off=3 * N + 1)], sh_d, nv_d, rec_d)
    with pytest.raises(ValueError):
        m.ulsch_mmse_2layers_grid(rx_d, ch_d, n_rx, rs, cs, [dict(good, ch_off=cs + 8 - 31)], sh_d, nv_d, rec_d)      # the last pair leaves ch
    with pytest.raises(ValueError):
        m.ulsch_mmse_2layers_grid(rx_d, ch_d, n_rx, rs, cs, [dict(good, plane=2000, sym_off=900)], sh_d, nv_d, rec_d)
    with pytest.raises(ValueError):
        m.ulsch_channel_level_grid_mmse(ch_d, n_rx, cs, [dict(good, ch_off=cs + 8 - 31)], mc_d, out=lv_d)
    # a stream that is being captured
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    note = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        note.add_(1)
        rc_c = mmse("device", [good], stream=side.cuda_stream)
        err_c = m.last_error()
        rc_l = level("device", [good], stream=side.cuda_stream)
        err_l = m.last_error()
    assert rc_c < 0 and "captured" in err_c and rc_l < 0 and "captured" in err_l
    torch.cuda.synchronize()
    assert (rec_d.cpu().numpy() == CANARY).all() and (rec_h == CANARY).all()
    assert (lv_d.cpu().numpy() == -7).all() and (lv_h == -7).all()
    # and the same arguments without the fault are accepted: a zero channel gives zeros, in the segment's doubled range alone
    assert mmse("device", [good]) == 0 and mmse("host", [good]) == 0 and level("device", [good]) == 0 and level("host", [good]) == 0
    torch.cuda.synchronize()
    for rec in (rec_h, rec_d.cpu().numpy()):
        lo = 2 * 2 * good["sym_off"]
        for k in range(3):
            o = 2 * k * good["plane"] + lo
            assert (rec[o:o + 4 * good["nb_re"]] == 0).all() and rec[o - 1] == CANARY and rec[o + 4 * good["nb_re"]] == CANARY
    assert lv_h[0] == 0 and int(lv_d[0]) == 0
