"""The two-layer max-log ML receiver on the GPU (nrLDPC_hip_ulsch_ml_2layers_grid / _channel_level_grid_ml), bit for bit against the
numpy restatement of the reference (rx_ml_np.py) on arrays extracted in numpy; its write set; HOST against DEVICE mode; its
refusals; and end to end from dlsch_encode_symbols with Nl = 2 through the channel that test_rx_ml_host.py fixes, level, ML and
decode_scrambled on one stream, once with the DMRS estimator of ports 0 and 1 in front.

A thread takes the group of REs 4g .. 4g + 3 of its segment, a workgroup PIECE_GROUPS of them.  A segment whose RE w is the first
one behind the grid's wrap (start_re = N - p(w)) has the wrap between two groups when w % 4 == 0 and inside a group otherwise;
grid_case() places every pattern both ways and checks that it did."""
import numpy as np
import pytest

import ul_slot_np as U
from rx_ml_np import level_ml_np, llr_np, ml_np
from test_gpu_rx_grid import extract_np, p_of
from test_gpu_rx_mmse import level_case
from test_rx_ml_host import ml_e2e_case, ml_e2e_llr
from test_rx_mmse_host import mmse_e2e_channel

pytestmark = pytest.mark.gpu
CANARY = 0x5a5a
FULL, DMRS1, DMRS2 = 0, 1, 2
PER_RB = {FULL: 12, DMRS1: 6, DMRS2: 8}
PIECE_GROUPS = 256                     # NR_RXF_THREADS: the groups of one workgroup


def pairs_np(rx, ch, s, n_rx):
    """rx int16 [n_rx, nb_re, 2], ch int16 [2, n_rx, nb_re, 2] of a segment; ch holds the 2 n_rx pairs one stride apart"""
    a, b = extract_np(rx, ch, s)
    return a, b.reshape(2, n_rx, s["nb_re"], 2)


def grid_case(rng, qms, n_rx):
    """Two blocks with a shift each, block tb at Qm qms[tb].  Block 0 (N = 128): every pattern with 1 and 3 RBs -- DMRS1 gives 6 and
    18 REs, a partial last group -- each with the wrap between two groups, inside one, and not at all.  Block 1 (N = 2048): 90 RBs
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
                w = 4 * max(1, nb // 8) if rb < 90 else 4 * (PIECE_GROUPS + 1)          # the first RE behind the wrap
                w += place == "inside"
                assert 0 < w < nb
                start_re = N - p_of(pattern, w) if place != "none" else 7
                if place != "none":
                    kinds.add((pattern, rb, w % 4 == 0))
                mine.append(dict(tb=tb, Qm=qms[tb], pattern=pattern, nb_re=nb, sym_off=off, fft_size=N, start_re=start_re, rx_off=rx_at, ch_off=ch_at,
                                 rec_off=rec_at))
                off += nb + len(mine) % 3
                rx_at += N + len(mine) % 2
                ch_at += p_of(pattern, nb - 1) + 1 + len(mine) % 4
        plane = 2 * off + int(rng.integers(0, 5))
        for s in mine:
            s["plane"] = plane
        segs += mine
        rec_at += qms[tb] * plane + 2 * int(rng.integers(0, 4))
    assert kinds == {(p, rb, b) for p in (FULL, DMRS1, DMRS2) for rb in (1, 3) for b in (True, False)} | {(FULL, 90, True), (FULL, 90, False)}
    big = [s for s in segs if s["nb_re"] == 1080]
    assert big and all((s["nb_re"] + 3) // 4 > PIECE_GROUPS for s in big)                # it really spans two workgroups
    assert any(s["sym_off"] & 1 for s in segs) and any(s["nb_re"] % 4 for s in segs)
    rx_stride, ch_stride = rx_at + 11, ch_at + 6
    rx = rng.integers(-32768, 32768, (n_rx, rx_stride, 2)).astype(np.int16)
    ch = rng.integers(-32768, 32768, (2 * n_rx, ch_stride, 2)).astype(np.int16)
    for s in segs:                                                                         # block 1: a channel of moderate size
        if s["tb"] == 1:
            ch[:, s["ch_off"]:s["ch_off"] + p_of(s["pattern"], s["nb_re"] - 1) + 1] >>= 5
    shift = np.array([3, 9] if qms[0] == 2 else [0, 6], np.int32)
    want = np.full(rec_at + 64, CANARY, np.int16)
    for s in segs:
        a, b = pairs_np(rx, ch, s, n_rx)
        llr_np(want, ml_np(a, b, s["Qm"], int(shift[s["tb"]])), s["Qm"], s["sym_off"], s["rec_off"])
    return segs, rx, ch, rx_stride, ch_stride, shift, want


@pytest.mark.parametrize("n_rx,qms", [(2, (2, 2)), (4, (2, 2)), (3, (2, 2)), (2, (4, 4)), (4, (4, 4)), (3, (4, 4)), (2, (2, 4)), (4, (4, 2)), (3, (2, 4))])
def test_ml_grid_equals_numpy(hip, n_rx, qms):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(3000 * qms[0] + 100 * qms[1] + n_rx)
    segs, rx, ch, rx_stride, ch_stride, shift, want = grid_case(rng, qms, n_rx)
    rx0, ch0 = rx.copy(), ch.copy()
    # the write set: only int16 rec_off + 2 Qm sym_off .. rec_off + 2 Qm (sym_off + nb_re) - 1 of each segment differ from the canary
    touched = np.zeros(want.size, bool)
    for s in segs:
        o = s["rec_off"] + 2 * s["Qm"] * s["sym_off"]
        assert not touched[o:o + 2 * s["Qm"] * s["nb_re"]].any()
        touched[o:o + 2 * s["Qm"] * s["nb_re"]] = True
    assert (want[~touched] == CANARY).all() and (~touched).sum() > 100
    # host mode
    llr = np.full(want.size, CANARY, np.int16)
    m.ulsch_ml_2layers_grid(rx.reshape(-1), ch.reshape(-1), n_rx, rx_stride, ch_stride, segs, shift, llr)
    assert np.array_equal(llr, want), (qms, n_rx, "host", np.flatnonzero(llr != want)[:8])
    assert np.array_equal(rx, rx0) and np.array_equal(ch, ch0)
    # device mode, the LLR array 16-, 4- and 8-byte aligned
    rx_d, ch_d = torch.from_numpy(rx.reshape(-1)).cuda(), torch.from_numpy(ch.reshape(-1)).cuda()
    sh_d = torch.from_numpy(shift).cuda()
    for pad in (0, 2, 4):
        llr_d = torch.full((want.size + 8,), CANARY, dtype=torch.int16, device="cuda")
        m.ulsch_ml_2layers_grid(rx_d, ch_d, n_rx, rx_stride, ch_stride, segs, sh_d, llr_d[pad:])
        torch.cuda.synchronize()
        got = llr_d.cpu().numpy()
        assert (got[:pad] == CANARY).all() and (got[pad + want.size:] == CANARY).all()
        assert np.array_equal(got[pad:pad + want.size], want), (qms, n_rx, pad, np.flatnonzero(got[pad:pad + want.size] != want)[:8])
        assert np.array_equal(got[pad:pad + want.size], llr)                       # HOST and DEVICE modes agree
    assert np.array_equal(rx_d.cpu().numpy(), rx0.reshape(-1)) and np.array_equal(ch_d.cpu().numpy(), ch0.reshape(-1))


@pytest.mark.parametrize("n_rx", [2, 4, 3])
def test_level_grid_ml_equals_numpy(hip, n_rx):
    import torch
    m = hip.ldpc
    ch, cs, first, max_ch = level_case(n_rx)
    first = [dict(f, Qm=2 + 2 * (f["tb"] & 1)) for f in first]
    want = np.zeros(3, np.int32)
    for f in first:
        pairs = extract_np(ch[:1], ch, f)[1].reshape(2, n_rx, f["nb_re"], 2)
        want[f["tb"]] = level_ml_np(pairs, int(max_ch[f["tb"]]))[0]
    assert len(set(want.tolist())) > 1
    got = m.ulsch_channel_level_grid_ml(ch.reshape(-1), n_rx, cs, first, max_ch)
    assert got.tolist() == want.tolist()
    lv_d = torch.full((5,), -7, dtype=torch.int32, device="cuda")
    m.ulsch_channel_level_grid_ml(torch.from_numpy(ch.reshape(-1)).cuda(), n_rx, cs, first, torch.from_numpy(max_ch).cuda(), out=lv_d)
    torch.cuda.synchronize()
    assert lv_d.cpu().numpy().tolist() == want.tolist() + [-7, -7]


# ---- end to end ----------------------------------------------------------------------------------------------------------
def decode_scrambled(m, tb, scr, llr_d, side):
    """ulsch_decode_scrambled on `side`; returns the tensors"""
    import torch
    po, co, ho, nseg = m.tb_layout([tb])
    rxt = [dict(tb, round=0, llrLen=0)]
    harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
    out = torch.zeros(int(po[-1]) + 16, dtype=torch.uint8, device="cuda")
    ack = torch.zeros(1, dtype=torch.uint8, device="cuda")
    itm = torch.zeros(1, dtype=torch.int32, device="cuda")
    m.ulsch_decode_scrambled_device(rxt, llr_d, harq, out, ack, itm, [scr])
    return out, ack, itm, harq


@pytest.mark.parametrize("Qm,n_rx", [(2, 2), (2, 4), (4, 2), (4, 4)])
def test_two_layer_front_then_decode_scrambled(hip, Qm, n_rx):
    """dlsch_encode_symbols with Nl = 2 as the transmitter, the channel test_rx_ml_host.py decodes with the reference arithmetic
    alone, estimates supplied by the test; level -> ML -> decode_scrambled on one stream"""
    import torch
    m = hip.ldpc
    tb, scr, pay, syms, H, max_ch, seed = ml_e2e_case(Qm, n_rx)
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
    lv = level_ml_np(ch_e[:, :, :syms[0]], max_ch)[0]
    assert lv == 9
    llr_want = np.zeros(int(co[-1]) + 16, np.int16)
    llr_want[co[0]:co[0] + tb["G"]] = ml_e2e_llr(tb, syms, rx_e, ch_e, lv)
    outs = []
    side = torch.cuda.Stream()
    for which in (0, 1):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            if which == 0:
                rx_d, ch_d = torch.from_numpy(rx.reshape(-1)).cuda(), torch.from_numpy(ch.reshape(-1)).cuda()
                llr = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
                lv_d = torch.zeros(1, dtype=torch.int32, device="cuda")
                mc_d = torch.tensor([max_ch], dtype=torch.int32, device="cuda")
                m.ulsch_channel_level_grid_ml(ch_d, n_rx, ch_stride, first, mc_d, out=lv_d)
                m.ulsch_ml_2layers_grid(rx_d, ch_d, n_rx, rx_stride, ch_stride, segs, lv_d, llr)
            else:
                llr = torch.from_numpy(llr_want).cuda()
            out, ack, itm, harq = decode_scrambled(m, tb, scr, llr, side)
        torch.cuda.synchronize()
        if which == 0:
            assert lv_d.cpu().numpy().tolist() == [lv] and np.array_equal(llr.cpu().numpy(), llr_want)
        outs.append((out.cpu().numpy()[po[0]:po[0] + tb["A"] // 8], ack.cpu().numpy(), itm.cpu().numpy(), harq.cpu().numpy()))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    assert outs[0][1].all() and np.array_equal(outs[0][0], pay)


def test_selective_slot_with_the_estimator_in_front(hip):
    """A two-layer 16QAM block on a frequency-selective 4 x 2 channel with DMRS ports 0 and 1 on the air (ul_slot_np.build_slot):
    pusch_channel_estimation for both layers' descriptors, channel_level_grid_ml, ml_2layers_grid and decode_scrambled on one side
    stream.  ul_ch equals the CPU form's estimates, the level and the LLRs the numpy receiver's on those estimates, and the block
    decodes."""
    import torch
    m = hip.ldpc
    case = U._case("2L-T1I-ml", U.T1I, (0, 1), 4, 4, 512, (7, -6, 5, -7), U.GAIN_2L, 0.007, 10, 0.50, 31, delay_factor=2.0)
    sl = U.build_slot(m, case)
    tb, n_rx = sl["tb"], 4
    ch_want = U.estimate_host(m, sl)
    lv_want = level_ml_np(U._extract(sl, ch_want, sl["first"][0])[1].reshape(2, n_rx, -1, 2), sl["max_ch"])[0]
    assert lv_want == 9
    co = m.tb_layout([tb])[1]
    llr_want = np.zeros(int(co[-1]) + 16, np.int16)
    for s in sl["gsegs"]:
        a, b = U._extract(sl, ch_want, s)
        llr_np(llr_want, ml_np(a, b.reshape(2, n_rx, s["nb_re"], 2), 4, lv_want), 4, s["sym_off"], s["rec_off"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rx_d = torch.from_numpy(sl["rx"].reshape(-1).copy()).cuda()
        ch_d = torch.full((2 * n_rx * sl["ch_stride"] * 2,), U.FILL, dtype=torch.int16, device="cuda")
        llr = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
        lv_d = torch.zeros(1, dtype=torch.int32, device="cuda")
        mc_d = torch.tensor([sl["max_ch"]], dtype=torch.int32, device="cuda")
        m.pusch_channel_estimation(rx_d, sl["rx_stride"], ch_d, sl["ch_stride"], n_rx, sl["csegs"], torch.from_numpy(sl["delay"].copy()).cuda())
        m.ulsch_channel_level_grid_ml(ch_d, n_rx, sl["ch_stride"], sl["first"], mc_d, out=lv_d)
        m.ulsch_ml_2layers_grid(rx_d, ch_d, n_rx, sl["rx_stride"], sl["ch_stride"], sl["gsegs"], lv_d, llr)
        out, ack, itm, harq = decode_scrambled(m, tb, sl["scr"], llr, side)
    torch.cuda.synchronize()
    assert np.array_equal(ch_d.cpu().numpy().reshape(-1, 2), ch_want)
    assert int(lv_d[0]) == lv_want and np.array_equal(llr.cpu().numpy(), llr_want)
    assert ack.cpu().numpy().all() and np.array_equal(out.cpu().numpy()[:tb["A"] // 8], sl["pay"]), itm


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_rx_ml_invalid_input(hip):
    import torch
    m = hip.ldpc
    L = m._rxl_lib()
    n_rx, N = 2, 128
    rs, cs = 2 * N, N + 8
    good = dict(tb=0, Qm=4, pattern=DMRS1, nb_re=16, plane=64, sym_off=4, fft_size=N, start_re=100, rx_off=N, ch_off=3, rec_off=0)
    rx_h, ch_h = np.zeros(2 * 8 * rs, np.int16), np.zeros(2 * 2 * 8 * cs, np.int16)
    llr_h, sh_h, mc_h, lv_h = np.full(1024, CANARY, np.int16), np.zeros(2, np.int32), np.zeros(2, np.int32), np.full(2, -7, np.int32)
    dev = lambda a: torch.from_numpy(a.copy()).cuda()
    rx_d, ch_d, llr_d, sh_d, mc_d, lv_d = dev(rx_h), dev(ch_h), dev(llr_h), dev(sh_h), dev(mc_h), dev(lv_h)
    addr = lambda a: a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()

    def ml(mode, segs, n=n_rx, mem=None, stream=None, desc=True, **swap):
        """swap: an array's name -> None, or another address"""
        arrs = dict(rx=rx_h, ch=ch_h, shift=sh_h, llr=llr_h) if mode == "host" else dict(rx=rx_d, ch=ch_d, shift=sh_d, llr=llr_d)
        p = {k: swap.get(k, addr(v)) for k, v in arrs.items()}
        mem = (m.MEM_HOST if mode == "host" else m.MEM_DEVICE) if mem is None else mem
        return L.nrLDPC_hip_ulsch_ml_2layers_grid(p["rx"], p["ch"], n, rs, cs, m._rx_grid_seg_array(segs) if desc else None, len(segs), p["shift"],
                                                  p["llr"], mem, stream)

    def level(mode, fs, n=n_rx, mem=None, stream=None, desc=True, **swap):
        arrs = dict(ch=ch_h, max_ch=mc_h, out=lv_h) if mode == "host" else dict(ch=ch_d, max_ch=mc_d, out=lv_d)
        p = {k: swap.get(k, addr(v)) for k, v in arrs.items()}
        mem = (m.MEM_HOST if mode == "host" else m.MEM_DEVICE) if mem is None else mem
        return L.nrLDPC_hip_ulsch_channel_level_grid_ml(p["ch"], n, cs, m._rx_grid_seg_array(fs) if desc else None, len(fs), p["max_ch"], p["out"],
                                                        mem, stream)

    for mode in ("host", "device"):
        bad_calls = [
            (lambda: ml(mode, [good], rx=None), "null"), (lambda: ml(mode, [good], ch=None), "null"),
            (lambda: ml(mode, [good], shift=None), "null"), (lambda: ml(mode, [good], llr=None), "null"), (lambda: ml(mode, [good], desc=False), "null"),
            (lambda: ml(mode, [good], n=0), "n_rx"), (lambda: ml(mode, [good], n=9), "n_rx"),
            (lambda: ml(mode, [dict(good, Qm=6)]), "Qm"), (lambda: ml(mode, [dict(good, Qm=8)]), "Qm"), (lambda: ml(mode, [dict(good, Qm=3)]), "Qm"),
            (lambda: ml(mode, [dict(good, rec_off=3)]), "even"),
            (lambda: ml(mode, [dict(good, sym_off=17)]), "plane"),                                 # 2 (17 + 16) = 66 > 64
            (lambda: ml(mode, [dict(good, sym_off=0, nb_re=16), dict(good, sym_off=15, nb_re=8)]), "overlap"),     # RE 15 twice
            (lambda: ml(mode, [dict(good, Qm=2, sym_off=0, nb_re=16), dict(good, Qm=4, rec_off=60, sym_off=0, nb_re=4)]), "overlap"),   # int16 60 .. 63 twice
            (lambda: ml(mode, [dict(good, pattern=FULL, fft_size=1 << 21, nb_re=(1 << 18) + 1, plane=1 << 20)]), "2^21"),
            (lambda: ml(mode, [good], mem=7), "mem"),
            (lambda: ml(mode, [dict(good, pattern=3)]), "pattern"),
            (lambda: ml(mode, [dict(good, start_re=N)]), "start_re"), (lambda: ml(mode, [dict(good, fft_size=0)]), "start_re"),
            (lambda: ml(mode, [dict(good, plane=300, nb_re=65)]), "count"),
            (lambda: level(mode, [good], ch=None), "null"), (lambda: level(mode, [good], out=None), "null"),
            (lambda: level(mode, [good], max_ch=None), "null"), (lambda: level(mode, [good], desc=False), "null"),
            (lambda: level(mode, [good], n=0), "n_rx"), (lambda: level(mode, [good], n=9), "n_rx"),
            (lambda: level(mode, [dict(good, nb_re=0)]), "no REs"),
            (lambda: level(mode, [dict(good, tb=1)]), "tb"), (lambda: level(mode, [good, good]), "tb"),
            (lambda: level(mode, [good], mem=3), "mem"),
            (lambda: level(mode, [dict(good, pattern=7)]), "pattern"), (lambda: level(mode, [dict(good, nb_re=65)]), "count"),
        ]
        for call, why in bad_calls:
            assert call() < 0, (mode, why)
            assert why in m.last_error(), (mode, why, m.last_error())
    # DEVICE mem with a host array, and an LLR array that is not 4-byte aligned
    for name, host in (("rx", rx_h), ("ch", ch_h), ("shift", sh_h), ("llr", llr_h)):
        assert ml("device", [good], **{name: addr(host)}) < 0 and "device memory" in m.last_error(), name
    assert ml("device", [good], llr=llr_d.data_ptr() + 2) < 0 and "4-byte" in m.last_error()
    for name, host in (("ch", ch_h), ("max_ch", mc_h), ("out", lv_h)):
        assert level("device", [good], **{name: addr(host)}) < 0 and "device memory" in m.last_error(), name
    # the wrappers know the extents: a descriptor that reaches outside is refused before the call
    with pytest.raises(ValueError):
        m.ulsch_ml_2layers_grid(rx_d, ch_d, n_rx, rs, cs, [dict(good, rx_off=15 * N + 1)], sh_d, llr_d)
    with pytest.raises(ValueError):
        m.ulsch_ml_2layers_grid(rx_d, ch_d, n_rx, rs, cs, [dict(good, ch_off=13 * cs - 31)], sh_d, llr_d)             # the last pair leaves ch
    with pytest.raises(ValueError):
        m.ulsch_ml_2layers_grid(rx_d, ch_d, n_rx, rs, cs, [dict(good, plane=2000, sym_off=900)], sh_d, llr_d)
    with pytest.raises(ValueError):
        m.ulsch_channel_level_grid_ml(ch_d, n_rx, cs, [dict(good, ch_off=13 * cs - 31)], mc_d, out=lv_d)
    # a stream that is being captured
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    note = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        note.add_(1)
        rc_c = ml("device", [good], stream=side.cuda_stream)
        err_c = m.last_error()
        rc_l = level("device", [good], stream=side.cuda_stream)
        err_l = m.last_error()
    assert rc_c < 0 and "captured" in err_c and rc_l < 0 and "captured" in err_l
    torch.cuda.synchronize()
    assert (llr_d.cpu().numpy() == CANARY).all() and (llr_h == CANARY).all()
    assert (lv_d.cpu().numpy() == -7).all() and (lv_h == -7).all()
    # and the same arguments without the fault are accepted, for 2, 3 and 8 antennas: a zero channel gives zero LLRs, in the
    # segment's range alone
    for n in (2, 3, 8):
        assert ml("device", [good], n=n) == 0 and ml("host", [good], n=n) == 0 and level("device", [good], n=n) == 0 and level("host", [good], n=n) == 0
    torch.cuda.synchronize()
    for llr in (llr_h, llr_d.cpu().numpy()):
        o, n = 2 * 4 * good["sym_off"], 2 * 4 * good["nb_re"]
        assert (llr[o:o + n] == 0).all() and (llr[:o] == CANARY).all() and (llr[o + n:] == CANARY).all()
    assert lv_h[0] == 0 and int(lv_d[0]) == 0
