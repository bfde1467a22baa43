"""The UL receive front on the GPU (nrLDPC_hip_ulsch_channel_level / _channel_compensation) against the numpy restatement of the
reference (rx_front_np.py), bit for bit; composed with nrLDPC_hip_ulsch_llr; and end to end in front of
nrLDPC_hip_ulsch_decode_symbols against the existing path fed with numpy-compensated records."""
import ctypes as C

import numpy as np
import pytest

from qam_np import demap_np
from rx_front_np import compensate_np, level_np
from test_gpu_tb_chain import valid_tbs
from test_gpu_tb_scrambled import rand_scr

pytestmark = pytest.mark.gpu
CANARY = 0x5a5a
SEG_LENGTHS = [1, 3, 4, 6 * 51, 12 * 273, 4093]
SHIFTS = (0, 1, 7, 12, 15, 16, 31)


def kernel_case(rng, Qm, n_rx, n_blocks=3):
    """blocks with several segments each; gaps of 0..3 c16 between segments so that the outputs start 16-, 4-, 8- and 12-byte
    aligned; records with room for four planes whatever the Qm; inputs with a gap between the antennas.  Returns the descriptors,
    the inputs [n_rx, stride, 2], the record array size and what it must hold afterwards."""
    segs, at, rec_at = [], 3, 2
    blocks = []
    for b in range(n_blocks):
        lens = [int(x) for x in rng.permutation(SEG_LENGTHS)][:3 + b] if b else list(SEG_LENGTHS)
        offs, off = [], int(rng.integers(0, 4))
        for k, nb in enumerate(lens):
            offs.append(off)
            off += nb + (k + b) % 4
        plane = off + int(rng.integers(0, 5))
        for nb, so in zip(lens, offs):
            segs.append(dict(tb=b, Qm=Qm, nb_re=nb, plane=plane, sym_off=so, rx_off=at, ch_off=at + 1, rec_off=rec_at))
            at += nb + int(rng.integers(0, 3))
        blocks.append((rec_at, plane))
        rec_at += 2 * 4 * plane + 2 * int(rng.integers(0, 4))
    stride = at + 7
    rx = rng.integers(-32768, 32768, (n_rx, stride, 2)).astype(np.int16)
    ch = rng.integers(-32768, 32768, (n_rx, stride, 2)).astype(np.int16)
    for b in range(n_blocks):                                     # some blocks with a channel of moderate size
        if b % 2:
            for s in segs:
                if s["tb"] == b:
                    ch[:, s["ch_off"]:s["ch_off"] + s["nb_re"]] >>= 4 + b
    shift = np.array([SHIFTS[(b + Qm + n_rx) % len(SHIFTS)] for b in range(n_blocks)], np.int32)
    want = np.full(rec_at + 64, CANARY, np.int16)
    for s in segs:
        nb = s["nb_re"]
        planes = compensate_np(rx[:, s["rx_off"]:s["rx_off"] + nb], ch[:, s["ch_off"]:s["ch_off"] + nb], Qm, int(shift[s["tb"]]))
        for k in range(Qm // 2):
            o = s["rec_off"] + 2 * (k * s["plane"] + s["sym_off"])
            want[o:o + 2 * nb] = planes[k].reshape(-1)
    return segs, rx, ch, stride, shift, want


@pytest.mark.parametrize("n_rx", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("Qm", [2, 4, 6, 8])
def test_compensation_and_level_against_numpy(hip, Qm, n_rx):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(1000 * Qm + n_rx)
    segs, rx, ch, stride, shift, want = kernel_case(rng, Qm, n_rx)
    n_blocks = len(shift)
    first = [next(s for s in segs if s["tb"] == b) for b in range(n_blocks)][::-1]      # any order: tb names the block
    lv_want = np.array([level_np(ch[:, s["ch_off"]:s["ch_off"] + s["nb_re"]])[0] for s in first[::-1]], np.int32)
    rx0, ch0 = rx.copy(), ch.copy()
    # host mode
    rec = np.full(want.size, CANARY, np.int16)
    m.ulsch_channel_compensation(rx.reshape(-1), ch.reshape(-1), n_rx, stride, segs, shift, rec)
    assert np.array_equal(rec, want), (Qm, n_rx, "host", np.flatnonzero(rec != want)[:8])
    assert np.array_equal(m.ulsch_channel_level(ch.reshape(-1), n_rx, stride, first), lv_want)
    assert np.array_equal(rx, rx0) and np.array_equal(ch, ch0)
    # device mode, the record array 16-, 4- and 8-byte aligned
    rx_d, ch_d = torch.from_numpy(rx.reshape(-1)).cuda(), torch.from_numpy(ch.reshape(-1)).cuda()
    sh_d = torch.from_numpy(shift).cuda()
    for pad in (0, 2, 4):
        rec_d = torch.full((want.size + 8,), CANARY, dtype=torch.int16, device="cuda")
        lv_d = torch.full((n_blocks + 2,), -7, dtype=torch.int32, device="cuda")
        m.ulsch_channel_level(ch_d, n_rx, stride, first, out=lv_d)
        m.ulsch_channel_compensation(rx_d, ch_d, n_rx, stride, segs, sh_d, rec_d[pad:])
        torch.cuda.synchronize()
        got = rec_d.cpu().numpy()
        assert (got[:pad] == CANARY).all() and (got[pad + want.size:] == CANARY).all()
        assert np.array_equal(got[pad:pad + want.size], want), (Qm, n_rx, pad, np.flatnonzero(got[pad:pad + want.size] != want)[:8])
        assert lv_d.cpu().numpy().tolist() == lv_want.tolist() + [-7, -7]
    assert np.array_equal(rx_d.cpu().numpy(), rx0.reshape(-1)) and np.array_equal(ch_d.cpu().numpy(), ch0.reshape(-1))
    # the shift the level call wrote, used from device memory by the compensation call on the same stream
    rec_d = torch.full((want.size,), CANARY, dtype=torch.int16, device="cuda")
    lv_d = torch.zeros(n_blocks, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.ulsch_channel_level(ch_d, n_rx, stride, first, out=lv_d)
        m.ulsch_channel_compensation(rx_d, ch_d, n_rx, stride, segs, lv_d, rec_d)
    torch.cuda.synchronize()
    rec = np.full(want.size, CANARY, np.int16)
    m.ulsch_channel_compensation(rx.reshape(-1), ch.reshape(-1), n_rx, stride, segs, lv_want, rec)
    assert np.array_equal(rec_d.cpu().numpy(), rec)


@pytest.mark.parametrize("Qm", [2, 4, 6, 8])
def test_compensation_then_llr_equals_demap_of_numpy(hip, Qm):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(70 + Qm)
    n_rx, nb_re, s = 4, 12 * 51 + 6 * 51, 13
    g = rng.integers(-3000, 3000, (n_rx, 1, 2))
    ch = (g + rng.integers(-40, 40, (n_rx, nb_re, 2))).astype(np.int16)
    rx = rng.integers(-6000, 6000, (n_rx, nb_re, 2)).astype(np.int16)
    planes = compensate_np(rx, ch, Qm, s)
    want = demap_np(planes[0], [planes[k] for k in range(1, Qm // 2)], Qm)
    segs = [dict(tb=0, Qm=Qm, nb_re=nb_re, plane=nb_re, sym_off=0, rx_off=0, ch_off=0, rec_off=0)]
    rec = torch.zeros(Qm * nb_re, dtype=torch.int16, device="cuda")
    m.ulsch_channel_compensation(torch.from_numpy(rx.reshape(-1)).cuda(), torch.from_numpy(ch.reshape(-1)).cuda(), n_rx, nb_re, segs,
                                 torch.tensor([s], dtype=torch.int32, device="cuda"), rec)
    pl = [rec[2 * nb_re * k:2 * nb_re * (k + 1)] for k in range(Qm // 2)]
    out = torch.zeros(Qm * nb_re, dtype=torch.int16, device="cuda")
    m.ulsch_llr(pl[0], pl[1:], Qm, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.asarray(want).reshape(-1))


# ---- end to end: extracted REs + channel estimates -> level -> compensation -> decode_symbols ------------------------------
def slot_symbols(rb):
    """13 data-bearing OFDM symbols of unequal size: a DMRS symbol with half the REs among them"""
    return [12 * rb] * 2 + [6 * rb] + [12 * rb] * 10


def e2e_blocks(Qm):
    mk = lambda rb, bits, BG: dict(A=valid_tbs(bits, BG), G=Qm * sum(slot_symbols(rb)), BG=BG, Qm=Qm, Nl=1, rv=0, tbslbrm=0)
    return [(mk(20, 150 * 20 * Qm * 2 // 5, 1), 20), (mk(51, 150 * 51 * Qm // 2, 1), 51), (mk(3, 150 * 3 * Qm // 3, 2), 3)]


def through_channel(rng, tx, n_rx, sigma):
    """per-antenna flat complex gain and additive noise: y = g x / 23170 + n, the estimate h = g (c16, rounded)"""
    S = tx.shape[0]
    x = (tx[:, 0].astype(np.float64) + 1j * tx[:, 1]) / 23170.0
    mag, ph = rng.uniform(1200, 2600, n_rx), rng.uniform(0, 2 * np.pi, n_rx)
    g = mag * np.exp(1j * ph)
    h = np.rint(np.stack([g.real, g.imag], 1)).astype(np.int16)                 # [n_rx, 2]
    gq = h[:, 0].astype(np.float64) + 1j * h[:, 1]
    y = gq[:, None] * x[None, :] + sigma * 1500 * (rng.standard_normal((n_rx, S)) + 1j * rng.standard_normal((n_rx, S)))
    rx = np.clip(np.rint(np.stack([y.real, y.imag], 2)), -32768, 32767).astype(np.int16)
    return rx, np.repeat(h[:, None, :], S, 1)


def run_e2e(m, rng, Qm, n_rx, rounds, library, expect_all_ack=False):
    import torch
    blocks = e2e_blocks(Qm)
    tbs = [b[0] for b in blocks]
    n = len(tbs)
    scr = rand_scr(rng, n)
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    po, co, ho, nseg = m.tb_layout(tbs)
    segs, first, rec_off, n_in = m.rx_front_segments(tbs, [slot_symbols(rb) for _, rb in blocks])
    assert rec_off == [int(c) for c in co[:n]]
    stride = n_in + 5
    harq = [torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda") for _ in range(2)]
    ids = [[7100 + i for i in range(n)], [7200 + i for i in range(n)]]
    llrlen = [[0] * n, [0] * n]
    side = torch.cuda.Stream()
    for rnd, (rv, sigma) in enumerate(rounds):
        cur = [dict(t, rv=rv) for t in tbs]
        tx = m.dlsch_encode_symbols_host(cur, pays, scr)
        rx = np.full((n_rx, stride, 2), 1234, np.int16)
        ch = np.full((n_rx, stride, 2), -4321, np.int16)
        at = 0
        for i, t in enumerate(tbs):
            S = t["G"] // Qm
            rx[:, at:at + S], ch[:, at:at + S] = through_channel(rng, tx[i][0], n_rx, sigma)
            at += S
        assert at == n_in
        # the existing path: numpy level and compensation, pack_symbol_records, decode_symbols
        lv = [level_np(ch[:, s["ch_off"]:s["ch_off"] + s["nb_re"]])[0] for s in first]
        rec_np = np.zeros(int(co[-1]) + 16, np.int16)
        for i, t in enumerate(tbs):
            mine = [s for s in segs if s["tb"] == i]
            parts = [compensate_np(rx[:, s["rx_off"]:s["rx_off"] + s["nb_re"]], ch[:, s["ch_off"]:s["ch_off"] + s["nb_re"]], Qm, lv[i]) for s in mine]
            rec_np[co[i]:co[i] + t["G"]] = m.pack_symbol_records([[np.concatenate([p[k] for p in parts]) for k in range(Qm // 2)]])[0]
        outs = []
        for which in (0, 1):
            rxt = [dict(t, round=rnd, llrLen=llrlen[which][i]) for i, t in enumerate(cur)]
            pay = torch.zeros(int(po[-1]) + 16, dtype=torch.uint8, device="cuda")
            ack = torch.zeros(n, dtype=torch.uint8, device="cuda")
            itm = torch.zeros(n, dtype=torch.int32, device="cuda")
            kw = dict(harq_ids=ids[which]) if library else {}
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                if which == 0:                                            # everything on the device, one stream
                    rx_d, ch_d = torch.from_numpy(rx.reshape(-1)).cuda(), torch.from_numpy(ch.reshape(-1)).cuda()
                    rec = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
                    lv_d = torch.zeros(n, dtype=torch.int32, device="cuda")
                    m.ulsch_channel_level(ch_d, n_rx, stride, first, out=lv_d)
                    m.ulsch_channel_compensation(rx_d, ch_d, n_rx, stride, segs, lv_d, rec)
                else:
                    rec = torch.from_numpy(rec_np).cuda()
                m.ulsch_decode_symbols_device(rxt, rec, None if library else harq[which], pay, ack, itm, scr, **kw)
            torch.cuda.synchronize()
            if which == 0:
                assert lv_d.cpu().numpy().tolist() == lv
                assert np.array_equal(rec.cpu().numpy(), rec_np)
            llrlen[which] = [t["llrLen"] for t in rxt]
            ph = pay.cpu().numpy()
            outs.append(([ph[po[i]:po[i] + t["A"] // 8] for i, t in enumerate(tbs)], ack.cpu().numpy(), itm.cpu().numpy()))
        for i in range(n):
            assert np.array_equal(outs[0][0][i], outs[1][0][i]), (Qm, rnd, i)
        assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2]), (Qm, rnd)
        assert llrlen[0] == llrlen[1]
        if library:
            for i in range(n):
                assert np.array_equal(m.harq_read(ids[0][i], nseg[i] * m.HARQ_STRIDE), m.harq_read(ids[1][i], nseg[i] * m.HARQ_STRIDE)), (rnd, i)
        else:
            assert torch.equal(harq[0], harq[1]), (Qm, rnd)
        if expect_all_ack:
            assert outs[0][1].all()
            for i in range(n):
                assert np.array_equal(outs[0][0][i], pays[i]), i
    if library:
        for i in ids[0] + ids[1]:
            m.harq_release(i)


@pytest.mark.parametrize("library", [False, True], ids=["harq_device", "harq_library"])
@pytest.mark.parametrize("Qm", [2, 4, 6, 8])
def test_front_then_decode_symbols_equals_numpy_records(hip, Qm, library):
    """first transmission, then an rv 2 retransmission into the same soft buffers"""
    run_e2e(hip.ldpc, np.random.default_rng(40 + Qm + 100 * library), Qm, 4 if Qm != 4 else 2, ((0, 0.5), (2, 0.3)), library)


def test_front_noiseless_decodes_the_payloads(hip):
    run_e2e(hip.ldpc, np.random.default_rng(9), 6, 4, ((0, 0.0),), False, expect_all_ack=True)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_rx_front_invalid_input(hip):
    import torch
    m = hip.ldpc
    L = m._rxf_lib()
    n_rx, stride = 2, 64
    good = dict(tb=0, Qm=4, nb_re=16, plane=32, sym_off=4, rx_off=0, ch_off=0, rec_off=0)
    rx_h = np.zeros(2 * n_rx * stride, np.int16)
    rec_h = np.full(512, CANARY, np.int16)
    sh_h = np.zeros(2, np.int32)
    lv_h = np.full(2, -7, np.int32)
    rx_d = torch.zeros(2 * n_rx * stride, dtype=torch.int16, device="cuda")
    rec_d = torch.full((512,), CANARY, dtype=torch.int16, device="cuda")
    sh_d = torch.zeros(2, dtype=torch.int32, device="cuda")
    lv_d = torch.full((2,), -7, dtype=torch.int32, device="cuda")

    def comp(mode, segs, rx=True, ch=True, shift=True, rec=True, n=n_rx, mem=None, stream=None, desc=True, rec_ptr=None):
        src, r, s = (rx_h.ctypes.data, rec_h.ctypes.data, sh_h.ctypes.data) if mode == "host" else (rx_d.data_ptr(), rec_d.data_ptr(), sh_d.data_ptr())
        mem = (m.MEM_HOST if mode == "host" else m.MEM_DEVICE) if mem is None else mem
        return L.nrLDPC_hip_ulsch_channel_compensation(src if rx else None, src if ch else None, n, stride, m._rx_seg_array(segs) if desc else None,
                                                       len(segs), s if shift else None, (rec_ptr or r) if rec else None, mem, stream)

    def level(mode, fs, ch=True, out=True, n=n_rx, mem=None, stream=None, desc=True):
        src, o = (rx_h.ctypes.data, lv_h.ctypes.data) if mode == "host" else (rx_d.data_ptr(), lv_d.data_ptr())
        mem = (m.MEM_HOST if mode == "host" else m.MEM_DEVICE) if mem is None else mem
        return L.nrLDPC_hip_ulsch_channel_level(src if ch else None, n, stride, m._rx_seg_array(fs) if desc else None, len(fs), o if out else None,
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
            (lambda: comp(mode, [good, dict(good, sym_off=10, nb_re=8)]), "overlap"),                 # within plane 0
            (lambda: comp(mode, [good, dict(good, Qm=2, rec_off=2 * 32, sym_off=19, nb_re=2)]), "overlap"),  # its plane 0 on the other's plane 1
            (lambda: comp(mode, [dict(good, Qm=8, nb_re=(1 << 18) + 1, plane=1 << 19)]), "2^21"),
            (lambda: comp(mode, [good], mem=7), "mem"),
            (lambda: level(mode, [good], ch=False), "null"), (lambda: level(mode, [good], out=False), "null"),
            (lambda: level(mode, [good], desc=False), "null"),
            (lambda: level(mode, [good], n=0), "n_rx"), (lambda: level(mode, [good], n=9), "n_rx"),
            (lambda: level(mode, [dict(good, nb_re=0)]), "no REs"),
            (lambda: level(mode, [dict(good, tb=1)]), "tb"), (lambda: level(mode, [good, good]), "tb"),
            (lambda: level(mode, [good], mem=3), "mem"),
        ]
        for call, why in bad_calls:
            assert call() < 0, (mode, why)
            assert why in m.last_error(), (mode, why, m.last_error())
    # DEVICE mem with a host array, and a record that is not 4-byte aligned
    assert L.nrLDPC_hip_ulsch_channel_compensation(rx_h.ctypes.data, rx_d.data_ptr(), n_rx, stride, m._rx_seg_array([good]), 1, sh_d.data_ptr(),
                                                   rec_d.data_ptr(), m.MEM_DEVICE, None) < 0 and "device memory" in m.last_error()
    assert L.nrLDPC_hip_ulsch_channel_compensation(rx_d.data_ptr(), rx_d.data_ptr(), n_rx, stride, m._rx_seg_array([good]), 1, sh_h.ctypes.data,
                                                   rec_d.data_ptr(), m.MEM_DEVICE, None) < 0 and "device memory" in m.last_error()
    assert comp("device", [good], rec_ptr=rec_d.data_ptr() + 2) < 0 and "4-byte" in m.last_error()
    assert L.nrLDPC_hip_ulsch_channel_level(rx_d.data_ptr(), n_rx, stride, m._rx_seg_array([good]), 1, lv_h.ctypes.data, m.MEM_DEVICE, None) < 0
    assert "device memory" in m.last_error()
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
