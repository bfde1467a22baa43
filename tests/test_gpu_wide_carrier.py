"""The slot-level kernels at full carrier width -- 273 PRBs on a 4096-point grid (C4), 275 on 8192 (C8), 273 on 6144 (C6) -- in DEVICE
and HOST mode against the CPU forms at the same descriptors, bit for bit, on canary-filled outputs: channel estimation
(tb_rx_chest.hip), the grid source of the receive front (tb_rx_front.hip: compensation and level), PDSCH mapping and precoded mapping
(tb_tx_map.hip); then one slot of the whole C4 carrier from layer symbols through mapping, estimation, level, compensation and
decoding on one stream.  The descriptors come from the shape lists of test_wide_carrier_host.py, which holds the CPU forms to the
literal restatements of the reference at those shapes.

Each test computes from the kernels' documented constants -- 256 output units per workgroup of the estimation kernels (a unit is a
4-RE group of the interpolating modes, a PRB of the averaging ones), 256 thread groups of 4 REs = 1024 REs per workgroup of the
RE-group kernels, a group's first RE being 4 g - phase -- how many workgroups (pieces) a (descriptor, antenna) pair gets and where the
wrap at fft_size falls, and asserts the coverage it claims."""
import numpy as np
import pytest

from rx_front_np import compensate_np, level_np
from test_gpu_pdsch_map import CANARY, PORTS, dl_alloc
from test_gpu_pdsch_map import host_form as map_host_form
from test_gpu_pdsch_precode import EXTREME, prg_edges_inside_groups, table_for
from test_gpu_pdsch_precode import host_form as precode_host_form
from test_gpu_rx_chest import host_form as chest_host_form
from test_gpu_rx_grid import PER_RB, SHIFTS, extract_np, p_of
from test_gpu_tb_chain import valid_tbs
from test_gpu_tb_scrambled import rand_scr
from test_wide_carrier_host import CARRIERS, CHE_THREADS, GROUP_RES, chest_pieces, chest_seg, chest_shapes, chest_wrap_piece, map_allocs

pytestmark = pytest.mark.gpu

T1I, T2I, T1A, T2A = 0, 1, 2, 3
FULL, DMRS1, DMRS2 = 0, 1, 2


def re_pieces(n_re, phase):
    """workgroups of an RE-group kernel over n_re REs whose first group starts at RE -phase"""
    return -(-(n_re + phase) // GROUP_RES)


# ---- channel estimation ----------------------------------------------------------------------------------------------------
def wide_chest_case(rng, n_rx):
    """The wide descriptors of chest_shapes() with three small ones (1, 3 and 25 PRBs) between them, each in an OFDM symbol of its
    own; ch_off takes every residue mod 4 among the wide ones; an odd antenna stride for odd n_rx."""
    wide = [dict(s, N=CARRIERS[s["carrier"]][0]) for s in chest_shapes()]
    small = [dict(mode=T1I, port=0, rb=1, k0=0, prb0=7, N=128), dict(mode=T2A, port=4, rb=3, k0=512 - 7, prb0=11, N=512),
             dict(mode=T2I, port=2, rb=25, k0=1536 - 36, prb0=40, N=1536)]
    order = wide[:3] + small[:1] + wide[3:6] + small[1:2] + wide[6:9] + small[2:] + wide[9:]
    segs, rx_at, at = [], 2, 3
    for i, s in enumerate(order):
        at += (i & 3) + 1
        re_offset = 12 * s["prb0"]
        segs.append(dict(mode=s["mode"], port=s["port"], fft_size=s["N"], start_re=s["k0"], rb_size=s["rb"], dmrs_offset=re_offset // (3 if s["mode"] & 1 else 2),
                         c_init=int(rng.integers(0, 1 << 31)), delay_off=i * n_rx, rx_off=rx_at, ch_off=at))
        if "carrier" in s:                                               # the shared builder gives the same descriptor
            ref_seg = chest_seg(s, segs[-1]["c_init"], rx_off=rx_at, ch_off=at, delay_off=i * n_rx)[0]
            assert ref_seg == segs[-1]
        at += 12 * s["rb"] + 3
        rx_at += s["N"] + (i & 1)
    rs, cs = rx_at + 5, at + 6 + (n_rx & 1)
    rx = rng.integers(-32768, 32768, (n_rx * rs, 2)).astype(np.int16)
    rx[::7] = rng.choice([32767, -32768], (len(rx[::7]), 2))
    delay = rng.integers(-24, 25, len(segs) * n_rx).astype(np.int32)
    return segs, rx, rs, cs, delay


def assert_chest_coverage(segs, n_rx, cs):
    wide = [s for s in segs if s["rb_size"] >= 257]
    assert len(wide) == 11 and sorted(s["rb_size"] for s in segs if s["rb_size"] < 257) == [1, 3, 25]
    assert {s["ch_off"] % 4 for s in wide} == {0, 1, 2, 3} and {s["fft_size"] for s in wide} == {4096, 6144, 8192}
    n_wg = 0
    for mode in (T1I, T2I, T1A, T2A):
        mine = [s for s in wide if s["mode"] == mode]
        units = [(3 if mode in (T1I, T2I) else 1) * s["rb_size"] for s in mine]
        pieces = [-(-u // CHE_THREADS) for u in units]
        assert pieces == [chest_pieces(mode, s["rb_size"]) for s in mine] and set(pieces) == {4 if mode in (T1I, T2I) else 2}
        assert {s["rb_size"] for s in mine} >= ({273, 275} | ({257} if mode in (T1A, T2A) else set()))
        assert max(s["dmrs_offset"] for s in mine) >= 1200
        wraps = {chest_wrap_piece(mode, s["fft_size"], s["start_re"]) for s in mine}
        assert pieces[0] - 1 in wraps                                    # a wrap inside the last piece
        n_wg += n_rx * sum(pieces)
    assert n_wg == n_rx * (5 * 4 + 6 * 2)                               # five interpolating and six averaging wide descriptors
    assert any(chest_wrap_piece(s["mode"], s["fft_size"], s["start_re"]) == 1 for s in wide if s["mode"] in (T1I, T2I))   # a piece > 0, not the last
    if n_rx & 1:
        assert cs % 2 == 1


@pytest.mark.parametrize("n_rx", [1, 2, 4, 3])
def test_wide_estimation_equals_the_host_form(hip, n_rx):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(5100 + n_rx)
    segs, rx, rs, cs, delay = wide_chest_case(rng, n_rx)
    assert_chest_coverage(segs, n_rx, cs)
    rx_d = torch.from_numpy(rx).cuda()
    for dl in (delay, None):
        want = chest_host_form(m, segs, rx, rs, cs, n_rx, dl)
        written = want != CANARY
        assert written.any() and not written.all()
        ch_d = torch.full((n_rx * cs, 2), CANARY, dtype=torch.int16, device="cuda")
        dl_d = None if dl is None else torch.from_numpy(dl).cuda()
        m.pusch_channel_estimation(rx_d, rs, ch_d, cs, n_rx, segs, dl_d)
        torch.cuda.synchronize()
        got = ch_d.cpu().numpy()
        assert np.array_equal(got, want), ("device", n_rx, np.argwhere(got != want)[:4])
        ch_h = np.full((n_rx * cs, 2), CANARY, np.int16)
        m.pusch_channel_estimation(rx, rs, ch_h, cs, n_rx, segs, dl)
        assert np.array_equal(ch_h, want), ("host", n_rx, np.argwhere(ch_h != want)[:4])


# ---- grid compensation and level -------------------------------------------------------------------------------------------
def first_behind_the_wrap(pattern, N, start_re, nb):
    return next(j for j in range(nb) if start_re + p_of(pattern, j) >= N)


def wide_grid_case(rng, Qm, n_rx):
    """Block 0: every pattern over the 273 PRBs of C4, once at the carrier's first subcarrier with the wrap inside a thread group and
    once with the wrap in the segment's last piece, between two thread groups.  Block 1: DMRS2 over the 275 PRBs of C8.  Every
    segment in an OFDM symbol and a channel range of its own; sym_off chosen as grid_case of test_gpu_rx_grid.py chooses it."""
    segs, info = [], []
    rx_at, ch_at, rec_at = 3, 5, 2
    plans = [(0, "C4", pat, place) for pat in (FULL, DMRS1, DMRS2) for place in ("fco", "last")] + [(1, "C8", DMRS2, "fco")]
    for tb in (0, 1):
        off, mine = int(rng.integers(0, 4)), []
        for _, carrier, pattern, place in (p for p in plans if p[0] == tb):
            N, rb, fco = CARRIERS[carrier]
            nb = PER_RB[pattern] * rb
            if place == "fco":
                start_re, between = fco, False
                w = first_behind_the_wrap(pattern, N, start_re, nb)
            else:
                w = (re_pieces(nb, 0) - 1) * GROUP_RES + 40
                start_re, between = N - p_of(pattern, w), True
                assert first_behind_the_wrap(pattern, N, start_re, nb) == w
            while ((w + rec_at // 2 + off) % 4 == 0) != between:
                off += 1
            phase = (rec_at // 2 + off) & 3
            info.append(dict(pattern=pattern, carrier=carrier, pieces=re_pieces(nb, phase), wrap_piece=(w + phase) // GROUP_RES, between=(w + phase) % 4 == 0))
            mine.append(dict(tb=tb, Qm=Qm, pattern=pattern, nb_re=nb, sym_off=off, fft_size=N, start_re=start_re, rx_off=rx_at, ch_off=ch_at, rec_off=rec_at))
            off += nb + len(mine) % 3
            rx_at += N + len(mine) % 2
            ch_at += p_of(pattern, nb - 1) + 1 + len(mine) % 4
        plane = off + int(rng.integers(0, 5))
        for s in mine:
            s["plane"] = plane
        segs += mine
        rec_at += 2 * 4 * plane + 2 * int(rng.integers(0, 4))
    # the coverage: pieces 0..3 (FULL), 0..2 (DMRS2), 0..1 (DMRS1); the wrap in a piece > 0 for every pattern, inside and between groups
    assert [(i["pattern"], i["pieces"]) for i in info] == [(FULL, 4), (FULL, 4), (DMRS1, 2), (DMRS1, 2), (DMRS2, 3), (DMRS2, 3), (DMRS2, 3)]
    assert [(i["wrap_piece"], i["between"]) for i in info] == [(1, False), (3, True), (0, False), (1, True), (1, False), (2, True), (1, False)]
    rx_stride, ch_stride = rx_at + 11, ch_at + 6
    rx = rng.integers(-32768, 32768, (n_rx, rx_stride, 2)).astype(np.int16)
    ch = rng.integers(-32768, 32768, (n_rx, ch_stride, 2)).astype(np.int16)
    ch[:, [c for s in segs if s["tb"] == 1 for c in range(s["ch_off"], s["ch_off"] + p_of(s["pattern"], s["nb_re"] - 1) + 1)]] >>= 5
    shift = np.array([SHIFTS[(tb + Qm + n_rx) % len(SHIFTS)] for tb in range(2)], np.int32)
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


@pytest.mark.parametrize("n_rx,Qm", [(1, 2), (2, 4), (4, 6), (8, 8), (3, 2)])
def test_wide_grid_compensation_and_level(hip, n_rx, Qm):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(5200 + 10 * Qm + n_rx)
    segs, ext_segs, rx, ch, rx_stride, ch_stride, rx_e, ch_e, shift, want = wide_grid_case(rng, Qm, n_rx)
    n_ext = rx_e.shape[1]
    # measurement symbols: block 0's 273-PRB segment of each pattern in turn (3276, 1638, 2184 terms), block 1's 275-PRB DMRS2 segment
    fi = [6, 2 * (n_rx % 3)]
    assert segs[fi[1]]["nb_re"] == PER_RB[n_rx % 3] * 273 and segs[fi[0]]["nb_re"] == 8 * 275
    first, ext_first = [segs[i] for i in fi], [ext_segs[i] for i in fi]
    lv_want = np.array([level_np(extract_np(rx, ch, segs[i])[1])[0] for i in fi[::-1]], np.int32)
    rx0, ch0 = rx.copy(), ch.copy()
    # host mode
    rec = np.full(want.size, CANARY, np.int16)
    m.ulsch_channel_compensation_grid(rx.reshape(-1), ch.reshape(-1), n_rx, rx_stride, ch_stride, segs, shift, rec)
    assert np.array_equal(rec, want), (Qm, n_rx, "host", np.flatnonzero(rec != want)[:8])
    assert np.array_equal(m.ulsch_channel_level_grid(ch.reshape(-1), n_rx, ch_stride, first), lv_want)
    assert np.array_equal(rx, rx0) and np.array_equal(ch, ch0)
    # device mode, the record array 16-, 4- and 8-byte aligned; the existing calls on the numpy-extracted arrays beside it
    rx_d, ch_d = torch.from_numpy(rx.reshape(-1)).cuda(), torch.from_numpy(ch.reshape(-1)).cuda()
    rxe_d, che_d = torch.from_numpy(rx_e.reshape(-1)).cuda(), torch.from_numpy(ch_e.reshape(-1)).cuda()
    sh_d = torch.from_numpy(shift).cuda()
    for pad in (0, 2, 4):
        rec_d = torch.full((want.size + 8,), CANARY, dtype=torch.int16, device="cuda")
        old_d = torch.full((want.size + 8,), CANARY, dtype=torch.int16, device="cuda")
        lv_d = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        lo_d = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        assert rec_d.data_ptr() % 16 == 0
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


# ---- PDSCH mapping ---------------------------------------------------------------------------------------------------------
def wide_map_case(m, rng, n_tx, Nl, carriers=("C4", "C6", "C8"), stride4=False, extra=0):
    """the descriptors of map_allocs(Nl) -- three symbols per allocation -- each allocation in a grid range and a layer range of its
    own, tx_off + start_re cycling through the residues mod 4; an odd antenna stride (the phase differs per antenna) unless stride4;
    `extra` c16 of room behind the last allocation"""
    allocs = [a for a in map_allocs(Nl) if {v[0]: k for k, v in CARRIERS.items()}[a["fft_size"]] in carriers]
    at, lay_at = 0, 1
    for i, a in enumerate(allocs):
        N = a["fft_size"]
        start_re = (a["first_carrier_offset"] + 12 * (a["rb_start"] + a["bwp_start"])) % N
        a["tx_slot_off"] = at + (i - start_re) % 4                      # symbols 2..4 are written: within [at + 2 N, at + 5 N + 3)
        a["lay_off"] = 2 * lay_at
        at += 5 * N + 4
        lay_at += Nl * a["plane"] + (i % 3)
    segs = m.pdsch_map_segments(allocs)
    assert len(segs) == 3 * len(allocs)
    stride = (at + 5 + extra) | 1
    if stride4:
        stride += 4 - stride % 4
    lay = rng.integers(-32768, 32768, (lay_at + 4, 2)).astype(np.int16)
    lay[::7] = rng.choice([32767, -32768], (len(lay[::7]), 2))
    return segs, lay, stride


def map_phase(s, a, stride):
    """of antenna a's first RE, for a 16-byte aligned grid array"""
    return (s["tx_off"] + a * stride + s["start_re"]) & 3


def assert_map_coverage(segs, stride, n_tx):
    c4 = [s for s in segs if s["fft_size"] == 4096]
    assert {(s["pattern"], s["ncdm"]) for s in c4} == set(PORTS)
    assert all(s["nb_re"] == PORTS[(s["pattern"], s["ncdm"])][1] * s["rb_size"] for s in segs)
    assert {(s["fft_size"], s["rb_size"]) for s in segs} == {(4096, 273), (6144, 273), (8192, 275)}
    assert {s["pattern"] for s in segs if s["fft_size"] == 8192} == {FULL, DMRS1, DMRS2}
    assert {(s["tx_off"] + s["start_re"]) % 4 for s in c4} == {0, 1, 2, 3} and stride % 2 == 1
    assert {s["amp"] for s in segs} == {1, 512, 32767} and {s["l_prime"] for s in segs if s["pattern"]} == {0, 1}
    assert max(s["dmrs_offset"] for s in segs if s["pattern"] == DMRS1) >= 1200 and max(s["dmrs_offset"] for s in segs if s["pattern"] == DMRS2) >= 1200
    inside = between = 0
    wrap_pieces = set()
    for s in segs:
        for a in range(n_tx):
            phase = map_phase(s, a, stride)
            assert re_pieces(12 * s["rb_size"], phase) == 4
            at_wrap = s["fft_size"] - s["start_re"]                      # the allocation RE on grid subcarrier 0
            assert 0 < at_wrap < 12 * s["rb_size"]
            wrap_pieces.add((at_wrap + phase) // GROUP_RES)
            if (at_wrap + phase) % 4:
                inside += 1
            else:
                between += 1
    assert inside > 0 and between > 0 and wrap_pieces >= {0, 1, 3}      # behind the first piece, and in the last


@pytest.mark.parametrize("n_tx,Nl", [(1, 1), (4, 4), (3, 2)])
def test_wide_mapping_equals_the_host_form(hip, n_tx, Nl):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(5300 + 10 * n_tx + Nl)
    segs, lay, stride = wide_map_case(m, rng, n_tx, Nl)
    assert_map_coverage(segs, stride, n_tx)
    want = map_host_form(m, segs, lay, stride, n_tx)
    written = (want != CANARY).any(-1)
    assert written.sum() >= n_tx * sum(12 * s["rb_size"] for s in segs) - 8 and not written.all()   # a value may equal the canary by chance
    tx_d = torch.full((n_tx * stride, 2), CANARY, dtype=torch.int16, device="cuda")
    assert tx_d.data_ptr() % 16 == 0
    m.pdsch_resource_mapping(torch.from_numpy(lay).cuda(), tx_d, stride, n_tx, segs)
    torch.cuda.synchronize()
    got = tx_d.cpu().numpy()
    assert np.array_equal(got, want), ("device", n_tx, Nl, np.argwhere(got != want)[:4])
    tx_h = np.full((n_tx * stride, 2), CANARY, np.int16)
    m.pdsch_resource_mapping(lay, tx_h, stride, n_tx, segs)
    assert np.array_equal(tx_h, want), ("host", n_tx, Nl, np.argwhere(tx_h != want)[:4])


# ---- precoded mapping ------------------------------------------------------------------------------------------------------
def wide_precoded_case(m, rng, n_tx, Nl, stride4):
    """the C4 descriptors of wide_map_case with prg_size 2, 4 (the last PRG holds one RB), wideband and 0 in turn, PMI lists mixing 0
    and the three matrices of table_for; behind them the hot descriptor of test_gpu_pdsch_precode.py (no DMRS, amp 32767, extreme
    layer values, every PRG of 3 RBs through the extreme matrix) widened to 273 RBs"""
    N, rb, fco = CARRIERS["C4"]
    segs, lay, stride = wide_map_case(m, rng, n_tx, Nl, carriers=("C4",), stride4=stride4, extra=N + 8)
    hot = dict(pattern=FULL, Nl=Nl, ncdm=0, l_prime=0, port=[], amp=32767, fft_size=N, start_re=fco, rb_size=rb, nb_re=12 * rb, sym_off=1, plane=12 * rb + 2,
               dmrs_offset=0, c_init=0, tx_off=stride - 7 - N, lay_off=2 * len(lay))
    assert max(s["tx_off"] for s in segs) + N <= hot["tx_off"]
    lay = np.concatenate([lay, rng.choice(EXTREME, (Nl * hot["plane"], 2)).astype(np.int16)])
    segs = segs + [hot]
    prgs, pmis = [], [500]
    for i, s in enumerate(segs):
        size = 3 if s is hot else (2, 4, rb, 0)[i % 4]
        n = -(-rb // size) if size else 0
        prgs.append(dict(prg_size=size, pmi_off=len(pmis), pmi_count=n))
        pmis += [500] * n if s is hot else [(11, 0, 3, 3, 0, 0, 500)[(q + i) % 7] for q in range(n)]
    return segs, prgs, pmis, lay, stride


def prg_edges_in_late_pieces(segs, prgs, pmis, stride, n_tx):
    """PRG boundaries between two different PMIs that lie in piece 2 or 3 of an antenna"""
    n = 0
    for s, g in zip(segs, prgs):
        for q in range(1, g["pmi_count"]):
            i = 12 * g["prg_size"] * q
            if pmis[g["pmi_off"] + q] != pmis[g["pmi_off"] + q - 1] and i < 12 * s["rb_size"]:
                n += sum(1 for a in range(n_tx) if (i + map_phase(s, a, stride)) // GROUP_RES >= 2)
    return n


@pytest.mark.parametrize("n_tx,Nl,stride4", [(2, 1, False), (8, 4, True), (3, 2, False)])
def test_wide_precoded_mapping_equals_the_host_form(hip, n_tx, Nl, stride4):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(5400 + 10 * n_tx + Nl)
    segs, prgs, pmis, lay, stride = wide_precoded_case(m, rng, n_tx, Nl, stride4)
    table = table_for(rng, Nl)
    assert {g["prg_size"] for g in prgs} == {0, 2, 3, 4, 273} and {0, 3, 11, 500} == set(pmis)
    assert {(s["pattern"], s["ncdm"]) for s in segs} == set(PORTS) and all(s["rb_size"] == 273 for s in segs)
    assert all(re_pieces(12 * s["rb_size"], map_phase(s, a, stride)) == 4 for s in segs for a in range(n_tx))
    assert prg_edges_inside_groups(segs, prgs, pmis, stride, n_tx) > 0 and prg_edges_in_late_pieces(segs, prgs, pmis, stride, n_tx) > 0
    want = precode_host_form(m, segs, prgs, pmis, table, lay, stride, n_tx)
    written = (want != CANARY).any(-1)
    assert written.sum() >= n_tx * sum(12 * s["rb_size"] for s in segs) - 8 and not written.all()
    if Nl > 1:                                                         # the hot descriptor clamps in both directions
        h = segs[-1]
        hot = want.reshape(n_tx, stride, 2)[:, h["tx_off"]:h["tx_off"] + h["fft_size"]]
        assert (hot == 32767).any() and (hot == -32768).any()
    lay_d = torch.from_numpy(lay).cuda()
    tx_d = torch.full((n_tx * stride, 2), CANARY, dtype=torch.int16, device="cuda")
    assert tx_d.data_ptr() % 16 == 0
    m.pdsch_resource_mapping_precoded(lay_d, tx_d, stride, n_tx, segs, prgs, pmis, table)
    torch.cuda.synchronize()
    got = tx_d.cpu().numpy()
    assert np.array_equal(got, want), ("device", n_tx, Nl, np.argwhere(got != want)[:4])
    tx_h = np.full((n_tx * stride, 2), CANARY, np.int16)
    m.pdsch_resource_mapping_precoded(lay, tx_h, stride, n_tx, segs, prgs, pmis, table)
    assert np.array_equal(tx_h, want), ("host", n_tx, Nl, np.argwhere(tx_h != want)[:4])
    # all-zero PMIs: the unit call at the same width
    zeros = [0] * len(pmis)
    unit = torch.full((n_tx * stride, 2), CANARY, dtype=torch.int16, device="cuda")
    got0 = torch.full((n_tx * stride, 2), CANARY, dtype=torch.int16, device="cuda")
    m.pdsch_resource_mapping(lay_d, unit, stride, n_tx, segs)
    m.pdsch_resource_mapping_precoded(lay_d, got0, stride, n_tx, segs, prgs, zeros, None)
    torch.cuda.synchronize()
    assert torch.equal(got0, unit) and not bool((unit == CANARY).all())
    got_h = np.full((n_tx * stride, 2), CANARY, np.int16)
    m.pdsch_resource_mapping_precoded(lay, got_h, stride, n_tx, segs, prgs, zeros, None)
    assert np.array_equal(got_h, unit.cpu().numpy())
    assert np.array_equal(unit.cpu().numpy(), map_host_form(m, segs, lay, stride, n_tx))


# ---- one wide slot, end to end ---------------------------------------------------------------------------------------------
_slots = {}


def wide_slot(m, variant):
    """The whole C4 carrier (rb_start = bwp_start = 0), 14 symbols, type-1 DMRS on symbol 2, two CDM groups without data, noiseless.
    (a) one layer on one antenna, 16QAM, amp 512, unit mapping; (b) one layer on two antennas through one wideband matrix with the
    weights (16384, 0) and (0, -16384), QPSK, both antennas received.  Everything the CPU forms make of it, computed once: the grid
    (pdsch_map_host / pdsch_precode_host), the estimates (pusch_chest_host), the level (ulsch_extract_host + ulsch_level_host) and the
    records (ulsch_compensate_host), composed as slot_case of test_gpu_slot_calls.py composes them."""
    if variant in _slots:
        return _slots[variant]
    rng = np.random.default_rng(31 + len(variant))
    N, rb, fco = CARRIERS["C4"]
    Qm, n_ant = (4, 1) if variant == "a" else (2, 2)
    S = 13 * 12 * rb
    c = dict(N=N, rb=rb, S=S, Qm=Qm, n_ant=n_ant)
    tbs = c["tbs"] = [dict(A=valid_tbs(S * Qm // 2, 1), G=Qm * S, BG=1, Qm=Qm, Nl=1, rv=0, tbslbrm=0)]
    c["scr"] = rand_scr(rng, 1)
    c["pays"] = [rng.integers(0, 256, tbs[0]["A"] // 8, dtype=np.uint8)]
    po, co, ho, _ = c["layout"] = m.tb_layout(tbs)
    dl = dl_alloc(N, rb, fco, 1, 0, 2, 0b1, 1 << 2, S, 5, 123, 1, 512, 3, 0, 0, 0)
    assert dl["first_carrier_offset"] == fco
    ul = dict(tb=0, Qm=Qm, dmrs_config_type=0, num_dmrs_cdm_grps_no_data=2, dmrs_symbol=2, fft_size=N, first_carrier_offset=fco, bwp_start=0,
              rb_start=0, rb_size=rb, start_symbol=0, nr_of_symbols=14, ul_dmrs_symb_pos=1 << 2, plane=S, rx_slot_off=3, ch_off=9, rec_off=int(co[0]))
    cfg = dict(slot=5, scid=1, dmrs_scrambling_id=123, port=0, chest_freq=0)
    if variant == "a":
        c["msegs"] = m.pdsch_map_segments([dl])
    else:
        c["pmis"] = [1]
        c["table"] = [dict(pm_idx=1, numLayers=1, num_ant_ports=2, weights=[[(16384, 0), (0, -16384)]])]
        c["msegs"], c["prgs"] = m.pdsch_precode_segments([dl], [dict(prg_size=rb, pmi_off=0, pmi_count=1)], 1)
    c["gsegs"], c["first"] = m.pusch_grid_segments([ul])
    c["csegs"] = m.pusch_chest_segments([ul], [cfg], n_ant)
    assert len(c["msegs"]) == 14 and len(c["gsegs"]) == 13 and len(c["csegs"]) == 1
    assert [(s["c_init"], s["dmrs_offset"], s["start_re"]) for s in c["csegs"]] == [(s["c_init"], s["dmrs_offset"], s["start_re"]) for s in c["msegs"] if s["pattern"]]
    assert c["csegs"][0]["mode"] == T1I and chest_pieces(T1I, rb) == 4 and all(s["nb_re"] == 12 * rb for s in c["gsegs"])
    lay = c["lay"] = np.ascontiguousarray(m.dlsch_encode_symbols_host(tbs, c["pays"], c["scr"])[0]).reshape(-1, 2)
    stride = c["stride"] = 14 * N + 16
    # the grid
    grid = np.zeros((n_ant * stride, 2), np.int16)
    for i, s in enumerate(c["msegs"]):
        for a in range(n_ant):
            seg = dict(s, tx_off=s["tx_off"] + a * stride)
            if variant == "a":
                m.pdsch_map_host(lay, seg, a, grid)
            else:
                m.pdsch_precode_host(lay, seg, c["prgs"][i], c["pmis"], c["table"], n_ant, a, grid)
    c["grid"] = grid
    # the estimates (delay 0), the level of the measurement symbol, the records
    ch = np.zeros((n_ant * stride, 2), np.int16)
    for s in c["csegs"]:
        for a in range(n_ant):
            m.pusch_chest_host(grid, dict(s, rx_off=s["rx_off"] + a * stride, ch_off=s["ch_off"] + a * stride), 0, ch)
    c["ch"] = ch
    rx_e, ch_e = np.zeros((n_ant, S, 2), np.int16), np.zeros((n_ant, S, 2), np.int16)
    for s in c["gsegs"]:
        o, nb = s["sym_off"], s["nb_re"]
        for a in range(n_ant):
            rx_e[a, o:o + nb], ch_e[a, o:o + nb] = m.ulsch_extract_host(grid[a * stride + s["rx_off"]:a * stride + s["rx_off"] + N],
                                                                        ch[a * stride + s["ch_off"]:a * stride + s["ch_off"] + 12 * rb], s["pattern"], N, s["start_re"], nb)
    f = c["first"][0]
    c["lv"] = m.ulsch_level_host(np.ascontiguousarray(ch_e[:, f["sym_off"]:f["sym_off"] + f["nb_re"]]), n_ant, f["nb_re"], f["nb_re"])[0]
    rec = np.zeros(int(co[-1]) + 16, np.int16)
    for s in c["gsegs"]:
        o, nb = s["sym_off"], s["nb_re"]
        pl = m.ulsch_compensate_host(np.ascontiguousarray(rx_e[:, o:o + nb]), np.ascontiguousarray(ch_e[:, o:o + nb]), n_ant, nb, nb, Qm, c["lv"])
        for k in range(Qm // 2):
            at = s["rec_off"] + 2 * (k * S + o)
            rec[at:at + 2 * nb] = pl[k].reshape(-1)
    c["rec"] = rec
    _slots[variant] = c
    return c


@pytest.mark.parametrize("variant", ["a", "b"])
def test_wide_loop_back_through_the_ul_receive_front(hip, variant):
    """test_loop_back_through_the_ul_receive_front of test_gpu_pdsch_map.py over the whole C4 carrier: mapping (unit or precoded) ->
    pusch_channel_estimation (delay NULL) -> channel_level_grid -> channel_compensation_grid -> ulsch_decode_symbols_device on one
    non-default stream returns the payload bytes with ACK; and the grid, the estimates, the level and the records on the way equal
    what the CPU forms make of the same layer symbols."""
    import torch
    m = hip.ldpc
    c = wide_slot(m, variant)
    N, S, n_ant, stride, tbs = c["N"], c["S"], c["n_ant"], c["stride"], c["tbs"]
    po, co, ho, _ = c["layout"]
    # before any GPU time: the chosen amplitudes give equalised symbols that are neither all saturated nor all zero
    y = c["rec"][int(co[0]):int(co[0]) + 2 * S].astype(np.int32)
    print("wide slot", variant, "level", c["lv"], "|y| min/median/max", np.abs(y).min(), int(np.median(np.abs(y))), np.abs(y).max())
    assert np.abs(y).max() < 32767 and np.abs(y).min() > 0 and 2 <= c["lv"] <= 14
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lay_d = torch.from_numpy(c["lay"].reshape(-1)).cuda()
        grid = torch.zeros(2 * n_ant * stride, dtype=torch.int16, device="cuda")
        if variant == "a":
            m.pdsch_resource_mapping(lay_d, grid, stride, n_ant, c["msegs"])
        else:
            m.pdsch_resource_mapping_precoded(lay_d, grid, stride, n_ant, c["msegs"], c["prgs"], c["pmis"], c["table"])
        ch_d = torch.zeros(2 * n_ant * stride, dtype=torch.int16, device="cuda")
        harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
        out = torch.zeros(int(po[-1]) + 16, dtype=torch.uint8, device="cuda")
        ack = torch.zeros(1, dtype=torch.uint8, device="cuda")
        itm = torch.zeros(1, dtype=torch.int32, device="cuda")
        rec = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
        lv_d = torch.zeros(1, dtype=torch.int32, device="cuda")
        m.pusch_channel_estimation(grid, stride, ch_d, stride, n_ant, c["csegs"], None)
        m.ulsch_channel_level_grid(ch_d, n_ant, stride, c["first"], out=lv_d)
        m.ulsch_channel_compensation_grid(grid, ch_d, n_ant, stride, stride, c["gsegs"], lv_d, rec)
        m.ulsch_decode_symbols_device([dict(t, round=0, llrLen=0) for t in tbs], rec, harq, out, ack, itm, c["scr"])
    torch.cuda.synchronize()
    assert np.array_equal(grid.cpu().numpy(), c["grid"].reshape(-1)), "grid"
    got_ch = ch_d.cpu().numpy()
    assert np.array_equal(got_ch, c["ch"].reshape(-1)), ("estimates", np.flatnonzero(got_ch != c["ch"].reshape(-1))[:8])
    assert lv_d.cpu().numpy().tolist() == [c["lv"]]
    got_rec = rec.cpu().numpy()
    assert np.array_equal(got_rec, c["rec"]), ("records", np.flatnonzero(got_rec != c["rec"])[:8])
    assert ack.cpu().numpy().all()
    assert np.array_equal(out.cpu().numpy()[:tbs[0]["A"] // 8], c["pays"][0])
