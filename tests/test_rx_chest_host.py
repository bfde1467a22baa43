"""PUSCH DMRS channel estimation in closed form per output unit (csrc/nr_chest.h through nrLDPC_hip_pusch_chest_host,
nrLDPC_hip_pusch_dmrs_host, nrLDPC_hip_delay_table_host and nrLDPC_hip_pusch_chest_segments, CPU only) against the literal Python
restatement of the reference's loops (rx_chest_np.py), and the refusals of the interface.

On the order of the saturating adds of TYPE1_INTERP: the weights that reach one 4-RE group always add up to one (p0 + p1p2 + middle
+ last resolve to 1/4, 1/8 and 1/2 shares), every rotated LS value is an int16, each term exceeds its share by at most one, and the
accumulator starts from zero.  A partial sum over a proper subset of the terms therefore stays below 7/8 of full scale, and only the
last term can be clamped (by a few units, all terms of one sign).  A clamp followed by a term of the other sign -- the only way the
order can show -- cannot occur; test_type1_interp_saturation checks the clamp that does occur and that the collected terms give the
same sum in reversed order.  The header keeps the reference's order anyway."""
import itertools

import numpy as np
import pytest

import rx_chest_np as ref

T1I, T2I, T1A, T2A = 0, 1, 2, 3
DELAYS = (-25, -20, -3, 0, 7, 20, 25)


def placements(N, rb, mode):
    """k0: at 0, ending at N - 1, the wrap between two PRBs, inside a PRB, inside a pilot pair (type 1: k0 + 4n + 2 crosses N; type 2:
    k0 + 6m + 1 crosses N)"""
    out = [0, N - 12 * rb, (N - 12 * (rb // 2 + 1)) % N if rb > 1 else N - 6, N - 6, N - 2 if mode in (T1I, T1A) else N - 1, N - 7]
    return sorted(set(out))


def make_seg(mode, port, N, k0, rb, dmrs_offset, c_init, rx_off=0, ch_off=0, delay_off=0):
    return dict(mode=mode, port=port, fft_size=N, start_re=k0, rb_size=rb, dmrs_offset=dmrs_offset, c_init=c_init, rx_off=rx_off, ch_off=ch_off,
                delay_off=delay_off)


def reaches_n(mode, port, N, k0, rb):
    if mode == T1I or not (port >> 1) & 1:
        return False
    used = (lambda t: t % 6 < 2) if mode in (T2I, T2A) else (lambda t: t % 2 == 0)
    return any(used(t) and (k0 + t) % N == N - 1 for t in range(12 * rb))


def run_ref(rx, soffset, seg, d, re_offset, **kw):
    lst = [(int(a), int(b)) for a, b in rx]
    out = ref.pusch_channel_estimation(lst, soffset, seg["fft_size"], seg["start_re"], seg["rb_size"], seg["port"], seg["mode"] & 1, seg["mode"] >> 1,
                                       seg["c_init"], re_offset, d, **kw)
    return np.array(out, np.int64).astype(np.int16)


def run_host(m, rx, seg, d, pad=7):
    ch = np.full((pad + 12 * seg["rb_size"] + pad, 2), 0x5a5a, np.int16)
    m.pusch_chest_host(rx, dict(seg, ch_off=pad), d, ch)
    assert np.all(ch[:pad] == 0x5a5a) and np.all(ch[pad + 12 * seg["rb_size"]:] == 0x5a5a), "the write set is 12 rb_size entries"
    return ch[pad:pad + 12 * seg["rb_size"]]


@pytest.mark.parametrize("mode", [T1I, T2I, T1A, T2A])
def test_host_form_equals_the_literal_loops(built, mode):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rng = np.random.default_rng(100 + mode)
    ports = itertools.cycle(range(12 if mode & 1 else 8))
    delays = itertools.cycle(DELAYS)
    kinds = itertools.cycle(("random", "random", "extreme"))
    seen_ports, seen_delays, n = set(), set(), 0
    for N in (128, 512, 1536):
        for rb in (1, 2, 3, 5, 25):
            if 12 * rb > N:
                continue
            for k0 in placements(N, rb, mode):
                port, d, kind = next(ports), next(delays), next(kinds)
                if reaches_n(mode, port, N, k0, rb):
                    port &= ~2
                soffset = N
                rx = (rng.integers(-32768, 32768, (2 * N + 3, 2)) if kind == "random" else rng.choice([32767, -32768, -32767], (2 * N + 3, 2))).astype(np.int16)
                prb0 = int(rng.integers(0, 50))
                re_offset = 12 * prb0
                seg = make_seg(mode, port, N, k0, rb, re_offset // (3 if mode & 1 else 2), ref.c_init_pusch(int(rng.integers(0, 20)), 2, 40 + n, n & 1),
                               rx_off=soffset)
                want = run_ref(rx, soffset, seg, d, re_offset, literal_type2_avg=False)
                got = run_host(m, rx, seg, d)
                assert np.array_equal(got, want[:12 * rb]), (mode, N, rb, k0, port, d, kind)
                seen_ports.add(port)
                seen_delays.add(d)
                n += 1
    assert seen_delays == set(DELAYS) and seen_ports >= set(range(12 if mode & 1 else 8)) - {2, 3, 6, 7, 10, 11} and n > 40


@pytest.mark.parametrize("mode", [T1I, T2I, T1A, T2A])
def test_every_port(built, mode):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rng = np.random.default_rng(7)
    N, rb, k0 = 128, 3, 100                                             # straddles the wrap; k0 even: nushift never reaches N
    rx = rng.integers(-32768, 32768, (N, 2)).astype(np.int16)
    for port in range(12 if mode & 1 else 8):
        seg = make_seg(mode, port, N, k0, rb, 24, 0x1234567 + port)
        want = run_ref(rx, 0, seg, 5, 48 if not mode & 1 else 72, literal_type2_avg=False)
        assert np.array_equal(run_host(m, rx, seg, 5), want[:12 * rb]), port


def test_type1_interp_saturation(built):
    """All rotated LS values at +32767: every group's terms add up to 32768 and the last one is clamped.  See the module docstring
    for why no input makes the order of the terms observable."""
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    N, rb, k0 = 128, 2, 0
    c_init = 0x2345
    pil = ref.pusch_dmrs_rx(c_init, 0, rb, 0, 0)
    rx = np.zeros((N, 2), np.int16)
    for k, (pr, pi) in enumerate(pil):                                   # rx = 23170 conj-aligned: each product 16383 + 0j, a pair 32766
        rx[2 * k] = (23170 if pr > 0 else -23170, -23170 if pi > 0 else 23170)
    seg = make_seg(T1I, 0, N, k0, rb, 0, c_init)
    terms = []
    want = run_ref(rx, 0, seg, 0, 0, terms=terms)
    got = run_host(m, rx, seg, 0)
    assert np.array_equal(got, want[:12 * rb])
    clamped = 0
    for idx in range(12 * rb):
        for c in range(2):
            ts = [t for (i, cc, y, t) in terms if i == idx and cc == c]
            fwd = rev = 0
            for t in ts:
                fwd = ref.sat16(fwd + t)
            for t in reversed(ts):
                rev = ref.sat16(rev + t)
            assert fwd == rev
            clamped += sum(ts) != fwd
    assert clamped > 0 and want[:12 * rb, 0].max() == 32767


def test_type1_interp_group_weights_add_up_to_one():
    """What the module docstring's argument rests on: whatever rb_size, the filter weights that reach one output entry add up to
    16384, half of Q15 full scale, and a term is twice the mulhrs product.  Taken from the restatement's own window walk: every
    rotated LS value is made (16384, 0) (a pair of products of 8192 each, delay 0), for which 2 mulhrs(16384, w) = w exactly, so the
    collected terms of an entry are the weights it received."""
    for rb in (1, 2, 3, 5, 25):
        N, c_init = 512, 0x2345 + rb
        pil = ref.pusch_dmrs_rx(c_init, 0, rb, 0, 0)
        rx = [(0, 0)] * N
        for k, (pr, pi) in enumerate(pil):                               # (p rx) >> 16 = (46340 * 11586) >> 16 = 8192 + 0j
            rx[2 * k] = (11586 if pr > 0 else -11586, -11586 if pi > 0 else 11586)
        terms = []
        out = ref.pusch_channel_estimation(rx, 0, N, 0, rb, 0, 0, 0, c_init, 0, 0, terms=terms)
        assert all(c == 0 for (_, c, _, _) in terms)
        for idx in range(12 * rb):
            ts = [t for (i, c, y, t) in terms if i == idx]
            assert sum(ts) == 16384 and 2 <= len(ts) <= 8 and out[idx] == (16384, 0), (rb, idx, ts)


@pytest.mark.parametrize("mode", [T1I, T2I, T1A, T2A])
def test_shifted_ports_on_every_placement(built, mode):
    """Ports 2 and 3 (type 1: delta = 1 in TYPE1_INTERP, nushift = 1 in TYPE1_AVG) and 2, 3, 6, 10 (type 2: nushift = 1) on every
    placement of test_host_form_equals_the_literal_loops, the wrap placements included, wherever the descriptor is not refused."""
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rng = np.random.default_rng(300 + mode)
    ran = {}
    for N in (128, 512):
        for rb in (1, 2, 3, 5):
            for k0 in placements(N, rb, mode):
                for port, d in zip((2, 3, 6, 10) if mode & 1 else (2, 3), DELAYS[1:]):
                    key = (N, rb, k0)
                    ran.setdefault(key, 0)
                    if reaches_n(mode, port, N, k0, rb):
                        continue
                    rx = rng.integers(-32768, 32768, (2 * N + 3, 2)).astype(np.int16)
                    re_offset = 12 * int(rng.integers(0, 50))
                    seg = make_seg(mode, port, N, k0, rb, re_offset // (3 if mode & 1 else 2), ref.c_init_pusch(5, 3, 77 + port, port & 1), rx_off=N)
                    want = run_ref(rx, N, seg, d, re_offset, literal_type2_avg=False)
                    assert np.array_equal(run_host(m, rx, seg, d), want[:12 * rb]), (mode, N, rb, k0, port, d)
                    ran[key] += 1
    # a placement is left out only where the shifted read would reach index N, which the interface refuses
    for (N, rb, k0), cnt in ran.items():
        assert cnt > 0 or reaches_n(mode, 2, N, k0, rb), (mode, N, rb, k0)
    assert sum(1 for (N, rb, k0), cnt in ran.items() if cnt and k0 + 12 * rb > N) >= 4


def test_pilots(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    for dmrs_type, port, off, c_init in [(0, 0, 0, 1), (0, 1, 7, 0x7fffffff), (0, 5, 300, 0x12345), (1, 0, 4, 99), (1, 11, 1091, 0x55aa55), (1, 7, 33, 0)]:
        want = ref.pusch_dmrs_rx(c_init, port, 7, off * (2 if dmrs_type == 0 else 3), dmrs_type)
        got = m.pusch_dmrs_host(c_init, off, len(want), port, dmrs_type)
        assert np.array_equal(got, np.array(want, np.int16)), (dmrs_type, port, off)
    # by hand: c_init = 0 leaves x2 = 0 and c(n) = x1(n + 1600), whose first eight bits are 0,0,0,0, 0,0,1,0: pilots 0..2 are
    # (23170, -23170), pilot 3 has bit(2i) set and is (-23170, -23170); port 1 negates the odd ones
    assert ref.gold_bits(0, 8) == (0, 0, 0, 0, 0, 0, 1, 0)
    hand = [(23170, -23170)] * 3 + [(-23170, -23170)]
    assert np.array_equal(m.pusch_dmrs_host(0, 0, 4, 0, 0), np.array(hand, np.int16))
    hand1 = [(r, i) if k % 2 == 0 else (-r, -i) for k, (r, i) in enumerate(hand)]
    assert np.array_equal(m.pusch_dmrs_host(0, 0, 4, 1, 0), np.array(hand1, np.int16))
    assert set(np.abs(m.pusch_dmrs_host(5, 3, 64, 3, 1)).reshape(-1).tolist()) == {23170}


def test_delay_tables(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    for N in (128, 1536):
        for d in DELAYS:
            assert np.array_equal(m.delay_table_host(N, d), np.array(ref.delay_table_row(N, d), np.int16)), (N, d)
    assert np.array_equal(m.delay_table_host(512, 0), np.tile(np.array([256, 0], np.int16), (512, 1)))
    assert np.array_equal(m.delay_table_host(512, 25), m.delay_table_host(512, 20))
    t = m.delay_table_host(128, 1)
    assert tuple(t[32]) == (0, 256) and tuple(t[64]) == (-256, 0) and tuple(t[16]) == (181, 181)
    # delay 0 is the identity of the rotation: (x 256) >> 8
    rng = np.random.default_rng(3)
    rx = rng.integers(-32768, 32768, (128, 2)).astype(np.int16)
    seg = make_seg(T2I, 0, 128, 10, 4, 0, 77)
    ls = run_ref(rx, 0, seg, 0, 0)
    assert np.array_equal(run_host(m, rx, seg, 0), ls[:48])
    assert not np.array_equal(run_host(m, rx, seg, 9), ls[:48])


def test_type2_avg_deviations(built):
    """The two defects of the reference's TYPE2_AVG that are not reproduced: where the literal form differs, and only there."""
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rng = np.random.default_rng(11)
    N, rb, k0, port, c_init = 128, 4, 40, 0, 4242
    rx = rng.integers(-3000, 3000, (2 * N, 2)).astype(np.int16)
    pil = ref.pusch_dmrs_rx(c_init, port, rb, 0, 1)

    def hand(pilots, bases, b):
        s = [0, 0]
        for t, (pi_, base) in enumerate(zip(pilots, bases)):
            x = rx[base + (k0 + 12 * b + 6 * (t >> 1) + (t & 1)) % N]
            p = ref.c32_mul_shift(pil[pi_], (int(x[0]), int(x[1])), 15)
            s = [s[0] + p[0], s[1] + p[1]]
        return ref.c16_div(s, 4)
    for soffset in (0, N):
        seg = make_seg(T2A, port, N, k0, rb, 0, c_init, rx_off=soffset)
        got = run_host(m, rx, seg, 0)
        lit = run_ref(rx, soffset, seg, 0, 0, literal_type2_avg=True)
        for b in range(rb):
            assert tuple(got[12 * b]) == hand(range(4 * b, 4 * b + 4), [soffset] * 4, b)
            lit_pilots = [0, 1, 2, 2] if b == 0 else range(4 * b - 1, 4 * b + 3)            # :361-370
            lit_bases = [soffset, 0, 0, 0] if b == 0 else [0] * 4                            # :355-368, :388-435
            assert tuple(lit[12 * b]) == hand(lit_pilots, lit_bases, b)
            assert np.all(got[12 * b:12 * b + 12] == got[12 * b]) and np.all(lit[12 * b:12 * b + 12] == lit[12 * b])
        assert not np.array_equal(got, lit[:12 * rb])


def test_spill_and_memset_are_not_reproduced(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rng = np.random.default_rng(12)
    N, rb = 128, 2
    rx = rng.integers(-32768, 32768, (N, 2)).astype(np.int16)
    seg = make_seg(T1I, 2, N, 5, rb, 6, 31337)
    want = run_ref(rx, 0, seg, -3, 12)
    assert np.any(want[12 * rb:12 * rb + 4] != 0) and not np.any(want[12 * rb + 4:])       # the reference's spill: four entries
    assert np.array_equal(run_host(m, rx, seg, -3), want[:12 * rb])                          # run_host checks the canaries


def test_refusals(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rx, ch = np.zeros((2 * 128, 2), np.int16), np.zeros((2 * 128, 2), np.int16)
    good = make_seg(T1I, 0, 128, 0, 2, 0, 1)
    for change, reason in [(dict(mode=4), "mode must be"), (dict(port=8), "port must be"), (dict(mode=T2I, port=12), "port must be"),
                           (dict(rb_size=0), "rb_size is 0"), (dict(rb_size=11), "wider than fft_size"), (dict(start_re=128), "start_re must be below"),
                           (dict(fft_size=1000, rb_size=2), "fft_size must be"), (dict(fft_size=64, rb_size=2), "fft_size must be"),
                           (dict(c_init=1 << 31), "c_init"), (dict(dmrs_offset=(1 << 20) + 1), "dmrs_offset"),
                           (dict(mode=T1A, port=2, start_re=127), "index fft_size"), (dict(mode=T2I, port=2, start_re=121), "index fft_size"),
                           (dict(mode=T2A, port=3, start_re=126), "index fft_size")]:
        seg = dict(good, **change)
        big_rx = np.zeros((4096, 2), np.int16)
        with pytest.raises(RuntimeError, match=reason):
            m.pusch_chest_host(big_rx, seg, 0, np.zeros((4096, 2), np.int16))
        # the GPU call refuses the same descriptors before it touches a device
        with pytest.raises(RuntimeError, match=reason):
            m.pusch_channel_estimation(big_rx, 0, np.zeros((4096, 2), np.int16), 0, 1, [seg])
    for n_rx in (0, 9):
        with pytest.raises(RuntimeError, match="n_rx must be 1..8"):
            m.pusch_channel_estimation(rx, 0, ch, 0, n_rx, [])
    with pytest.raises(RuntimeError, match="overlap"):
        m.pusch_channel_estimation(rx, 128, ch, 12, 2, [good])                               # antenna 1 writes over antenna 0's tail
    with pytest.raises(RuntimeError, match="overlap"):
        m.pusch_channel_estimation(rx, 128, ch, 128, 2, [good, dict(good, ch_off=20)])
    L = pkg.ldpc._chest_lib()
    arr = pkg.ldpc._chest_seg_array([good])
    assert L.nrLDPC_hip_pusch_channel_estimation(None, 0, ch.ctypes.data, 0, 1, arr, 1, None, 0, None) == -1 and "null" in m.last_error()
    assert L.nrLDPC_hip_pusch_channel_estimation(rx.ctypes.data, 0, ch.ctypes.data, 0, 1, arr, 1, None, 7, None) == -1 and "mem must be" in m.last_error()
    # the wrappers know the extents
    with pytest.raises(ValueError, match="leaves the grid"):
        m.pusch_channel_estimation(rx, 128, ch, 128, 3, [good])
    with pytest.raises(ValueError, match="estimates leave"):
        m.pusch_channel_estimation(rx, 0, ch, 0, 1, [dict(good, ch_off=250)])
    with pytest.raises(ValueError, match="delays leave"):
        m.pusch_channel_estimation(rx, 128, ch, 128, 2, [dict(good, delay_off=1)], est_delay=np.zeros(2, np.int32))
    with pytest.raises(RuntimeError, match="type must be"):
        m.pusch_dmrs_host(1, 0, 4, 0, 2)
    with pytest.raises(RuntimeError, match="fft_size must be"):
        m.delay_table_host(100, 0)


def alloc(**kw):
    a = dict(tb=0, Qm=2, dmrs_config_type=0, num_dmrs_cdm_grps_no_data=1, dmrs_symbol=2, fft_size=512, first_carrier_offset=512 - 6 * 25, bwp_start=1,
             rb_start=3, rb_size=5, start_symbol=0, nr_of_symbols=14, ul_dmrs_symb_pos=1 << 2, plane=100000, rx_slot_off=512 * 14, ch_off=77, rec_off=0)
    a.update(kw)
    return a


def test_chest_segments(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    for dmrs_type in (0, 1):
        for pos in ([2], [2, 11], [2, 7, 11]):
            for chest_freq in (0, 1):
                mask = sum(1 << s for s in pos)
                a0 = alloc(dmrs_config_type=dmrs_type, ul_dmrs_symb_pos=mask, dmrs_symbol=pos[0])
                a1 = alloc(tb=1, dmrs_config_type=dmrs_type, ul_dmrs_symb_pos=mask, dmrs_symbol=pos[-1], rb_start=10, rb_size=2, ch_off=77 + 14 * 512)
                cfg = [dict(slot=3, scid=1, dmrs_scrambling_id=321, port=1, chest_freq=chest_freq), dict(slot=3, scid=0, dmrs_scrambling_id=5, port=4, chest_freq=chest_freq)]
                segs = m.pusch_chest_segments([a0, a1], cfg, 2)
                assert len(segs) == 2 * len(pos)
                for i, (a, c) in enumerate([(a0, cfg[0]), (a1, cfg[1])]):
                    for k, sym in enumerate(pos):
                        s = segs[i * len(pos) + k]
                        assert s == dict(mode=dmrs_type + 2 * chest_freq, port=c["port"], fft_size=512,
                                         start_re=(a["first_carrier_offset"] + 12 * (a["bwp_start"] + a["rb_start"])) % 512, rb_size=a["rb_size"],
                                         dmrs_offset=12 * (a["bwp_start"] + a["rb_start"]) // (2 if dmrs_type == 0 else 3),
                                         c_init=ref.c_init_pusch(3, sym, c["dmrs_scrambling_id"], c["scid"]), delay_off=2 * (i * len(pos) + k),
                                         rx_off=a["rx_slot_off"] + sym * 512, ch_off=a["ch_off"] + sym * 512)
                # the estimates land where the grid calls read them
                gsegs, first = m.pusch_grid_segments([a0, a1])
                for i, a in enumerate((a0, a1)):
                    mine = [s["ch_off"] for s in segs[i * len(pos):(i + 1) * len(pos)]]
                    assert first[i]["ch_off"] in mine and all(g["ch_off"] in mine for g in gsegs if g["tb"] == i)
    c = dict(slot=0, scid=0, dmrs_scrambling_id=0, port=0, chest_freq=0)
    for bad_a, bad_c, reason in [(dict(nr_of_symbols=15), {}, "within the slot"), (dict(rb_size=0), {}, "rb_size is 0"), (dict(rb_size=43), {}, "wider than"),
                                 (dict(first_carrier_offset=512), {}, "first_carrier_offset"), (dict(dmrs_config_type=2), {}, "dmrs_config_type"),
                                 ({}, dict(chest_freq=2), "chest_freq"), ({}, dict(scid=2), "scid"), ({}, dict(port=8), "port must be"),
                                 ({}, dict(slot=160), "slot"), ({}, dict(dmrs_scrambling_id=65536), "dmrs_scrambling_id"), (dict(fft_size=500, first_carrier_offset=0), {}, "fft_size must be")]:
        with pytest.raises(RuntimeError, match=reason):
            m.pusch_chest_segments([alloc(**bad_a)], [dict(c, **bad_c)], 1)
    with pytest.raises(RuntimeError, match="n_rx must be"):
        m.pusch_chest_segments([alloc()], [c], 0)
    with pytest.raises(RuntimeError, match="more descriptors than cap"):
        m.pusch_chest_segments([alloc(ul_dmrs_symb_pos=(1 << 2) | (1 << 7))], [c], 1, cap=1)
