"""The RB extraction in closed form (csrc/nr_rx_grid.h through nrLDPC_hip_ulsch_extract_host and nrLDPC_hip_pusch_grid_segments,
CPU only) against the literal numpy restatement of the reference's loops (rx_grid_np.py); the refusals of the grid interface; and
the HOST-mode grid calls against the existing HOST-mode calls on extracted arrays (those stage through the GPU)."""
import ctypes as C

import numpy as np
import pytest

from rx_grid_np import extract_rbs, get_nb_re_pusch, symbol_loop

FULL, DMRS1, DMRS2 = 0, 1, 2
PER_RB = {FULL: 12, DMRS1: 6, DMRS2: 8}
# N -> N_RB of the carrier (first_carrier_offset = N - 6 N_RB)
CARRIERS = {128: 10, 1536: 106, 4096: 273}


def p_of(pattern, j):
    """the table of the header, written independently: FULL j, DMRS1 2j + 1, DMRS2 6 (j / 4) + 2 + j % 4"""
    return [lambda j: j, lambda j: 2 * j + 1, lambda j: 6 * (j // 4) + 2 + j % 4][pattern](j)


def placements(N, n_rb):
    """(rb_start, rb_size): before the wrap, ending exactly at N, straddling it by one RB, starting at subcarrier 0, in the upper
    half only, and the whole band; sizes 1 and 2 at each place"""
    half = n_rb // 2                                   # RB `half` starts at grid subcarrier 0 (N_RB even) or holds it (odd)
    out = [(0, 1), (1, 2), (0, half), (half - 1, 1), (half - 2, 2), (half - 1, 2), (half - 2, 3), (half, 1), (half, 2), (half + 1, n_rb - half - 1),
           (0, n_rb), (half - 3, 7 if n_rb >= half + 4 else 4)]
    return [(s, z) for s, z in out if s >= 0 and z >= 1 and s + z <= n_rb]


def grid_case(rng, N, n_sym=1):
    rx = rng.integers(-32768, 32768, (n_sym * N + 5, 2)).astype(np.int16)
    ch = rng.integers(-32768, 32768, (n_sym * N + 5, 2)).astype(np.int16)
    return rx, ch


@pytest.mark.parametrize("N", sorted(CARRIERS))
def test_extract_host_equals_the_literal_loops(built, N):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rng = np.random.default_rng(N)
    n_rb = CARRIERS[N]
    fp = dict(first_carrier_offset=N - 6 * n_rb, ofdm_symbol_size=N)
    rx, ch = grid_case(rng, N, 2)
    seen = set()
    for rb_start, rb_size in placements(N, n_rb):
        for bwp_start in (0, 1):
            if rb_start + bwp_start + rb_size > n_rb:
                continue
            start_re = (fp["first_carrier_offset"] + (rb_start + bwp_start) * 12) % N
            seen.add("before" if start_re + 12 * rb_size < N and start_re else "ends" if start_re + 12 * rb_size == N else
                     "zero" if start_re == 0 else "straddles")
            for pattern in (FULL, DMRS1, DMRS2):
                pdu = dict(rb_start=rb_start, bwp_start=bwp_start, rb_size=rb_size, dmrs_config_type=0 if pattern != DMRS2 else 1)
                rxoffset, choffset = N, 3
                want_rx, want_ch = extract_rbs(rx, ch, rxoffset, choffset, int(pattern != FULL), pdu, fp, fix_352=True)
                nb_re = PER_RB[pattern] * rb_size
                assert len(want_rx) == nb_re == len(want_ch)
                got_rx, got_ch = m.ulsch_extract_host(rx[rxoffset:rxoffset + N], ch[choffset:], pattern, N, start_re, nb_re)
                assert np.array_equal(got_rx, want_rx) and np.array_equal(got_ch, want_ch), (N, rb_start, rb_size, pattern)
                # the closed form itself
                idx = np.array([p_of(pattern, j) for j in range(nb_re)])
                assert np.array_equal(rx[rxoffset + (start_re + idx) % N], want_rx) and np.array_equal(ch[choffset + idx], want_ch)
                # the first nb_re of the sequence: fewer REs than the pattern holds are a prefix
                for part in {1, nb_re // 2, nb_re - 1} - {0}:
                    a, b = m.ulsch_extract_host(rx[rxoffset:rxoffset + N], ch[choffset:], pattern, N, start_re, part)
                    assert np.array_equal(a, want_rx[:part]) and np.array_equal(b, want_ch[:part])
    # with an odd N_RB (273) grid subcarrier 0 lies in the middle of an RB: no allocation ends at N or starts at 0
    assert seen == ({"before", "ends", "zero", "straddles"} if n_rb % 2 == 0 else {"before", "straddles"})


def test_the_unflagged_literal_differs_at_352(built):
    """The one-piece type-2 branch reads rxF[idx], not rxF[start_re + idx]: the deviation, kept visible"""
    N, n_rb = 128, 10
    rng = np.random.default_rng(352)
    fp = dict(first_carrier_offset=N - 6 * n_rb, ofdm_symbol_size=N)
    rx, ch = grid_case(rng, N)
    pdu = dict(rb_start=1, bwp_start=0, rb_size=2, dmrs_config_type=1)       # start_re = 80, one piece
    lit, lit_ch = extract_rbs(rx, ch, 0, 0, 1, pdu, fp)
    fixed, fixed_ch = extract_rbs(rx, ch, 0, 0, 1, pdu, fp, fix_352=True)
    assert not np.array_equal(lit, fixed) and np.array_equal(lit_ch, fixed_ch)
    assert np.array_equal(lit, rx[[p_of(DMRS2, j) for j in range(16)]])          # the literal reads from subcarrier 0 of the grid
    pdu = dict(rb_start=5, bwp_start=0, rb_size=2, dmrs_config_type=1)       # start_re = 0: the two agree
    assert np.array_equal(extract_rbs(rx, ch, 0, 0, 1, pdu, fp)[0], extract_rbs(rx, ch, 0, 0, 1, pdu, fp, fix_352=True)[0])


def alloc(**kw):
    a = dict(tb=0, Qm=6, dmrs_config_type=0, num_dmrs_cdm_grps_no_data=1, dmrs_symbol=2, fft_size=128, first_carrier_offset=128 - 60, bwp_start=1,
             rb_start=3, rb_size=3, start_symbol=0, nr_of_symbols=14, ul_dmrs_symb_pos=1 << 2, plane=4096, rx_slot_off=14 * 128, ch_off=7, rec_off=10)
    a.update(kw)
    return a


@pytest.mark.parametrize("dmrs_type", [0, 1])
@pytest.mark.parametrize("cdm", [1, 2])
def test_pusch_grid_segments_equals_the_symbol_loop(built, dmrs_type, cdm):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    if (dmrs_type, cdm) == (1, 2):
        with pytest.raises(RuntimeError):
            m.pusch_grid_segments([alloc(dmrs_config_type=1, num_dmrs_cdm_grps_no_data=2)])
        assert "type 2" in m.last_error()
        return
    # DMRS in the middle; DMRS on the first symbol; DMRS on the last symbol of a short allocation; two DMRS symbols apart; none
    shapes = [(0, 14, 1 << 2), (2, 12, 1 << 2), (0, 14, 1 << 0), (4, 6, 1 << 9), (0, 14, (1 << 2) | (1 << 11)), (1, 4, 0), (3, 1, 1 << 3)]
    allocs = []
    for i, (s0, ns, pos) in enumerate(shapes):
        if ns == 1 and pos and dmrs_type == 0 and cdm == 2:
            continue                                                  # its only symbol has no REs: refused, below
        allocs.append(alloc(tb=i, Qm=(2, 4, 6, 8)[i % 4], dmrs_config_type=dmrs_type, num_dmrs_cdm_grps_no_data=cdm, start_symbol=s0,
                            nr_of_symbols=ns, ul_dmrs_symb_pos=pos, rb_size=1 + i, rb_start=i, dmrs_symbol=(pos & -pos).bit_length() - 1 if pos else 0,
                            rec_off=1000 * i, ch_off=5 + i))
    segs, first = m.pusch_grid_segments(allocs)
    want, want_first = [], []
    for a in allocs:
        pdu = dict(a, start_symbol_index=a["start_symbol"])
        meas, rows = symbol_loop(pdu, a["Qm"])
        start_re = (a["first_carrier_offset"] + (a["rb_start"] + a["bwp_start"]) * 12) % a["fft_size"]
        for symbol, nb_re, sym_off in rows:
            is_dmrs = (a["ul_dmrs_symb_pos"] >> symbol) & 1
            d = dict(tb=a["tb"], Qm=a["Qm"], pattern=(DMRS1 if dmrs_type == 0 else DMRS2) if is_dmrs else FULL, nb_re=nb_re, plane=a["plane"],
                     sym_off=sym_off, fft_size=a["fft_size"], start_re=start_re, rx_off=a["rx_slot_off"] + symbol * a["fft_size"],
                     ch_off=a["ch_off"] + a["dmrs_symbol"] * a["fft_size"], rec_off=a["rec_off"])
            want.append(d)
            if symbol == meas:
                want_first.append(d)
    assert segs == want and first == want_first
    if dmrs_type == 0 and cdm == 2:                                   # no segment for the DMRS symbols; a DMRS first symbol is not measured
        assert all(s["pattern"] == FULL for s in segs) and first[2]["rx_off"] == 14 * 128 + 128
    else:
        assert first[2]["pattern"] != FULL and first[2]["nb_re"] == 3 * (6 if dmrs_type == 0 else 8)
    assert get_nb_re_pusch(dict(allocs[0], start_symbol_index=0), 2) == (12 - cdm * (6 if dmrs_type == 0 else 4)) * allocs[0]["rb_size"]


# (start_symbol, nr_of_symbols, DMRS symbols): two and three DMRS symbols; DMRS on the first symbol; one DMRS symbol behind the start;
# DMRS bits outside the allocation's symbols on both sides (1 and 12), two inside
FOLLOW_SHAPES = [(0, 14, (2, 11)), (0, 14, (2, 7, 11)), (0, 14, (0, 5, 10)), (1, 12, (3,)), (3, 8, (1, 5, 9, 12))]


@pytest.mark.parametrize("dmrs_type,cdm", [(0, 1), (0, 2), (1, 1)])
def test_pusch_grid_segments_follows_the_reference_dmrs_symbol(built, dmrs_type, cdm):
    """dmrs_symbol = 255: ch_off per segment from the restatement of the reference's own writes to pusch_vars->dmrs_symbol
    (rx_grid_np.dmrs_symbol_rule), not from the implementation's formula.  With one CDM group without data (either type) every DMRS
    symbol has REs and a symbol job, and the library's descriptors are the restated reference's.  With two (type 1) they DEPART from
    it, deliberately: the reference creates no job for a symbol without REs (:1666), :1408 never runs for its DMRS
    symbols and every symbol keeps the first DMRS symbol's estimates; the library moves on to each DMRS symbol's estimates all the
    same, which is the restatement with that gate lifted (job_for_every_symbol).  Both expectations are stated below."""
    import openairinterface5g_amd as pkg
    from rx_grid_np import dmrs_symbol_rule, get_next_dmrs_symbol_in_slot
    m = pkg.ldpc
    assert m.DMRS_SYMBOL_FOLLOW == 255
    allocs = [alloc(tb=i, Qm=(2, 4, 6, 8)[i % 4], dmrs_config_type=dmrs_type, num_dmrs_cdm_grps_no_data=cdm, start_symbol=s0, nr_of_symbols=ns,
                    ul_dmrs_symb_pos=sum(1 << d for d in dm), rb_size=1 + i, rb_start=i, dmrs_symbol=m.DMRS_SYMBOL_FOLLOW, rec_off=1000 * i,
                    ch_off=5 + i) for i, (s0, ns, dm) in enumerate(FOLLOW_SHAPES)]
    segs, first = m.pusch_grid_segments(allocs)
    want, want_first, spans = [], [], []
    for a, (s0, ns, dm) in zip(allocs, FOLLOW_SHAPES):
        pdu = dict(a, start_symbol_index=a["start_symbol"])
        meas, rows = symbol_loop(pdu, a["Qm"])
        with_res = [symbol for symbol, _, _ in rows]
        inside = [d for d in dm if s0 <= d < s0 + ns]
        ref_level, ref_read = dmrs_symbol_rule(pdu, chest_time=0)                             # the reference as written
        level, read = dmrs_symbol_rule(pdu, chest_time=0, job_for_every_symbol=True)          # what the library does
        # the library's rule in words: the latest DMRS symbol of the allocation at or before the symbol, the first one in front of it
        assert level == ref_level == inside[0] and read == {s: max([d for d in inside if d <= s], default=inside[0]) for s in with_res}
        if cdm == 1:
            assert ref_read == read
        else:                                                           # the departure: the reference never leaves the first DMRS symbol
            assert ref_read == {s: inside[0] for s in with_res} and not set(inside) & set(with_res)
            assert {s for s in with_res if ref_read[s] != read[s]} == ({s for s in with_res if s > inside[1]} if len(inside) > 1 else set())
        # chest_time = 1 changes the level's symbol alone, and only where :1535-1537's end_symbol = nr_of_symbols ends the search early
        level1, read1 = dmrs_symbol_rule(pdu, chest_time=1)
        assert read1 == ref_read and level1 == (level if level < ns else 255) == get_next_dmrs_symbol_in_slot(a["ul_dmrs_symb_pos"], s0, ns) & 0xff
        start_re = (a["first_carrier_offset"] + (a["rb_start"] + a["bwp_start"]) * 12) % a["fft_size"]
        for symbol, nb_re, sym_off in rows:
            is_dmrs = (a["ul_dmrs_symb_pos"] >> symbol) & 1
            d = dict(tb=a["tb"], Qm=a["Qm"], pattern=(DMRS1 if dmrs_type == 0 else DMRS2) if is_dmrs else FULL, nb_re=nb_re, plane=a["plane"],
                     sym_off=sym_off, fft_size=a["fft_size"], start_re=start_re, rx_off=a["rx_slot_off"] + symbol * a["fft_size"],
                     ch_off=a["ch_off"] + read[symbol] * a["fft_size"], rec_off=a["rec_off"])
            want.append(d)
            if symbol == meas:
                want_first.append(dict(d, ch_off=a["ch_off"] + level * a["fft_size"]))
        spans.append(sorted({read[symbol] for symbol, _, _ in rows}))
    early = dict(allocs[0], start_symbol_index=4, nr_of_symbols=6, ul_dmrs_symb_pos=1 << 9)          # the early end of :1535-1537's search
    assert dmrs_symbol_rule(early, chest_time=1)[0] == 255 and dmrs_symbol_rule(early, chest_time=0)[0] == 9
    assert segs == want and first == want_first
    assert spans == [[d for d in dm if s0 <= d < s0 + ns] for s0, ns, dm in FOLLOW_SHAPES]      # every DMRS symbol inside serves a span
    # an explicit symbol keeps its meaning: the same descriptors but for ch_off, which names that symbol everywhere
    for d_sym in (0, 2, 13):
        e_segs, e_first = m.pusch_grid_segments([dict(a, dmrs_symbol=d_sym) for a in allocs])
        off = {a["tb"]: a["ch_off"] + d_sym * a["fft_size"] for a in allocs}
        assert e_segs == [dict(s, ch_off=off[s["tb"]]) for s in want] and e_first == [dict(s, ch_off=off[s["tb"]]) for s in want_first]
    # with one DMRS symbol the two modes agree
    one = [a for a, (_, _, dm) in zip(allocs, FOLLOW_SHAPES) if len(dm) == 1]
    assert m.pusch_grid_segments(one) == m.pusch_grid_segments([dict(a, dmrs_symbol=3) for a in one])


def test_pusch_grid_segments_dmrs_symbol_refusals(built):
    """14..254 name no symbol; 255 needs a DMRS symbol inside the allocation.  Neither refusal writes anything."""
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    L = m._rxg_lib()
    bad = [(dict(dmrs_symbol=14), "0..13 or 255"), (dict(dmrs_symbol=100), "0..13 or 255"), (dict(dmrs_symbol=254), "0..13 or 255"),
           (dict(dmrs_symbol=255, ul_dmrs_symb_pos=0), "needs a DMRS symbol"),
           (dict(dmrs_symbol=255, start_symbol=4, nr_of_symbols=5, ul_dmrs_symb_pos=(1 << 2) | (1 << 10)), "needs a DMRS symbol")]
    for change, why in bad:
        with pytest.raises(RuntimeError):
            m.pusch_grid_segments([alloc(), alloc(**change)])
        assert why in m.last_error(), (change, m.last_error())
        arr = (m.nrLDPC_hip_pusch_alloc_t * 2)(*[m.nrLDPC_hip_pusch_alloc_t(**{k: a.get(k, 0) for k in m._RXG_ALLOC_KEYS}) for a in (alloc(), alloc(**change))])
        out, first, n = (m.nrLDPC_hip_rx_grid_seg_t * 28)(), (m.nrLDPC_hip_rx_grid_seg_t * 2)(), C.c_uint32(77)
        assert L.nrLDPC_hip_pusch_grid_segments(arr, 2, out, 28, first, C.byref(n)) < 0 and why in m.last_error()
        assert n.value == 77 and bytes(out) == bytes(C.sizeof(out)) and bytes(first) == bytes(C.sizeof(first))
    # the explicit symbol need not be a DMRS symbol of the allocation (the caller decides), and no DMRS symbol at all is fine with one
    m.pusch_grid_segments([alloc(dmrs_symbol=13), alloc(dmrs_symbol=0, ul_dmrs_symb_pos=0)])


def test_pusch_grid_segments_refusals(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    bad = [
        (dict(start_symbol=3, nr_of_symbols=12), "14"), (dict(start_symbol=14, nr_of_symbols=1), "14"), (dict(nr_of_symbols=0), "14"),
        (dict(ul_dmrs_symb_pos=0b1100), "adjacent"), (dict(ul_dmrs_symb_pos=(1 << 13) | 1), "adjacent"),
        (dict(rb_size=0), "rb_size"), (dict(rb_size=11), "wider"), (dict(fft_size=0), "wider"),
        (dict(plane=12 * 3 * 13 + 6 * 3 - 1), "plane"),
        (dict(dmrs_config_type=1, num_dmrs_cdm_grps_no_data=2), "type 2"),
        (dict(dmrs_config_type=2), "dmrs_config_type"), (dict(num_dmrs_cdm_grps_no_data=0), "cdm"), (dict(num_dmrs_cdm_grps_no_data=3), "cdm"),
        (dict(Qm=5), "Qm"), (dict(first_carrier_offset=128), "first_carrier_offset"),
        (dict(start_symbol=2, nr_of_symbols=1, num_dmrs_cdm_grps_no_data=2), "no symbol"),
    ]
    for change, why in bad:
        with pytest.raises(RuntimeError):
            m.pusch_grid_segments([alloc(), alloc(**change)])
        assert why in m.last_error(), (change, m.last_error())
    # adjacent DMRS symbols outside the allocation's symbols are not looked at, as in the reference
    m.pusch_grid_segments([alloc(start_symbol=4, nr_of_symbols=5, ul_dmrs_symb_pos=0b11 | (1 << 6))])
    # plane exactly reached is fine; too small a cap is refused and nothing is written
    m.pusch_grid_segments([alloc(plane=12 * 3 * 13 + 6 * 3)])
    L = m._rxg_lib()
    arr = (m.nrLDPC_hip_pusch_alloc_t * 1)(m.nrLDPC_hip_pusch_alloc_t(**{k: alloc().get(k, 0) for k in m._RXG_ALLOC_KEYS}))
    out, first, n = (m.nrLDPC_hip_rx_grid_seg_t * 14)(), (m.nrLDPC_hip_rx_grid_seg_t * 1)(), C.c_uint32(77)
    assert L.nrLDPC_hip_pusch_grid_segments(arr, 1, out, 13, first, C.byref(n)) < 0 and "cap" in m.last_error()
    assert n.value == 77 and bytes(out) == bytes(C.sizeof(out)) and bytes(first) == bytes(C.sizeof(first))
    assert L.nrLDPC_hip_pusch_grid_segments(arr, 1, out, 14, first, C.byref(n)) == 0 and n.value == 14


def test_extract_host_refusals(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    z = np.zeros((128, 2), np.int16)
    for args, why in (((3, 128, 0, 4), "pattern"), ((FULL, 128, 128, 4), "start_re"), ((FULL, 0, 0, 4), "start_re"),
                      ((FULL, 128, 5, 129), "count"), ((DMRS1, 128, 5, 65), "count"), ((DMRS2, 128, 5, 85), "count")):
        with pytest.raises(RuntimeError):
            m.ulsch_extract_host(z, z, *args)
        assert why in m.last_error(), (args, m.last_error())
    # the largest counts: p(nb_re - 1) = 127, 127, 6*21 + 1 = 127 -- DMRS2 takes 4*21 + 0 REs below 128 (126, 127 are pilots' places)
    for pattern, nb in ((FULL, 128), (DMRS1, 64), (DMRS2, 84)):
        assert p_of(pattern, nb - 1) < 128 <= p_of(pattern, nb)
        m.ulsch_extract_host(z, z, pattern, 128, 5, nb)


# ---- the HOST-mode grid calls (they stage through the GPU) against the existing HOST-mode calls on extracted arrays --------
@pytest.mark.gpu
@pytest.mark.parametrize("n_rx", [1, 2, 4])
def test_host_mode_grid_calls_equal_the_existing_calls_on_extracted_arrays(hip, n_rx):
    m = hip.ldpc
    rng = np.random.default_rng(60 + n_rx)
    N, n_rb = 128, 10
    allocs = [alloc(tb=0, Qm=6, rb_start=2, rb_size=3, bwp_start=1, rec_off=0, plane=12 * 3 * 13 + 18, dmrs_symbol=2),          # straddles the wrap
              alloc(tb=1, Qm=4, rb_start=6, rb_size=2, bwp_start=0, rec_off=2 * 4 * 500, plane=12 * 2 * 13 + 16 + 3, dmrs_config_type=1,
                    ul_dmrs_symb_pos=1 << 0, dmrs_symbol=0)]                                                                      # DMRS2 first: measured
    segs, first = m.pusch_grid_segments(allocs)
    rx_stride, ch_stride = 28 * N + 9, 14 * N + 40
    rx = rng.integers(-32768, 32768, (n_rx, rx_stride, 2)).astype(np.int16)
    ch = (rng.integers(-32768, 32768, (n_rx, ch_stride, 2)) >> 3).astype(np.int16)
    # the extracted arrays, segment after segment, with the closed form in numpy
    ext_segs, at = [], 0
    total = sum(s["nb_re"] for s in segs)
    rx_e, ch_e = np.zeros((n_rx, total, 2), np.int16), np.zeros((n_rx, total, 2), np.int16)
    for s in segs:
        idx = np.array([p_of(s["pattern"], j) for j in range(s["nb_re"])])
        rx_e[:, at:at + s["nb_re"]] = rx[:, s["rx_off"] + (s["start_re"] + idx) % N]
        ch_e[:, at:at + s["nb_re"]] = ch[:, s["ch_off"] + idx]
        ext_segs.append(dict(tb=s["tb"], Qm=s["Qm"], nb_re=s["nb_re"], plane=s["plane"], sym_off=s["sym_off"], rx_off=at, ch_off=at, rec_off=s["rec_off"]))
        at += s["nb_re"]
    ext_first = [next(e for e, s in zip(ext_segs, segs) if s == f) for f in first]
    rx0, ch0 = rx.copy(), ch.copy()
    lv = m.ulsch_channel_level_grid(ch.reshape(-1), n_rx, ch_stride, first)
    assert np.array_equal(lv, m.ulsch_channel_level(ch_e.reshape(-1), n_rx, total, ext_first))
    got, want = np.full(2 * 4 * 1100, 0x5a5a, np.int16), np.full(2 * 4 * 1100, 0x5a5a, np.int16)
    m.ulsch_channel_compensation_grid(rx.reshape(-1), ch.reshape(-1), n_rx, rx_stride, ch_stride, segs, lv, got)
    m.ulsch_channel_compensation(rx_e.reshape(-1), ch_e.reshape(-1), n_rx, total, ext_segs, lv, want)
    assert np.array_equal(got, want) and (want != 0x5a5a).sum() > total
    assert np.array_equal(rx, rx0) and np.array_equal(ch, ch0)
    # a descriptor that reaches outside the arrays is refused by the wrapper, which knows their extent
    with pytest.raises(ValueError):
        m.ulsch_channel_compensation_grid(rx.reshape(-1)[:-2 * 20 * N], ch.reshape(-1), n_rx, rx_stride, ch_stride, segs, lv, got)
    with pytest.raises(ValueError):
        m.ulsch_channel_level_grid(ch.reshape(-1)[:2 * ((n_rx - 1) * ch_stride + 7)], n_rx, ch_stride, first)
