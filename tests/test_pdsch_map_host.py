"""PDSCH resource mapping with DMRS in closed form per RE (csrc/nr_pdsch_map.h through nrLDPC_hip_pdsch_map_host,
nrLDPC_hip_pdsch_dmrs_host and nrLDPC_hip_pdsch_map_segments, CPU only) against the literal Python restatement of the reference's
loops (pdsch_map_np.py), the two defects of the reference that are not reproduced, hand-computed values, a loop-back through the
PUSCH channel estimator's CPU form, and the refusals of the interface that need no device."""
import itertools

import numpy as np
import pytest

import pdsch_map_np as ref

FULL, DMRS1, DMRS2 = 0, 1, 2
CANARY = 0x5a5a
FILL = (CANARY, CANARY)


def alloc(typ, ports, ncdm, N, rb, start_re, amp, symb_pos, start_symbol, n_sym, Nl=1, rb_start=3, bwp_start=5, si=0, slot=7, nid=333, scid=1, plane=0,
          tx_slot_off=0, lay_off=0):
    """an allocation for both sides; first_carrier_offset is chosen so that the allocation starts at grid subcarrier start_re"""
    fco = (start_re - 12 * (rb_start + bwp_start)) % N
    return dict(Nl=Nl, plane=plane, dmrs_config_type=typ, num_dmrs_cdm_grps_no_data=ncdm, dmrs_ports=ports, scid=scid, dl_dmrs_scrambling_id=nid,
                slot=slot, si_rnti=si, rnti=ref.SI_RNTI if si else 0x1234, amp=amp, fft_size=N, first_carrier_offset=fco, bwp_start=bwp_start,
                rb_start=rb_start, rb_size=rb, start_symbol=start_symbol, nr_of_symbols=n_sym, dl_dmrs_symb_pos=symb_pos, tx_slot_off=tx_slot_off,
                lay_off=lay_off)


def pattern_count(typ, port, ncdm, rb, dmrs):
    """data REs of a symbol, from the issue's definition: pilot test first, then i % 2 >= ncdm / i % 6 >= 2 ncdm"""
    if not dmrs:
        return 12 * rb
    delta = ref.get_delta(port, typ)
    pil = (lambda i: i % 2 == delta) if typ == 0 else (lambda i: i % 6 in (delta, delta + 1))
    dat = (lambda i: i % 2 >= ncdm) if typ == 0 else (lambda i: i % 6 >= 2 * ncdm)
    return sum(1 for i in range(12 * rb) if not pil(i) and dat(i))


def plane_of(a):
    ports = [ref.get_dmrs_port(l, a["dmrs_ports"]) for l in range(a["Nl"])]
    return sum(pattern_count(a["dmrs_config_type"], ports[0], a["num_dmrs_cdm_grps_no_data"], a["rb_size"], bool(a["dl_dmrs_symb_pos"] & (1 << s)))
               for s in range(a["start_symbol"], a["start_symbol"] + a["nr_of_symbols"]))


def rand_layers(rng, Nl, plane, extra=2):
    lay = rng.integers(-32768, 32768, (Nl, plane + extra, 2)).astype(np.int16)
    lay[:, ::5] = rng.choice([32767, -32768, -32767], (Nl, len(range(0, plane + extra, 5)), 2))
    return lay


def run_ref(a, lay, n_tx, **kw):
    tx, used = ref.pdsch_resource_mapping(a, [[(int(r), int(i)) for r, i in lay[l]] for l in range(a["Nl"])], n_tx, fill=FILL, **kw)
    return np.array(tx, np.int64).astype(np.int16), used                # [n_tx, 14, N, 2]


def run_host(m, a, lay, n_tx, segs=None):
    """every (descriptor, antenna) through pdsch_map_host into a canary-filled slot"""
    N = a["fft_size"]
    segs = m.pdsch_map_segments([a]) if segs is None else segs
    tx = np.full((n_tx, 14, N, 2), CANARY, np.int16)
    planes = np.ascontiguousarray(lay[:, :a["plane"]])
    for s in segs:
        for ant in range(n_tx):
            m.pdsch_map_host(planes, dict(s, tx_off=s["tx_off"] + ant * 14 * N), ant if ant < a["Nl"] else -1, tx.reshape(-1, 2))
    return tx, segs


def starts(N, rb):
    """at 0, the wrap inside a 4-group (and a PRB), inside a PRB on a 4-group boundary, between PRBs"""
    out = [0, (N - 6) % N, (N - 8) % N]
    if rb > 1:
        out.append(N - 12 * (rb // 2))
    return out


def sweep():
    """types 1 and 2 x every port x ncdm, with the sizes, placements and amplitudes cycled so that each occurs; then every
    (rb, N, placement) with the ports cycled"""
    rbs, Ns, amps = itertools.cycle((1, 2, 3, 5, 25, 106)), itertools.cycle((128, 256, 1536)), itertools.cycle((1, 512, 32767))
    kinds = itertools.cycle(range(4))
    for typ in (0, 1):
        for port in range(8 if typ == 0 else 12):
            for ncdm in range(1, 3 if typ == 0 else 4):
                rb, N = next(rbs), next(Ns)
                while 12 * rb > N:
                    N = next(Ns)
                st = starts(N, rb)
                yield typ, port, ncdm, N, rb, st[next(kinds) % len(st)], next(amps)
    ports = [itertools.cycle(range(8)), itertools.cycle(range(12))]
    for N in (128, 256, 1536):
        for rb in (1, 2, 3, 5, 25, 106):
            if 12 * rb > N:
                continue
            for k0 in starts(N, rb):
                typ = (rb + k0) & 1
                port = next(ports[typ])
                # the CDM groups without data include the port's own, as a scheduler has it
                yield typ, port, ref.table(typ)[port][1] + 1, N, rb, k0, next(amps)


def test_host_form_equals_the_literal_loops_without_the_defects(built):
    """three symbols per case: DMRS with l' = 0, DMRS with l' = 1, no DMRS; one layer, two antennas (the second receives zeros)"""
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rng = np.random.default_rng(2024)
    seen = set()
    for typ, port, ncdm, N, rb, k0, amp in sweep():
        a = alloc(typ, 1 << port, ncdm, N, rb, k0, amp, 0b1100, 2, 3, bwp_start=int(rng.integers(0, N // 12 - 3)))   # the reference wraps start_sc once: < 2 N
        a["plane"] = plane_of(a)
        lay = rand_layers(rng, 1, a["plane"])
        want, used = run_ref(a, lay, 2, literal_tail=False, literal_allowed=False)
        assert used == [a["plane"]]
        got, segs = run_host(m, a, lay, 2)
        assert [s["pattern"] for s in segs] == [DMRS1 + typ, DMRS1 + typ, FULL] and [s["l_prime"] for s in segs] == [0, 1, 0]
        assert np.array_equal(got, want), (typ, port, ncdm, N, rb, k0, amp, np.argwhere(got != want)[:4])
        assert np.all(got[1][want[1] != CANARY] == 0) and (got[0] != CANARY).all(-1).sum() == 3 * 12 * rb
        seen.add((typ, port, ncdm))
        seen.update({("rb", rb), ("N", N), ("amp", amp), ("wrap", 0 < N - k0 < 12 * rb and (N - k0) % 4 != 0), ("wrap12", k0 and (N - k0) % 12 == 0)})
    assert all((0, p, c) in seen for p in range(8) for c in (1, 2)) and all((1, p, c) in seen for p in range(12) for c in (1, 2, 3))
    assert all(("rb", r) in seen for r in (1, 2, 3, 5, 25, 106)) and all(("N", n) in seen for n in (128, 256, 1536))
    assert all(("amp", x) in seen for x in (1, 512, 32767)) and ("wrap", True) in seen and ("wrap12", True) in seen


def test_defect_a_the_scalar_tail_differs_at_the_last_len_mod_4_res_of_each_piece(built):
    """:428-435 / :460-467 store ((x amp) >> 14) + 1 without the final shift: only at the last len % 4 REs of each of the two pieces of
    a symbol that wraps, and nowhere when both lengths are multiples of four"""
    rng = np.random.default_rng(5)
    N, rb = 128, 5
    for k0, expect in ((N - 30, {28, 29, 58, 59}), (N - 13, {12, 57, 58, 59}), (N - 24, set()), (20, set())):
        a = alloc(0, 1, 1, N, rb, k0, 512, 0, 4, 1)
        a["plane"] = 12 * rb
        lay = (rng.integers(1000, 30000, (1, a["plane"] + 2, 2)) * rng.choice([-1, 1], (1, a["plane"] + 2, 2))).astype(np.int16)
        lit, _ = run_ref(a, lay, 1)
        fixed, _ = run_ref(a, lay, 1, literal_tail=False)
        diff = {(int(k) - k0) % N for k in np.argwhere((lit[0, 4] != fixed[0, 4]).any(-1)).ravel()}
        assert diff == expect, (k0, sorted(diff))
        assert np.array_equal(np.delete(lit, 4, 1), np.delete(fixed, 4, 1))


def test_defect_b_the_first_subcarrier_of_a_dmrs_symbol(built):
    """allowed_xlsch_re_in_dmrs_symbol takes diff = fft_size at k == start_sc.  Over every port whose CDM group is among those
    without data, both types, every ncdm and fft_size 128, 256 and 1536, the literal form differs only for type 2, two groups, delta =
    2 and fft_size = 256 (256 % 6 = 4): there a data symbol lands on the allocation's first subcarrier and every later data RE takes
    the entry one further, so the differing REs are subcarrier 0 and every data RE (i % 6 >= 4)."""
    rb = 3
    hit = 0
    for typ in (0, 1):
        for port in range(8 if typ == 0 else 12):
            group = ref.table(typ)[port][1]
            for ncdm in range(group + 1, 3 if typ == 0 else 4):
                for N in (128, 256, 1536):
                    a = alloc(typ, 1 << port, ncdm, N, rb, N - 7, 32767, 1 << 2, 2, 1)
                    a["plane"] = plane_of(a)
                    lay = np.zeros((1, a["plane"] + 2, 2), np.int16)
                    lay[0, :, 0] = 100 + 3 * np.arange(a["plane"] + 2)          # all different after the scaling by 32767 / 32768
                    lay[0, :, 1] = -lay[0, :, 0]
                    lit, used = run_ref(a, lay, 1, literal_tail=False)
                    fixed, _ = run_ref(a, lay, 1, literal_tail=False, literal_allowed=False)
                    diff = {(int(k) - (N - 7)) % N for k in np.argwhere((lit[0, 2] != fixed[0, 2]).any(-1)).ravel()}
                    if typ == 1 and ncdm == 2 and ref.get_delta(port, typ) == 2 and N == 256:
                        assert diff == {0} | {i for i in range(12 * rb) if i % 6 >= 4} and used == [a["plane"] + 1]
                        hit += 1
                    else:
                        assert diff == set() and used == [a["plane"]], (typ, port, ncdm, N)
    assert hit == 4                                                     # ports 2, 3, 8 and 9


def test_hand_computed_values(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    N = 128
    lay = np.array([[3, -3], [3, -3], [3, -3], [3, -3], [3, -3], [3, -3]], np.int16)
    # a pilot with Wt Wf = -1: type 1, port 1, k' = 1, amp 1001: 16384 * -1001 >> 15 = floor(-500.5) = -501, and -16384 * -1001 >> 15 = 500
    seg = dict(pattern=DMRS1, Nl=1, ncdm=1, l_prime=0, port=[1], amp=1001, fft_size=N, start_re=0, rb_size=1, nb_re=6, sym_off=0, plane=6,
               dmrs_offset=0, c_init=12345, tx_off=0, lay_off=0)
    tx = m.pdsch_map_host(lay, seg, 0, np.full((N, 2), CANARY, np.int16))
    pil = m.pdsch_dmrs_host(12345, 0, 6).astype(np.int64)
    assert set(np.abs(pil).ravel()) == {16384}
    for j in range(6):
        for c in range(2):
            want = (500 if pil[j, c] > 0 else -501) if j % 2 == 0 else (-501 if pil[j, c] > 0 else 500)
            assert tx[2 * j, c] == want, (j, c)
    # the same port with l' = 1 (Wt = 1 for port 1) changes nothing; port 5 with l' = 1 (Wt = -1) negates every pilot's factor
    tx5 = m.pdsch_map_host(lay, dict(seg, port=[5], l_prime=1), 0, np.full((N, 2), CANARY, np.int16))
    for j in range(6):
        for c in range(2):
            want = (-501 if pil[j, c] > 0 else 500) if j % 2 == 0 else (500 if pil[j, c] > 0 else -501)
            assert tx5[2 * j, c] == want, (j, c)
    # a truncating data RE of a DMRS symbol: 3 * 8192 >> 15 = 0 and -3 * 8192 >> 15 = floor(-0.75) = -1 (odd subcarriers, ncdm = 1)
    tx = m.pdsch_map_host(lay, dict(seg, amp=8192), 0, np.full((N, 2), CANARY, np.int16))
    assert np.array_equal(tx[1:12:2], np.array([[0, -1]] * 6, np.int16))
    # the same values in a symbol without DMRS round: (((3 * 8192) >> 14) + 1) >> 1 = 1, (((-3 * 8192) >> 14) + 1) >> 1 = (-2 + 1) >> 1 = -1
    full = dict(seg, pattern=FULL, ncdm=0, amp=8192, rb_size=1, nb_re=12, plane=12)
    tx = m.pdsch_map_host(np.array([[3, -3]] * 12, np.int16), full, 0, np.full((N, 2), CANARY, np.int16))
    assert np.array_equal(tx[:12], np.array([[1, -1]] * 12, np.int16)) and np.all(tx[12:] == CANARY)


def test_pilots_are_the_qpsk_points_of_the_gold_bits_and_the_ul_pilots_their_conjugates(built):
    """pdsch_dmrs_host = mod_table(2)[bit 2s | bit 2s+1 << 1].  The PUSCH receiver's pilot of the same sequence symbol (port 0) is the
    conjugate of the same point at the receiver's own scale: the DL table holds +-16384 (32768 * 0.70711 * 0.70711 in float), the UL
    receive table +-23170, so the relation is checked on the unit points."""
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    tab = m.mod_table(2)
    for c_init, off, n in ((1, 0, 40), (0x7fffffff, 17, 333), (123456789, 1 << 12, 100)):
        w0 = (2 * off) // 32
        words = m.gold_words(c_init, w0, (2 * (off + n) + 31) // 32 - w0 + 1)
        bit = lambda b: int(words[b // 32 - w0] >> (b % 32)) & 1
        idx = np.array([bit(2 * (off + k)) | (bit(2 * (off + k) + 1) << 1) for k in range(n)])
        got = m.pdsch_dmrs_host(c_init, off, n)
        assert np.array_equal(got, tab[idx])
        for typ in (0, 1):
            ul = m.pusch_dmrs_host(c_init, off, n, 0, typ).astype(np.int64)
            assert np.array_equal(ul[:, 0] // 23170, got[:, 0].astype(np.int64) // 16384)
            assert np.array_equal(ul[:, 1] // 23170, -(got[:, 1].astype(np.int64) // 16384))
            assert set(np.abs(ul).ravel()) == {23170}
    assert m.pdsch_dmrs_host(5, 0, 0).shape == (0, 2)
    with pytest.raises(RuntimeError, match="c_init"):
        m.pdsch_dmrs_host(1 << 31, 0, 4)
    with pytest.raises(RuntimeError, match="2\\^20"):
        m.pdsch_dmrs_host(1, (1 << 20) + 1, 4)


SEG_CASES = [
    # typ, ports bitmap, Nl, ncdm, symb_pos, start, n_sym, si
    (0, 0b0001, 1, 1, 1 << 2, 0, 14, 0),                 # single-symbol DMRS
    (0, 0b0011, 2, 1, 0b11 << 2 | 0b11 << 10, 1, 13, 0),  # two double-symbol DMRS pairs: l' = 0, 1, 0, 1
    (1, 0b0101, 2, 2, 1 << 3 | 1 << 7 | 1 << 11, 2, 12, 0),
    (0, 0b10100101, 4, 2, 0b11 << 2, 0, 14, 0),          # ports 0, 2, 5, 7: both CDM groups, Wt = -1 on two of them
    (1, 0b110000001100, 4, 3, 0b11 << 3, 0, 9, 0),       # ports 2, 3, 10, 11
    (0, 0, 1, 2, 1 << 2, 2, 6, 1),                       # DCI 1_0 (empty bitmap: port 0), SI-RNTI: the reference point leaves bwp_start out
    (1, 0b0010, 1, 1, 1 << 2 | 1 << 3, 3, 4, 1),         # starts on the second symbol of the pair: l' = 1 from the whole bitmap's l0
]


@pytest.mark.parametrize("case", range(len(SEG_CASES)))
def test_segments_equal_the_restatement(built, case):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    typ, ports, Nl, ncdm, pos, start, n_sym, si = SEG_CASES[case]
    rng = np.random.default_rng(300 + case)
    N, rb = 256, 5
    a = alloc(typ, ports, ncdm, N, rb, N - 19, 700, pos, start, n_sym, Nl=Nl, si=si, slot=11 + case, nid=1000 * case + 7, scid=case & 1, tx_slot_off=9,
              lay_off=6)
    plist = [ref.get_dmrs_port(l, ports) for l in range(Nl)]
    counts = {pattern_count(typ, p, ncdm, rb, True) for p in plist}
    assert len(counts) == 1, "the case must give every layer the same number of data REs"
    a["plane"] = plane_of(a)
    segs = m.pdsch_map_segments([a])
    want = ref.symbol_params(a)
    assert len(segs) == n_sym
    off = 0
    for s, w in zip(segs, want):
        assert s["pattern"] == ((DMRS1 + typ) if w["dmrs"] else FULL) and s["Nl"] == Nl and s["amp"] == 700
        assert s["start_re"] == ref.start_subcarrier(a) == N - 19 and s["fft_size"] == N and s["rb_size"] == rb
        assert s["tx_off"] == 9 + w["symbol"] * N and s["lay_off"] == 6 and s["plane"] == a["plane"] and s["sym_off"] == off
        assert s["nb_re"] == pattern_count(typ, plist[0], ncdm, rb, w["dmrs"])
        off += s["nb_re"]
        if w["dmrs"]:
            assert (s["l_prime"], s["dmrs_offset"], s["c_init"], s["ncdm"]) == (w["l_prime"], w["dmrs_idx"], w["c_init"], ncdm)
            assert s["port"][:Nl] == plist
    assert off == a["plane"]
    # and the slot through the descriptors equals the loops (one antenna more than layers)
    lay = rand_layers(rng, Nl, a["plane"], extra=0)
    n_tx = Nl + 1
    refa = dict(a, tx_slot_off=0, lay_off=0)
    wantx, used = run_ref(refa, lay, n_tx, literal_tail=False, literal_allowed=False)
    got, _ = run_host(m, refa, lay, n_tx)
    assert used == [a["plane"]] * Nl and np.array_equal(got, wantx)


def test_segments_refusals(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    good = alloc(0, 0b11, 1, 128, 5, 100, 512, 1 << 2, 0, 14, Nl=2)
    good["plane"] = plane_of(good)
    assert len(m.pdsch_map_segments([good])) == 14

    def refused(match, cap=None, **kw):
        with pytest.raises(RuntimeError, match=match):
            m.pdsch_map_segments([dict(good, **kw)], cap=cap)
    refused("add up", plane=good["plane"] + 1)                          # the running sum differs from plane at the end
    refused("add up", plane=good["plane"] - 1)
    refused("within the slot", start_symbol=3, nr_of_symbols=12)
    refused("within the slot", nr_of_symbols=0)
    refused("no port for a layer", dmrs_ports=0b100)
    refused("cap", cap=13)
    # what the mapping call would refuse
    refused("Nl must be", Nl=5)
    refused("Nl must be", Nl=0)
    refused("amp must be", amp=0)
    refused("amp must be", amp=32768)
    refused("amp must be", amp=-5)
    refused("rb_size is 0", rb_size=0)
    refused("wider than fft_size", rb_size=11)
    refused("fft_size must be", fft_size=384, first_carrier_offset=0)
    refused("first_carrier_offset", first_carrier_offset=128)
    refused("dmrs_config_type", dmrs_config_type=2)
    refused("must be 1..2 for type 1", num_dmrs_cdm_grps_no_data=3)
    refused("must be 1..2 for type 1", num_dmrs_cdm_grps_no_data=0)
    refused("must be 1..2 for type 1", num_dmrs_cdm_grps_no_data=257)
    refused("port must be", dmrs_ports=0b100000001)                     # port 8 in type 1
    refused("nb_re is not", dmrs_ports=0b101)                           # ports 0 and 2 with one group without data: 6 and 0 data REs per PRB
    refused("lay_off must be even", lay_off=3)
    refused("scid", scid=2)
    refused("dl_dmrs_scrambling_id", dl_dmrs_scrambling_id=1 << 16)
    refused("slot must be", slot=160)


def test_loop_back_through_the_pusch_estimator(built):
    """One layer (type 1, port 0, ncdm = 2, amp 512, 25 RBs) mapped by pdsch_map_host and read back by nrLDPC_hip_pusch_chest_host
    (TYPE1_INTERP, delay 0) with the same c_init and dmrs_offset.  A pilot is (+-16384 * 512) >> 15 = +-256 exactly on both components;
    the estimator multiplies by the conjugate at +-23170 and shift 16 and adds the two pilots of a pair: 2 * ((2 * 256 * 23170) >> 16) =
    362, the same for every pair, imaginary part 0.  Its interpolation then adds shares of that value through mulhrs and a doubling:
    eight shares of 1/8 in the middle (8 * 2 * 23 = 368), coarser shares at the two edges (362 and 366) -- the estimator's own rounding
    of a constant.  Observed here over the 300 estimates: real parts 362 .. 368 (spread 6), imaginary parts all 0 (spread 0).  The
    bounds are the observed spreads + 1."""
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    N, rb = 512, 25
    c_init, off = ref.c_init_pdsch(4, 2, 99, 0), 48
    seg = dict(pattern=DMRS1, Nl=1, ncdm=2, l_prime=0, port=[0], amp=512, fft_size=N, start_re=N - 100, rb_size=rb, nb_re=0, sym_off=0, plane=0,
               dmrs_offset=off, c_init=c_init, tx_off=0, lay_off=0)
    tx = m.pdsch_map_host(np.zeros((1, 2), np.int16), seg, 0, np.zeros((N, 2), np.int16))
    ch = np.full((12 * rb, 2), CANARY, np.int16)
    m.pusch_chest_host(tx, dict(mode=0, port=0, fft_size=N, start_re=N - 100, rb_size=rb, dmrs_offset=off, c_init=c_init, rx_off=0, ch_off=0, delay_off=0),
                       0, ch)
    re, im = ch[:, 0].astype(int), ch[:, 1].astype(int)
    print("loop-back real", re.min(), re.max(), "imag", im.min(), im.max())
    assert re.max() - re.min() <= 6 + 1 and im.max() - im.min() <= 0 + 1
    assert abs(im).max() <= 1 and abs(int(np.median(re)) - 368) <= 1


def test_mapping_refusals_that_need_no_device(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    L = m._pdm_lib()
    N = 128
    good = dict(pattern=DMRS1, Nl=1, ncdm=1, l_prime=0, port=[0], amp=512, fft_size=N, start_re=100, rb_size=2, nb_re=12, sym_off=0, plane=12,
                dmrs_offset=0, c_init=5, tx_off=0, lay_off=0)
    lay, tx = np.zeros((2 * 24, 2), np.int16), np.full((4 * N, 2), CANARY, np.int16)

    def call(segs, n_tx=1, stride=N, layers=lay.ctypes.data, out=tx.ctypes.data, mem=m.MEM_HOST, n=None):
        return L.nrLDPC_hip_pdsch_resource_mapping(layers, out, stride, n_tx, m._pdm_seg_array(segs), len(segs) if n is None else n, mem, None)

    def refused(match, segs, host=True, **kw):
        assert call(segs, **kw) < 0 and match in m.last_error(), m.last_error()
        if host:                                                        # the CPU form checks a descriptor the same way
            with pytest.raises(RuntimeError, match=match.replace("^", "\\^")):
                m.pdsch_map_host(lay, segs[0], 0, tx)
    refused("null argument", [good], layers=None, host=False)
    refused("null argument", [good], out=None, host=False)
    refused("n_tx must be 1..8", [good], n_tx=0, host=False)
    refused("n_tx must be 1..8", [good], n_tx=9, host=False)
    refused("n_tx is below", [dict(good, Nl=2, port=[0, 1], plane=12)], n_tx=1, host=False)
    refused("mem must be", [good], mem=7, host=False)
    refused("pattern must be", [dict(good, pattern=3)])
    refused("Nl must be", [dict(good, Nl=0)])
    refused("Nl must be", [dict(good, Nl=5)], n_tx=8)
    refused("ncdm must be", [dict(good, ncdm=0)])
    refused("ncdm must be", [dict(good, ncdm=3)])
    refused("ncdm must be", [dict(good, pattern=DMRS2, ncdm=4)])
    refused("l_prime must be", [dict(good, l_prime=2)])
    refused("port must be", [dict(good, port=[8])])
    refused("port must be", [dict(good, pattern=DMRS2, port=[12])])
    refused("amp must be positive", [dict(good, amp=0)])
    refused("amp must be positive", [dict(good, amp=-3)])
    refused("rb_size is 0", [dict(good, rb_size=0)])
    refused("wider than fft_size", [dict(good, rb_size=11)])
    refused("start_re must be below", [dict(good, start_re=N)])
    refused("fft_size must be", [dict(good, fft_size=384)])
    refused("nb_re is not", [dict(good, nb_re=11)])
    refused("nb_re is not", [dict(good, pattern=FULL, ncdm=0)])
    refused("nb_re is not", [dict(good, Nl=2, port=[0, 2], plane=24)], n_tx=2)
    refused("above plane", [dict(good, sym_off=1)])
    refused("c_init must be below 2^31", [dict(good, c_init=1 << 31)])
    refused("dmrs_offset above 2^20", [dict(good, dmrs_offset=(1 << 20) + 1)])
    refused("lay_off must be even", [dict(good, lay_off=1)])
    refused("overlap", [good, dict(good, tx_off=20)], host=False)                   # REs 100..123 and 120..143
    refused("overlap", [good, dict(good, start_re=N - 12, tx_off=110)], host=False)  # the wrapped piece of the second, 110..121, meets the first
    refused("overlap", [good], n_tx=2, stride=20, host=False)                       # across antennas through a short stride
    assert np.all(tx == CANARY), "a refused call writes nothing"
    with pytest.raises(RuntimeError, match="layer must be below Nl"):
        m.pdsch_map_host(lay, good, 1, tx)
    assert call([], n=0) == 0                                           # no descriptors: nothing to do, no device needed
