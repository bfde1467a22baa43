"""PDSCH precoding on the CPU (csrc/nr_pdsch_map.h through nrLDPC_hip_pdsch_precode_host and nrLDPC_hip_pdsch_precode_segments)
against the literal restatement of the reference (pdsch_precode_np.py): the two restatements of nr_layer_precoder_simd agree with
each other and with the library on every RE; hand-computed values; the one deviation (the reference's nr_layer_precoder_cm steps)
pinned from both sides; PMI 0 is the unit call byte for byte; the builder; every refusal with its wording.  No GPU."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pdsch_precode_np as pre
from test_pdsch_map_host import CANARY, FILL, alloc, plane_of, rand_layers, run_host, run_ref

ROOT = Path(__file__).resolve().parent.parent
# the first Nl set bits are the layers' ports; every port of a row has the same number of data REs: (type, ncdm) -> bitmap
PORTS = {(0, 1): 0b110011, (0, 2): 0b10000111, (1, 1): 0b11000011, (1, 2): 0b1100001100, (1, 3): 0b100000011001}
EXTREME = (32767, -32768, -32767)
MILD = (0, 23170, -23170, 16384, -16384)


def first_bits(bitmap, n):
    out = 0
    for b in range(12):
        if (bitmap >> b) & 1 and n:
            out |= 1 << b
            n -= 1
    return out


def make_alloc(typ, ncdm, Nl, N, rb, k0, amp, n_sym=2):
    """DMRS on the first symbol, none on the others: two of the three patterns per allocation"""
    a = alloc(typ, first_bits(PORTS[(typ, ncdm)], Nl), ncdm, N, rb, k0, amp, 0b0100, 2, n_sym, Nl=Nl, bwp_start=1)
    a["plane"] = plane_of(a)
    return a


def matrices(rng, Nl, n_ports, values, count=3):
    """the table as the restatement indexes it: entry pmi - 1 carries pm_idx = pmi"""
    return [dict(pm_idx=t + 1, numLayers=Nl, num_ant_ports=n_ports,
                 weights=[[tuple(int(v) for v in rng.choice(values, 2)) for _ in range(n_ports)] for _ in range(Nl)]) for t in range(count)]


def mapped_grids(a, lay):
    """txdataF_precoding[layer][symbol][sc] of the reference, from the mapping restatement without its two defects"""
    tx, used = run_ref(a, lay, a["Nl"], literal_tail=False, literal_allowed=False)
    assert used == [a["plane"]] * a["Nl"]
    return [[[tuple(int(v) for v in c) for c in sym] for sym in layer] for layer in tx]


def as_array(tx):
    return np.array(tx, np.int64).astype(np.int16)


def run_lib(m, a, prg, pmis, table, lay, n_tx):
    """the builder's descriptors, every (descriptor, antenna) through pdsch_precode_host into a canary-filled slot"""
    N = a["fft_size"]
    segs, prgs = m.pdsch_precode_segments([a], [prg], len(pmis))
    tx = np.full((n_tx, 14, N, 2), CANARY, np.int16)
    planes = np.ascontiguousarray(lay[:, :a["plane"]])
    for s, g in zip(segs, prgs):
        for ant in range(n_tx):
            m.pdsch_precode_host(planes, dict(s, tx_off=s["tx_off"] + ant * 14 * N), g, pmis, table, n_tx, ant, tx.reshape(-1, 2))
    return tx


def pmi_list(rng, rb, prg_size, idx):
    """one PMI per PRG, 0 and others mixed where there is more than one; now and then an entry more than needed"""
    n = 1 if prg_size == 0 else -(-rb // prg_size)
    out = [int(v) for v in rng.integers(0, 4, n)]
    if n > 1:
        out[idx % n] = 0
        out[(idx + 1) % n] = 1 + idx % 3
    elif idx % 4:
        out[0] = 1 + idx % 3
    return out + [2] * (idx % 2)


def test_simd_restatements_and_host_form_agree(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rng = np.random.default_rng(77)
    idx, seen, up, down = 0, set(), False, False
    kinds = [(0, 1), (1, 1), (1, 2), (0, 2), (1, 3)]
    for Nl in (1, 2, 3, 4):
        for n_tx in (2, 3, 4, 8):
            if n_tx < Nl:
                continue
            for rb in (1, 2, 3, 5):
                for prg_size in (0, 1, 2, 3, rb, rb + 5):
                    idx += 1
                    N = (128, 256)[idx % 2]
                    k0 = [N - 6, N - 12 if rb > 1 else N - 2, N - 12 * rb, N - 12 * rb - 4][idx % 4]   # in a 4-group, between RBs, at the end, none
                    typ, ncdm = kinds[idx % 5]
                    hot = idx % 3 == 0
                    a = make_alloc(typ, ncdm, Nl, N, rb, k0, 32767 if hot else 512)
                    lay = rand_layers(rng, Nl, a["plane"])
                    if hot:
                        lay[:, ::2] = rng.choice(EXTREME, lay[:, ::2].shape)
                    table = matrices(rng, Nl, 8 if idx % 2 else n_tx, EXTREME + (12345,) if hot else MILD + (32767, -32768, 7))
                    pmis = pmi_list(rng, rb, prg_size, idx)
                    prg = dict(prg_size=prg_size, pmi_off=0, pmi_count=len(pmis))
                    mapped = mapped_grids(a, lay)
                    lanes, _ = pre.precode_all_simd(a, mapped, n_tx, prg_size, pmis, table, fill=FILL)
                    per_re, (u, d) = pre.precode_all_simd(a, mapped, n_tx, prg_size, pmis, table, fill=FILL, per_re=True)
                    up, down = up or u, down or d
                    assert lanes == per_re, (Nl, n_tx, rb, prg_size, N, k0)
                    got = run_lib(m, a, prg, pmis, table[::-1], lay, n_tx)                  # the library finds a matrix by its pm_idx
                    want = as_array(lanes)
                    assert np.array_equal(got, want), (Nl, n_tx, rb, prg_size, N, k0, typ, ncdm, np.argwhere(got != want)[:4])
                    assert (want != CANARY).all(-1).sum() == n_tx * 2 * 12 * rb
                    seen.update({("pattern", 0), ("pattern", 1 + typ), ("wrap", idx % 4), ("N", N), ("mixed", prg_size > 0 and 0 in pmis and any(pmis))})
    assert up and down, "the saturating cases clamp in both directions"
    assert all(("pattern", k) in seen for k in range(3)) and all(("wrap", k) in seen for k in range(4)) and ("mixed", True) in seen


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """tests/pdsch_precode_check.c over the plain-C header, with the host sanitizers"""
    exe = tmp_path_factory.mktemp("pdsch_precode") / "pdsch_precode_check"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    str(ROOT / "openairinterface5g_amd" / "csrc"), "-o", str(exe), str(ROOT / "tests" / "pdsch_precode_check.c")], check=True)
    return exe


def word(c):
    return "%08x" % ((c[0] & 0xffff) | ((c[1] & 0xffff) << 16))


def header_value(check, xs, ws, pmi=1, ant=0):
    pad = [(0, 0)] * (4 - len(xs))
    r = subprocess.run([str(check), str(len(xs)), str(pmi), str(ant)] + [word(c) for c in xs + pad + ws + pad], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    v = int(r.stdout.split()[0], 16)
    s16 = lambda x: x - 65536 if x & 0x8000 else x
    return s16(v & 0xffff), s16(v >> 16)


def simd_value(xs, ws):
    """four copies of the RE through the lane-by-lane restatement"""
    out = [None] * 4
    pre.nr_layer_precoder_simd(len(xs), [{0: [x] * 4} for x in xs], 0, dict(weights=[[w] for w in ws]), 0, 0, 4, out)
    assert out[0] == out[1] == out[2] == out[3]
    return out[0]


@pytest.mark.parametrize("xs,ws,want", [
    ([(1000, -2000)], [(0, 32767)], (1999, 999)),                       # "j": re = -x.i, im = x.r, each times 32767 / 32768, floored
    ([(-32768, -32768)], [(-32768, -32768)], (0, 0)),                   # both madd sums are 2^31, which wraps; -2^31 >> 15 has low half 0
    ([(32767, 0), (32767, 0)], [(32767, 0), (32767, 0)], (32767, 0)),   # 32766 + 32766 clamps
    ([(-32768, 0), (32767, 0)], [(32767, 0), (-32768, 0)], (-32768, 0)),  # -32767 - 32767 clamps
    ([(3, 4)], [(32767, 0)], (2, 3)),                                   # the shift floors
    ([(0, 1)], [(0, -32768)], (-1, 0)),                                 # -w.i stays -32768: re = x.i (-32768) >> 15
])
def test_hand_computed_values(check, xs, ws, want):
    assert pre.precode_re(xs, ws)[0] == want
    assert simd_value(xs, ws) == want
    assert header_value(check, xs, ws) == want


def test_header_arithmetic_at_the_extremes(check):
    """the values the library cannot reach through amp (a mapped value of -32768): every combination of extreme components, one and
    two layers, the stand-alone program under the sanitizers against both restatements"""
    vals = (-32768, -32767, 32767, 0, 1)
    cs = [(a, b) for a in vals for b in vals]
    rng = np.random.default_rng(5)
    groups, want = [], []
    for x in cs:
        for w in cs:
            x2, w2 = cs[int(rng.integers(len(cs)))], cs[int(rng.integers(len(cs)))]
            for xs, ws in (([x], [w]), ([x, x2], [w, w2])):
                pad = [(0, 0)] * (4 - len(xs))
                groups += [str(len(xs)), "1", "0"] + [word(c) for c in xs + pad + ws + pad]
                want.append(pre.precode_re(xs, ws)[0])
                assert simd_value(xs, ws) == want[-1]
    r = subprocess.run([str(check)] + groups, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = [int(v, 16) for v in r.stdout.split()]
    assert got == [int(word(c), 16) for c in want]
    # pmi 0: the copy of the antenna's layer, 0 behind the layers
    assert header_value(check, [(5, -6), (7, 8)], [(9, 9), (9, 9)], pmi=0, ant=1) == (7, 8)
    assert header_value(check, [(5, -6), (7, 8)], [(9, 9), (9, 9)], pmi=0, ant=2) == (0, 0)


def deviation_case(rng, hot):
    """three RBs, two PRGs of one matrix each, ending exactly at the symbol's end: the reference's last RB step goes through cm"""
    N, rb, Nl, n_tx = 128, 3, 2, 4
    a = make_alloc(0, 1, Nl, N, rb, N - 12 * rb, 32767 if hot else 512)
    lay = rand_layers(rng, Nl, a["plane"])
    if hot:
        lay[:] = rng.choice(EXTREME, lay.shape)
    table = matrices(rng, Nl, n_tx, EXTREME if hot else MILD)
    return a, lay, table, [1, 2], dict(prg_size=2, pmi_off=0, pmi_count=2), n_tx


def test_the_deviation_from_the_reference_is_the_cm_steps_alone(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rng = np.random.default_rng(11)
    # moderate values: the library is the reference's RB loop, cm steps included
    a, lay, table, pmis, prg, n_tx = deviation_case(rng, False)
    mapped = mapped_grids(a, lay)
    loop, path = pre.precoding_loop(a, mapped, n_tx, prg["prg_size"], pmis, table, fill=FILL)
    kinds = {p for sym in path for p in sym if p}
    assert kinds == {"simd", "cm"}
    got = run_lib(m, a, prg, pmis, table, lay, n_tx)
    assert np.array_equal(got, as_array(loop))
    # saturating values: the reference's cm REs wrap where the SIMD path clamps; the library is the SIMD definition there too
    a, lay, table, pmis, prg, n_tx = deviation_case(rng, True)
    mapped = mapped_grids(a, lay)
    loop, path = pre.precoding_loop(a, mapped, n_tx, prg["prg_size"], pmis, table, fill=FILL)
    simd, (up, down) = pre.precode_all_simd(a, mapped, n_tx, prg["prg_size"], pmis, table, fill=FILL, per_re=True)
    assert up or down
    got, loop, simd = run_lib(m, a, prg, pmis, table, lay, n_tx), as_array(loop), as_array(simd)
    assert np.array_equal(got, simd)
    cm = np.array([[p == "cm" for p in sym] for sym in path])
    differs = (loop != simd).any(-1)
    assert differs[:, cm].any() and not differs[:, ~cm].any()


def test_all_zero_pmis_equal_the_unit_host_form(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rng = np.random.default_rng(3)
    for typ, ncdm, Nl, n_tx, prg_size in ((0, 1, 2, 4, 2), (1, 2, 3, 3, 0), (1, 1, 1, 1, 1)):
        a = make_alloc(typ, ncdm, Nl, 256, 5, 256 - 30, 9000, n_sym=3)
        lay = rand_layers(rng, Nl, a["plane"])
        pmis = [0] * 5
        want, _ = run_host(m, a, lay, n_tx)
        got = run_lib(m, a, dict(prg_size=prg_size, pmi_off=0, pmi_count=5), pmis, matrices(rng, Nl, 8, MILD) if n_tx > 1 else None, lay, n_tx)
        assert got.tobytes() == want.tobytes()


def test_builder_emits_the_unit_descriptors_and_the_shared_range(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    a = make_alloc(0, 1, 2, 256, 5, 100, 512, n_sym=5)
    b = make_alloc(1, 2, 3, 128, 3, 120, 700, n_sym=2)
    b["tx_slot_off"], b["lay_off"] = 14 * 256 + 3, 2 * 2 * a["plane"]
    ga, gb = dict(prg_size=2, pmi_off=4, pmi_count=3), dict(prg_size=0, pmi_off=0, pmi_count=0)
    segs, prgs = m.pdsch_precode_segments([a, b], [ga, gb], 7)
    assert segs == m.pdsch_map_segments([a, b]) and len(segs) == 7
    assert prgs == [ga] * 5 + [gb] * 2
    for bad, words in ((dict(ga, pmi_count=2), "shorter than ceil"), (dict(ga, pmi_off=5), "outside the PMI list")):
        with pytest.raises(RuntimeError, match=words):
            m.pdsch_precode_segments([a, b], [bad, gb], 7)
    with pytest.raises(RuntimeError, match="more descriptors than cap"):
        m.pdsch_precode_segments([a, b], [ga, gb], 7, cap=6)
    with pytest.raises(RuntimeError, match="pdsch_map_segments: Nl must be"):
        m.pdsch_precode_segments([dict(a, Nl=5)], [ga], 7)


def test_refusals_leave_the_output_alone(built):
    """each refusal of the issue's list, through the CPU form and through the GPU call in HOST mode (refused ahead of any device
    work, so no GPU is needed), with its wording and the canary intact"""
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    N, Nl = 128, 2
    seg = dict(pattern=0, Nl=Nl, ncdm=0, l_prime=0, port=[], amp=512, fft_size=N, start_re=100, rb_size=3, nb_re=36, sym_off=0, plane=36, dmrs_offset=0,
               c_init=0, tx_off=0, lay_off=0)
    lay = np.full((Nl * 36, 2), 640, np.int16)                                             # mapped: mulhrs(640, 512) = 10
    mat = dict(pm_idx=7, numLayers=Nl, num_ant_ports=4, weights=[[(16384, 0)] * 4] * Nl)
    prg = dict(prg_size=2, pmi_off=1, pmi_count=2)
    pmis = [9, 7, 0]
    cases = [
        (dict(seg=dict(seg, amp=0)), "amp must be positive"),                                  # what the unit call refuses
        (dict(seg=dict(seg, nb_re=35)), "nb_re is not the number"),
        (dict(n_tx=1, seg=dict(seg, Nl=1, nb_re=36), pm=[dict(mat, numLayers=1)]), "n_tx must be at least 2"),
        (dict(n_tx=1), "n_tx is below a descriptor's Nl"),
        (dict(pmis=[9, 8, 0]), "no entry of the precoding-matrix table carries"),
        (dict(pm=[mat, dict(mat)]), "appears twice"),
        (dict(pm=[dict(mat, numLayers=3)]), "numLayers of a precoding matrix is not the descriptor's Nl"),
        (dict(pm=[dict(mat, num_ant_ports=3)]), "num_ant_ports of a precoding matrix must be n_tx..8"),
        (dict(pm=[dict(mat, num_ant_ports=9)]), "num_ant_ports of a precoding matrix must be n_tx..8"),
        (dict(pm=[mat, dict(mat, pm_idx=0)]), "pm_idx 0 in the precoding-matrix table"),
        (dict(prg=dict(prg, pmi_count=1)), "shorter than ceil"),
        (dict(prg=dict(prg, pmi_off=2)), "outside the PMI list"),
        (dict(pmis=[]), "outside the PMI list"),
        (dict(pm=None), "needs the precoding-matrix table"),
    ]
    for kw, words in cases:
        arg = dict(seg=seg, prg=prg, pmis=pmis, pm=[mat], n_tx=4)
        arg.update(kw)
        tx = np.full((4 * N, 2), CANARY, np.int16)
        with pytest.raises(RuntimeError, match="pdsch_precode_host: .*" + words):
            m.pdsch_precode_host(lay, arg["seg"], arg["prg"], arg["pmis"], arg["pm"], arg["n_tx"], 0, tx)
        with pytest.raises(RuntimeError, match="pdsch_resource_mapping_precoded: .*" + words):
            m.pdsch_resource_mapping_precoded(lay.reshape(-1), tx.reshape(-1), N, arg["n_tx"], [arg["seg"]], [arg["prg"]], arg["pmis"], arg["pm"])
        assert (tx == CANARY).all(), words
    tx = np.full((4 * N, 2), CANARY, np.int16)
    with pytest.raises(RuntimeError, match="ant must be below n_tx"):
        m.pdsch_precode_host(lay, seg, prg, pmis, [mat], 4, 4, tx)
    with pytest.raises(RuntimeError, match="overlap"):
        m.pdsch_resource_mapping_precoded(lay.reshape(-1), tx.reshape(-1), 20, 4, [seg], [prg], pmis, [mat])
    with pytest.raises(ValueError, match="one PRG record per descriptor"):
        m.pdsch_resource_mapping_precoded(lay.reshape(-1), tx.reshape(-1), N, 4, [seg], [], pmis, [mat])
    with pytest.raises(ValueError, match="leaves the grid array"):
        m.pdsch_resource_mapping_precoded(lay.reshape(-1), tx.reshape(-1)[:-8], N, 4, [seg], [prg], pmis, [mat])
    assert (tx == CANARY).all()
    # and the good call: PRG 0 (RBs 0, 1) through matrix 7 = half of each layer summed, PRG 1 (RB 2) unit
    m.pdsch_precode_host(lay, seg, prg, pmis, [mat], 4, 3, tx)
    out = tx[:N]
    assert (out[100:124] == 10).all() and (out[124:] == 0).all() and (out[:8] == 0).all() and (out[8:100] == CANARY).all()
