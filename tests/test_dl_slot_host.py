"""The DL transmit grid of the CPU forms (pdsch_map_segments / pdsch_precode_segments, pdsch_map_host / pdsch_precode_host per
(descriptor, antenna); no GPU) against dl_slot_np.py, a float64 PDSCH transmitter that knows only TS 38.211 / 38.214.  Every other
DL test compares the library with a restatement of the reference; this one would notice a misreading that the two share.

The bound on |txdataF - (amp / sqrt 2) model| per component, term by term (bound_of() below).  s = amp / 32768.

  table.  nr_gen_mod_table computes level * 32768 * c_Qm * 0.70711 in float32, c_Qm = 0.70711, 0.31623, 0.15430, 0.076696 for 1 / sqrt
      2, 10, 42, 170, and truncates to int16: at most 1 LSB, plus the relative error of c_Qm * 0.70711 against 1 / sqrt(2 norm) and
      five float32 roundings (two constants, three products; 2^-24 each), times the largest table component 32768 / sqrt 2 * max|d|
      (max|d| = 1, 3, 7, 15 over sqrt 2, 10, 42, 170).  T(Qm) = 1.15, 1.26, 1.44, 1.06 for Qm = 2, 4, 6, 8.  The ideal value of a table
      entry is 32768 / sqrt 2 times the model's component, so s times the entry is (amp / sqrt 2) model to within s T.
  scaling.  The entry is multiplied by amp / 32768: s T(Qm) for data, s T(2) for a pilot (a QPSK point times +-1).
  rounding.  A symbol without DMRS rounds to nearest (mulhrs): 0.5.  Pilots, and data in a DMRS symbol, are floored by an arithmetic
      shift: 1.  The REs of CDM groups without data are written as 0 and are 0 in the model; they take the DMRS symbol's bound.
  mapped value's bound  m = s T(Qm) + 0.5 in a symbol without DMRS, s max(T(Qm), T(2)) + 1 in a DMRS symbol.
  precoded.  A term is floor((x_r w_r - x_i w_i) / 32768) (or the imaginary counterpart): an error of m in x moves it by at most
      (|w_r| + |w_i|) / 32768 m, and its floor adds 1; the terms add up without saturating because the weights of every antenna are
      chosen with sum_l (|w_r| + |w_i|) <= 32767.  Antenna a: sum_l ((|w_r| + |w_i|) / 32768 m + 1).  W itself is exact: the model
      takes weights / 32768.  An RB of a PRG with PMI 0 is a copy: m.

The derived figure is the bound; nothing in it is measured.  Each case prints the largest error of the host form next to it, and
DESIGN section 4.13.2 records both.

The perturbations (perturbations() below) are small mistakes of the kind a restatement could share with the code, built by editing
descriptors or planes and run through the same host forms.  Each must miss the case's largest bound by three times on at least
one RE in every case it applies to; where it is listed for a case and changes nothing, the test fails."""
import re
from pathlib import Path

import numpy as np
import pytest

import dl_slot_np as D
import oracle_lib as O
from layer_np import symbols_np

CANARY = 0x5a5a
NAMES = [c["name"] for c in D.CASES]
TX_OFF = 3                              # the slot's first c16 in an antenna's array
PAD = 7                                 # c16 behind the slot
C_QM = {2: 0.70711, 4: 0.31623, 6: 0.15430, 8: 0.076696}
NORM = {2: 2.0, 4: 10.0, 6: 42.0, 8: 170.0}
MISS = 3.0                              # by how much a perturbation must miss the bound


def table_term(Qm):
    """T(Qm) of the module docstring, in LSB of the constellation table"""
    rel = abs(C_QM[Qm] * 0.70711 * np.sqrt(2.0 * NORM[Qm]) - 1.0) + 5 * 2.0 ** -24
    largest = 32768.0 / np.sqrt(2.0) * (2 ** (Qm // 2) - 1) / np.sqrt(NORM[Qm])
    return 1.0 + rel * largest


def data_res_per_prb(typ, ncdm, port):
    """REs of a PRB of a DMRS symbol that carry PDSCH: outside the CDM groups 0 .. ncdm - 1 and outside the port's own pilots"""
    comb, width = (2, 1) if typ == 0 else (6, 2)
    deltas = {(g if typ == 0 else 2 * g) for g in range(ncdm)} | {D.dmrs_table(typ)[port][2]}
    return sum(1 for r in range(12) if not any((r - d) % comb < width for d in deltas))


def plane_of(typ, ncdm, port, pos, start, n_sym, rb):
    return sum(rb * (data_res_per_prb(typ, ncdm, port) if pos & (1 << l) else 12) for l in range(start, start + n_sym))


def make_alloc(c, plane, **kw):
    N, (bwp, rbs) = c["N"], c["first_rb"]
    k0 = N - 12 * (c["rb"] // 2) - 5                                    # the wrap lies inside a PRB and inside a group of four REs
    a = dict(Nl=c["Nl"], plane=plane, dmrs_config_type=c["typ"], num_dmrs_cdm_grps_no_data=c["ncdm"], dmrs_ports=c["ports"], scid=int(c["name"]) & 1,
             dl_dmrs_scrambling_id=1000 + 37 * int(c["name"]), slot=int(c["name"]) + 2, si_rnti=c["si"], amp=c["amp"], fft_size=N,
             first_carrier_offset=(k0 - 12 * (bwp + rbs)) % N, bwp_start=bwp, rb_start=rbs, rb_size=c["rb"], start_symbol=c["start"],
             nr_of_symbols=c["n_sym"], dl_dmrs_symb_pos=c["pos"], tx_slot_off=TX_OFF, lay_off=0)
    a.update(kw)
    return a


def descriptors(m, c, a, prg=None):
    """(descriptors, their PRG records or None) of one allocation"""
    if c["prg"] is None:
        return m.pdsch_map_segments([a]), None
    prg = dict(prg_size=c["prg"], pmi_off=0, pmi_count=len(c["pmis"])) if prg is None else prg
    return m.pdsch_precode_segments([a], [prg], len(c["pmis"]))


def matrices_for(rng, c):
    """one matrix per PMI in use: int16 weights [Nl][n_tx][2] with sum_l (|w_r| + |w_i|) <= 32767 on every antenna, both parts of
    every weight away from 0"""
    out = []
    for pmi in sorted(set(c["pmis"]) - {0}):
        mag = rng.uniform(0.5, 0.98, (c["Nl"], c["n_tx"])) * 32767 / (np.sqrt(2.0) * c["Nl"])
        ph = rng.uniform(0.15, np.pi / 2 - 0.15, (c["Nl"], c["n_tx"])) + np.pi / 2 * rng.integers(0, 4, (c["Nl"], c["n_tx"]))
        w = np.rint(np.stack([mag * np.cos(ph), mag * np.sin(ph)], -1)).astype(np.int16)
        assert (np.abs(w.astype(np.int64)).sum(axis=(0, 2)) <= 32767).all() and (np.abs(w) > 100).all()
        out.append(dict(pm_idx=pmi, numLayers=c["Nl"], num_ant_ports=c["n_tx"], weights=w))
    return out


def model_matrices(table):
    return {t["pm_idx"]: (t["weights"][..., 0].astype(np.float64) + 1j * t["weights"][..., 1]) / 32768.0 for t in table}


def bound_of(c, mask, table):
    """the bound per antenna and RE, float64 [n_tx, 14, N] (0 outside the allocation), from the case alone"""
    s = c["amp"] / 32768.0
    mapped = np.zeros(14)
    for l in range(c["start"], c["start"] + c["n_sym"]):
        mapped[l] = s * max(table_term(c["Qm"]), table_term(2)) + 1.0 if c["pos"] & (1 << l) else s * table_term(c["Qm"]) + 0.5
    b = np.zeros((c["n_tx"], 14, c["N"]))
    k0 = int(np.flatnonzero(mask[c["start"]] & ~np.roll(mask[c["start"]], 1))[0])   # the allocation's first subcarrier on the grid
    W = {t["pm_idx"]: np.abs(t["weights"].astype(np.float64)).sum(-1) / 32768.0 for t in table}
    for rb in range(c["rb"]):
        pmi = c["pmis"][rb // c["prg"]] if c["prg"] else 0
        ks = (k0 + 12 * rb + np.arange(12)) % c["N"]
        for a in range(c["n_tx"]):
            per_sym = mapped if pmi == 0 else sum(W[pmi][l, a] * mapped + (mapped > 0) for l in range(c["Nl"]))
            b[a][:, ks] = per_sym[:, None]
    return b * mask[None]


def build_slot(m, c):
    """The transport block, the layer planes, the descriptors, the model's grid and the bound of one case"""
    from test_gpu_tb_chain import valid_tbs
    rng = np.random.default_rng(7100 + int(c["name"]))
    ports = D.ports_of(c["ports"], c["Nl"])
    S = plane_of(c["typ"], c["ncdm"], ports[0], c["pos"], c["start"], c["n_sym"], c["rb"])
    assert all(plane_of(c["typ"], c["ncdm"], p, c["pos"], c["start"], c["n_sym"], c["rb"]) == S for p in ports)
    G = c["Qm"] * c["Nl"] * S
    tb = dict(A=valid_tbs(G // 2, c["BG"]), G=G, BG=c["BG"], Qm=c["Qm"], Nl=c["Nl"], rv=0, tbslbrm=0)
    scr = (0xffff if c["si"] else int(rng.integers(1, 0xfff0)), 0, int(rng.integers(0, 1024)))
    pay = rng.integers(0, 256, tb["A"] // 8, dtype=np.uint8)
    bits = O.dlsch_encode(tb, pay)
    tx = symbols_np(bits, scr, c["Qm"], c["Nl"])                       # = dlsch_encode_symbols_host, which needs a GPU (the GPU test checks)
    assert tx.shape == (c["Nl"], S, 2)
    a = make_alloc(c, S)
    segs, prgs = descriptors(m, c, a)
    table = matrices_for(rng, c)
    p = dict(a, Qm=c["Qm"], rnti=scr[0], q=scr[1], n_id=scr[2])
    grid, mask = D.pdsch_grid(p, bits, c["n_tx"], beta_dmrs=1.0, prg_size=c["prg"] or 0, pmis=c["pmis"], matrices=model_matrices(table))
    want = c["amp"] / np.sqrt(2.0) * np.stack([grid.real, grid.imag], -1)
    return dict(case=c, tb=tb, scr=scr, pay=pay, bits=bits, tx=tx, alloc=a, segs=segs, prgs=prgs, table=table, model=grid, mask=mask, want=want,
                bound=bound_of(c, mask, table), stride=14 * c["N"] + TX_OFF + PAD, p=p)


_SLOTS = {}


def slot_of(m, name):
    """The case's slot, built once per session and shared; nobody writes to it."""
    if name not in _SLOTS:
        _SLOTS[name] = build_slot(m, D.CASE_BY_NAME[name])
        for v in _SLOTS[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _SLOTS[name]


def run_host(m, sl, segs=None, prgs=None, planes=None, pmis=None, table=None, dmrs_unit=False):
    """every (descriptor, antenna) through the host forms into a canary-filled array of n_tx + 1 antennas: int16 [n_tx + 1, stride, 2]"""
    c = sl["case"]
    segs, prgs = sl["segs"] if segs is None else segs, sl["prgs"] if prgs is None else prgs
    planes = np.ascontiguousarray(sl["tx"] if planes is None else planes)
    pmis, table = c["pmis"] if pmis is None else pmis, sl["table"] if table is None else table
    tx = np.full(((c["n_tx"] + 1) * sl["stride"], 2), CANARY, np.int16)
    for i, s in enumerate(segs):
        for ant in range(c["n_tx"]):
            d = dict(s, tx_off=s["tx_off"] + ant * sl["stride"])
            if c["prg"] is not None and not (dmrs_unit and s["pattern"]):
                m.pdsch_precode_host(planes, d, prgs[i], pmis, table, c["n_tx"], ant, tx)
            else:
                m.pdsch_map_host(planes, d, ant if ant < c["Nl"] else -1, tx)
    return tx.reshape(c["n_tx"] + 1, sl["stride"], 2)


def slot_view(sl, tx):
    """the slot of every antenna: [n_tx, 14, N, 2]"""
    c = sl["case"]
    return tx[:c["n_tx"], TX_OFF:TX_OFF + 14 * c["N"]].reshape(c["n_tx"], 14, c["N"], 2)


def grid_error(sl, tx):
    """|txdataF - (amp / sqrt 2) model| per antenna, RE and component on the allocation, 0 elsewhere: float64 [n_tx, 14, N, 2]"""
    return np.abs(slot_view(sl, tx).astype(np.float64) - sl["want"]) * sl["mask"][None, :, :, None]


def check_grid(sl, tx, who):
    """the assertion of the issue: the bound at every RE of the allocation, the fill everywhere else.  Returns the largest error."""
    c = sl["case"]
    err = grid_error(sl, tx)
    over = err > sl["bound"][..., None]
    assert not over.any(), (who, c["name"], np.argwhere(over)[:4], float(err.max()))
    outside = np.ones(tx.shape[:2], bool)
    outside[:c["n_tx"], TX_OFF:TX_OFF + 14 * c["N"]] = ~np.broadcast_to(sl["mask"].reshape(-1), (c["n_tx"], 14 * c["N"]))
    assert (tx[outside] == np.int16(CANARY)).all(), (who, c["name"], "written outside the allocation")
    inside = slot_view(sl, tx)[:, sl["mask"]]
    assert (inside != np.int16(CANARY)).any(-1).mean() > 0.99, (who, c["name"], "the allocation is not written")
    if c["prg"] is None:                                               # without precoding, what the model leaves empty is exactly 0
        empty = (sl["model"] == 0) & sl["mask"][None]
        assert (slot_view(sl, tx)[empty] == 0).all(), (who, c["name"])
    return float(err.max())


# ---- the model itself ------------------------------------------------------------------------------------------------------
def test_the_model_names_no_restatement_and_no_library_generator():
    src = (Path(__file__).resolve().parent / "dl_slot_np.py").read_text()
    assert re.findall(r"^\s*(?:import|from)\s+(\S+)", src, re.M) == ["numpy"] and not re.search(
        r"pdsch_map_np|pdsch_precode_np|layer_np|qam_np|rx_\w*_np|ul_slot_np|gold_words|mod_table|pdsch_dmrs_host|pusch_dmrs_host|layer_mapping", src)


def test_gold_words_of_the_model_equal_the_library(built):
    import openairinterface5g_amd as pkg
    for c_init, w0, n in ((1, 0, 8), (0x7fffffff, 5, 40), (D.dmrs_c_init(19, 13, 65535, 1), 123, 17)):
        bits = D.gold(c_init, 32 * (w0 + n))[32 * w0:].reshape(n, 32).astype(np.uint64)
        words = (bits << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)
        assert np.array_equal(words, np.asarray(pkg.ldpc.gold_words(c_init, w0, n), np.uint32)), (c_init, w0)


def test_dmrs_tables_are_orthogonal_within_a_cdm_group():
    for typ, n_ports, n_groups in ((0, 8, 2), (1, 12, 3)):
        rows = D.dmrs_table(typ)
        assert [r[0] for r in rows] == list(range(n_ports))
        for g in range(n_groups):
            mine = [r for r in rows if r[1] == g]
            assert len(mine) == 4 and all(r[2] == (g if typ == 0 else 2 * g) for r in mine)
            vec = np.array([[wf * wt for wt in r[5:7] for wf in r[3:5]] for r in mine])
            assert np.array_equal(vec @ vec.T, 4 * np.eye(4, dtype=int)), (typ, g)


def test_constellations_have_unit_power_and_gray_neighbours():
    for Qm in (2, 4, 6, 8):
        idx = np.arange(1 << Qm)
        bits = ((idx[:, None] >> np.arange(Qm)) & 1).reshape(-1)       # point i from the bits b(k) = bit k of i
        d = D.modulate(bits, Qm)
        assert abs(np.mean(np.abs(d) ** 2) - 1.0) < 1e-12 and len(set(np.round(d, 9))) == 1 << Qm
        step = 2.0 / np.sqrt(NORM[Qm])
        dist = np.abs(d[:, None] - d[None, :])
        near = np.abs(dist - step) < 1e-9
        assert near.sum() == 2 * 2 * (2 ** (Qm // 2)) * (2 ** (Qm // 2) - 1)   # every edge of the square lattice, both directions
        flips = np.array([[bin(i ^ j).count("1") for j in idx] for i in idx])
        assert (flips[near] == 1).all(), Qm


def test_l_prime_and_ports():
    assert D.l_primes(0b11 << 2) == {2: 0, 3: 1} and D.l_primes(1 << 2 | 1 << 7 | 1 << 11) == {2: 0, 7: 0, 11: 0}
    assert D.l_primes(0b11 << 2 | 0b11 << 10) == {2: 0, 3: 1, 10: 0, 11: 1}
    assert D.ports_of(0, 1) == [0] and D.ports_of(0b10100101, 4) == [0, 2, 5, 7] and D.ports_of(0b110000001100, 2) == [2, 3]


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def prg_kinds(c):
    """the kinds of PRG a case holds: 'unit' (PMI 0), 'full' (prg_size RBs through a matrix), 'partial' (fewer), 'wideband'"""
    out = set()
    if c["prg"]:
        for q, pmi in enumerate(c["pmis"][:-(-c["rb"] // c["prg"])]):
            n = min(c["prg"], c["rb"] - q * c["prg"])
            out.add("unit" if pmi == 0 else "wideband" if n == c["rb"] else "full" if n == c["prg"] else "partial")
    return out


def test_the_cases_cover_what_they_are_meant_to():
    seen = dict(typ=set(), lp=set(), wt=set(), delta=set(), ncdm=set(), Nl=set(), prg=set(), amp=set(), Qm=set())
    for c in D.CASES:
        N, first = c["N"], sum(c["first_rb"])
        assert 128 <= N <= 512 and 2 <= c["rb"] <= 6 and c["n_sym"] <= 14 and first % 2 == 1 and c["n_tx"] >= c["Nl"]
        k0 = (make_alloc(c, 0)["first_carrier_offset"] + 12 * first) % N
        assert k0 + 12 * c["rb"] > N, "the allocation runs over the end of the grid"
        rows = [D.dmrs_table(c["typ"])[p] for p in D.ports_of(c["ports"], c["Nl"])]
        assert all(r[1] < c["ncdm"] for r in rows), "a port's CDM group is among those without data, as a scheduler has it"
        lps = {v for l, v in D.l_primes(c["pos"]).items() if c["start"] <= l < c["start"] + c["n_sym"]}
        seen["typ"].add(c["typ"])
        seen["lp"] |= lps
        seen["wt"] |= {r[6] for r in rows if 1 in lps}
        seen["delta"] |= {(c["typ"], r[2]) for r in rows}
        seen["ncdm"].add(c["ncdm"])
        seen["Nl"].add(c["Nl"])
        seen["prg"] |= prg_kinds(c)
        seen["amp"].add(c["amp"])
        seen["Qm"].add(c["Qm"])
        if c["prg"]:
            assert len(c["pmis"]) == -(-c["rb"] // c["prg"])
    assert seen["typ"] == {0, 1} and seen["lp"] == {0, 1} and -1 in seen["wt"]
    assert seen["delta"] == {(0, 0), (0, 1), (1, 0), (1, 2), (1, 4)}
    assert seen["ncdm"] == {1, 2, 3} and seen["Nl"] == {1, 2, 3, 4}
    assert seen["prg"] == {"unit", "full", "partial", "wideband"} and seen["amp"] == {512, 8192, 32767} and seen["Qm"] == {2, 4, 6, 8}
    # the allocation of case 8 starts on the second symbol of its pair, case 7 is the SI-RNTI one, case 11's first RB is no PRG edge
    c8, c7, c11 = D.CASE_BY_NAME["8"], D.CASE_BY_NAME["7"], D.CASE_BY_NAME["11"]
    assert D.l_primes(c8["pos"])[c8["start"]] == 1 and c7["si"] == 1 and c7["ports"] == 0 and c7["first_rb"][0] > 0
    assert sum(c11["first_rb"]) % c11["prg"] != 0


# ---- perturbations -------------------------------------------------------------------------------------------------------------
def replane(tx, plane):
    out = np.zeros((tx.shape[0], plane, 2), np.int16)
    n = min(plane, tx.shape[1])
    out[:, :n] = tx[:, :n]
    return out


def rebuilt(m, sl, **kw):
    """descriptors and planes of the case's allocation with some fields changed (the plane follows the new number of data REs)"""
    c = sl["case"]
    a = dict(sl["alloc"], **kw)
    port0 = D.ports_of(a["dmrs_ports"], c["Nl"])[0]
    a["plane"] = plane_of(c["typ"], a["num_dmrs_cdm_grps_no_data"], port0, c["pos"], c["start"], c["n_sym"], c["rb"])
    segs, prgs = descriptors(m, c, a)
    return dict(segs=segs, prgs=prgs, planes=replane(sl["tx"], a["plane"]))


def edit_dmrs(sl, fn):
    return dict(segs=[fn(dict(s, port=list(s["port"]))) if s["pattern"] else s for s in sl["segs"]])


def perturbations(m, sl):
    """name -> keyword arguments of run_host, for the perturbations that apply to the case"""
    c = sl["case"]
    typ, ncdm, Nl = c["typ"], c["ncdm"], c["Nl"]
    rows = D.dmrs_table(typ)
    ports = D.ports_of(c["ports"], Nl)
    out = {}

    def set_port(s, layer, port):
        s["port"][layer] = port
        return s
    out["port of the last layer replaced by its CDM-group neighbour (w_f)"] = edit_dmrs(sl, lambda s: set_port(s, Nl - 1, ports[Nl - 1] ^ 1))
    minus = [l for l, p in enumerate(ports) if rows[p][6] == -1]
    if minus and any(s["pattern"] and s["l_prime"] for s in sl["segs"]):
        out["l_prime flipped on the pair's second symbol (w_t)"] = edit_dmrs(sl, lambda s: dict(s, l_prime=s["l_prime"] ^ 1) if s["l_prime"] else s)
    out["dmrs_offset + 1"] = edit_dmrs(sl, lambda s: dict(s, dmrs_offset=s["dmrs_offset"] + 1))
    sym_of = lambda s: (s["tx_off"] - TX_OFF) // c["N"]
    a = sl["alloc"]
    out["c_init of the next symbol"] = edit_dmrs(sl, lambda s: dict(s, c_init=D.dmrs_c_init(a["slot"], sym_of(s) + 1, a["dl_dmrs_scrambling_id"], a["scid"])))
    if ncdm >= 2:                                                      # another group without data: the number of data REs stays
        other = [r[0] for r in rows if r[1] != rows[ports[0]][1] and r[1] < ncdm and r[3:] == rows[ports[0]][3:]][0]
        out["port of layer 0 replaced by one of another CDM group (Delta)"] = edit_dmrs(sl, lambda s: set_port(s, 0, other))
    else:                                                              # one group without data: every layer moves, and the data REs with it
        out["ports replaced by those of the next CDM group (Delta)"] = rebuilt(m, sl, dmrs_ports=(c["ports"] or 1) << 2)
    if ncdm >= 2 and all(rows[p][1] < ncdm - 1 for p in ports):
        out["ncdm one less: data on a muted comb"] = rebuilt(m, sl, num_dmrs_cdm_grps_no_data=ncdm - 1)
    i = [i for i in range(1, len(sl["segs"])) if sl["segs"][i - 1]["pattern"] and not sl["segs"][i]["pattern"]][0]
    s = sl["segs"][i]
    step = 1 if s["sym_off"] + 1 + s["nb_re"] <= s["plane"] else -1
    out["sym_off of the symbol after a DMRS symbol off by one"] = dict(segs=sl["segs"][:i] + [dict(s, sym_off=s["sym_off"] + step)] + sl["segs"][i + 1:])
    if any(s["pattern"] and s["nb_re"] for s in sl["segs"]):
        late = lambda s: dict(s, sym_off=s["sym_off"] + 1) if s["nb_re"] and s["sym_off"] + 1 + s["nb_re"] <= s["plane"] else s
        out["data of the DMRS symbols read one plane entry late"] = edit_dmrs(sl, late)
    if Nl >= 2:
        out["layer planes 0 and 1 swapped"] = dict(planes=np.concatenate([sl["tx"][1::-1], sl["tx"][2:]]))
    if c["si"]:
        out["built with si_rnti = 0"] = rebuilt(m, sl, si_rnti=0)
    if c["prg"] is not None:
        out["DMRS through the unit call, data precoded"] = dict(dmrs_unit=True)
        if len(set(c["pmis"])) > 1:
            out["PMIs rotated by one PRG"] = dict(pmis=c["pmis"][1:] + c["pmis"][:1])
        if c["prg"] < c["rb"]:
            out["prg_size + 1"] = dict(prgs=[dict(g, prg_size=g["prg_size"] + 1) for g in sl["prgs"]])
        out["matrices conjugated"] = dict(table=[dict(t, weights=t["weights"] * np.array([1, -1], np.int16)) for t in sl["table"]])
    return out


EXPECTED = {  # the perturbations beyond the five that apply to every case
    "l_prime": {"4", "5", "10"}, "ncdm one less": {"7", "10"}, "planes": {"3", "4", "5", "6", "9", "10", "12"}, "si_rnti": {"7"},
    "entry late": {"1", "2", "6", "8", "9", "10", "11", "12"}, "DMRS through": {"9", "10", "11"}, "PMIs rotated": {"9", "11"}, "prg_size": {"9", "11"}, "conjugated": {"9", "10", "11"}}


@pytest.mark.parametrize("name", NAMES)
def test_grid_of_the_cpu_forms_against_the_model(built, name):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    sl = slot_of(m, name)
    c = sl["case"]
    assert len(sl["segs"]) == c["n_sym"] and sum(s["nb_re"] for s in sl["segs"]) == sl["tx"].shape[1]
    b_max = float(sl["bound"].max())
    e_max = check_grid(sl, run_host(m, sl), "host form")
    print(f"case {name}: host form error {e_max:.3f} / bound {b_max:.3f} (amp {c['amp']}, Qm {c['Qm']}, T = {table_term(c['Qm']):.3f})")
    pert = perturbations(m, sl)
    for key, cases in EXPECTED.items():
        assert any(key in k for k in pert) == (name in cases), (name, key)
    assert len(pert) == 5 + sum(name in cases for cases in EXPECTED.values())
    ratios = {}
    for what, kw in pert.items():
        ratios[what] = float(grid_error(sl, run_host(m, sl, **kw)).max()) / b_max
        print(f"    {what}: {ratios[what]:.0f} x bound")
    assert all(r >= MISS for r in ratios.values()), (name, {k: r for k, r in ratios.items() if r < MISS})
    print(f"case {name}: smallest perturbation ratio {min(ratios.values()):.0f}")


def test_prg_rule_of_the_library_is_the_allocation_relative_one(built):
    """Case 11 starts at CRB 7 with P' = 4.  38.214 5.1.2.3 counts PRGs from CRB 0: {7}, {8..11}, {12}.  The library, as the reference
    and the FAPI PDU, counts them from the allocation's first RB: {7..10}, {11, 12}.  The model takes either; the
    grid of the CPU forms lies within the bound of the second and misses the first, so the deviation stays visible."""
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    sl = slot_of(m, "11")
    c = sl["case"]
    first = sum(c["first_rb"])
    assert [D.prg_of_rb(rb, first, 4, "allocation") for rb in range(6)] == [0, 0, 0, 0, 1, 1]
    assert [D.prg_of_rb(rb, first, 4, "crb") for rb in range(6)] == [0, 1, 1, 1, 1, 2]
    grid, mask = D.pdsch_grid(sl["p"], sl["bits"], c["n_tx"], prg_size=4, pmis=[1, 2, 2], matrices=model_matrices(sl["table"]), prg_origin="crb")
    assert np.array_equal(mask, sl["mask"])
    want = c["amp"] / np.sqrt(2.0) * np.stack([grid.real, grid.imag], -1)
    err = np.abs(slot_view(sl, run_host(m, sl)).astype(np.float64) - want) * mask[None, :, :, None]
    assert err.max() >= MISS * sl["bound"].max()


def test_beta_dmrs_of_the_library_is_one(built):
    """38.214 Table 4.1-1 gives the pilots sqrt(ncdm) of the data's amplitude; the reference, and the library with it, sends them
    at the data's.  With beta = sqrt 2 the model's pilots of case 7 (ncdm = 2) lie 0.41 * amp / 2 off the grid."""
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    sl = slot_of(m, "7")
    c = sl["case"]
    grid, _ = D.pdsch_grid(sl["p"], sl["bits"], c["n_tx"], beta_dmrs=np.sqrt(2.0))
    want = c["amp"] / np.sqrt(2.0) * np.stack([grid.real, grid.imag], -1)
    err = np.abs(slot_view(sl, run_host(m, sl)).astype(np.float64) - want) * sl["mask"][None, :, :, None]
    assert abs(err.max() - (np.sqrt(2.0) - 1) * c["amp"] / 2) <= sl["bound"].max()


# ---- loop-back through the UL receive front: the transmit grid read as the received one, identity channel, no noise -------------
LOOP_N, LOOP_RB, LOOP_FIRST_RB, LOOP_K0 = 256, 8, (1, 2), 256 - 41
LOOPS = {
    "a": dict(typ=0, ports=(1,), ncdm=1, Qm=4, amp=512, n_ant=1, precoded=False),      # w_f alternates
    "b": dict(typ=0, ports=(2,), ncdm=2, Qm=6, amp=512, n_ant=1, precoded=False),      # Delta = 1
    "c": dict(typ=1, ports=(1,), ncdm=1, Qm=4, amp=512, n_ant=1, precoded=False),      # type 2
    "d": dict(typ=0, ports=(0, 1), ncdm=1, Qm=6, amp=600, n_ant=2, precoded=False),    # two layers, layer a on antenna a
    "e": dict(typ=0, ports=(0, 1), ncdm=1, Qm=8, amp=2048, n_ant=4, precoded=True),    # two layers through one matrix onto four antennas
}
LOOP_PMI, LOOP_NVAR, LOOP_CH_OFF = 5, 4, 9


def build_loop(m, key):
    """Both sides' descriptors of one loop-back case, and the channel the receiver must find: H[l][a] = amp / sqrt 2 * W[l][a] (the
    unit matrix without precoding), the gain of a unit-power layer symbol on the grid"""
    import ul_slot_np as U
    from test_gpu_tb_chain import valid_tbs
    c = LOOPS[key]
    rng = np.random.default_rng(7300 + ord(key))
    N, rb, (bwp, rbs), typ, L, n_ant, Qm = LOOP_N, LOOP_RB, LOOP_FIRST_RB, c["typ"], len(c["ports"]), c["n_ant"], c["Qm"]
    S = rb * (13 * 12 + data_res_per_prb(typ, c["ncdm"], c["ports"][0]))
    G = Qm * L * S
    tb = dict(A=valid_tbs(G // 2, 1), G=G, BG=1, Qm=Qm, Nl=L, rv=0, tbslbrm=0)
    scr = (int(rng.integers(1, 0xfff0)), 0, int(rng.integers(0, 1024)))
    pay = rng.integers(0, 256, tb["A"] // 8, dtype=np.uint8)
    fco = (LOOP_K0 - 12 * (bwp + rbs)) % N
    slot, scid, nid = int(rng.integers(0, 20)), int(rng.integers(0, 2)), int(rng.integers(0, 65536))
    dl = dict(Nl=L, plane=S, dmrs_config_type=typ, num_dmrs_cdm_grps_no_data=c["ncdm"], dmrs_ports=sum(1 << p for p in c["ports"]), scid=scid,
              dl_dmrs_scrambling_id=nid, slot=slot, si_rnti=0, amp=c["amp"], fft_size=N, first_carrier_offset=fco, bwp_start=bwp, rb_start=rbs, rb_size=rb,
              start_symbol=0, nr_of_symbols=14, dl_dmrs_symb_pos=1 << 2, tx_slot_off=TX_OFF, lay_off=0)
    stride = 14 * N + TX_OFF + PAD
    ch_stride = 14 * N + 64
    ul = dict(tb=0, Qm=Qm, dmrs_config_type=typ, num_dmrs_cdm_grps_no_data=c["ncdm"], dmrs_symbol=2, fft_size=N, first_carrier_offset=fco, bwp_start=bwp,
              rb_start=rbs, rb_size=rb, start_symbol=0, nr_of_symbols=14, ul_dmrs_symb_pos=1 << 2, plane=G // Qm, rx_slot_off=TX_OFF, ch_off=LOOP_CH_OFF,
              rec_off=0)
    cfg = dict(slot=slot, scid=scid, dmrs_scrambling_id=nid, port=c["ports"][0], chest_freq=0)
    W = np.eye(L, n_ant, dtype=np.complex128)
    table, prgs, pmis = None, None, []
    if c["precoded"]:
        # equal moduli, layer 1 = layer 0 turned and sign-alternated over the antennas: the two rows are orthogonal
        ph = rng.uniform(0, 2 * np.pi, n_ant)
        row = 9700.0 * np.exp(1j * ph)
        w = np.stack([row, row * np.exp(1j * rng.uniform(0, 2 * np.pi)) * (-1.0) ** np.arange(n_ant)])
        wq = np.rint(np.stack([w.real, w.imag], -1)).astype(np.int16)
        assert (np.abs(wq.astype(np.int64)).sum(axis=(0, 2)) <= 32767).all()
        table, pmis = [dict(pm_idx=LOOP_PMI, numLayers=L, num_ant_ports=n_ant, weights=wq)], [LOOP_PMI]
        msegs, prgs = m.pdsch_precode_segments([dl], [dict(prg_size=rb, pmi_off=0, pmi_count=1)], 1)
        W = (wq[..., 0] + 1j * wq[..., 1]) / 32768.0
    else:
        msegs = m.pdsch_map_segments([dl])
    gsegs, first = m.pusch_grid_segments([ul])
    csegs = U.chest_descriptors(m, ul, cfg, c["ports"], n_ant, ch_stride)
    dm = [s for s in msegs if s["pattern"]]
    assert len(dm) == 1 and len(csegs) == L and dm[0]["port"][:L] == list(c["ports"]) == [s["port"] for s in csegs]
    assert all((s["c_init"], s["dmrs_offset"], s["start_re"]) == (dm[0]["c_init"], dm[0]["dmrs_offset"], dm[0]["start_re"]) for s in csegs)
    H = c["amp"] / np.sqrt(2.0) * W
    max_ch = int(np.ceil(max(np.abs(H.real).max(), np.abs(H.imag).max()))) + 8
    if L == 2:   # the band DESIGN 4.11.1 names for the MMSE receiver: the level is the loudest pair's, log2_approx of it stays 18
        p = np.abs(H) ** 2
        assert 2 ** 17 <= p.max() < 2 ** 18 and ((p == 0) | ((p >= 2 ** 17) & (p < 2 ** 18))).all() and max_ch < 2048
    return dict(case=dict(n_layers=L, n_rx=n_ant, N=N, rb=rb, Qm=Qm), loop=c, tb=tb, scr=scr, pay=pay, dl=dl, msegs=msegs, prgs=prgs, pmis=pmis, table=table,
                gsegs=gsegs, first=first, csegs=csegs, delay=np.zeros(L * n_ant, np.int32), rx_stride=stride, stride=stride, ch_stride=ch_stride, H=H,
                max_ch=max_ch, nvar=LOOP_NVAR)


def loop_grid_host(m, lp, planes):
    """the transmit grid of the host forms, zeros where nothing is sent: int16 [n_ant, stride, 2]"""
    c, n_ant, L = lp["loop"], lp["case"]["n_rx"], lp["case"]["n_layers"]
    tx = np.zeros((n_ant * lp["stride"], 2), np.int16)
    planes = np.ascontiguousarray(planes)
    for i, s in enumerate(lp["msegs"]):
        for ant in range(n_ant):
            d = dict(s, tx_off=s["tx_off"] + ant * lp["stride"])
            if c["precoded"]:
                m.pdsch_precode_host(planes, d, lp["prgs"][i], lp["pmis"], lp["table"], n_ant, ant, tx)
            else:
                m.pdsch_map_host(planes, d, ant if ant < L else -1, tx)
    return tx.reshape(n_ant, lp["stride"], 2)


@pytest.mark.parametrize("key", sorted(LOOPS))
def test_loop_back_on_the_cpu_forms(built, key):
    """what test_gpu_dl_slot.py runs on the GPU, on the CPU forms: the estimates lie at H, and the payload comes back with ACK"""
    import openairinterface5g_amd as pkg
    import ul_slot_np as U
    m = pkg.ldpc
    lp = build_loop(m, key)
    planes = symbols_np(O.dlsch_encode(lp["tb"], lp["pay"]), lp["scr"], lp["case"]["Qm"], lp["case"]["n_layers"])
    sl = dict(lp, rx=loop_grid_host(m, lp, planes))
    ch = U.estimate_host(m, sl)
    est = U.planes_of(sl, ch).astype(np.float64)
    off = np.abs(est - np.stack([lp["H"].real, lp["H"].imag], -1)[:, :, None, :]).max()
    print(f"loop {key}: |est - H| <= {off:.1f} with |H| up to {np.abs(lp['H']).max():.0f}")
    assert off <= 0.03 * np.abs(lp["H"]).max()
    lv, rec = U.front_records(sl, ch, m)
    got, ack, iters = U.decode_record(sl, rec)
    assert ack and np.array_equal(got, lp["pay"]), (key, lv, iters)
