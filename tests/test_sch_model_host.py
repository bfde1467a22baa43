"""sch_np.py, the coding chain written from TS 38.212 alone, against facts from outside this repository's reading of the
reference (the CRC catalogue's check values, the reference-COMPILED code words of tests/golden/ref_encoder.npz); then the oracle,
the library's host helpers and the kernels as written (tests/emul) against the model, on the cases of sch_cases.py; then the
mutations: each deliberate misreading of the standard must change the model's output on at least one case (no GPU)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
import sch_cases as SC
import sch_np as S
from common import load_ref_code_words, load_ref_transport_blocks

IDS = [c["id"] for c in SC.CASES]


def payload_of(tb, seed=0):
    return np.random.default_rng(4100 + tb["A"] + seed).integers(0, 256, tb["A"] // 8, dtype=np.uint8)


_BLOCKS = {}


def blocks_of(case):
    """(payload, sizes, [d_r]) of a case by the unmutated model, computed once"""
    if case["id"] not in _BLOCKS:
        pay = payload_of(case["tb"])
        s, ds = S.code_blocks(case["tb"], pay)
        _BLOCKS[case["id"]] = (pay, s, np.stack(ds))
    return _BLOCKS[case["id"]]


def model_bits(case):
    pay, s, ds = blocks_of(case)
    seg, idx = S.positions(case["tb"])
    return ds[seg, idx].astype(np.uint8)


# ---- the model against facts it shares with nobody here -------------------------------------------------------------------
def test_the_model_names_numpy_and_the_graph_tables_only():
    src = (Path(__file__).resolve().parent / "sch_np.py").read_text()
    assert re.findall(r"^\s*(?:import|from)\s+(.+)$", src, re.M) == ["numpy as np", "oracle_lib import graph"]
    code = src.split('"""', 2)[2]                                     # (the module's docstring says what it stays away from)
    assert not re.search(r"openairinterface5g_amd|softbuf_np|nr_schsim|callers_np|\bO\.|oracle_lib|dlsch_encode|rate_match\(|segmentation\(|"
                         r"get_E|interleave\(|csrc|ctypes|import", code.replace("import numpy as np", "", 1).replace("from oracle_lib import graph", "", 1))
    assert len(re.findall(r"\bgraph\(", code)) == 1
    src = (Path(__file__).resolve().parent / "sch_cases.py").read_text()
    assert re.findall(r"^\s*(?:import|from)\s+(.+)$", src, re.M) == ["numpy as np", "sch_np as S"]


def test_crc_check_values_of_the_catalogue():
    msg = np.unpackbits(np.frombuffer(b"123456789", np.uint8))
    value = lambda g: int("".join(str(b) for b in S.crc_parity(msg, g)), 2)
    assert (value(S.G_CRC24A), value(S.G_CRC24B), value(S.G_CRC16)) == (0xCDE703, 0x23EF52, 0x31C3)
    assert S.crc_attach(msg, S.G_CRC16).size == msg.size + 16 and not S.crc_parity(S.crc_attach(msg, S.G_CRC24B), S.G_CRC24B).any()


def test_reference_compiled_code_words_and_transport_blocks():
    n_tb = n_cw = 0
    for c in load_ref_transport_blocks():
        s, ds = S.code_blocks(c["tb"], c["payload"])
        assert (s["C"], s["Zc"], s["K"], s["F"], s["Kb"]) == (c["C"], c["Z"], c["K"], c["F"], c["Kb"]), c["tb"]
        assert s["byte_contract"]
        for d, w in zip(ds, c["code_words"]):
            k = np.arange(d.size)
            assert np.array_equal(d == S.NULL, (k >= s["Kp"] - 2 * s["Zc"]) & (k < s["K"] - 2 * s["Zc"]))
            assert np.array_equal(np.where(d == S.NULL, 0, d), w), c["tb"]
            n_cw += 1
        assert np.array_equal(S.dlsch(c["tb"], c["payload"]), c["coded"]), c["tb"]
        n_tb += 1
    print(f"{n_tb} reference transport blocks, {n_cw} code words")
    assert n_tb >= 8 and n_cw >= 46


def test_model_h_annihilates_the_reference_compiled_code_words():
    n = 0
    for v in load_ref_code_words():
        Z = v["Z"]
        info = np.unpackbits(np.asarray(v["info"], np.uint8))[:S.KB_FULL[v["BG"]] * Z]
        word = np.concatenate([info, v["coded"][info.size - 2 * Z:]])
        assert np.array_equal(info[2 * Z:], v["coded"][:info.size - 2 * Z])
        assert not S.syndrome(v["BG"], Z, word).any(), (v["BG"], Z)
        flipped = word.copy()
        flipped[(7 * n) % word.size] ^= 1
        assert S.syndrome(v["BG"], Z, flipped).any()
        n += 1
    assert n == 213


def test_segmentation_of_the_model_takes_any_block_length():
    """B that no byte-aligned caller produces: the blocks' payload parts give B back, every block of C > 1 passes CRC24B over its K'
    bits, the fillers are the last F, and the byte contract is reported as unmet"""
    rng = np.random.default_rng(12)
    with pytest.raises(ValueError):
        S.segment_sizes(3841, 2)                                       # B' = 3889 on two blocks: 5.2.2 has no K' for it
    for BG, B in ((1, 37), (2, 193), (2, 3842), (1, 8450), (1, 16851), (2, 7635)):
        b = rng.integers(0, 2, B, dtype=np.uint8)
        s, cs = S.segment(b, BG)
        assert not s["byte_contract"] and len(cs) == s["C"] == (1 if B <= S.KCB[BG] else -(-B // (S.KCB[BG] - 24)))
        back = []
        for c in cs:
            assert (c[:s["Kp"]] != S.NULL).all() and (c[s["Kp"]:] == S.NULL).all() and c.size == s["K"]
            if s["C"] > 1:
                assert not S.crc_parity(c[:s["Kp"]].astype(np.uint8), S.G_CRC24B).any()
            back.append(c[:s["Kp"] - s["L"]])
        assert np.array_equal(np.concatenate(back), b)
        d = S.ldpc_encode(cs[0], BG, s["Zc"])                          # (its own syndrome check runs inside)
        assert (d == S.NULL).sum() == s["F"]


# ---- the cases ---------------------------------------------------------------------------------------------------------
def test_every_edge_is_reached_and_counted():
    count = dict.fromkeys(SC.ALL_EDGES, 0)
    for c in SC.CASES:
        p = S.plan(c["tb"])
        assert p["byte_contract"] and c["tb"]["G"] % (c["tb"]["Qm"] * c["tb"]["Nl"]) == 0
        assert p["Zc"] <= 64 or (p["BG"] == 2 and p["B"] in (560, 640, 648)) or p["A"] in (3824, 3832) or p["C"] >= 3 or abs(p["B"] - S.KCB[p["BG"]]) <= 16, c["id"]
        if p["C"] >= 3:                                               # the boundary block: the first C - (G / (Nl Qm)) mod C are the short ones
            q = c["tb"]["G"] // (c["tb"]["Qm"] * c["tb"]["Nl"])
            first_long = p["C"] - q % p["C"]
            assert all(E == p["E"][0] for E in p["E"][:first_long]) and all(E == p["E"][0] + c["tb"]["Qm"] * c["tb"]["Nl"] for E in p["E"][first_long:])
            assert 0 < first_long < p["C"] and sum(p["E"]) == c["tb"]["G"]
        for e in SC.edges_of(c["tb"]):
            count[e] = count.get(e, 0) + 1
    print(f"{len(SC.CASES)} cases, {len(count)} edges")
    for e, n in count.items():
        print(f"    {n:3d}  {e}")
    assert not [e for e, n in count.items() if n == 0]
    assert set(SC.ALL_EDGES) <= set(count)


# ---- the oracle and the library's host helpers against the model ---------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_oracle_chain_equals_the_model(cid):
    c = SC.CASES[IDS.index(cid)]
    tb = c["tb"]
    pay, s, _ = blocks_of(c)
    p = S.plan(tb)
    o = O.segmentation(None, p["B"], tb["BG"])
    assert (o["C"], o["K"], o["Z"], o["F"], o["Kb"]) == (p["C"], p["K"], p["Zc"], p["F"], p["Kb"])
    assert [O.get_E(tb["G"], p["C"], tb["Qm"], tb["Nl"], r) for r in range(p["C"])] == p["E"]
    want = model_bits(c)
    assert np.array_equal(O.dlsch_encode(tb, pay), want), tb
    assert np.array_equal(S.dlsch(tb, pay), want)
    # the way back: round 0 at the case's rv, a second round at the next rv, seeded LLRs in +-200
    rng = np.random.default_rng(99)
    rounds = [dict(tb), dict(tb, rv=(tb["rv"] + 1) % 4)]
    llrs = [rng.integers(-200, 201, tb["G"]).astype(np.int16) for _ in rounds]
    harq = [rng.integers(-3000, 3000, p["N"]).astype(np.int16) for _ in range(p["C"])]
    for rnd, (t, llr) in enumerate(zip(rounds, llrs)):
        off = 0
        for r, E in enumerate(p["E"]):
            e = O.deinterleave(E, t["Qm"], llr[off:off + E])
            if rnd == 0:
                harq[r][:] = 0                                         # (nr_ulsch_decoding clears d on a first transmission)
            rc, d = O.rate_match_rx(t["tbslbrm"], t["BG"], p["Zc"], harq[r], e, p["C"], t["rv"], 1 if rnd == 0 else 0, E, p["F"], p["fs"])
            assert rc == 0
            harq[r][:] = d
            off += E
        for r, b in enumerate(S.soft_buffers(rounds[:rnd + 1], llrs[:rnd + 1])):
            assert np.array_equal(harq[r][:p["Ncb"]], b), (cid, rnd, r)


def test_host_helpers_of_the_library_equal_the_model(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    for c in SC.CASES:
        tb, p = c["tb"], S.plan(c["tb"])
        g = m.nr_segmentation(p["B"], tb["BG"])
        assert g is not None and (g["C"], g["K"], g["Z"], g["F"], g["Kb"]) == (p["C"], p["K"], p["Zc"], p["F"], p["Kb"]), c["id"]
        assert [m.nr_get_E(tb["G"], p["C"], tb["Qm"], tb["Nl"], r) for r in range(p["C"])] == p["E"], c["id"]
    # every B the thresholds lie between, byte aligned or not: the sizes agree wherever 5.2.2 defines them, and the library
    # refuses exactly the blocks outside its byte contract
    n_refused = 0
    for BG in (1, 2):
        for B in list(range(24, 1200)) + list(range(3800, 3900)) + list(range(7600, 7700)) + list(range(8400, 8500)) + list(range(16800, 16900)):
            try:
                s = S.segment_sizes(B, BG)
            except ValueError:
                continue
            g = m.nr_segmentation(B, BG)
            assert (g is not None) == s["byte_contract"], (B, BG)
            n_refused += g is None
            if g is not None:
                assert (g["C"], g["K"], g["Z"], g["F"], g["Kb"]) == (s["C"], s["K"], s["Zc"], s["F"], s["Kb"]), (B, BG)
            o = O.segmentation(None, B, BG)
            assert (o["C"], o["K"], o["Z"], o["F"], o["Kb"]) == (s["C"], s["K"], s["Zc"], s["F"], s["Kb"]), (B, BG)
    assert n_refused > 1000


# ---- the kernels as written, on the CPU ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul(built):
    L = C.CDLL(str(Path(__file__).resolve().parent / "emul" / "libldpc_emul.so"))
    L.tb_emul_tx_select.argtypes = [C.c_uint32, C.c_int] + [C.c_uint32] * 3 + [C.c_int, C.c_int] + [C.c_uint32] * 3 + [C.c_int] + [C.c_void_p] * 2
    L.tb_emul_rx_dematch.argtypes = [C.c_uint32, C.c_int] + [C.c_uint32] * 4 + [C.c_int] + [C.c_uint32] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 3
    L.tb_emul_rx_dematch_cut.argtypes = ([C.c_uint32, C.c_int] + [C.c_uint32] * 4 + [C.c_int] + [C.c_uint32] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 3)
    L.tb_emul_first_tx_columns.argtypes = [C.c_uint32, C.c_int] + [C.c_uint32] * 4 + [C.c_int, C.c_uint32]
    return L


def direct_blocks():
    """(BG, Zc, Kb, F, C, tbslbrm, rv, E, Qm) the chain calls cannot reach: Zc 6, 7, 15, 36 and F no multiple of 8, plus every block
    of every case"""
    out = []
    n = 0
    for BG, Zc, Kb, F in ((1, 6, 22, 0), (1, 6, 22, 5), (1, 7, 22, 30), (1, 15, 22, 13), (1, 36, 22, 41), (2, 6, 6, 27), (2, 7, 8, 17), (2, 15, 10, 3),
                          (2, 15, 9, 22), (2, 36, 8, 90), (2, 36, 10, 0)):
        K, N = S.KB_FULL[BG] * Zc, S.NCOL[BG] * Zc
        assert F >= K - Kb * Zc
        fe = K - 2 * Zc
        for ncb in (None, fe + 1, fe + 2 * Zc + 1, N - Zc - 4):
            T = 0
            if ncb is not None:
                while SC.lbrm_for(ncb, 1) is None:
                    ncb += 1
                T = SC.lbrm_for(ncb, 1)
            Ncb = S.circular_buffer_len(N, 1, T)
            V = Ncb - F
            for rv in range(4):
                Qm = (2, 4, 6, 8)[n % 4]
                n += 1
                least = -(-(K - F - 2 * Zc) // Qm) * Qm                # (below it the library refuses: test_refusal_... below)
                for E in sorted({least, max(least, (V - 1) // Qm * Qm), -(-(Ncb + 3) // Qm) * Qm, -(-(3 * V + 5) // Qm) * Qm}):
                    out.append((BG, Zc, Kb, F, 1, T, rv, E, Qm))
    return out


def test_tx_selection_of_the_kernel_equals_the_model(emul):
    rng = np.random.default_rng(515)
    n = odd_f = 0
    encoded = {}
    for BG, Zc, Kb, F, Cn, T, rv, E, Qm in direct_blocks():
        K = S.KB_FULL[BG] * Zc
        if (BG, Zc, F) not in encoded:
            c = rng.integers(0, 2, K).astype(np.int8)
            c[K - F:] = S.NULL
            encoded[(BG, Zc, F)] = (c, S.ldpc_encode(c, BG, Zc))
        c, d = encoded[(BG, Zc, F)]
        seg = np.packbits(np.concatenate([np.where(c == S.NULL, 0, c).astype(np.uint8), np.zeros((-K) % 8, np.uint8)]))
        idx, Ncb, k0 = S.block_positions(BG, Zc, K, F, Cn, T, rv, E, Qm)
        want = d[idx]
        assert (want != S.NULL).all()
        out = np.full(E + 16, 0x77, np.uint8)
        got = out[8:8 + E]
        rc = emul.tb_emul_tx_select(T, BG, Zc, Cn, F, Kb, rv, E, Qm, 32, 64, seg.ctypes.data, got.ctypes.data)
        assert rc == -(-(E // Qm) // 32), (BG, Zc, Kb, F, T, rv, E, Qm, rc)
        assert np.array_equal(got, want.astype(np.uint8)), (BG, Zc, Kb, F, T, rv, E, Qm)
        assert (out[:8] == 0x77).all() and (out[8 + E:] == 0x77).all()
        n += 1
        odd_f += F % 8 != 0
    print(f"{n} blocks through the TX selection, {odd_f} with F no multiple of 8")
    assert n > 500 and odd_f > 300


def rx_blocks():
    """direct_blocks() and every distinct block of the cases (the Zc the chain calls take, at the edges the cases sit on)"""
    out = direct_blocks()
    for c in SC.CASES:
        tb, p = c["tb"], S.plan(c["tb"])
        if p["Zc"] <= 64:
            out += [(tb["BG"], p["Zc"], p["Kb"], p["F"], p["C"], tb["tbslbrm"], tb["rv"], E, tb["Qm"]) for E in sorted(set(p["E"]))]
    return out


def test_rx_dematching_of_the_kernel_equals_the_model(emul):
    """round 0 on a dirty buffer (the kernel clears it) and a combining round on a dirty buffer, [0, Ncb) against the plain sum"""
    rng = np.random.default_rng(616)
    n = 0
    for BG, Zc, Kb, F, Cn, T, rv, E, Qm in rx_blocks():
        K, N = S.KB_FULL[BG] * Zc, S.NCOL[BG] * Zc
        idx, Ncb, k0 = S.block_positions(BG, Zc, K, F, Cn, T, rv, E, Qm)
        f = rng.integers(-200, 201, E).astype(np.int16)
        add = np.zeros(Ncb, np.int64)
        np.add.at(add, idx, f.astype(np.int64))
        num_llr = (S.NCOL[BG] + 2) * Zc
        for clear in (1, 0):
            w0 = rng.integers(-2000, 2000, N + 16).astype(np.int16)
            w = w0.copy()
            l = np.zeros(num_llr + 8, np.int8)
            span = emul.tb_emul_rx_dematch(T, BG, Zc, Cn, F, K, rv, E, Qm, num_llr, clear, 256, f.ctypes.data, w.ctypes.data, l.ctypes.data)
            assert span > 0, (BG, Zc, F, T, rv, E, Qm)
            want = add if clear else add + w0[:Ncb]
            assert np.array_equal(w[:Ncb].astype(np.int64), want), (BG, Zc, Kb, F, T, rv, E, Qm, clear)
            assert np.array_equal(w[N:], w0[N:])
            n += 1
    print(f"{n} de-matching runs")
    assert n > 1200


def test_rx_dematching_on_a_cut_graph_equals_the_model(emul):
    """tb_emul_rx_dematch_cut: a first transmission is decoded on the rate mode's graph cut behind the last column it reaches (num_llr =
    max(tb_emul_first_tx_columns, core columns + 1) Zc) while the soft buffer is cleared for the whole mode (np_mode uncut); a
    combining round is never cut.  [0, Ncb) is the plain sum all the same.  The rate mode is the one nr_get_R_ldpc_decoder names
    for the block."""
    rng = np.random.default_rng(717)
    n = cut = 0
    for BG, Zc, Kb, F, Cn, T, rv, E, Qm in rx_blocks():
        K, N = S.KB_FULL[BG] * Zc, S.NCOL[BG] * Zc
        idx, Ncb, k0 = S.block_positions(BG, Zc, K, F, Cn, T, rv, E, Qm)
        f = rng.integers(-200, 201, E).astype(np.int16)
        add = np.zeros(Ncb, np.int64)
        np.add.at(add, idx, f.astype(np.int64))
        ncols = O.NCOLS[(BG, O.get_R(rv, E, BG, Zc, 0, 0)[0])]
        reach = emul.tb_emul_first_tx_columns(T, BG, Zc, Cn, F, K, rv, E)
        assert reach > 0
        ncut = min(ncols, max(reach, (26 if BG == 1 else 14) + 1))
        for clear in (1, 0):
            nc = ncut if clear else ncols
            w0 = rng.integers(-2000, 2000, N + 16).astype(np.int16)
            w = w0.copy()
            l = np.full(ncols * Zc + 8, 0x11, np.int8)
            span = emul.tb_emul_rx_dematch_cut(T, BG, Zc, Cn, F, K, rv, E, Qm, nc * Zc, ncols * Zc - 2 * Zc, clear, 256, f.ctypes.data, w.ctypes.data,
                                               l.ctypes.data)
            assert span > 0, (BG, Zc, F, T, rv, E, Qm)
            want = add if clear else add + w0[:Ncb]
            assert np.array_equal(w[:Ncb].astype(np.int64), want), (BG, Zc, Kb, F, T, rv, E, Qm, clear, nc, ncols)
            assert np.array_equal(w[N:], w0[N:]) and (l[nc * Zc:] == 0x11).all()
            n += 1
            cut += clear and nc < ncols
    print(f"{n} de-matching runs through the cut entry, {cut} of them on a cut graph")
    assert n > 1200 and cut > 100


def test_refusals_of_the_documented_contract(emul):
    """5.4.2.1 defines a block with E below K' - 2 Zc and a circular buffer that ends before or inside the fillers; the reference reports
    "invalid parameters" or is outside its own contract there, and nr_hip_rate_match_geometry documents the refusal of all three.
    The model gives the bits; the emulated kernel's entry refuses; test_gpu_sch_model.py asserts the call's message."""
    kinds = []
    for tb in SC.REFUSED:
        p = S.plan(tb)
        E = p["E"][0]
        kinds.append("E below the first filler" if E < p["fs"] else "Ncb before the fillers" if p["Ncb"] < p["fs"] else
                     "Ncb inside the fillers" if p["Ncb"] < p["fe"] else None)
        assert kinds[-1] == tb["kind"] and S.dlsch(tb, payload_of(tb)).size == tb["G"]
        out = np.zeros(tb["G"] + 64, np.uint8)
        seg = np.zeros(p["K"] // 8 + 1, np.uint8)
        assert emul.tb_emul_tx_select(tb["tbslbrm"], tb["BG"], p["Zc"], 1, p["F"], p["Kb"], 0, E, 2, 32, 64, seg.ctypes.data, out.ctypes.data) == -1
        assert emul.tb_emul_first_tx_columns(tb["tbslbrm"], tb["BG"], p["Zc"], 1, p["F"], p["K"], 0, E) == -1
    assert len(set(kinds)) == 3


# ---- mutations ----------------------------------------------------------------------------------------------------------
POSITION_ONLY = {m for m in S.MUTATIONS if m.startswith("k0") or m in (
    "wrap modulo N under LBRM", "N_ref: division by C before the 3/2", "E_r rule with <", "larger E first", "interleaver transposed",
    "fillers transmitted", "filler range one bit early")}


def applies(mut, tb, p):
    """whether a mutation can change anything for a case at all (a necessary condition, from the clause it sits in)"""
    m = re.match(r"k0 numerator \+ 1, BG(\d) rv(\d)", mut)
    if m:
        return tb["BG"] == int(m.group(1)) and tb["rv"] == int(m.group(2))
    lbrm = p["Ncb"] < p["N"]
    return {"k0 not scaled by Ncb / N": lbrm and tb["rv"] > 0, "k0 floor after the multiplication by Zc": lbrm and tb["rv"] > 0,
            "wrap modulo N under LBRM": lbrm, "N_ref: division by C before the 3/2": bool(tb["tbslbrm"]) and p["C"] > 1,
            "E_r rule with <": len(set(p["E"])) > 1, "larger E first": len(set(p["E"])) > 1, "interleaver transposed": True,
            "fillers transmitted": p["F"] > 0, "filler range one bit early": p["F"] > 0, "CB CRC over the fillers too": p["C"] > 1 and p["F"] > 0,
            "CRC24A for the code blocks": p["C"] > 1, "CB CRC at C = 1": p["C"] == 1, "A >= 3824": tb["A"] == 3824,
            "Kb threshold 640 with >=": p["B"] == 640 and tb["BG"] == 2, "Kb threshold 560 with >=": p["B"] == 560 and tb["BG"] == 2,
            "Kb threshold 192 with >=": p["B"] == 192 and tb["BG"] == 2, "Zc with Kb Zc > K'": p["Kb"] * p["Zc"] == p["Kp"],
            "circulants shifted left": True, "payload bytes LSB first": True}[mut]


def mutated_bits(case, mut):
    tb = case["tb"]
    try:
        if mut in POSITION_ONLY:
            _, _, ds = blocks_of(case)
            seg, idx = S.positions(tb, mut)
            return np.where(ds[seg, idx] == S.NULL, 0, ds[seg, idx]).astype(np.uint8)
        return S.dlsch(tb, payload_of(tb), mut)
    except (ValueError, AssertionError, IndexError):
        return None                                                   # the misreading does not even yield G bits


# where applies() is also sufficient: every case of the clause sees the mutation (circulants: Zc = 2 shifts alike both ways; the k0
# and filler ones can select the same bits, or bits that happen to be equal)
EXACT = {"E_r rule with <", "larger E first", "interleaver transposed", "CB CRC over the fillers too", "CRC24A for the code blocks", "CB CRC at C = 1",
         "A >= 3824", "Kb threshold 640 with >=", "Kb threshold 560 with >=", "Kb threshold 192 with >=", "Zc with Kb Zc > K'", "payload bytes LSB first"}

# the cases that see each mutation, by their index in SC.CASES (DESIGN 4.3.1 carries the same table): a change of the case list
# that takes a case away from a mutation fails here
SEEN_BY = {
    "k0 numerator + 1, BG1 rv0": "00-03 16-18 22 36",
    "k0 numerator + 1, BG1 rv1": "23 38 58 61-67",
    "k0 numerator + 1, BG1 rv2": "20 24 40-41",
    "k0 numerator + 1, BG1 rv3": "21 25 42 75-79",
    "k0 numerator + 1, BG2 rv0": "04-08 10-15 26-28 32 44",
    "k0 numerator + 1, BG2 rv1": "09 29 33 46-47 80-84",
    "k0 numerator + 1, BG2 rv2": "30 34 48 68-74",
    "k0 numerator + 1, BG2 rv3": "31 35 50",
    "k0 not scaled by Ncb / N": "09 39 41 43 47 49 51-60 68-79",
    "k0 floor after the multiplication by Zc": "09 41 43 47 49 51 58-59 68-79",
    "wrap modulo N under LBRM": "09 37 39 41 43 45 47 49 51-55 57-60 69-71 73-79",
    "N_ref: division by C before the 3/2": "09",
    "E_r rule with <": "08",
    "larger E first": "08",
    "interleaver transposed": "00-84",
    "fillers transmitted": "00-01 03 05 07-15 17-19 21-23 25-28 31-32 35-39 41-45 47 49-55 57-67 69 71 74 76 79 82 84",
    "filler range one bit early": "00 03 05 07-11 14 19 22 26-27 31 44-45 47 49-55 57-64 69 71 73-75 82-84",
    "CB CRC over the fillers too": "03 05 07-09",
    "CRC24A for the code blocks": "03 05 07-09",
    "CB CRC at C = 1": "00-02 04 06 10-84",
    "A >= 3824": "00 04 06",
    "Kb threshold 640 with >=": "14",
    "Kb threshold 560 with >=": "12",
    "Kb threshold 192 with >=": "10",
    "Zc with Kb Zc > K'": "02 04 06 10 16 26 28 57",
    "circulants shifted left": "10-11 13 16-51 55-84",
    "payload bytes LSB first": "10-11 13 16-84",
}


def as_ranges(ids):
    ids, out, i = sorted(ids), [], 0
    while i < len(ids):
        j = i
        while j + 1 < len(ids) and ids[j + 1] == ids[j] + 1:
            j += 1
        out.append("%02d" % ids[i] if i == j else "%02d-%02d" % (ids[i], ids[j]))
        i = j + 1
    return " ".join(out)


def test_every_mutation_is_seen_by_exactly_the_cases_of_the_table():
    """Every mutation on every case: the set of cases whose output changes is the pinned one, lies inside the mutation's clause
    (applies()) and, for the EXACT ones, is the whole clause.  Left out as too slow for what they add: the two mutations that touch
    every block (circulants, payload bit order) on the cases with Zc > 64, and the mutations of the encoder's side on the cases with Zc
    > 72 that lie outside their clause."""
    assert set(SEEN_BY) == set(S.MUTATIONS)
    for mut in S.MUTATIONS:
        seen, clause = [], []
        for i, c in enumerate(SC.CASES):
            tb, p = c["tb"], S.plan(c["tb"])
            inside = applies(mut, tb, p)
            if mut in ("circulants shifted left", "payload bytes LSB first") and p["Zc"] > 64:
                continue
            if mut not in POSITION_ONLY and p["Zc"] > 72 and not inside:
                continue
            got = mutated_bits(c, mut)
            if got is None or got.size != tb["G"] or not np.array_equal(got, model_bits(c)):
                assert inside, (mut, c["id"])
                seen.append(i)
            clause += [i] if inside else []
        print(f"    {len(seen):3d}  {mut}: {as_ranges(seen)}")
        assert seen and as_ranges(seen) == SEEN_BY[mut], (mut, as_ranges(seen))
        assert mut not in EXACT or seen == clause, (mut, as_ranges(clause))
